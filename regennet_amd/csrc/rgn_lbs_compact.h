// The load-time compaction behind rgn_body_set_joint_regressors (rgn_lbs.hip): the body restricted to the vertices the regressed joint types touch.
// Host code only - no device call, no HIP header - so that tools/joints_args_check.cpp can run it under the host sanitizers on a machine without a GPU.
//
//   S    = the picked vertices (vertex_joints) united with the columns of J_regressor_extra that hold a non-zero, sorted ascending, padded to a
//          multiple of 32 with entries that carry zeros throughout (template, blend shapes, skinning weights, joint weights): a pad vertex is 0
//   cut  = v_template / shapedirs / posedirs / lbs_weights restricted to S, in the layouts rgn_body_create lays down for k_lbs_skin (Vp := Sp)
//   wj   = the [Np + Jr] x |S| joint weights as the A operand of v_mfma_f32_32x32x2_f32 whose B operand is the skinned tile AS IT LEAVES THE
//          ACCUMULATORS: register q of half-wave h holds vertex 8 (q / 4) + 4 h + (q % 4) of the tile, so k-step q takes k = h from that vertex, and
//          wj [tile][q][lane] = W[row = lane & 31][32 tile + 8 (q / 4) + 4 (lane >> 5) + (q % 4)]  (rows past Np + Jr: 0). A picked row holds a single 1.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace rgn {

constexpr int LBS_MAX_JOINT_ROWS = 32;              // Np + Jr: the M of the one MFMA tile the joint weights fill (the reference's count is 30)

struct LbsDims {
    int V, J, Jp, nb, nbp, K, Kp;
    bool pose;
};

struct LbsCompact {
    int nS = 0, Sp = 0, Np = 0, Jr = 0;
    std::vector<int32_t> S;                         // [nS] vertex ids, ascending
    std::vector<float> blob;                        // vt [nS,3] | sd [nS,3,nb] | vtp [3][Sp] | sdp [nbp][3][Sp] | pd [Kp][3][Sp] | wt [Jp][Sp] | wj [Sp/32][16][64]
    size_t o_vt = 0, o_sd = 0, o_vtp = 0, o_sdp = 0, o_pd = 0, o_wt = 0, o_wj = 0;
};

// what rgn_body_set_joint_regressors refuses that needs no body: "" when the counts and pointers are good
inline std::string lbs_regressor_args(int Np, const int32_t* picks, int Jr, const float* reg) {
    if (Np < 0 || Jr < 0) return "Np or Jr < 0";
    if (Np + Jr < 1) return "Np and Jr are both 0";
    if (Np + Jr > LBS_MAX_JOINT_ROWS) return "Np + Jr = " + std::to_string(Np + Jr) + " > 32";
    if (Np > 0 && !picks) return "Np > 0 without vertex_joints";
    if (Jr > 0 && !reg) return "Jr > 0 without a regressor";
    return "";
}

// "" and `c` filled, or why not. v_template [V,3], shapedirs [V,3,nb] (nb > 0), posedirs [K,3V] (d.pose), lbs_weights [V,J]: the arrays rgn_body_create took.
inline std::string lbs_compact(const LbsDims& d, const float* v_template, const float* shapedirs, const float* posedirs, const float* lbs_weights, int Np,
                               const int32_t* picks, int Jr, const float* reg, LbsCompact& c) {
    std::string why = lbs_regressor_args(Np, picks, Jr, reg);
    if (!why.empty()) return why;
    std::vector<uint8_t> used((size_t)d.V, 0);
    for (int i = 0; i < Np; ++i) {
        if (picks[i] < 0 || picks[i] >= d.V) return "vertex_joints[" + std::to_string(i) + "] outside [0, V)";
        used[picks[i]] = 1;
    }
    for (int r = 0; r < Jr; ++r)
        for (int v = 0; v < d.V; ++v) {
            const float w = reg[(size_t)r * d.V + v];
            if (!std::isfinite(w)) return "regressor[" + std::to_string(r) + "][" + std::to_string(v) + "] is not finite";
            if (w != 0.f) used[v] = 1;
        }
    c = LbsCompact();
    c.Np = Np;
    c.Jr = Jr;
    std::vector<int32_t> at((size_t)d.V, -1);      // vertex -> its place in S
    for (int v = 0; v < d.V; ++v)
        if (used[v]) {
            at[v] = (int32_t)c.S.size();
            c.S.push_back(v);
        }
    c.nS = (int)c.S.size();
    const int Sp = c.Sp = c.nS ? (c.nS + 31) / 32 * 32 : 32;
    const size_t n_vt = (size_t)3 * c.nS, n_sd = (size_t)3 * c.nS * d.nb, n_vtp = (size_t)3 * Sp, n_sdp = (size_t)d.nbp * 3 * Sp,
                 n_pd = d.pose ? (size_t)d.Kp * 3 * Sp : 0, n_wt = (size_t)d.Jp * Sp, n_wj = (size_t)(Sp / 32) * 16 * 64;
    c.o_vt = 0;
    c.o_sd = c.o_vt + n_vt;
    c.o_vtp = c.o_sd + n_sd;
    c.o_sdp = c.o_vtp + n_vtp;
    c.o_pd = c.o_sdp + n_sdp;
    c.o_wt = c.o_pd + n_pd;
    c.o_wj = c.o_wt + n_wt;
    c.blob.assign(c.o_wj + n_wj, 0.f);
    float *vt = c.blob.data() + c.o_vt, *sd = c.blob.data() + c.o_sd, *vtp = c.blob.data() + c.o_vtp, *sdp = c.blob.data() + c.o_sdp,
          *pd = c.blob.data() + c.o_pd, *wt = c.blob.data() + c.o_wt, *wj = c.blob.data() + c.o_wj;
    for (int s = 0; s < c.nS; ++s) {
        const size_t v = (size_t)c.S[s];
        for (int cc = 0; cc < 3; ++cc) {
            vt[3 * s + cc] = vtp[(size_t)cc * Sp + s] = v_template[3 * v + cc];
            for (int k = 0; k < d.nb; ++k)
                sd[((size_t)3 * s + cc) * d.nb + k] = sdp[((size_t)k * 3 + cc) * Sp + s] = shapedirs[(3 * v + cc) * d.nb + k];
            if (d.pose)
                for (int k = 0; k < d.K; ++k) pd[((size_t)k * 3 + cc) * Sp + s] = posedirs[(size_t)k * 3 * d.V + 3 * v + cc];
        }
        for (int j = 0; j < d.J; ++j) wt[(size_t)j * Sp + s] = lbs_weights[v * d.J + j];
    }
    auto weight = [&](int row, int s) -> float {    // W[row][S[s]]
        if (row >= Np + Jr || s >= c.nS) return 0.f;
        if (row < Np) return at[picks[row]] == s ? 1.f : 0.f;
        return reg[(size_t)(row - Np) * d.V + c.S[s]];
    };
    for (int t = 0; t < Sp / 32; ++t)
        for (int q = 0; q < 16; ++q)
            for (int l = 0; l < 64; ++l) wj[((size_t)t * 16 + q) * 64 + l] = weight(l & 31, 32 * t + 8 * (q >> 2) + 4 * (l >> 5) + (q & 3));
    return "";
}

}  // namespace rgn
