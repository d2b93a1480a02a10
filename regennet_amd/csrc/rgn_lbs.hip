// Linear blend skinning: the body layer's VERTICES behind Rotation2xyz / Rotation2xyz_x with jointstype='vertices' (model/rotation2xyz.py:236-249 /
// :303-321; the arithmetic is smplx.lbs.lbs as the two wrappers call it), straight from the sampler's [B, rows, feats, T] layout to
// [B, V, 3 P, T] vertex positions (rgn_rot2verts), over mesh data that lives on the device behind a handle of its own (rgn_body_*).
//
//   v_shaped = v_template + shapedirs . betas                      k_lbs_shape, once per call into the workspace
//   R_j (identity joints := I), pf = (R_j - I)_{j >= 1},           k_lbs_chain: the two phases of k_fk (rgn_fk.h, shared, not copied) per tile of 32
//   A_j = [Rg_j | tg_j - Rg_j . j_j] down the parent table           frames -> workspace  A [tile][J][12][32], pf [tile][K][32], hdr [tile][4][32]
//   v_posed = v_shaped + posedirs^T . pf                           k_lbs_skin: one wave per (32 frames x 32 vertices), on the fp32-input MFMA
//   T_v = sum_j w[v, j] A_j ; vertex = T_v[:, :3] . v_posed + T_v[:, 3], masked, + translation
//
// k_lbs_skin. v_mfma_f32_32x32x2_f32 puts its N index on the lane and its M index in the 16 result registers, so FRAMES are N and VERTICES are M: every
// store of a half-wave is a run of 32 consecutive t of one (vertex, channel), and the pose-blend result (three tiles: x, y, z of 32 vertices) sits in
// the registers in exactly the arrangement the skinning tiles T[r][c] come out in, so applying T is per-register arithmetic with no lane movement.
// The products are exact fp32 and each sum runs in k order from its start value (v_shaped for the pose blend, 0 for the blend of transforms): a vertex's
// result depends on its own columns of posedirs / lbs_weights and on its frame alone, never on the tile it shares or the batch around it.
//   A operand (M x K)  posedirs re-laid out at rgn_body_create as [K][3][Vp] / lbs_weights as [Jp][Vp]: lane l reads [k = 2 s + (l >> 5)][v0 + (l & 31)],
//                      two runs of 128 B, straight from global memory (L2: the workgroups of a launch wave walk the same vertex range)
//   B operand (K x N)  pf: the tile's [K][32] image, copied once per workgroup into LDS (conflict-free: consecutive lanes, consecutive floats);
//                      A_j: [j][component][32 frames] from the workspace, 128-B runs
// A workgroup is 4 waves on one frame tile; wave w takes every 4th vertex tile of the workgroup's range. Masking is by FRAME TILE: a tile whose 32
// frames are all masked costs no arithmetic in either kernel and is filled with 0 (+ translation); a tile with some live frames computes all 32
// lanes (a lane is a frame, an MFMA column) and selects 0 for the masked ones afterwards. No atomics, no cross-workgroup traffic, 64-bit indices.
//
// rgn_rot2verts_shaped: a body shape per frame, read on the device. k_lbs_shape is not launched and no shaped template exists; k_lbs_chain<true> takes
// each lane's rest joints from its betas and writes them as further rows AHEAD of pf, k_lbs_skin<true> walks the shape planes and the posedirs planes
// as one operand from v_template:   v_posed = v_template + [shapedirs; posedirs]^T . [betas; pf].   The <false> forms are the kernels described above.
//
// rgn_rot2joints / rgn_rot2joints_shaped: the joint types the reference's SMPL layer regresses from the mesh (model/smpl.py:76-98, under
// model/rotation2xyz.py:17-155) - index maps into [chain joints | vertices[:, vertex_joints] | J_regressor_extra . vertices]. The body is cut to the
// vertices those touch at rgn_body_set_joint_regressors (rgn_lbs_compact.h), k_lbs_chain also leaves its joint translations, and k_lbs_joints runs
// k_lbs_skin's wave body (lbs_wave_tile: one definition, two callers) over the cut body and weighs each skinned tile into joints in registers.
#include "rgn_fk.h"
#include "rgn_lbs_compact.h"

#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

using namespace rgn;

namespace {

constexpr int LBS_MAX_V = 65536, LBS_MAX_BETAS = 16;
constexpr int LBS_KGROUP = 8;                       // posedirs rows per prefetch group (4 MFMA k-steps): K is padded to a multiple with zero rows
constexpr int LBS_WAVES = 4, LBS_THREADS = 64 * LBS_WAVES;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct LbsBetas {
    float b[LBS_MAX_BETAS];
    int32_t n;
};
struct LbsRest {
    float j[FK_MAX_JOINTS][3];                       // rest joints (absolute), for A_j's translation column
};
struct LbsWork {                                    // the workspace, carved up: offsets in floats, and its size
    uint64_t vsh, hdr, A, pf, jw, bytes;            // (jw: the chain's joint translations, rgn_rot2joints alone)
};
constexpr int LBS_MAX_MAP = 64;
struct LbsMap {                                     // a joint type: output row m is all_joints[idx[m]], all_joints = [J chain joints | Np picked | Jr regressed]
    int32_t n, root;
    uint8_t idx[LBS_MAX_MAP];
};

inline int round_up(int a, int m) { return (a + m - 1) / m * m; }

// ---- v_shaped [3][Vp] (pad 0) ---------------------------------------------------------------------------------------------------------------
__global__ void k_lbs_shape(const float* __restrict__ vt, const float* __restrict__ sd, float* __restrict__ vsh, int V, int Vp, int nb, const LbsBetas be) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 3 * Vp) return;
    const int c = idx / Vp, v = idx - c * Vp;
    float s = 0.f;
    if (v < V) {
        s = vt[3 * v + c];
        for (int k = 0; k < be.n; ++k) s = fmaf(be.b[k], sd[((size_t)3 * v + c) * nb + k], s);
    }
    vsh[idx] = s;
}

// ---- stage 1: rows -> A, pf, hdr per frame tile ---------------------------------------------------------------------------------------------
// SHAPED (rgn_rot2verts_shaped): the frame's betas sit in registers; the chain's offsets and A_j's rest joint come from them (rgn_fk.h), and they are
// written as the first nbp rows of the tile's feature image, ahead of the pose feature, for the shape blend that rides k_lbs_skin's k-loop.
// k_lbs_chain<false> looks at neither `sh` nor `nbp`. jw (rgn_rot2joints; else null): the chain's joint translations too, [tile][J][3][32].
template <bool SHAPED>
__global__ __launch_bounds__(FK_THREADS) void k_lbs_chain(const float* __restrict__ x, const uint8_t* __restrict__ mask, float* __restrict__ rotmat,
                                                          float* __restrict__ hdr, float* __restrict__ Aw, float* __restrict__ pfw, int B, int T, int P, int J,
                                                          int C, int rep, int flags, unsigned long long identity, const FkSkel sk, const LbsRest rest,
                                                          const FkShape sh, int nbp, float* __restrict__ jw) {
    extern __shared__ __attribute__((aligned(16))) float g[];       // [J][13][32]
    const int fl = threadIdx.x & (FK_FRAMES - 1), w = threadIdx.x / FK_FRAMES;
    const long long tile = blockIdx.x;
    const FkFrame fr = fk_frame(x, mask, tile, fl, B, T, P, J, C, flags);
    const bool keep = fr.live && fr.keep;
    if (w == 0) {
        float* hd = hdr + tile * 4 * FK_FRAMES + fl;
#pragma unroll
        for (int c = 0; c < 3; ++c) hd[c * FK_FRAMES] = fr.tr[c];
        hd[3 * FK_FRAMES] = keep ? 1.f : 0.f;
    }
    const bool any = __syncthreads_or(keep);        // a fully masked tile costs no arithmetic (the matrices rotmat asks for excepted)
    if (!any && !rotmat) return;
    const int K = 9 * (J - 1), k0 = SHAPED ? nbp : 0, KT = k0 + K;      // the tile's feature image: [k0 beta rows | K pose rows][32]
    [[maybe_unused]] float be[FK_MAX_BETAS];
    if constexpr (SHAPED) {
        fk_load_betas(sh, fr, be);
        if (w == 0 && any) {
            float* pb = pfw + tile * KT * FK_FRAMES + fl;
#pragma unroll
            for (int k = 0; k < FK_MAX_BETAS; ++k)
                if (k < nbp) pb[k * FK_FRAMES] = be[k];
        }
    }
    fk_local_matrices(g, fr, T, J, rep, flags & RGN_R2X_GLOB, sk, fl, w, [&](int i, float (&m)[9]) {
        if (rotmat && fr.live) {                    // the matrices as rgn_rot2xyz returns them: before identity joints are replaced
            float* rm = rotmat + (fr.f * J + i) * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) rm[k] = m[k];
        }
        if (identity >> i & 1) {
#pragma unroll
            for (int k = 0; k < 9; ++k) m[k] = (k & 3) == 0 ? 1.f : 0.f;
        }
        if (i > 0 && any) {                         // pose feature (R_i - I), row-major
            float* pf = pfw + (tile * KT + k0 + 9 * (i - 1)) * FK_FRAMES + fl;
#pragma unroll
            for (int k = 0; k < 9; ++k) pf[k * FK_FRAMES] = (k & 3) == 0 ? m[k] - 1.f : m[k];
        }
    });
    if (!any) return;
    __syncthreads();
    auto emit = [&](int i, const float (&pos)[3], const float* gi) {
        float* a = Aw + (tile * J + i) * 12 * FK_FRAMES + fl;
        float ji[3] = {rest.j[i][0], rest.j[i][1], rest.j[i][2]};
        if constexpr (SHAPED) fk_shape_add(sh, i, -1, be, ji);          // the frame's own rest joint
        const float j0 = ji[0], j1 = ji[1], j2 = ji[2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {               // A_i = [Rg | tg - Rg . j_i]
            const float r0 = gi[(3 * r) * FK_FRAMES], r1 = gi[(3 * r + 1) * FK_FRAMES], r2 = gi[(3 * r + 2) * FK_FRAMES];
            a[(4 * r) * FK_FRAMES] = r0;
            a[(4 * r + 1) * FK_FRAMES] = r1;
            a[(4 * r + 2) * FK_FRAMES] = r2;
            a[(4 * r + 3) * FK_FRAMES] = pos[r] - (r0 * j0 + r1 * j1 + r2 * j2);
        }
        if (jw) {
#pragma unroll
            for (int r = 0; r < 3; ++r) jw[((tile * J + i) * 3 + r) * FK_FRAMES + fl] = pos[r];
        }
    };
    if constexpr (SHAPED) fk_chain_rel(g, sk, fl, w, FkShapedRel{sk, sh, be}, emit);
    else fk_chain(g, sk, fl, w, emit);
}

// ---- stage 2: pose blend + skinning, one wave per (32 frames x 32 vertices) ------------------------------------------------------------------
__device__ __forceinline__ void lbs_load_pd(float (&a)[4][3], const float* __restrict__ p, size_t Vp) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < 3; ++c) a[u][c] = p[(size_t)(6 * u + c) * Vp];
}

// The wave body k_lbs_skin and k_lbs_joints share: 32 frames (lanes) x the 32 vertices from v0 - pose (and shape) blend from the tile's feature image
// in LDS, then per output channel r the blend of transforms and its application. sink(r, q, v, o) sees channel r of vertex v = v0 + 8 (q / 4) + 4 h
// + (q % 4) for this lane's frame, unmasked and untranslated: register q of the accumulator arrangement. vsh: the start planes [3][Vp]; At: the frame
// tile's transforms [J][12][32]; pd / Wt: the planes rgn_body_create (or the compaction, with Vp := Sp) laid down.
template <class Sink>
__device__ __forceinline__ void lbs_wave_tile(const float* __restrict__ vsh, const float* __restrict__ At, const float* spf, const float* __restrict__ pd,
                                              const float* __restrict__ Wt, int Vp, int v0, int J, int Jp, int Kp, int pose, int lane, Sink&& sink) {
    const int fl = lane & 31, h = lane >> 5;
    f32x16 vp[3];                               // v_posed: [c] register q = vertex v0 + 8 (q / 4) + 4 h + (q % 4), this lane's frame
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int q = 0; q < 16; ++q) vp[c][q] = vsh[(size_t)c * Vp + v0 + 8 * (q >> 2) + 4 * h + (q & 3)];
    if (pose) {
        const float* pl = pd + (size_t)(3 * h) * Vp + v0 + fl;      // + (6 s + c) Vp: row 2 s + h, component c
        float an[4][3];
        lbs_load_pd(an, pl, Vp);
        for (int g = 0; g < Kp / LBS_KGROUP; ++g) {
            float ac[4][3];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int c = 0; c < 3; ++c) ac[u][c] = an[u][c];
            if ((g + 1) * LBS_KGROUP < Kp) lbs_load_pd(an, pl + (size_t)(g + 1) * 24 * Vp, Vp);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float bv = spf[(g * 4 + u) * 64 + lane];
#pragma unroll
                for (int c = 0; c < 3; ++c) vp[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[u][c], bv, vp[c], 0, 0, 0);
            }
        }
    }
    const float* wl = Wt + (size_t)h * Vp + v0 + fl;                // + 2 s Vp
    const float* al = At + h * 12 * FK_FRAMES + fl;                 // + 2 s * 12 * 32 + component * 32
#pragma unroll 1
    for (int r = 0; r < 3; ++r) {
        f32x16 tm[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int q = 0; q < 16; ++q) tm[c][q] = 0.f;
        for (int s = 0; s < Jp / 2; ++s) {
            const float wv = wl[(size_t)2 * s * Vp];
            const bool in = 2 * s + h < J;      // (the pad joint of an odd J: weight 0, and no read past the tile's transforms)
            float bv[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) bv[c] = in ? al[(2 * s * 12 + 4 * r + c) * FK_FRAMES] : 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) tm[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, bv[c], tm[c], 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int v = v0 + 8 * (q >> 2) + 4 * h + (q & 3);
            float o = tm[0][q] * vp[0][q];
            o = fmaf(tm[1][q], vp[1][q], o);
            o = fmaf(tm[2][q], vp[2][q], o);
            o += tm[3][q];
            sink(r, q, v, o);
        }
    }
}

// SHAPED (rgn_rot2verts_shaped): the shape blend rides the same k-loop. The body keeps its shape directions as nbp further planes directly AHEAD of the
// posedirs planes, the shaped chain kernel writes the frame's betas as nbp rows ahead of the pose feature, so `pd` / `Kp` / `krows` name the longer
// operands and `vsh` the template's planes: v_posed = v_template + [shapedirs; posedirs]^T . [betas; pf], summed in that order like v_shaped was.
// k_lbs_skin<false> does not look at `krows`.
template <bool SHAPED>
__global__ __launch_bounds__(LBS_THREADS, 2) void k_lbs_skin(const float* __restrict__ vsh, const float* __restrict__ hdr, const float* __restrict__ Aw,
                                                             const float* __restrict__ pfw, const float* __restrict__ pd, const float* __restrict__ Wt,
                                                             float* __restrict__ out, int B, int T, int P, int V, int Vp, int J, int Jp, int Kp, int pose,
                                                             int tiles_per_wg, int addtr, int krows) {
    extern __shared__ __attribute__((aligned(16))) float spf[];     // [Kp][32]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fl = lane & 31, h = lane >> 5;
    const long long tile = blockIdx.x, NF = (long long)B * P * T, f = tile * FK_FRAMES + fl;
    const bool live = f < NF;
    const long long fc = live ? f : NF - 1;
    const int t = (int)(fc % T), p = (int)((fc / T) % P);
    const long long b = fc / ((long long)T * P);
    const float* hd = hdr + tile * 4 * FK_FRAMES + fl;
    const float tr[3] = {hd[0], hd[FK_FRAMES], hd[2 * FK_FRAMES]};
    const bool keep = hd[3 * FK_FRAMES] != 0.f;
    const bool any = __syncthreads_or(keep);
    float* __restrict__ ob = out + ((b * V * 3 * P + 3 * p) * (long long)T + t);                // + vertex * 3 P T + channel * T
    const long long vstride = (long long)3 * P * T;
    const int K = SHAPED ? krows : 9 * (J - 1);     // rows of the tile's feature image in the workspace
    if (any && pose) {
        const float* src = pfw + tile * K * FK_FRAMES;
        for (int i = threadIdx.x; i < Kp * FK_FRAMES; i += LBS_THREADS) spf[i] = i < K * FK_FRAMES ? src[i] : 0.f;
        __syncthreads();
    }
    for (int it = wave; it < tiles_per_wg; it += LBS_WAVES) {
        const int v0 = (blockIdx.y * tiles_per_wg + it) * 32;
        if (v0 >= V) break;
        if (!any) {                                 // every frame of the tile is masked: 0, then the translation
            if (live)
                for (int i = h; i < 32 && v0 + i < V; i += 2)
#pragma unroll
                    for (int c = 0; c < 3; ++c) __builtin_nontemporal_store(addtr ? 0.f + tr[c] : 0.f, ob + (v0 + i) * vstride + c * (long long)T);
            continue;
        }
        lbs_wave_tile(vsh, Aw + tile * J * 12 * FK_FRAMES, spf, pd, Wt, Vp, v0, J, Jp, Kp, pose, lane, [&](int r, int, int v, float o) {
            o = keep ? o : 0.f;
            if (addtr) o += tr[r];
            if (live && v < V) __builtin_nontemporal_store(o, ob + v * vstride + r * (long long)T);
        });
    }
}

// ---- the regressed joint types: skin the vertices of S in registers, weigh them into joints, never write them -------------------------------------
// One workgroup per frame tile; wave w walks every 4th vertex tile of the compacted body (vsh / pd / Wt: its planes, Sp vertices) through the wave body
// above. A skinned tile leaves that body in the accumulator arrangement, which IS a B operand (K x N: register q of half-wave h gives k = h of k-step
// q, frames on N) of the same MFMA shape, so   joints[row, t] += W[row, v] . vertex[v, t]   is 16 MFMAs per channel against Wj, the joint weights
// permuted at load time to the vertex order of the registers (rgn_lbs_compact.h). Exact products; a picked row's only non-zero is a 1, so it is that
// vertex. Each wave sums its tiles in order, the four partial sums meet in LDS (over the feature image, which is done with) and are added in wave
// order, and the epilogue gathers all_joints[map[m]] - chain joints from the chain's translations jw, the rest from the sums -, zeroes masked frames,
// subtracts row `root` and adds the translation as k_fk does. The order of every sum depends on the body alone.
template <bool SHAPED>
__global__ __launch_bounds__(LBS_THREADS) void k_lbs_joints(const float* __restrict__ vsh, const float* __restrict__ hdr, const float* __restrict__ Aw,
                                                            const float* __restrict__ pfw, const float* __restrict__ jw, const float* __restrict__ pd,
                                                            const float* __restrict__ Wt, const float* __restrict__ Wj, float* __restrict__ out, int B, int T,
                                                            int P, int Sp, int J, int Jp, int Kp, int pose, int addtr, int krows, const LbsMap map) {
    extern __shared__ __attribute__((aligned(16))) float spf[];     // [Kp][32], then the partial sums [4 waves][3][32 rows][32 frames]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fl = lane & 31, h = lane >> 5;
    const long long tile = blockIdx.x, NF = (long long)B * P * T, f = tile * FK_FRAMES + fl;
    const bool live = f < NF;
    const long long fc = live ? f : NF - 1;
    const int t = (int)(fc % T), p = (int)((fc / T) % P);
    const long long b = fc / ((long long)T * P);
    const float* hd = hdr + tile * 4 * FK_FRAMES + fl;
    const float tr[3] = {hd[0], hd[FK_FRAMES], hd[2 * FK_FRAMES]};
    const bool keep = hd[3 * FK_FRAMES] != 0.f;
    const bool any = __syncthreads_or(keep);
    float* __restrict__ ob = out + ((b * map.n * 3 * P + 3 * p) * (long long)T + t);            // + row * 3 P T + channel * T
    const long long mstride = (long long)3 * P * T;
    const int rows = 3 * map.n;                     // (row, channel) pairs: a thread keeps its frame (256 = 8 x 32) and walks every 8th
    if (!any) {                                     // every frame of the tile is masked: 0, then the translation
        if (live)
            for (int e = threadIdx.x >> 5; e < rows; e += LBS_THREADS / 32) {
                const int m = e / 3, c = e - 3 * m;
                ob[m * mstride + c * (long long)T] = addtr ? 0.f + (c == 0 ? tr[0] : c == 1 ? tr[1] : tr[2]) : 0.f;
            }
        return;
    }
    const int K = SHAPED ? krows : 9 * (J - 1);
    if (pose) {
        const float* src = pfw + tile * K * FK_FRAMES;
        for (int i = threadIdx.x; i < Kp * FK_FRAMES; i += LBS_THREADS) spf[i] = i < K * FK_FRAMES ? src[i] : 0.f;
        __syncthreads();
    }
    f32x16 acc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[c][q] = 0.f;
    for (int it = wave; it < Sp / 32; it += LBS_WAVES) {
        float wa[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) wa[q] = Wj[((size_t)it * 16 + q) * 64 + lane];
        lbs_wave_tile(vsh, Aw + tile * J * 12 * FK_FRAMES, spf, pd, Wt, Sp, it * 32, J, Jp, Kp, pose, lane, [&](int r, int q, int, float o) {
            if (r == 0) acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[q], o, acc[0], 0, 0, 0);
            else if (r == 1) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[q], o, acc[1], 0, 0, 0);
            else acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[q], o, acc[2], 0, 0, 0);
        });
    }
    __syncthreads();                                // every wave is done with the feature image
    constexpr int WSTRIDE = 3 * 32 * FK_FRAMES;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int q = 0; q < 16; ++q) spf[wave * WSTRIDE + (c * 32 + 8 * (q >> 2) + 4 * h + (q & 3)) * FK_FRAMES + fl] = acc[c][q];
    __syncthreads();
    auto joint = [&](int a, int c) -> float {       // all_joints[a], channel c, this thread's frame
        if (a < J) return jw[((tile * J + a) * 3 + c) * FK_FRAMES + fl];
        const float* pp = spf + (c * 32 + (a - J)) * FK_FRAMES + fl;
        return ((pp[0] + pp[WSTRIDE]) + pp[2 * WSTRIDE]) + pp[3 * WSTRIDE];
    };
    float rt[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) rt[c] = joint(map.idx[map.root], c);
    if (live)
        for (int e = threadIdx.x >> 5; e < rows; e += LBS_THREADS / 32) {
            const int m = e / 3, c = e - 3 * m;
            float v = keep ? joint(map.idx[m], c) - (c == 0 ? rt[0] : c == 1 ? rt[1] : rt[2]) : 0.f;       // masked: 0, then the root row (0 - 0)
            if (addtr) v += c == 0 ? tr[0] : c == 1 ? tr[1] : tr[2];
            ob[m * mstride + c * (long long)T] = v;
        }
}

}  // namespace

// ---- the handle ------------------------------------------------------------------------------------------------------------------------------
struct rgn_body_ctx {
    int device = 0, V = 0, Vp = 0, J = 0, Jp = 0, nb = 0, nbp = 0, K = 0, Kp = 0;
    bool pose = false;
    unsigned long long identity = 0;
    // v_template [V,3] | shapedirs [V,3,nb] | v_template as planes [3][Vp] | shapedirs as planes [nbp][3][Vp] | posedirs [Kp][3][Vp] | weights [Jp][Vp]
    // (the shape planes end where the posedirs planes begin: the shaped skinning kernel walks both as one operand of nbp + Kp rows)
    float* blob = nullptr;
    float *vt = nullptr, *sd = nullptr, *vtp = nullptr, *sdp = nullptr, *pd = nullptr, *wt = nullptr;
    // rgn_body_set_joint_regressors: the arrays as rgn_body_create took them (host), and the body cut to S on the device (rgn_lbs_compact.h)
    std::vector<float> h_vt, h_sd, h_pd, h_wt;
    float* jblob = nullptr;
    float *jvt = nullptr, *jsd = nullptr, *jvtp = nullptr, *jsdp = nullptr, *jpd = nullptr, *jwt = nullptr, *jwj = nullptr;
    int Np = 0, Jr = 0, nS = 0, Sp = 0;
    std::string err;
    int fail(int code, const std::string& m) {
        err = m;
        return code;
    }
};

namespace {

thread_local std::string g_body_create_error;

#define LBS_HIP(h, expr)                                                                                \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) return (h)->fail(RGN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// no C++ exception crosses the C boundary (see rgn_guard in rgn_abi.cpp)
template <class F>
int body_guard(rgn_body_ctx* h, const char* fn, F&& body) noexcept {
    try {
        return body();
    } catch (const std::exception& e) {
        try {
            std::string m = std::string(fn) + ": C++ exception at the boundary: " + e.what();
            if (h) h->err.swap(m);
            else g_body_create_error.swap(m);
        } catch (...) {
        }
        return RGN_ERR_INTERNAL;
    } catch (...) {
        return RGN_ERR_INTERNAL;
    }
}

LbsWork carve(const rgn_body_ctx* c, long long NF) {
    const uint64_t ntiles = (uint64_t)((NF + FK_FRAMES - 1) / FK_FRAMES);
    LbsWork w;
    w.vsh = 0;
    w.hdr = w.vsh + (uint64_t)3 * c->Vp;
    w.A = w.hdr + ntiles * 4 * FK_FRAMES;
    w.pf = w.A + ntiles * c->J * 12 * FK_FRAMES;
    w.bytes = (w.pf + ntiles * c->K * FK_FRAMES) * sizeof(float);
    return w;
}

// ... of rgn_rot2verts_shaped: no shaped template, and nbp beta rows ahead of each tile's pose feature
LbsWork carve_shaped(const rgn_body_ctx* c, long long NF) {
    const uint64_t ntiles = (uint64_t)((NF + FK_FRAMES - 1) / FK_FRAMES);
    LbsWork w;
    w.vsh = 0;
    w.hdr = 0;
    w.A = w.hdr + ntiles * 4 * FK_FRAMES;
    w.pf = w.A + ntiles * c->J * 12 * FK_FRAMES;
    w.bytes = (w.pf + ntiles * (c->nbp + c->K) * FK_FRAMES) * sizeof(float);
    return w;
}

// ... of rgn_rot2joints / rgn_rot2joints_shaped: the chain's outputs with its joint translations, and (one shape) the shaped template of the Sp
// vertices of S. Nothing in it grows with V.
LbsWork carve_joints(const rgn_body_ctx* c, long long NF, bool shaped) {
    const uint64_t ntiles = (uint64_t)((NF + FK_FRAMES - 1) / FK_FRAMES);
    LbsWork w;
    w.vsh = 0;
    w.hdr = w.vsh + (shaped ? 0 : (uint64_t)3 * c->Sp);
    w.A = w.hdr + ntiles * 4 * FK_FRAMES;
    w.pf = w.A + ntiles * c->J * 12 * FK_FRAMES;
    w.jw = w.pf + ntiles * ((shaped ? c->nbp : 0) + c->K) * FK_FRAMES;
    w.bytes = (w.jw + ntiles * c->J * 3 * FK_FRAMES) * sizeof(float);
    return w;
}

constexpr int LBS_JOINTS_SUMS = LBS_WAVES * 3 * 32 * FK_FRAMES * (int)sizeof(float);       // k_lbs_joints' partial sums in LDS: 48 KB

struct JointsArgs {                                 // what rgn_rot2joints and rgn_rot2joints_shaped share
    const float* x;
    const uint8_t* mask;
    int32_t B, T;
    const float* rest_joints;
    const int32_t* parents;
    int32_t pose_rep, num_person, flags;
    const float* glob_rot;
    int32_t n_map;
    const int32_t* map;
    int32_t root;
    float *joints, *rotmat;
    void* work;
    uint64_t work_bytes;
    void* stream;
};

// betas: the one shape (host, nullable) of rgn_rot2joints; sh: the per-frame shape arguments of rgn_rot2joints_shaped
template <bool SHAPED>
int rot2joints(rgn_body_ctx* h, const char* fn, const JointsArgs& a, const float* betas, const FkShape& sh) {
    auto bad = [&](const std::string& m) -> int {
        if (h) return h->fail(RGN_ERR_INVALID_ARG, std::string(fn) + ": " + m);
        g_body_create_error = std::string(fn) + ": " + m;
        return RGN_ERR_INVALID_ARG;
    };
    if (!a.x || !a.joints || !a.rest_joints || !a.parents) return bad("null x, joints, rest_joints or parents");
    if constexpr (SHAPED)
        if (const char* why = fk_check_shape(sh.sj, sh.nb, sh.betas, sh.sb, sh.sp, sh.st)) return bad(why);
    if (a.B < 1 || a.T < 1) return bad("B < 1 or T < 1");
    if (a.num_person < 1) return bad("num_person < 1");
    if (a.pose_rep < RGN_POSE_ROT6D || a.pose_rep > RGN_POSE_ROTMAT) return bad("unknown pose_rep");
    if (a.flags & ~(RGN_R2X_TRANSLATION | RGN_R2X_GLOB | RGN_R2X_VERTSTRANS)) return bad("unknown flag");
    if (!(a.flags & RGN_R2X_GLOB) && !a.glob_rot) return bad("glob_rot is required when RGN_R2X_GLOB is not set");
    if (a.n_map < 1 || a.n_map > LBS_MAX_MAP) return bad("n_map outside [1, 64]");
    if (!a.map) return bad("null map");
    if (a.root < 0 || a.root >= a.n_map) return bad("root outside [0, n_map)");
    for (int i = 0; i < a.n_map; ++i)
        if (a.map[i] < 0) return bad("map[" + std::to_string(i) + "] < 0");
    if (!h) return bad("null handle");
    if (!h->jblob) return bad("the body holds no joint regressors (rgn_body_set_joint_regressors)");
    const int J = h->J, nall = J + h->Np + h->Jr;
    LbsMap map{};
    map.n = a.n_map;
    map.root = a.root;
    for (int i = 0; i < a.n_map; ++i) {
        if (a.map[i] >= nall) return bad("map[" + std::to_string(i) + "] = " + std::to_string(a.map[i]) + " outside [0, J + Np + Jr) = [0, " + std::to_string(nall) + ")");
        map.idx[i] = (uint8_t)a.map[i];
    }
    if constexpr (SHAPED) {
        if (sh.nb > h->nb) return bad(std::to_string(sh.nb) + " betas, but the body holds " + std::to_string(h->nb) + " shape directions");
    } else {
        if (betas && h->nb == 0) return bad("betas given, but the body holds no shapedirs");
    }
    FkSkel sk;
    int at = -1;
    if (const char* why = fk_build_skel(J, a.rest_joints, a.parents, sk, at))
        return bad(at < 0 ? std::string(why) : "parents[" + std::to_string(at) + "] outside [0, " + std::to_string(at) + ")");
    if (!(a.flags & RGN_R2X_GLOB)) axis_angle_to_matrix_f32(a.glob_rot, sk.glob);
    const long long NF = (long long)a.B * a.num_person * a.T;
    const LbsWork w = carve_joints(h, NF, SHAPED);
    float* const wf = reinterpret_cast<float*>(a.work);
    if (!a.work || a.work_bytes < w.bytes)
        return bad("workspace of " + std::to_string(a.work_bytes) + " bytes, " + std::to_string(w.bytes) + " needed (" + fn + "_workspace)");
    LbsRest rest;
    std::memcpy(rest.j, a.rest_joints, sizeof(float) * 3 * J);
    LBS_HIP(h, hipSetDevice(h->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(a.stream);
    const int C = a.pose_rep == RGN_POSE_ROT6D ? 6 : a.pose_rep == RGN_POSE_ROTVEC ? 3 : a.pose_rep == RGN_POSE_ROTQUAT ? 4 : 9;
    const unsigned ntiles = (unsigned)((NF + FK_FRAMES - 1) / FK_FRAMES);
    if constexpr (!SHAPED) {
        LbsBetas be{};
        if (betas) {
            be.n = h->nb;
            std::memcpy(be.b, betas, sizeof(float) * h->nb);
        }
        hipLaunchKernelGGL(k_lbs_shape, dim3((3 * h->Sp + 255) / 256), dim3(256), 0, s, h->jvt, h->jsd, wf + w.vsh, h->nS, h->Sp, h->nb, be);
        LBS_HIP(h, hipGetLastError());
    }
    hipLaunchKernelGGL(k_lbs_chain<SHAPED>, dim3(ntiles), dim3(FK_THREADS), (size_t)J * FK_JSTRIDE * sizeof(float), s, a.x, a.mask, a.rotmat, wf + w.hdr, wf + w.A,
                       wf + w.pf, a.B, a.T, a.num_person, J, C, a.pose_rep, a.flags, h->identity, sk, rest, sh, SHAPED ? h->nbp : 0, wf + w.jw);
    LBS_HIP(h, hipGetLastError());
    const bool addtr = (a.flags & RGN_R2X_TRANSLATION) && (a.flags & RGN_R2X_VERTSTRANS);
    const int pose = SHAPED ? 1 : (h->pose ? 1 : 0);
    const int Kp = SHAPED ? h->nbp + (h->pose ? h->Kp : 0) : h->Kp;
    const size_t image = pose ? (size_t)Kp * FK_FRAMES * sizeof(float) : 0;
    hipLaunchKernelGGL(k_lbs_joints<SHAPED>, dim3(ntiles), dim3(LBS_THREADS), image > (size_t)LBS_JOINTS_SUMS ? image : (size_t)LBS_JOINTS_SUMS, s,
                       SHAPED ? h->jvtp : wf + w.vsh, wf + w.hdr, wf + w.A, wf + w.pf, wf + w.jw, SHAPED ? h->jsdp : h->jpd, h->jwt, h->jwj, a.joints, a.B, a.T,
                       a.num_person, h->Sp, J, h->Jp, Kp, pose, addtr ? 1 : 0, SHAPED ? h->nbp + h->K : 0, map);
    LBS_HIP(h, hipGetLastError());
    return RGN_OK;
}

int joints_workspace(rgn_body_ctx* b, const char* fn, int32_t B, int32_t T, int32_t num_person, uint64_t* nbytes, bool shaped) {
    if (!b) return RGN_ERR_INVALID_ARG;
    if (!nbytes) return b->fail(RGN_ERR_INVALID_ARG, std::string(fn) + ": null nbytes");
    if (B < 1 || T < 1 || num_person < 1) return b->fail(RGN_ERR_INVALID_ARG, std::string(fn) + ": B, T or num_person < 1");
    if (!b->jblob) return b->fail(RGN_ERR_INVALID_ARG, std::string(fn) + ": the body holds no joint regressors (rgn_body_set_joint_regressors)");
    *nbytes = carve_joints(b, (long long)B * num_person * T, shaped).bytes;
    return RGN_OK;
}

}  // namespace

extern "C" {

const char* rgn_body_last_error(rgn_body_handle b) { return b ? b->err.c_str() : g_body_create_error.c_str(); }

int rgn_body_create(int32_t device, int32_t V, int32_t J, int32_t nb, const float* v_template, const float* posedirs, const float* lbs_weights,
                    const float* shapedirs, const int32_t* identity_joints, int32_t n_identity, rgn_body_handle* out) {
    return body_guard(nullptr, "rgn_body_create", [&]() -> int {
        auto bad = [&](int code, const std::string& m) {
            g_body_create_error = "rgn_body_create: " + m;
            return code;
        };
        if (!out) return bad(RGN_ERR_INVALID_ARG, "null out");
        *out = nullptr;
        if (V < 1 || V > LBS_MAX_V) return bad(RGN_ERR_INVALID_ARG, "V outside [1, 65536]");
        if (J < 1 || J > FK_MAX_JOINTS) return bad(RGN_ERR_INVALID_ARG, "J outside [1, 64]");
        if (nb < 0 || nb > LBS_MAX_BETAS) return bad(RGN_ERR_INVALID_ARG, "nb outside [0, 16]");
        if (!v_template || !lbs_weights) return bad(RGN_ERR_INVALID_ARG, "null v_template or lbs_weights");
        if (nb > 0 && !shapedirs) return bad(RGN_ERR_INVALID_ARG, "nb > 0 without shapedirs");
        if (n_identity < 0 || n_identity > J || (n_identity > 0 && !identity_joints)) return bad(RGN_ERR_INVALID_ARG, "n_identity outside [0, J] or null identity_joints");
        unsigned long long identity = 0;
        for (int i = 0; i < n_identity; ++i) {
            if (identity_joints[i] < 1 || identity_joints[i] >= J)
                return bad(RGN_ERR_INVALID_ARG, "identity_joints[" + std::to_string(i) + "] outside [1, J)");
            identity |= 1ull << identity_joints[i];
        }
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return bad(RGN_ERR_HIP, "no HIP device visible");
        if (device < 0 || device >= ndev) return bad(RGN_ERR_INVALID_ARG, "device ordinal out of range");
        if (hipSetDevice(device) != hipSuccess) return bad(RGN_ERR_HIP, "hipSetDevice failed");

        std::unique_ptr<rgn_body_ctx> c(new rgn_body_ctx());
        c->device = device;
        c->V = V;
        c->Vp = round_up(V, 32);
        c->J = J;
        c->Jp = round_up(J, 2);
        c->nb = nb;
        c->nbp = round_up(nb, LBS_KGROUP);
        c->K = 9 * (J - 1);
        c->Kp = round_up(c->K, LBS_KGROUP);
        c->pose = posedirs != nullptr && J > 1;     // (no posedirs: no pose blend shapes)
        c->identity = identity;
        const size_t n_vt = (size_t)3 * V, n_sd = (size_t)3 * V * nb, n_pd = c->pose ? (size_t)c->Kp * 3 * c->Vp : 0, n_wt = (size_t)c->Jp * c->Vp;
        const size_t n_vtp = nb ? (size_t)3 * c->Vp : 0, n_sdp = (size_t)c->nbp * 3 * c->Vp;
        std::vector<float> host(n_vt + n_sd + n_vtp + n_sdp + n_pd + n_wt, 0.f);
        float *hvt = host.data(), *hsd = hvt + n_vt, *hvtp = hsd + n_sd, *hsdp = hvtp + n_vtp, *hpd = hsdp + n_sdp, *hwt = hpd + n_pd;
        std::memcpy(hvt, v_template, n_vt * sizeof(float));
        if (n_sd) std::memcpy(hsd, shapedirs, n_sd * sizeof(float));
        if (nb)                                     // the same component planes for the template and the shape directions (pad rows and vertices 0)
            for (int v = 0; v < V; ++v)
                for (int cc = 0; cc < 3; ++cc) {
                    hvtp[(size_t)cc * c->Vp + v] = v_template[3 * v + cc];
                    for (int k = 0; k < nb; ++k) hsdp[((size_t)k * 3 + cc) * c->Vp + v] = shapedirs[((size_t)3 * v + cc) * nb + k];
                }
        if (c->pose)                                // [K][3 V] -> [Kp][3][Vp]: component planes, so that a lane's 32 vertices are consecutive floats
            for (int k = 0; k < c->K; ++k)
                for (int v = 0; v < V; ++v)
                    for (int cc = 0; cc < 3; ++cc) hpd[((size_t)k * 3 + cc) * c->Vp + v] = posedirs[(size_t)k * 3 * V + 3 * v + cc];
        for (int v = 0; v < V; ++v)                 // [V][J] -> [Jp][Vp]
            for (int j = 0; j < J; ++j) hwt[(size_t)j * c->Vp + v] = lbs_weights[(size_t)v * J + j];
        c->h_vt.assign(v_template, v_template + n_vt);                  // kept for rgn_body_set_joint_regressors, which cuts them to its vertices
        if (n_sd) c->h_sd.assign(shapedirs, shapedirs + n_sd);
        if (c->pose) c->h_pd.assign(posedirs, posedirs + (size_t)c->K * 3 * V);
        c->h_wt.assign(lbs_weights, lbs_weights + (size_t)V * J);
        void* dev = nullptr;
        if (hipMalloc(&dev, host.size() * sizeof(float)) != hipSuccess) return bad(RGN_ERR_HIP, "hipMalloc of the mesh data failed");
        c->blob = reinterpret_cast<float*>(dev);
        if (hipMemcpy(dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(dev);
            return bad(RGN_ERR_HIP, "hipMemcpy of the mesh data failed");
        }
        c->vt = c->blob;
        c->sd = c->vt + n_vt;
        c->vtp = c->sd + n_sd;
        c->sdp = c->vtp + n_vtp;
        c->pd = c->sdp + n_sdp;
        c->wt = c->pd + n_pd;
        // (set here, not in the call: rgn_rot2verts may be running under a stream capture.) Dynamic LDS on top of the few static bytes of the
        // block-wide vote: k_lbs_chain J x 13 x 32 floats <= 104 KB; k_lbs_skin Kp x 32 floats <= 71 KB, which keeps two workgroups on a CU
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_lbs_chain<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           FK_MAX_JOINTS * FK_JSTRIDE * (int)sizeof(float));
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_lbs_skin<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    round_up(9 * (FK_MAX_JOINTS - 1), LBS_KGROUP) * FK_FRAMES * (int)sizeof(float));
        // ... and their shaped forms: the same chain image; the feature image longer by at most 16 beta rows (<= 73 KB: still two workgroups on a CU)
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_lbs_chain<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    FK_MAX_JOINTS * FK_JSTRIDE * (int)sizeof(float));
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_lbs_skin<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (LBS_MAX_BETAS + round_up(9 * (FK_MAX_JOINTS - 1), LBS_KGROUP)) * FK_FRAMES * (int)sizeof(float));
        if (e != hipSuccess) {
            (void)hipFree(dev);
            return bad(RGN_ERR_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e));
        }
        *out = c.release();
        return RGN_OK;
    });
}

int rgn_body_destroy(rgn_body_handle b) {
    return body_guard(nullptr, "rgn_body_destroy", [&]() -> int {   // (not b: the handle is gone by the time anything could be reported)
        if (!b) return RGN_ERR_INVALID_ARG;
        (void)hipSetDevice(b->device);
        (void)hipDeviceSynchronize();
        if (b->blob) (void)hipFree(b->blob);
        if (b->jblob) (void)hipFree(b->jblob);
        delete b;
        return RGN_OK;
    });
}

int rgn_rot2verts_workspace(rgn_body_handle b, int32_t B, int32_t T, int32_t num_person, uint64_t* nbytes) {
    return body_guard(b, "rgn_rot2verts_workspace", [&]() -> int {
        if (!b) return RGN_ERR_INVALID_ARG;
        if (!nbytes) return b->fail(RGN_ERR_INVALID_ARG, "rgn_rot2verts_workspace: null nbytes");
        if (B < 1 || T < 1 || num_person < 1) return b->fail(RGN_ERR_INVALID_ARG, "rgn_rot2verts_workspace: B, T or num_person < 1");
        *nbytes = carve(b, (long long)B * num_person * T).bytes;
        return RGN_OK;
    });
}

int rgn_rot2verts(rgn_body_handle h, const float* x, const uint8_t* mask, int32_t B, int32_t T, const float* rest_joints, const int32_t* parents,
                  int32_t pose_rep, int32_t num_person, int32_t flags, const float* glob_rot, const float* betas, float* verts, float* rotmat, void* work,
                  uint64_t work_bytes, void* stream) {
    return body_guard(h, "rgn_rot2verts", [&]() -> int {
        if (!h) return RGN_ERR_INVALID_ARG;
        if (!x || !verts || !rest_joints || !parents) return h->fail(RGN_ERR_INVALID_ARG, "rgn_rot2verts: null x, verts, rest_joints or parents");
        if (B < 1 || T < 1) return h->fail(RGN_ERR_INVALID_ARG, "rgn_rot2verts: B < 1 or T < 1");
        if (num_person < 1) return h->fail(RGN_ERR_INVALID_ARG, "rgn_rot2verts: num_person < 1");
        if (pose_rep < RGN_POSE_ROT6D || pose_rep > RGN_POSE_ROTMAT) return h->fail(RGN_ERR_INVALID_ARG, "rgn_rot2verts: unknown pose_rep");
        if (flags & ~(RGN_R2X_TRANSLATION | RGN_R2X_GLOB | RGN_R2X_VERTSTRANS)) return h->fail(RGN_ERR_INVALID_ARG, "rgn_rot2verts: unknown flag");
        if (!(flags & RGN_R2X_GLOB) && !glob_rot) return h->fail(RGN_ERR_INVALID_ARG, "rgn_rot2verts: glob_rot is required when RGN_R2X_GLOB is not set");
        if (betas && h->nb == 0) return h->fail(RGN_ERR_INVALID_ARG, "rgn_rot2verts: betas given, but the body holds no shapedirs");
        const int J = h->J;
        FkSkel sk;
        int at = -1;
        if (const char* why = fk_build_skel(J, rest_joints, parents, sk, at))
            return h->fail(RGN_ERR_INVALID_ARG, at < 0 ? std::string("rgn_rot2verts: ") + why
                                                       : "rgn_rot2verts: parents[" + std::to_string(at) + "] outside [0, " + std::to_string(at) + ")");
        if (!(flags & RGN_R2X_GLOB)) axis_angle_to_matrix_f32(glob_rot, sk.glob);
        const long long NF = (long long)B * num_person * T;
        const LbsWork w = carve(h, NF);
        float* const wf = reinterpret_cast<float*>(work);
        if (!work || work_bytes < w.bytes)
            return h->fail(RGN_ERR_INVALID_ARG, "rgn_rot2verts: workspace of " + std::to_string(work_bytes) + " bytes, " + std::to_string(w.bytes) +
                                                    " needed (rgn_rot2verts_workspace)");
        LbsRest rest;
        std::memcpy(rest.j, rest_joints, sizeof(float) * 3 * J);
        LbsBetas be{};
        if (betas) {
            be.n = h->nb;
            std::memcpy(be.b, betas, sizeof(float) * h->nb);
        }
        LBS_HIP(h, hipSetDevice(h->device));
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        const int C = pose_rep == RGN_POSE_ROT6D ? 6 : pose_rep == RGN_POSE_ROTVEC ? 3 : pose_rep == RGN_POSE_ROTQUAT ? 4 : 9;
        const unsigned ntiles = (unsigned)((NF + FK_FRAMES - 1) / FK_FRAMES);
        hipLaunchKernelGGL(k_lbs_shape, dim3((3 * h->Vp + 255) / 256), dim3(256), 0, s, h->vt, h->sd, wf + w.vsh, h->V, h->Vp, h->nb, be);
        LBS_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(k_lbs_chain<false>, dim3(ntiles), dim3(FK_THREADS), (size_t)J * FK_JSTRIDE * sizeof(float), s, x, mask, rotmat, wf + w.hdr, wf + w.A, wf + w.pf, B, T,
                           num_person, J, C, pose_rep, flags, h->identity, sk, rest, FkShape{}, 0, nullptr);
        LBS_HIP(h, hipGetLastError());
        const int vtiles = h->Vp / 32;
        // vertex tiles per workgroup (one pf image in LDS serves them all): 8 where that still leaves a few workgroups per CU, else one per wave
        const int tpw = (long long)ntiles * ((vtiles + 7) / 8) >= 2048 ? 8 : LBS_WAVES;
        const bool addtr = (flags & RGN_R2X_TRANSLATION) && (flags & RGN_R2X_VERTSTRANS);
        hipLaunchKernelGGL(k_lbs_skin<false>, dim3(ntiles, (vtiles + tpw - 1) / tpw), dim3(LBS_THREADS), h->pose ? (size_t)h->Kp * FK_FRAMES * sizeof(float) : 0, s,
                           wf + w.vsh, wf + w.hdr, wf + w.A, wf + w.pf, h->pd, h->wt, verts, B, T, num_person, h->V, h->Vp, J, h->Jp, h->Kp, h->pose ? 1 : 0, tpw, addtr ? 1 : 0, 0);
        LBS_HIP(h, hipGetLastError());
        return RGN_OK;
    });
}

int rgn_rot2verts_shaped_workspace(rgn_body_handle b, int32_t B, int32_t T, int32_t num_person, uint64_t* nbytes) {
    return body_guard(b, "rgn_rot2verts_shaped_workspace", [&]() -> int {
        if (!b) return RGN_ERR_INVALID_ARG;
        if (!nbytes) return b->fail(RGN_ERR_INVALID_ARG, "rgn_rot2verts_shaped_workspace: null nbytes");
        if (B < 1 || T < 1 || num_person < 1) return b->fail(RGN_ERR_INVALID_ARG, "rgn_rot2verts_shaped_workspace: B, T or num_person < 1");
        *nbytes = carve_shaped(b, (long long)B * num_person * T).bytes;
        return RGN_OK;
    });
}

int rgn_rot2verts_shaped(rgn_body_handle h, const float* x, const uint8_t* mask, int32_t B, int32_t T, const float* rest_joints, const int32_t* parents,
                         const float* shape_joints, int32_t nb, const float* betas, int64_t beta_stride_b, int64_t beta_stride_p, int64_t beta_stride_t,
                         int32_t pose_rep, int32_t num_person, int32_t flags, const float* glob_rot, float* verts, float* rotmat, void* work,
                         uint64_t work_bytes, void* stream) {
    return body_guard(h, "rgn_rot2verts_shaped", [&]() -> int {
        // the arguments first, the handle after them (text: rgn_body_last_error(NULL) while there is no handle)
        auto bad = [&](const std::string& m) -> int {
            if (h) return h->fail(RGN_ERR_INVALID_ARG, "rgn_rot2verts_shaped: " + m);
            g_body_create_error = "rgn_rot2verts_shaped: " + m;
            return RGN_ERR_INVALID_ARG;
        };
        if (!x || !verts || !rest_joints || !parents) return bad("null x, verts, rest_joints or parents");
        if (const char* why = fk_check_shape(shape_joints, nb, betas, beta_stride_b, beta_stride_p, beta_stride_t)) return bad(why);
        if (B < 1 || T < 1) return bad("B < 1 or T < 1");
        if (num_person < 1) return bad("num_person < 1");
        if (pose_rep < RGN_POSE_ROT6D || pose_rep > RGN_POSE_ROTMAT) return bad("unknown pose_rep");
        if (flags & ~(RGN_R2X_TRANSLATION | RGN_R2X_GLOB | RGN_R2X_VERTSTRANS)) return bad("unknown flag");
        if (!(flags & RGN_R2X_GLOB) && !glob_rot) return bad("glob_rot is required when RGN_R2X_GLOB is not set");
        if (!h) return bad("null handle");
        if (nb > h->nb) return bad(std::to_string(nb) + " betas, but the body holds " + std::to_string(h->nb) + " shape directions");
        const int J = h->J;
        FkSkel sk;
        int at = -1;
        if (const char* why = fk_build_skel(J, rest_joints, parents, sk, at))
            return bad(at < 0 ? std::string(why) : "parents[" + std::to_string(at) + "] outside [0, " + std::to_string(at) + ")");
        if (!(flags & RGN_R2X_GLOB)) axis_angle_to_matrix_f32(glob_rot, sk.glob);
        const long long NF = (long long)B * num_person * T;
        const LbsWork w = carve_shaped(h, NF);
        float* const wf = reinterpret_cast<float*>(work);
        if (!work || work_bytes < w.bytes)
            return bad("workspace of " + std::to_string(work_bytes) + " bytes, " + std::to_string(w.bytes) + " needed (rgn_rot2verts_shaped_workspace)");
        LbsRest rest;
        std::memcpy(rest.j, rest_joints, sizeof(float) * 3 * J);
        const FkShape sh{shape_joints, betas, beta_stride_b, beta_stride_p, beta_stride_t, nb};
        LBS_HIP(h, hipSetDevice(h->device));
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        const int C = pose_rep == RGN_POSE_ROT6D ? 6 : pose_rep == RGN_POSE_ROTVEC ? 3 : pose_rep == RGN_POSE_ROTQUAT ? 4 : 9;
        const unsigned ntiles = (unsigned)((NF + FK_FRAMES - 1) / FK_FRAMES);
        hipLaunchKernelGGL(k_lbs_chain<true>, dim3(ntiles), dim3(FK_THREADS), (size_t)J * FK_JSTRIDE * sizeof(float), s, x, mask, rotmat, wf + w.hdr, wf + w.A,
                           wf + w.pf, B, T, num_person, J, C, pose_rep, flags, h->identity, sk, rest, sh, h->nbp, nullptr);
        LBS_HIP(h, hipGetLastError());
        const int vtiles = h->Vp / 32;
        const int tpw = (long long)ntiles * ((vtiles + 7) / 8) >= 2048 ? 8 : LBS_WAVES;         // (as rgn_rot2verts)
        const bool addtr = (flags & RGN_R2X_TRANSLATION) && (flags & RGN_R2X_VERTSTRANS);
        const int Kp = h->nbp + (h->pose ? h->Kp : 0);                                         // k-rows of the one operand: shape planes, then posedirs
        hipLaunchKernelGGL(k_lbs_skin<true>, dim3(ntiles, (vtiles + tpw - 1) / tpw), dim3(LBS_THREADS), (size_t)Kp * FK_FRAMES * sizeof(float), s, h->vtp,
                           wf + w.hdr, wf + w.A, wf + w.pf, h->sdp, h->wt, verts, B, T, num_person, h->V, h->Vp, J, h->Jp, Kp, 1, tpw, addtr ? 1 : 0,
                           h->nbp + h->K);
        LBS_HIP(h, hipGetLastError());
        return RGN_OK;
    });
}

int rgn_body_set_joint_regressors(rgn_body_handle b, int32_t Np, const int32_t* vertex_joints, int32_t Jr, const float* regressor) {
    return body_guard(b, "rgn_body_set_joint_regressors", [&]() -> int {
        auto bad = [&](const std::string& m) -> int {
            if (b) return b->fail(RGN_ERR_INVALID_ARG, "rgn_body_set_joint_regressors: " + m);
            g_body_create_error = "rgn_body_set_joint_regressors: " + m;
            return RGN_ERR_INVALID_ARG;
        };
        const std::string args = lbs_regressor_args(Np, vertex_joints, Jr, regressor);
        if (!args.empty()) return bad(args);
        if (!b) return bad("null handle");
        LbsCompact c;
        const LbsDims d{b->V, b->J, b->Jp, b->nb, b->nbp, b->K, b->Kp, b->pose};
        const std::string why = lbs_compact(d, b->h_vt.data(), b->h_sd.data(), b->h_pd.data(), b->h_wt.data(), Np, vertex_joints, Jr, regressor, c);
        if (!why.empty()) return bad(why);
        LBS_HIP(b, hipSetDevice(b->device));
        void* dev = nullptr;
        LBS_HIP(b, hipMalloc(&dev, c.blob.size() * sizeof(float)));
        if (hipError_t e = hipMemcpy(dev, c.blob.data(), c.blob.size() * sizeof(float), hipMemcpyHostToDevice); e != hipSuccess) {
            (void)hipFree(dev);
            return b->fail(RGN_ERR_HIP, std::string("rgn_body_set_joint_regressors: hipMemcpy: ") + hipGetErrorString(e));
        }
        // (here, not in the call, which may run under a stream capture) the feature image as k_lbs_skin<true>'s, never less than the partial sums
        const int lds = (LBS_MAX_BETAS + round_up(9 * (FK_MAX_JOINTS - 1), LBS_KGROUP)) * FK_FRAMES * (int)sizeof(float);
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_lbs_joints<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_lbs_joints<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) {
            (void)hipFree(dev);
            return b->fail(RGN_ERR_HIP, std::string("rgn_body_set_joint_regressors: hipFuncSetAttribute: ") + hipGetErrorString(e));
        }
        static_assert(LBS_JOINTS_SUMS <= (LBS_MAX_BETAS + 9 * (FK_MAX_JOINTS - 1)) * FK_FRAMES * (int)sizeof(float), "the partial sums fit the LDS limit set above");
        if (b->jblob) {                             // a second call replaces the data, once nothing enqueued can still read it
            (void)hipDeviceSynchronize();
            (void)hipFree(b->jblob);
        }
        b->jblob = reinterpret_cast<float*>(dev);
        b->jvt = b->jblob + c.o_vt;
        b->jsd = b->jblob + c.o_sd;
        b->jvtp = b->jblob + c.o_vtp;
        b->jsdp = b->jblob + c.o_sdp;
        b->jpd = b->jblob + c.o_pd;
        b->jwt = b->jblob + c.o_wt;
        b->jwj = b->jblob + c.o_wj;
        b->Np = Np;
        b->Jr = Jr;
        b->nS = c.nS;
        b->Sp = c.Sp;
        return RGN_OK;
    });
}

int rgn_rot2joints_workspace(rgn_body_handle b, int32_t B, int32_t T, int32_t num_person, uint64_t* nbytes) {
    return body_guard(b, "rgn_rot2joints_workspace", [&]() -> int { return joints_workspace(b, "rgn_rot2joints_workspace", B, T, num_person, nbytes, false); });
}

int rgn_rot2joints_shaped_workspace(rgn_body_handle b, int32_t B, int32_t T, int32_t num_person, uint64_t* nbytes) {
    return body_guard(b, "rgn_rot2joints_shaped_workspace",
                      [&]() -> int { return joints_workspace(b, "rgn_rot2joints_shaped_workspace", B, T, num_person, nbytes, true); });
}

int rgn_rot2joints(rgn_body_handle h, const float* x, const uint8_t* mask, int32_t B, int32_t T, const float* rest_joints, const int32_t* parents,
                   int32_t pose_rep, int32_t num_person, int32_t flags, const float* glob_rot, const float* betas, int32_t n_map, const int32_t* map,
                   int32_t root, float* joints, float* rotmat, void* work, uint64_t work_bytes, void* stream) {
    return body_guard(h, "rgn_rot2joints", [&]() -> int {
        const JointsArgs a{x, mask, B, T, rest_joints, parents, pose_rep, num_person, flags, glob_rot, n_map, map, root, joints, rotmat, work, work_bytes, stream};
        return rot2joints<false>(h, "rgn_rot2joints", a, betas, FkShape{});
    });
}

int rgn_rot2joints_shaped(rgn_body_handle h, const float* x, const uint8_t* mask, int32_t B, int32_t T, const float* rest_joints, const int32_t* parents,
                          const float* shape_joints, int32_t nb, const float* betas, int64_t beta_stride_b, int64_t beta_stride_p, int64_t beta_stride_t,
                          int32_t pose_rep, int32_t num_person, int32_t flags, const float* glob_rot, int32_t n_map, const int32_t* map, int32_t root,
                          float* joints, float* rotmat, void* work, uint64_t work_bytes, void* stream) {
    return body_guard(h, "rgn_rot2joints_shaped", [&]() -> int {
        const JointsArgs a{x, mask, B, T, rest_joints, parents, pose_rep, num_person, flags, glob_rot, n_map, map, root, joints, rotmat, work, work_bytes, stream};
        return rot2joints<true>(h, "rgn_rot2joints_shaped", a, nullptr, FkShape{shape_joints, betas, beta_stride_b, beta_stride_p, beta_stride_t, nb});
    });
}

}  // extern "C"
