// The GRU cell's pieces that the recurrences share (rgn_gru.hip: the action classifier; rgn_t2m.hip: the bidirectional co-embedding encoders): the
// transcendentals, the three-gate k-loop on v_mfma_f32_16x16x4_f32 and the A-fragment packing of a [3 H, K] weight. One definition, so both kernels
// round alike.
#pragma once
#include <vector>

#include "rgn_device.h"
#include "rgn_gru_check.h"

namespace rgn {
namespace {

// sigma and tanh on exp(-|.|) <= 1 and v_rcp_f32 of a value in [1, 2]: finite for every finite argument, no inf / inf
__device__ __forceinline__ float gru_sigmoid(float v) {
    const float e = expf(-fabsf(v));
    const float r = __builtin_amdgcn_rcpf(1.0f + e);
    return v >= 0.f ? r : e * r;
}
__device__ __forceinline__ float gru_tanh(float v) {
    const float e = expf(-2.0f * fabsf(v));
    return copysignf((1.0f - e) * __builtin_amdgcn_rcpf(1.0f + e), v);
}

// acc_g[unit, seq] += sum_k W_g[unit, k] act[seq][k] for the three gates of one unit tile over `nchunks` k granules. Lane l holds A[unit l & 15][k] and
// B[k][seq l & 15] with k = 16 c + 4 (l >> 4) + j in instruction j of granule c: the same k on both sides. The next granule's fragments are in flight
// while this one's twelve MFMAs issue.
__device__ __forceinline__ void gru_gate_kloop(const float* __restrict__ wp, int nchunks, const float* act, int ld, int lane, f32x4& a0, f32x4& a1, f32x4& a2) {
    const f32x4* w = reinterpret_cast<const f32x4*>(wp) + lane;
    const float* b = act + (lane & 15) * ld + 4 * (lane >> 4);
    f32x4 w0 = w[0], w1 = w[64], w2 = w[128];
    for (int c = 0; c < nchunks; ++c) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(b + GRU_KC * c);
        const int cn = c + 1 < nchunks ? c + 1 : c;
        const f32x4 n0 = w[cn * 192], n1 = w[cn * 192 + 64], n2 = w[cn * 192 + 128];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[j], bv[j], a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[j], bv[j], a1, 0, 0, 0);
            a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(w2[j], bv[j], a2, 0, 0, 0);
        }
        w0 = n0; w1 = n1; w2 = n2;
    }
}

// W [3 H, K] row-major (gate order r, z, n) -> A fragments [H/16][Kp/16][3][64][4], zero beyond K
inline std::vector<float> gru_pack(const float* W, int H, int K) {
    const int Kp = gru_pad_k(K), kc = Kp / GRU_KC, nt = H / 16;
    std::vector<float> p((size_t)nt * kc * 768, 0.f);
    for (int u = 0; u < nt; ++u)
        for (int c = 0; c < kc; ++c)
            for (int g = 0; g < 3; ++g)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 4; ++j) {
                        const int k = c * GRU_KC + 4 * (l >> 4) + j;
                        if (k < K) p[(((size_t)u * kc + c) * 3 + g) * 256 + l * 4 + j] = W[((size_t)g * H + u * 16 + (l & 15)) * K + k];
                    }
    return p;
}

}  // namespace
}  // namespace rgn
