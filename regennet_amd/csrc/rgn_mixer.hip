// The time mix of arch='mlp' (the reference's DiffMLP, model/mlp.py:9-86; called at model/cmdm.py:239-242) and the elementwise ends of its stack.
//
//   per layer l:   x = h + e_l[b]                                   e_l = emb_fc_l(SiLU(emb)) + bias, a [d] vector per sample
//                  h = x + SiLU(W0_l . LN0_l(x) + b0_l[:, None])    W0_l [T, T] contracts over FRAMES, b0_l is per output frame     <- k_mix_time
//                  h = h + SiLU(LN1_l(h) . W1_l^T + b1_l)           [d, d]: the handle's ordinary GEMM on the LN1 image k_mix_time leaves
//
// One source, three operand formats of the frame contraction (MixFmt): fp32 FMA, bf16 MFMA, split-bf16 (hi, lo; three MFMAs per product).
//
// A workgroup owns ONE SAMPLE. That settles the three hazards of this layer without any cross-workgroup order:
//   * LayerNorm0 wants whole-row statistics while the contraction is per column: the statistics of all T rows are taken first (phase 1) and kept in LDS.
//   * the update is in place: a 64-column slab of LN0(x) is staged in LDS for ALL frames before any frame of the slab is written, and the residual
//     x(t, c) is re-read and written by the same thread (phase 2).
//   * LayerNorm1 wants whole rows of the result: the workgroup re-reads its own rows behind a barrier (phase 3) and leaves LN1(h) as the feature
//     mix's GEMM operand (fp32, or K32-blocked planes).
// The frame axis is padded to Tp = 32 ceil(T / 32): the padded k-rows of the staged operand are written as true zeros and the weight's k-padding
// columns are zeros of the packer (uninitialised LDS times a zero weight could still be NaN). Weight rows beyond T are clamped; their products are
// never stored.
// The feature mix's result s is not added to h by the GEMM (its epilogue is act(acc + bias + add)): the next reader of the stream adds it - the next
// layer's k_mix_time (sadd), or k_mix_fin behind the last layer, which also makes the output projection's operand.
#include "rgn_internal.h"
#include "rgn_device.h"

#include <hip/hip_runtime.h>

namespace rgn {

constexpr int MX_NT = 256, MX_NW = MX_NT / 64, MX_SLAB = 64;
constexpr int MX_TS = MIX_MAX_T + 8;   // row stride (elements) of the transposed 16-bit operand image: 336 bytes, 16-byte aligned fragments

template <int FMT>
__device__ __forceinline__ float mix_silu(float v) {
    return FMT == MXF_F32 ? v / (1.0f + expf(-v)) : v / (1.0f + __expf(-v));
}

template <int FMT>
__global__ __launch_bounds__(MX_NT) void k_mix_time(MixTimeArgs g) {
    __shared__ float mu[MIX_MAX_T], rs[MIX_MAX_T];
    // MXF_F32: U[Tp][64] fp32 | else Ut_hi[64][MX_TS] (+ Ut_lo) bf16, column-major so that a lane's 8 consecutive k are one 16-byte read
    __shared__ __attribute__((aligned(16))) char ubuf[FMT == MXF_F32 ? MIX_MAX_T * MX_SLAB * 4 : (FMT == MXF_X3 ? 2 : 1) * MX_SLAB * MX_TS * 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, T = g.T, Tp = g.Tp, d = g.d;
    float* h = g.h + (size_t)b * T * d;
    const float* sa = g.sadd ? g.sadd + (size_t)b * T * d : nullptr;
    const float* e = g.e + (size_t)b * g.lde;
    const float invd = 1.0f / (float)d;
    // the layer's input x(t, j): the stream, + the previous feature mix where it is still apart, + the per-sample vector
    auto xin = [&](int t, int j) {
        const size_t o = (size_t)t * d + j;
        float v = h[o];
        if (sa) v += sa[o];
        return v + e[j];
    };

    // ---- phase 1: LayerNorm0 statistics of every row (two-pass), a wave per row
    for (int t = wave; t < T; t += MX_NW) {
        float s = 0.f;
        for (int j = lane; j < d; j += 64) s += xin(t, j);
        const float mean = wave_sum_shfl(s) * invd;
        float q = 0.f;
        for (int j = lane; j < d; j += 64) {
            const float c = xin(t, j) - mean;
            q = fmaf(c, c, q);
        }
        const float var = wave_sum_shfl(q) * invd;
        if (lane == 0) {
            mu[t] = mean;
            rs[t] = 1.0f / sqrtf(var + 1e-5f);
        }
    }
    __syncthreads();

    // ---- phase 2: slab by slab of 64 columns: stage LN0(x) of all frames, contract over frames, x + SiLU(. + b0) back in place
    for (int c0 = 0; c0 < d; c0 += MX_SLAB) {
        {
            const int col = c0 + lane;
            const float gg = g.g0[col], bb = g.be0[col];
            for (int t = wave; t < Tp; t += MX_NW) {
                const float u = t < T ? (xin(t, col) - mu[t]) * rs[t] * gg + bb : 0.f;   // padded k-rows: true zeros
                if constexpr (FMT == MXF_F32) {
                    reinterpret_cast<float*>(ubuf)[t * MX_SLAB + lane] = u;
                } else {
                    __bf16* uh = reinterpret_cast<__bf16*>(ubuf);
                    const __bf16 hi = (__bf16)u;
                    uh[lane * MX_TS + t] = hi;
                    if constexpr (FMT == MXF_X3) uh[MX_SLAB * MX_TS + lane * MX_TS + t] = (__bf16)(u - (float)hi);
                }
            }
        }
        __syncthreads();
        if constexpr (FMT == MXF_F32) {
            const float* U = reinterpret_cast<const float*>(ubuf);
            for (int t0 = wave; t0 < T; t0 += 4 * MX_NW) {   // output frames t0 + 4 r, r < 4, of column c0 + lane
                const float* w[4];
                float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int tr = t0 + MX_NW * r;
                    w[r] = g.W0 + (size_t)(tr < T ? tr : T - 1) * Tp;
                }
                for (int t = 0; t < T; ++t) {
                    const float u = U[t * MX_SLAB + lane];
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[r] = fmaf(w[r][t], u, acc[r]);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int tr = t0 + MX_NW * r;
                    if (tr < T) {
                        const int col = c0 + lane;
                        const float x = xin(tr, col);
                        h[(size_t)tr * d + col] = x + mix_silu<FMT>(acc[r] + g.b0[tr]);
                    }
                }
            }
        } else {
            // A operand: W0 rows (output frames), B operand: the staged columns; accumulator register i of lane (l31, kh) = output frame
            // 32 mt + mfma32_row(i, kh), column 32 nt + l31 (rgn_layout.h, 4)
            const __bf16* uh = reinterpret_cast<const __bf16*>(ubuf);
            const int l31 = lane & 31, kh = lane >> 5;
            const int ntile = (Tp >> 5) * 2, nks = Tp >> 4;
            for (int tile = wave; tile < ntile; tile += MX_NW) {
                const int mt = tile >> 1, nt = tile & 1;
                int wrow = 32 * mt + l31;
                wrow = wrow < T ? wrow : T - 1;
                const __bf16* wh = g.W0hi + (size_t)wrow * Tp + 8 * kh;
                const __bf16* wl = FMT == MXF_X3 ? g.W0lo + (size_t)wrow * Tp + 8 * kh : nullptr;
                const __bf16* bh = uh + (32 * nt + l31) * MX_TS + 8 * kh;
                const __bf16* bl = bh + MX_SLAB * MX_TS;
                f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0.f;
                for (int ks = 0; ks < nks; ++ks) {
                    const bf16x8 a = *reinterpret_cast<const bf16x8*>(wh + 16 * ks);
                    const bf16x8 u = *reinterpret_cast<const bf16x8*>(bh + 16 * ks);
                    if constexpr (FMT == MXF_X3) {
                        const bf16x8 al = *reinterpret_cast<const bf16x8*>(wl + 16 * ks);
                        const bf16x8 ul = *reinterpret_cast<const bf16x8*>(bl + 16 * ks);
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, u, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, ul, acc, 0, 0, 0);
                    }
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, u, acc, 0, 0, 0);
                }
                const int col = c0 + 32 * nt + l31;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int tr = 32 * mt + mfma32_row(i, kh);
                    if (tr < T) {
                        const float x = xin(tr, col);
                        h[(size_t)tr * d + col] = x + mix_silu<FMT>(acc[i] + g.b0[tr]);
                    }
                }
            }
        }
        __syncthreads();   // the image is re-staged by the next slab; behind the last one: the rows are complete for phase 3
    }

    // ---- phase 3: w = LayerNorm1(h) of the sample's own rows -> the feature mix's GEMM operand
    for (int t = wave; t < T; t += MX_NW) {
        const float* hr = h + (size_t)t * d;
        float s = 0.f;
        for (int j = lane; j < d; j += 64) s += hr[j];
        const float mean = wave_sum_shfl(s) * invd;
        float q = 0.f;
        for (int j = lane; j < d; j += 64) {
            const float c = hr[j] - mean;
            q = fmaf(c, c, q);
        }
        const float rstd = 1.0f / sqrtf(wave_sum_shfl(q) * invd + 1e-5f);
        const int row = b * T + t;
        for (int j = lane; j < d; j += 64) {
            const float v = (hr[j] - mean) * rstd * g.g1[j] + g.be1[j];
            if constexpr (FMT == MXF_F32) g.w32[(size_t)row * d + j] = v;
            else plane_put(g.wp, row, j, v);
        }
    }
}

hipError_t launch_mix_time(const MixTimeArgs& g, int fmt, hipStream_t s) {
    if (!mix_supported(g.T, g.d) || g.Tp != (g.T + 31) / 32 * 32 || g.ns <= 0 || !g.h || !g.e || !g.b0) return hipErrorInvalidValue;
    if (fmt == MXF_F32 ? (!g.W0 || !g.w32) : (!g.W0hi || !g.wp.hi || (fmt == MXF_X3 && (!g.W0lo || !g.wp.lo)))) return hipErrorInvalidValue;
    const dim3 grid(g.ns), block(MX_NT);
    switch (fmt) {
        case MXF_F32: hipLaunchKernelGGL(k_mix_time<MXF_F32>, grid, block, 0, s, g); break;
        case MXF_BF16: hipLaunchKernelGGL(k_mix_time<MXF_BF16>, grid, block, 0, s, g); break;
        case MXF_X3: hipLaunchKernelGGL(k_mix_time<MXF_X3>, grid, block, 0, s, g); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// SiLU of the timestep (+ condition) embedding of every evaluation row: the operand of the one [Bm, d] x [d, L d] GEMM that makes all e_l
__global__ void k_mix_emb(const float* __restrict__ rows, const float* __restrict__ stepemb, const int* __restrict__ d_step, float* __restrict__ out, int d) {
    const int b = blockIdx.x;
    const float* se = stepemb ? stepemb + (size_t)(*d_step) * d : nullptr;   // sampling loop: the time part of this step
    for (int j = threadIdx.x; j < d; j += blockDim.x) {
        const float v = (se ? se[j] : 0.f) + (rows ? rows[(size_t)b * d + j] : 0.f);
        out[(size_t)b * d + j] = v / (1.0f + expf(-v));
    }
}
hipError_t launch_mix_emb(const float* rows, const float* stepemb, const int* d_step, float* out, int Bm, int d, hipStream_t s) {
    if (Bm <= 0 || (stepemb && !d_step)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mix_emb, dim3(Bm), dim3(256), 0, s, rows, stepemb, d_step, out, d);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_mix_fin(float* __restrict__ h, const float* __restrict__ sadd, Planes hp, int M, int d) {
    const size_t n = (size_t)M * d;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float v = h[i] + sadd[i];
        if (hp.hi) plane_put(hp, (int)(i / d), (int)(i % d), v);
        else h[i] = v;
    }
}
hipError_t launch_mix_fin(float* h, const float* sadd, Planes hp, int M, int d, hipStream_t s) {
    if (M <= 0 || !h || !sadd) return hipErrorInvalidValue;
    const size_t n = (size_t)M * d;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_mix_fin, dim3(blocks), dim3(256), 0, s, h, sadd, hp, M, d);
    return hipGetLastError();
}

}  // namespace rgn
