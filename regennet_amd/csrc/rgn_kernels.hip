// Device code for the ReGenNet sampling hot path on MI355X (gfx950, wave64, MFMA).
//
// Layouts:
//   boundary tensors   x, cmotion, out : fp32 [B, F=njoints*nfeats, T]   (frames contiguous)
//   token-major        xin  [B*Tq, F]   h [Bm*Tq, d]   qkv [Bm*Tq, 3d]   att [Bm*Tq, d]   ffn [Bm*Tq, ff]
//                      row = b*Tq + etd + t  (a sample's tokens are contiguous -> attention reads one slab)
//   weights            nn.Linear layout [N, Kp] (K contiguous, zero padded to a multiple of 16)
//
// Reference arithmetic replaced (file:line in the upstream repo) is cited per kernel.
#include "rgn_internal.h"
#include "rgn_device.h"
#include "rgn_sampler.h"

#include <hip/hip_runtime.h>
#include <math.h>

namespace rgn {

__device__ __forceinline__ float act_apply(float v, int act) {
    if (act == 1) return v * 0.5f * (1.0f + erff(v * 0.70710678118654752440f));  // F.gelu, exact erf
    if (act == 2) return v / (1.0f + __expf(-v));                                  // nn.SiLU (cmdm.py:293)
    if (act == 3) return fmaxf(v, 0.f);                                            // nn.ReLU (ST-GCN evaluator)
    return v;
}

// =================================================================================================
// GEMM  C[M,N] = act( A[M,K] * W[N,K]^T + bias[N] + add[r % add_mod, N] )
// Replaces every nn.Linear on the path (cmdm.py:61,291-295,307,337 and the in_proj/out_proj/linear1/
// linear2 of nn.TransformerDecoderLayer constructed at cmdm.py:75-81).
//
// F32 precision mode: v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate).
// Block = 128x128 output tile, 4 waves as 2x2, each wave 64x64 = 2x2 MFMA tiles (64 acc VGPRs).
// K is walked in 16-wide LDS tiles; rows are padded to 20 floats so that the 16 lanes of a
// ds_read_b128 group (consecutive rows, 80-byte stride) fall on disjoint bank quads.
// An 8-wide k chunk is contracted by 4 MFMAs: lanes 0-31 feed k = kc+j, lanes 32-63 feed k = kc+4+j
// for A and B alike (any consistent permutation of the contraction index is legal).
// =================================================================================================
constexpr int G_BM = 128, G_BN = 128, G_BK = 16, G_LD = G_BK + 4;

template <bool VEC_A>
__global__ __launch_bounds__(256) void k_gemm_f32(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) float As[G_BM * G_LD];
    __shared__ __attribute__((aligned(16))) float Ws[G_BN * G_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * G_BM, n0 = blockIdx.x * G_BN;
    const int lr = tid >> 2, lk = (tid & 3) * 4;  // staging: row (0..63, +64), k quad

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

    f32x4 ra[2], rw[2];
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int m = m0 + lr + 64 * i, k = k0 + lk;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (m < g.M) {
                const float* p = g.A + (size_t)m * g.lda + k;
                if (VEC_A) {
                    if (k < g.K) v = *reinterpret_cast<const f32x4*>(p);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (k + j < g.K) v[j] = p[j];
                }
            }
            ra[i] = v;
            const int n = n0 + lr + 64 * i;
            f32x4 w = {0.f, 0.f, 0.f, 0.f};
            if (n < g.N) w = *reinterpret_cast<const f32x4*>(g.W + (size_t)n * g.Kp + k);
            rw[i] = w;
        }
    };
    const int nk = g.Kp / G_BK;
    gload(0);
    for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *reinterpret_cast<f32x4*>(&As[(lr + 64 * i) * G_LD + lk]) = ra[i];
            *reinterpret_cast<f32x4*>(&Ws[(lr + 64 * i) * G_LD + lk]) = rw[i];
        }
        __syncthreads();
        if (kt + 1 < nk) gload((kt + 1) * G_BK);
#pragma unroll
        for (int kc = 0; kc < G_BK; kc += 8) {
            f32x4 a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = *reinterpret_cast<const f32x4*>(&As[(wm * 64 + t * 32 + (lane & 31)) * G_LD + kc + 4 * (lane >> 5)]);
                b[t] = *reinterpret_cast<const f32x4*>(&Ws[(wn * 64 + t * 32 + (lane & 31)) * G_LD + kc + 4 * (lane >> 5)]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                    for (int tb = 0; tb < 2; ++tb)
                        acc[ta][tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ta][j], b[tb][j], acc[ta][tb], 0, 0, 0);
        }
        __syncthreads();
    }
    // epilogue: C/D layout of 32x32 MFMA: col = lane&31, row = (i&3) + 8*(i>>2) + 4*(lane>>5)
#pragma unroll
    for (int tb = 0; tb < 2; ++tb) {
        const int n = n0 + wn * 64 + tb * 32 + (lane & 31);
        if (n >= g.N) continue;
        const float bias = g.bias ? g.bias[n] : 0.f;
#pragma unroll
        for (int ta = 0; ta < 2; ++ta) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int m = m0 + wm * 64 + ta * 32 + mfma32_row(i, lane >> 5);
                if (m >= g.M) continue;
                float v = acc[ta][tb][i] + bias;
                if (g.add) {
                    const int ar = g.add_mod ? (m % g.add_mod) : m;
                    v += g.add[(size_t)ar * g.ldadd + n];
                }
                g.C[(size_t)m * g.ldc + n] = act_apply(v, g.act);
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------
// BF16X3 / BF16 precision modes: v_mfma_f32_32x32x16_bf16, fp32 accumulate.
//   BF16X3: every fp32 operand is split x = hi + lo (both bf16, round-to-nearest-even) and the product
//           is formed as ah*bh + ah*bl + al*bh (the al*bl term, ~2^-18 relative, is dropped): three MFMAs
//           per tile pair, ~2^-16 relative accuracy per product — inside the 1e-3 end-to-end tolerance
//           where plain bf16 (2^-9) is not (SURVEY.md §7 "Precision vs. the 1e-3 abs tolerance").
//   Weights are pre-split on the host (Whi/Wlo [N,Kp] bf16); activations stay fp32 in HBM and are
//   split while being staged into LDS (v_cvt_pk_bf16_f32), so the residual stream never loses bits.
// Tile 128x128x32, 4 waves (2x2), wave tile 64x64 = 2x2 MFMA tiles; LDS rows padded to 40 bf16 (80 B)
// -> the 16 lanes of each ds_read_b128 group hit 16 disjoint bank quads.
// Blocks are remapped so that the column tiles of one A row-block run on the same XCD (shared L2).
// -------------------------------------------------------------------------------------------------
constexpr int H_BM = 128, H_BN = 128, H_BK = 32, H_LD = H_BK + 8;   // bf16 elements per LDS row

template <bool X3, bool VEC_A>
__global__ __launch_bounds__(256) void k_gemm_bf16(GemmArgs g, int nbx, int nby) {
    __shared__ __attribute__((aligned(16))) __bf16 Ah[H_BM * H_LD];
    __shared__ __attribute__((aligned(16))) __bf16 Al[X3 ? H_BM * H_LD : 8];
    __shared__ __attribute__((aligned(16))) __bf16 Wh[H_BN * H_LD];
    __shared__ __attribute__((aligned(16))) __bf16 Wl[X3 ? H_BN * H_LD : 8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // XCD-aware bijective remap: hardware places block b on XCD b%8; give each XCD a contiguous range of
    // virtual ids (n-tile fastest) so one A row-block is fetched into a single XCD's L2.
    const int nwg = nbx * nby, bid = blockIdx.x;
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int vid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    const int m0 = (vid / nbx) * H_BM, n0 = (vid % nbx) * H_BN;

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

    const int ar = tid >> 3, ak = (tid & 7) * 4;     // A staging: 8 threads x float4 cover one 32-float row
    const int wr = tid >> 2, wk = (tid & 3) * 8;     // W staging: 4 threads x 8 bf16 cover one 32-elem row
    f32x4 ra[4];
    u32x4 rwh[2], rwl[2];
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + ar + 32 * i, k = k0 + ak;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (m < g.M) {
                const float* p = g.A + (size_t)m * g.lda + k;
                if (VEC_A) {
                    if (k < g.K) v = *reinterpret_cast<const f32x4*>(p);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (k + j < g.K) v[j] = p[j];
                }
            }
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int n = n0 + wr + 64 * i;
            u32x4 h = {0u, 0u, 0u, 0u}, l = {0u, 0u, 0u, 0u};
            if (n < g.N) {
                const size_t o = (size_t)n * g.Kp + k0 + wk;
                h = *reinterpret_cast<const u32x4*>(g.Whi + o);
                if (X3) l = *reinterpret_cast<const u32x4*>(g.Wlo + o);
            }
            rwh[i] = h;
            rwl[i] = l;
        }
    };
    const int nk = g.Kp / H_BK;
    gload(0);
    for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bf16x4 hi, lo;
            split_bf16(ra[i], hi, lo);
            *reinterpret_cast<bf16x4*>(&Ah[(ar + 32 * i) * H_LD + ak]) = hi;
            if (X3) *reinterpret_cast<bf16x4*>(&Al[(ar + 32 * i) * H_LD + ak]) = lo;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *reinterpret_cast<u32x4*>(&Wh[(wr + 64 * i) * H_LD + wk]) = rwh[i];
            if (X3) *reinterpret_cast<u32x4*>(&Wl[(wr + 64 * i) * H_LD + wk]) = rwl[i];
        }
        __syncthreads();
        if (kt + 1 < nk) gload((kt + 1) * H_BK);
#pragma unroll
        for (int ks = 0; ks < H_BK; ks += 16) {
            bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int ao = (wm * 64 + t * 32 + (lane & 31)) * H_LD + ks + 8 * (lane >> 5);
                const int bo = (wn * 64 + t * 32 + (lane & 31)) * H_LD + ks + 8 * (lane >> 5);
                ah[t] = *reinterpret_cast<const bf16x8*>(&Ah[ao]);
                bh[t] = *reinterpret_cast<const bf16x8*>(&Wh[bo]);
                if (X3) {
                    al[t] = *reinterpret_cast<const bf16x8*>(&Al[ao]);
                    bl[t] = *reinterpret_cast<const bf16x8*>(&Wl[bo]);
                }
            }
#pragma unroll
            for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                for (int tb = 0; tb < 2; ++tb) {
                    if (X3) {   // small terms first, then the leading product
                        acc[ta][tb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[ta], bh[tb], acc[ta][tb], 0, 0, 0);
                        acc[ta][tb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[ta], bl[tb], acc[ta][tb], 0, 0, 0);
                    }
                    acc[ta][tb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[ta], bh[tb], acc[ta][tb], 0, 0, 0);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int tb = 0; tb < 2; ++tb) {
        const int n = n0 + wn * 64 + tb * 32 + (lane & 31);
        if (n >= g.N) continue;
        const float bias = g.bias ? g.bias[n] : 0.f;
#pragma unroll
        for (int ta = 0; ta < 2; ++ta) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                // (= mfma32_row(i, lane >> 5) of rgn_layout.h, spelled out: behind the function two forms of this kernel take 4 more VGPRs, one of them a wave per SIMD)
                const int m = m0 + wm * 64 + ta * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
                if (m >= g.M) continue;
                float v = acc[ta][tb][i] + bias;
                if (g.add) {
                    const int arow = g.add_mod ? (m % g.add_mod) : m;
                    v += g.add[(size_t)arow * g.ldadd + n];
                }
                g.C[(size_t)m * g.ldc + n] = act_apply(v, g.act);
            }
        }
    }
}

hipError_t launch_gemm(const GemmArgs& g, int precision, hipStream_t s) {
    const bool vec = (g.lda % 4 == 0) && (g.K % 4 == 0) && ((reinterpret_cast<uintptr_t>(g.A) & 15) == 0);
    if (precision == 0) {
        dim3 grid((g.N + G_BN - 1) / G_BN, (g.M + G_BM - 1) / G_BM);
        if (vec)
            hipLaunchKernelGGL(k_gemm_f32<true>, grid, dim3(256), 0, s, g);
        else
            hipLaunchKernelGGL(k_gemm_f32<false>, grid, dim3(256), 0, s, g);
        return hipGetLastError();
    }
    const int nbx = (g.N + H_BN - 1) / H_BN, nby = (g.M + H_BM - 1) / H_BM;
    dim3 grid(nbx * nby);
    if (precision == 1) {
        if (vec)
            hipLaunchKernelGGL((k_gemm_bf16<true, true>), grid, dim3(256), 0, s, g, nbx, nby);
        else
            hipLaunchKernelGGL((k_gemm_bf16<true, false>), grid, dim3(256), 0, s, g, nbx, nby);
    } else {
        if (vec)
            hipLaunchKernelGGL((k_gemm_bf16<false, true>), grid, dim3(256), 0, s, g, nbx, nby);
        else
            hipLaunchKernelGGL((k_gemm_bf16<false, false>), grid, dim3(256), 0, s, g, nbx, nby);
    }
    return hipGetLastError();
}

// =================================================================================================
// Residual LayerNorm(s): one wave per token row, row held in registers (lane owns VPL = d/64 CONSECUTIVE columns, so
// every access is one or two 16-byte vectors per lane: fp32 rows as float4, plane rows as 8 bf16).
//   out = LN_b( LN_a(in + resid) + addvec[row / Tq] + stepvec[*d_step] )   or   out = LN_a(in + resid)
// F32 mode: `in` already contains the residual (added in the producing GEMM's epilogue), resid is empty and the
// result goes to the fp32 residual stream `out`. bf16 modes: the residual stream exists only as split planes; it is
// added here (hi + lo) and the result is written as planes only (out == nullptr).
// Replaces norm1/norm2/norm3 of TransformerDecoderLayer (post-norm, eps=1e-5) and the add of the
// 1-token cross-attention result, which is constant over the sequence.
// =================================================================================================
template <int N>
__device__ __forceinline__ void ld_f32(const float* __restrict__ p, float* v) {
    if constexpr (N % 4 == 0) {
#pragma unroll
        for (int j = 0; j < N / 4; ++j) {
            const f32x4 t = reinterpret_cast<const f32x4*>(p)[j];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * j + e] = t[e];
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = p[j];
    }
}
template <int N>
__device__ __forceinline__ void st_f32(float* __restrict__ p, const float* v) {
    if constexpr (N % 4 == 0) {
#pragma unroll
        for (int j = 0; j < N / 4; ++j) {
            const f32x4 t = {v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]};
            reinterpret_cast<f32x4*>(p)[j] = t;
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) p[j] = v[j];
    }
}
template <int N>
__device__ __forceinline__ void ld_bf16_add(const __bf16* __restrict__ p, float* v) {   // v += p[0..N)
    typedef vec_t<__bf16, N> bf16xN;
    if constexpr (N == 1) {
        v[0] += (float)p[0];
    } else if constexpr (N <= 8) {
        const bf16xN t = *reinterpret_cast<const bf16xN*>(p);
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] += (float)t[e];
    } else {
        ld_bf16_add<8>(p, v);
        ld_bf16_add<N - 8>(p + 8, v + 8);
    }
}
template <int N>
__device__ __forceinline__ void st_split(__bf16* __restrict__ hi, __bf16* __restrict__ lo, const float* v) {
    typedef vec_t<__bf16, N> bf16xN;
    if constexpr (N == 1) {
        const __bf16 h = (__bf16)v[0];
        hi[0] = h;
        if (lo) lo[0] = (__bf16)(v[0] - (float)h);
    } else if constexpr (N <= 8) {
        bf16xN h, l;
#pragma unroll
        for (int e = 0; e < N; ++e) {
            h[e] = (__bf16)v[e];
            l[e] = (__bf16)(v[e] - (float)h[e]);
        }
        *reinterpret_cast<bf16xN*>(hi) = h;
        if (lo) *reinterpret_cast<bf16xN*>(lo) = l;
    } else {
        st_split<8>(hi, lo, v);
        st_split<N - 8>(hi + 8, lo ? lo + 8 : nullptr, v + 8);
    }
}

template <int VPL>
__global__ __launch_bounds__(256) void k_layernorm(const float* __restrict__ in, Planes resid, float* __restrict__ out, Planes op, int M, int d,
                                                    const float* __restrict__ ga, const float* __restrict__ ba,
                                                    const float* __restrict__ addvec, int ldadd,
                                                    const float* __restrict__ stepvec, int ldstep, const int* __restrict__ d_step,
                                                    int Tq, const float* __restrict__ gb, const float* __restrict__ bb) {
    const int lane = threadIdx.x & 63;
    // XCD-affine mapping: hardware places block b on XCD b%8; give every XCD one contiguous range of rows, the same
    // range whose tiles the neighbouring GEMMs compute on that XCD (their L2 still holds what this kernel reads/writes)
    const int vid = xcd_affine(blockIdx.x, gridDim.x);
    const int row = vid * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int c0 = lane * VPL;                                   // first of this lane's VPL consecutive columns
    float v[VPL], w[VPL], bsh[VPL];
    ld_f32<VPL>(in + (size_t)row * d + c0, v);
    if (resid.hi) {
        const size_t o = plane_off(resid.rows, row, c0);          // VPL divides 32: the run stays inside one K32 block
        ld_bf16_add<VPL>(resid.hi + o, v);
        if (resid.lo) ld_bf16_add<VPL>(resid.lo + o, v);
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) s += v[i];
    const float invd = 1.0f / (float)d;
    float mean = wave_sum_shfl(s) * invd;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const float c = v[i] - mean;
        q += c * c;
    }
    float rstd = 1.0f / sqrtf(wave_sum_shfl(q) * invd + 1e-5f);
    ld_f32<VPL>(ga + c0, w);
    ld_f32<VPL>(ba + c0, bsh);
#pragma unroll
    for (int i = 0; i < VPL; ++i) v[i] = (v[i] - mean) * rstd * w[i] + bsh[i];
    if (gb) {
        if (stepvec) {
            ld_f32<VPL>(stepvec + (size_t)(*d_step) * ldstep + c0, w);
#pragma unroll
            for (int i = 0; i < VPL; ++i) v[i] += w[i];
        }
        if (addvec) {
            ld_f32<VPL>(addvec + (size_t)(row / Tq) * ldadd + c0, w);
#pragma unroll
            for (int i = 0; i < VPL; ++i) v[i] += w[i];
        }
        s = 0.f;
#pragma unroll
        for (int i = 0; i < VPL; ++i) s += v[i];
        mean = wave_sum_shfl(s) * invd;
        q = 0.f;
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            const float c = v[i] - mean;
            q += c * c;
        }
        rstd = 1.0f / sqrtf(wave_sum_shfl(q) * invd + 1e-5f);
        ld_f32<VPL>(gb + c0, w);
        ld_f32<VPL>(bb + c0, bsh);
#pragma unroll
        for (int i = 0; i < VPL; ++i) v[i] = (v[i] - mean) * rstd * w[i] + bsh[i];
    }
    if (out) st_f32<VPL>(out + (size_t)row * d + c0, v);
    if (op.hi) {
        const size_t o = plane_off(op.rows, row, c0);
        st_split<VPL>(op.hi + o, op.lo ? op.lo + o : nullptr, v);
    }
}

hipError_t launch_layernorm(const float* in, Planes resid, float* out, Planes op, int M, int d, const float* ga, const float* ba,
                            const float* addvec, int ldadd, const float* stepvec, int ldstep, const int* d_step, int Tq,
                            const float* gb, const float* bb, hipStream_t s) {
    dim3 grid((M + 3) / 4), block(256);
#define RGN_LN(V) hipLaunchKernelGGL(k_layernorm<V>, grid, block, 0, s, in, resid, out, op, M, d, ga, ba, addvec, ldadd, stepvec, ldstep, d_step, Tq, gb, bb)
    switch (d / 64) {
        case 1: RGN_LN(1); break;
        case 2: RGN_LN(2); break;
        case 4: RGN_LN(4); break;
        case 8: RGN_LN(8); break;
        case 16: RGN_LN(16); break;
        default: return hipErrorInvalidValue;
    }
#undef RGN_LN
    return hipGetLastError();
}

// =================================================================================================
// Timestep embedding input: out[r,:] = pe[t_r,:]  (TimestepEmbedder.forward gather, cmdm.py:298).
// t_r comes from the device step table (sampling loop; bit-exact timestep_map lookup of
// _WrappedModel.__call__, respace.py:124-129) or from external int64 timesteps (rgn_denoise).
// =================================================================================================
__global__ void k_gather_pe(const float* __restrict__ pe, const StepCoef* __restrict__ tab, const int* __restrict__ d_step,
                            const SampleParams* __restrict__ sp, float* __restrict__ out, int Bm, int B, int d, int pe_len) {
    const int r = blockIdx.x;
    long long t;
    if (sp->t_ext)
        t = sp->t_ext[r % B];
    else
        t = tab[*d_step].t_model;
    t = t < 0 ? 0 : (t >= pe_len ? pe_len - 1 : t);   // never read outside the table (the Python boundary raises IndexError first)
    for (int c = threadIdx.x; c < d; c += blockDim.x) out[(size_t)r * d + c] = pe[(size_t)t * d + c];
}
hipError_t launch_gather_pe(const float* pe, const StepCoef* tab, const int* d_step, const SampleParams* sp,
                            float* out, int Bm, int B, int d, int pe_len, hipStream_t s) {
    hipLaunchKernelGGL(k_gather_pe, dim3(Bm), dim3(d >= 256 ? 256 : 64), 0, s, pe, tab, d_step, sp, out, Bm, B, d, pe_len);
    return hipGetLastError();
}

// schedule-time variant: out[i,:] = pe[timestep_map[i],:] for every loop index i (the timestep embedding of the
// sampling loop depends on the step only, so its MLP and the folded cross-attention GEMM run once per schedule)
__global__ void k_gather_pe_all(const float* __restrict__ pe, const StepCoef* __restrict__ tab, float* __restrict__ out, int d) {
    const int i = blockIdx.x;
    const long long t = tab[i].t_model;
    for (int c = threadIdx.x; c < d; c += blockDim.x) out[(size_t)i * d + c] = pe[(size_t)t * d + c];
}
hipError_t launch_gather_pe_all(const float* pe, const StepCoef* tab, float* out, int S, int d, hipStream_t s) {
    hipLaunchKernelGGL(k_gather_pe_all, dim3(S), dim3(d >= 256 ? 256 : 64), 0, s, pe, tab, out, d);
    return hipGetLastError();
}

// emb_trans_dec: token 0 of every sample is emb[b] (+ pe[0])            (cmdm.py:212-218)
__global__ void k_emb_rows(const float* __restrict__ emb, const float* __restrict__ stepemb, const int* __restrict__ d_step,
                           const float* __restrict__ pe, float* __restrict__ h, Planes hp, Dims dm, int wo_pos) {
    const int b = blockIdx.x;
    const float* se = stepemb ? stepemb + (size_t)(*d_step) * dm.d : nullptr;   // sampling loop: time part per step
    for (int c = threadIdx.x; c < dm.d; c += blockDim.x) {
        const float v = (emb ? emb[(size_t)b * dm.d + c] : 0.f) + (se ? se[c] : 0.f) + (wo_pos ? 0.f : pe[c]);
        h[(size_t)b * dm.Tq * dm.d + c] = v;
        if (hp.hi) plane_put(hp, b * dm.Tq, c, v);
    }
}
hipError_t launch_emb_rows(const float* emb, const float* stepemb, const int* d_step, const float* pe, float* h, Planes hp,
                           const Dims& dm, int wo_pos, hipStream_t s) {
    hipLaunchKernelGGL(k_emb_rows, dim3(dm.Bm), dim3(256), 0, s, emb, stepemb, d_step, pe, h, hp, dm, wo_pos);
    return hipGetLastError();
}

// c0[b*Tq + j, :] += pe[j, :]   (sequence_pos_encoder, cmdm.py:278-281) — hoisted, once per condition
__global__ void k_add_pe(float* __restrict__ c0, const float* __restrict__ pe, Dims dm) {
    const int r = blockIdx.x, j = r % dm.Tq;
    for (int c = threadIdx.x; c < dm.d; c += blockDim.x) c0[(size_t)r * dm.d + c] += pe[(size_t)j * dm.d + c];
}
hipError_t launch_add_pe(float* c0, const float* pe, const Dims& dm, hipStream_t s) {
    hipLaunchKernelGGL(k_add_pe, dim3(dm.B * dm.Tq), dim3(256), 0, s, c0, pe, dm);
    return hipGetLastError();
}

// =================================================================================================
// Boundary layout <-> token-major transposes, fused with the sampler arithmetic.
// =================================================================================================
// InputProcess permute (cmdm.py:312): x [B,F,T] -> xin[(b*Tq+etd+t), f]; 32x32 LDS tiles, both sides coalesced.
__global__ __launch_bounds__(256) void k_pack_x(const float* __restrict__ x, float* __restrict__ xin, Planes xp, int copies,
                                                 Dims dm) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, f0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int f = f0 + i, t = t0 + tx;
        tile[i][tx] = (f < dm.F && t < dm.T) ? x[((size_t)b * dm.F + f) * dm.T + t] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int t = t0 + i, f = f0 + tx;
        if (t < dm.T && f < dm.F) {
            const int row = b * dm.Tq + dm.etd + t;
            if (xin) xin[(size_t)row * dm.F + f] = tile[tx][i];
            if (xp.hi)
                for (int cpy = 0; cpy < copies; ++cpy) plane_put(xp, row + cpy * dm.B * dm.Tq, f, tile[tx][i]);
        }
    }
}
hipError_t launch_pack_x(const float* x, float* xin, Planes xp, int copies, const Dims& dm, hipStream_t s) {
    dim3 grid((dm.T + 31) / 32, (dm.F + 31) / 32, dm.B);
    hipLaunchKernelGGL(k_pack_x, grid, dim3(256), 0, s, x, xin, xp, copies, dm);
    return hipGetLastError();
}

__global__ void k_randn(float* __restrict__ x, int B, int FT, int T, unsigned long long seed, unsigned long long off, uint32_t stream) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * FT) return;
    const int b = (int)(idx / FT), e = (int)(idx - (size_t)b * FT);
    x[idx] = philox_normal(seed, off + b, stream, noise_elem(e / T, e % T));   // stream 0xFFFFFFFF = x_T draw, k = loop index k's noise
}
hipError_t launch_randn(float* x, int B, int FT, int T, unsigned long long seed, unsigned long long off, uint32_t stream, hipStream_t s) {
    const size_t n = (size_t)B * FT;
    hipLaunchKernelGGL(k_randn, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, B, FT, T, seed, off, stream);
    return hipGetLastError();
}

// Sampler update, one 32(f) x 32(t) tile per block: x0 = x0_c (OutputProcess permute cmdm.py:353-354) or the guided combination of x0_c and
// x0_u, then the step of rgn_sampler.h (guidance, in-painting select, clamp, noise, DDPM / DDIM update).
// Writes the new state in boundary layout [B,F,T] and token-major xin for the next step's GEMM.
// In sampling mode the LAST block to finish (of all k_update launches of the step: the chains' launches together cover the
// B samples once) also moves the device-side loop index on: *d_step -= 1 (ticket counters behind d_step[4]). Every block read *d_step before it took its
// ticket, and every other reader of *d_step (the layer kernels of a chain) precedes that chain's k_update in stream order.
// INPAINT: the forms that read the bound mask and motion (rgn_set_inpainting).
template <bool INPAINT>
__global__ __launch_bounds__(256) void k_update(const float* __restrict__ x0tok, const float* __restrict__ scale,
                                                 const StepCoef* __restrict__ tab, int* d_step,
                                                 const SampleParams* __restrict__ spp, float* __restrict__ xin, Planes xp,
                                                 Dims dm, int b0) {
    __shared__ float tc[32][33];
    __shared__ float tu[32][33];
    const SampleParams sp = *spp;
    const int b = b0 + blockIdx.z, f0 = blockIdx.y * 32, t0 = blockIdx.x * 32;   // samples [b0, b0 + gridDim.z)
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const size_t half = (size_t)dm.B * dm.Tq * dm.F;
    for (int i = ty; i < 32; i += 8) {   // token-major read, coalesced along f
        const int t = t0 + i, f = f0 + tx;
        float c = 0.f, u = 0.f;
        if (t < dm.T && f < dm.F) {
            const size_t o = ((size_t)b * dm.Tq + dm.etd + t) * dm.F + f;
            c = x0tok[o];
            if (sp.guided) u = x0tok[half + o];
        }
        tc[i][tx] = c;
        tu[i][tx] = u;
    }
    __syncthreads();
    const int step = (sp.mode == 0) ? *d_step : 0;
    StepCoef k;
    if (sp.mode == 0) k = tab[step];
    const size_t FT = (size_t)dm.F * dm.T;
    const float sc = sp.guided ? scale[b] : 0.f;
    const int bn = noise_motion(sp, b);
    for (int i = ty; i < 32; i += 8) {   // boundary layout, coalesced along t
        const int f = f0 + i, t = t0 + tx;
        float nv = 0.f;
        if (f < dm.F && t < dm.T) {
            const size_t o = (size_t)b * FT + (size_t)f * dm.T + t;
            unsigned char im = 0;
            float iv = 0.f;
            if constexpr (INPAINT) {
                im = sp.inpaint_mask && sp.inpaint_mask[o];
                if (im) iv = sp.inpaint_motion[o];
            }
            float x0 = tc[tx][i];
            if (sp.guided) x0 = guide(x0, tu[tx][i], sc);
            x0 = pred_x0<INPAINT>(x0, im, iv, sp.clip);
            if (sp.x0_out) sp.x0_out[o] = x0;
            if (sp.mode == 0) {
                nv = sampler_next(k, sp.sampler, x0, sp.x[o], step_eps(sp, step, dm.B, FT, bn, f, dm.T, t));
                sp.x[o] = nv;
            }
        }
        tc[tx][i] = nv;
    }
    if (sp.mode != 0) return;
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int t = t0 + i, f = f0 + tx;
        if (t < dm.T && f < dm.F) {
            const int row = b * dm.Tq + dm.etd + t;
            if (xin) xin[(size_t)row * dm.F + f] = tc[i][tx];
            if (xp.hi) {
                plane_put(xp, row, f, tc[i][tx]);
                if (sp.guided) plane_put(xp, row + dm.B * dm.Tq, f, tc[i][tx]);   // uncond half sees the same x_t
            }
        }
    }
    if (threadIdx.x == 0) {   // two-level tickets: [1 + b] counts the blocks of sample b, the last of them arrives at [0] for its sample
        int* tick = d_step + 4;
        if (atomicAdd(tick + 1 + b, 1) == (int)(gridDim.x * gridDim.y) - 1) {
            tick[1 + b] = 0;
            step_ticket(tick, dm.B, d_step, step - 1);
        }
    }
}
hipError_t launch_update(const float* x0tok, const float* scale, const StepCoef* tab, int* d_step,
                         const SampleParams* sp, float* xin, Planes xp, const Dims& dm, int b0, int nb, hipStream_t s, bool inpaint) {
    dim3 grid((dm.T + 31) / 32, (dm.F + 31) / 32, nb);
    return dispatch_bools([&](auto INP) {
        hipLaunchKernelGGL(k_update<decltype(INP)::value>, grid, dim3(256), 0, s, x0tok, scale, tab, d_step, sp, xin, xp, dm, b0);
        return hipGetLastError();
    }, inpaint);
}

__global__ void k_advance(int* d_step) { *d_step -= 1; }
hipError_t launch_advance(int* d_step, hipStream_t s) {
    hipLaunchKernelGGL(k_advance, dim3(1), dim3(1), 0, s, d_step);
    return hipGetLastError();
}

// EmbedAction.forward (cmdm.py:363-365): out[b,:] = table[action[b],:]
__global__ void k_cond_rows(const float* __restrict__ table, const int64_t* __restrict__ action, float* __restrict__ out,
                            int B, int d, int num_actions) {
    const int b = blockIdx.x;
    long long a = action[b];
    a = a < 0 ? 0 : (a >= num_actions ? num_actions - 1 : a);   // never read outside the table (the Python boundary raises IndexError first)
    for (int c = threadIdx.x; c < d; c += blockDim.x) out[(size_t)b * d + c] = table[(size_t)a * d + c];
}
hipError_t launch_cond_rows(const float* table, const int64_t* action, float* out, int B, int d, int num_actions, hipStream_t s) {
    hipLaunchKernelGGL(k_cond_rows, dim3(B), dim3(256), 0, s, table, action, out, B, d, num_actions);
    return hipGetLastError();
}
__global__ void k_fill_rows(float* __restrict__ out, const float* __restrict__ row, int rows, int d) {
    const int r = blockIdx.x;
    for (int c = threadIdx.x; c < d; c += blockDim.x) out[(size_t)r * d + c] = row ? row[c] : 0.f;
}
// fp32 -> bf16 (round to nearest even), 8 values per thread: the bf16 copy of the hoisted condition rows k_step adds (rgn_step.hip)
__global__ void k_cvt_bf16(const float* __restrict__ in, __bf16* __restrict__ out, long long n8) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    const f32x4 a = reinterpret_cast<const f32x4*>(in)[2 * i], b = reinterpret_cast<const f32x4*>(in)[2 * i + 1];
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = (__bf16)a[e]; o[4 + e] = (__bf16)b[e]; }
    reinterpret_cast<bf16x8*>(out)[i] = o;
}
hipError_t launch_cvt_bf16(const float* in, __bf16* out, size_t n, hipStream_t s) {   // n % 8 == 0
    if (n == 0) return hipSuccess;
    const long long n8 = (long long)(n / 8);
    hipLaunchKernelGGL(k_cvt_bf16, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, in, out, n8);
    return hipGetLastError();
}
// fp32 -> fp16 (rne) and bf16 -> fp16 in place: the fp16-operand form of k_layers (rgn_layers.hip, LayersArgs::f16) reads its condition rows and
// the residual-stream planes the up-front embedding wrote in that format (a bf16 value inside fp16's normal range converts exactly)
__global__ void k_cvt_f16(const float* __restrict__ in, _Float16* __restrict__ out, long long n8) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    const f32x4 a = reinterpret_cast<const f32x4*>(in)[2 * i], b = reinterpret_cast<const f32x4*>(in)[2 * i + 1];
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = (_Float16)a[e]; o[4 + e] = (_Float16)b[e]; }
    reinterpret_cast<f16x8*>(out)[i] = o;
}
__global__ void k_bf16_to_f16(__bf16* __restrict__ io, long long n8) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    const bf16x8 a = reinterpret_cast<const bf16x8*>(io)[i];
    f16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (_Float16)(float)a[e];
    reinterpret_cast<f16x8*>(io)[i] = o;
}
hipError_t launch_cvt_f16(const float* in, _Float16* out, size_t n, hipStream_t s) {   // n % 8 == 0
    if (n == 0) return hipSuccess;
    const long long n8 = (long long)(n / 8);
    hipLaunchKernelGGL(k_cvt_f16, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, in, out, n8);
    return hipGetLastError();
}
hipError_t launch_bf16_to_f16(__bf16* inout, size_t n, hipStream_t s) {   // n % 8 == 0
    if (n == 0) return hipSuccess;
    const long long n8 = (long long)(n / 8);
    hipLaunchKernelGGL(k_bf16_to_f16, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, inout, n8);
    return hipGetLastError();
}
hipError_t launch_fill_rows(float* out, const float* row, int rows, int d, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fill_rows, dim3(rows), dim3(256), 0, s, out, row, rows, d);
    return hipGetLastError();
}

// =================================================================================================
// next-1 row: rotation_6d_to_matrix (utils/rotation_conversions.py:513-534) — Gram-Schmidt.
// F.normalize semantics: v / max(||v||, 1e-12).
// =================================================================================================
__global__ void k_rot6d(const float* __restrict__ d6, float* __restrict__ mat, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = d6 + i * 6;
    float a1x = p[0], a1y = p[1], a1z = p[2], a2x = p[3], a2y = p[4], a2z = p[5];
    rot6d_to_matrix(a1x, a1y, a1z, a2x, a2y, a2z, mat + i * 9);       // (rgn_device.h: shared with the forward-kinematics kernel, rgn_fk.hip)
}
hipError_t launch_rot6d(const float* d6, float* mat, long long n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rot6d, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d6, mat, n);
    return hipGetLastError();
}

// next-2 row: scipy.ndimage.gaussian_filter1d(x, sigma, axis=-1, mode='reflect', truncate=4)
// (sample/cgenerate.py:142). One thread per output sample; taps recomputed (<= 2*4*sigma+1 of them).
__global__ void k_gauss1d(const float* __restrict__ x, float* __restrict__ out, long long rows, int T, float sigma,
                          int radius) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * T) return;
    const long long r = idx / T;
    const int t = (int)(idx - r * T);
    const float* xr = x + r * T;
    double wsum = 0.0, acc = 0.0;
    const double s2 = -0.5 / ((double)sigma * sigma);
    const int period = 2 * T;
    for (int j = -radius; j <= radius; ++j) {
        const double w = exp(s2 * j * j);
        int q = (t + j) % period;
        if (q < 0) q += period;
        if (q >= T) q = period - 1 - q;
        wsum += w;
        acc += w * (double)xr[q];
    }
    out[idx] = (float)(acc / wsum);
}
hipError_t launch_gauss1d(const float* x, float* out, long long rows, int T, float sigma, hipStream_t s) {
    const long long n = rows * T;
    if (n <= 0) return hipSuccess;
    const int radius = (int)(4.0f * sigma + 0.5f);
    hipLaunchKernelGGL(k_gauss1d, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, out, rows, T, sigma, radius);
    return hipGetLastError();
}

}  // namespace rgn
