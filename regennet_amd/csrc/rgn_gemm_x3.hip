// Split-bf16 ("bf16x3") MFMA GEMM on PRE-SPLIT operands — the dominant kernel of the hot path.
//
//   C[M,N] = act( (Ahi+Alo)[M,K] . (Whi+Wlo)[N,K]^T + bias + add )     with  a.b ~ ah.bh + ah.bl + al.bh
//
// Every activation that feeds a GEMM is stored by its producer as two bf16 planes (hi = rne(x),
// lo = rne(x - hi)), so this kernel is a pure bf16 GEMM with four operand planes: no VALU conversion in
// the main loop and all four planes go HBM/L2 -> LDS by direct-to-LDS DMA (global_load_lds_dwordx4,
// 1 KiB per wave-instruction, no VGPR round trip).
//
// Operand memory layout: the K32-blocked planes [Kp/32][rows][32] of rgn_layout.h (plane_off), so the [rows x 32] slice a
// block needs for one k-step is ONE contiguous run of 64-byte rows: every DMA wave-instruction (16 rows x 64 B) reads a
// contiguous, 1 KiB-aligned span = 8 full 128-byte lines. (With a plain row-major [rows][K] plane each instruction would
// touch 16 half-used lines.) The producers (LayerNorm, GEMM epilogues, attention, sampler update) write this layout directly.
//
// LDS image of one plane tile: the swizzled image of rgn_layout.h, written lane-linear by the DMA. The chunk permutation that
// makes the ds_read_b128 fragment reads conflict-free is applied to the per-lane global SOURCE address (img_dma_chunk) and
// again on the read (img_frag): the both-sides-or-neither rule for global_load_lds.
//
// Loop (shipped flavour): 128x128 tile, 4 waves, 2 LDS stages of 32 KiB -> two workgroups per CU, one hiding the
// other's barriers and epilogue. Per k-step: issue tile kt+1's DMA, counted wait (vmcnt) for tile kt, barrier, fragments
// + 24 MFMAs per wave, barrier. Measured with per-step cycle stamps (tools/gemm_bench -DRGN_GEMM_PROF): the step is
// bound by the ~20 B/clk a CU can pull from L2 through the vector-memory path (the 64 KiB the two resident workgroups
// request per step take ~3000 clk to land, the MFMAs ~1500), not by the matrix pipe. A 256x256 / 8-wave tile with one
// barrier per step and the DMA issued between MFMA groups (ILV = true, tools only) halves the bytes per MFMA and its
// loop runs at ~80 % MFMA occupancy, but at M = 15360 it leaves only 120-240 tiles for 256 CUs and nothing to hide its
// 256 KiB-per-tile epilogue behind: end to end it only ties (70 vs 72 us on linear1), so it is not shipped.
//
// The product of a fragment pair, the MFMA groups of the interleaved k-step, the fragment offsets and the paired-column plane store are the family's
// (rgn_dma_gemm.h: this kernel is the ancestor of the recogniser's three in rgn_sg_kernels.hip); here stand the stage DMA, the two loops and x3_epilogue.
#include <algorithm>
#include <cstdlib>
#include "rgn_dma_gemm.h"

#include <hip/hip_runtime.h>

namespace rgn {

__device__ __forceinline__ float x3_act(float v, int act) {
    if (act == 1) return gelu_as(v);
    if (act == 2) return v / (1.0f + __expf(-v));
    if (act == 3) return fmaxf(v, 0.f);
    return v;
}

// ---- epilogue ------------------------------------------------------------------------------------------
// Straight from the MFMA C/D layout (col = lane&31, row = (i&3) + 8*(i>>2) + 4*(lane>>5)): for a fixed register
// the two half-waves write two full 128-byte row segments (fp32) or two 64-byte segments of the K32-blocked bf16
// planes. Interior blocks take a branch-free path (CHECK = false): one pointer per tile, constant row strides,
// residual loads batched per tile; only edge blocks pay per-element bounds checks.
// mw / nw: first row / column of this wave's TM x TN tiles of 32x32.
// EPI: 0 plain, 1 the attention-ready scatter of the packed in_proj output, 2 the ST-GCN evaluator's GEMMs ((row % add_mod) addend)
template <int TM, int TN, int EPI, bool CHECK>
__device__ __forceinline__ void x3_epilogue(const GemmX3Args& g, f32x16 (&acc)[TM][TN], int mw, int nw, int lane) {
    constexpr bool QKV = EPI == 1;
    const int l31 = lane & 31, kh = lane >> 5;
        #pragma unroll
    for (int tb = 0; tb < TN; ++tb) {
        const int n = nw + tb * 32 + l31;
        const bool n_ok = !CHECK || n < g.N;
        const float bias = (g.bias && n_ok) ? g.bias[n] : 0.f;
#pragma unroll
        for (int ta = 0; ta < TM; ++ta) {
            const int mb = mw + ta * 32 + 4 * kh;      // row of register 0
            float r[16];
            if (EPI == 2 && g.add && g.add_mod > 0) {      // addend row = row % add_mod (a per-vertex bias: rows run (frame, vertex); add_mod >= 28)
                // (= dg_vertex_addend, spelled out: behind the function the 256 x 128 form takes 13 more VGPRs)
                const int base = (int)((unsigned)mb % (unsigned)g.add_mod);
                const float* ap = g.add + n;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    int rr = base + mfma32_row(i, 0);
                    rr = rr >= g.add_mod ? rr - g.add_mod : rr;
                    r[i] = n_ok ? ap[rr * g.ldadd] : 0.f;
                }
            } else if (g.add) {
                const float* ap = g.add + (size_t)mb * g.ldadd + n;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int ro = mfma32_row(i, 0);
                    r[i] = (!CHECK || (n_ok && mb + ro < g.M)) ? ap[(size_t)ro * g.ldadd] : 0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                float v = acc[ta][tb][i] + bias;
                if (g.add) v += r[i];
                r[i] = x3_act(v, g.act);
            }
            if constexpr (QKV) {   // attention-ready scatter of the packed in_proj output (see GemmX3Args)
                const int which = n / g.d, cin = n - which * g.d, hd = cin / g.dh, c = cin - hd * g.dh;
                __bf16* ph = which == 0 ? g.Qhi : (which == 1 ? g.Khi : g.Vthi);
                __bf16* pl = which == 0 ? g.Qlo : (which == 1 ? g.Klo : g.Vtlo);
                if (!CHECK) {                                          // pair adjacent columns across lane^1 -> 4-byte stores
                    const float sc = which == 0 ? g.qscale : 1.0f;
                    const bool odd = lane & 1;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        float c0, c1;
                        dg_pair_exchange((odd ? r[i + 8] : r[i]) * sc, (odd ? r[i] : r[i + 8]) * sc, odd, c0, c1);
                        const unsigned m = (unsigned)(mb + dg_pair_row(i, odd));
                        // m / Tq, m % Tq (exact: m*Tq < 2^32); Tq = 1 has no 32-bit magic (floor(2^32 / 1) + 1 wraps to 1): the quotient is m itself
                        const unsigned bb = g.Tq == 1 ? m : __umulhi(m, g.tq_magic), tt = m - bb * (unsigned)g.Tq;
                        dg_store_pair<false, true>(ph, pl, attn_slab_off(g.H, g.Tqp, g.dh, bb, hd, tt, c & ~1), c0, c1);
                    }
                } else {                                              // edge blocks
                    const float sc = which == 0 ? g.qscale : 1.0f;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int m = mb + mfma32_row(i, 0);
                        if (!n_ok || m >= g.M) continue;
                        const int bb = m / g.Tq, tt = m - bb * g.Tq;
                        const float x = r[i] * sc;
                        const __bf16 h = (__bf16)x;
                        const size_t o = attn_slab_off(g.H, g.Tqp, g.dh, bb, hd, tt, c);
                        ph[o] = h;
                        if (pl) pl[o] = (__bf16)(x - (float)h);
                    }
                }
            }
            if (!QKV && g.C) {
                float* cp = g.C + (size_t)mb * g.ldc + n;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int ro = mfma32_row(i, 0);
                    if (!CHECK || (n_ok && mb + ro < g.M)) cp[(size_t)ro * g.ldc] = r[i];
                }
            }
            if (!QKV && g.Chi) {   // K32-blocked planes [N/32][c_rows][32]: a 32-column tile is one contiguous run of rows
                if (!CHECK) {
                    const size_t o = plane_off(g.c_rows, mb, n & ~1);
                    const bool odd = lane & 1;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        float c0, c1;
                        dg_pair_columns(r, i, odd, c0, c1);
                        dg_store_pair<false, true>(g.Chi, g.Clo, o + dg_pair_row(i, odd) * 32, c0, c1);
                    }
                } else {
                    const size_t o = plane_off(g.c_rows, mb, n);
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int ro = mfma32_row(i, 0);
                        if (n_ok && mb + ro < g.M) {
                            const __bf16 h = (__bf16)r[i];
                            g.Chi[o + ro * 32] = h;
                            if (g.Clo) g.Clo[o + ro * 32] = (__bf16)(r[i] - (float)h);
                        }
                    }
                }
            }
        }
    }
}

#ifdef RGN_GEMM_PROF
__device__ long long g_prof[1024];   // tools only: per-k-step cycle stamps of one workgroup
#endif

// BM x BN block tile, WM x WN waves, each wave (BM/WM) x (BN/WN) = TM x TN tiles of 32x32.
// ILV = false: two barriers per k-step, the whole next tile's DMA issued at the top of the step (128x128, 2 WG / CU).
// ILV = true : one barrier per k-step, DMA pieces interleaved with the MFMAs of the first K half, fragments fetched one
//              MFMA group ahead (256x256, 1 WG / CU).
template <int BM, int BN, int WM, int WN, bool X3, bool ILV, int EPI>
__global__ __launch_bounds__(64 * WM * WN, (2 * 2 * (BM + BN) * 64 <= 80 * 1024) ? 2 : 1) void k_gemm_x3(GemmX3Args g, int nbx, int nby) {
    constexpr int NT = 64 * WM * WN;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int NPL = X3 ? 2 : 1;                         // planes per operand
    constexpr int A_BYTES = BM * 64, W_BYTES = BN * 64;     // one plane tile (32 bf16 per row)
    constexpr int STAGE = NPL * (A_BYTES + W_BYTES);
    constexpr int A_IT = BM * 4 / NT, W_IT = BN * 4 / NT;   // DMA instructions per thread per plane
    constexpr int LPT = NPL * (A_IT + W_IT);                // ... per thread per tile
    static_assert(BM * 4 % NT == 0 && BN * 4 % NT == 0, "tile/threads mismatch");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][Ahi|Alo|Whi|Wlo]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const DgTile t = dg_tile<BM, BN>(xcd_affine(blockIdx.x, nbx * nby), nbx);
    const int m0 = t.m0, n0 = t.n0;

    // per-thread DMA source byte offsets inside one k-block of a plane (k-invariant, 32-bit: a plane k-block is
    // rows x 64 B); the k-dependent part is a wave-uniform base pointer, so the DMA uses the SGPR-base + VGPR-offset form
    unsigned a_src[A_IT], w_src[W_IT];
#pragma unroll
    for (int it = 0; it < A_IT; ++it) {
        const int q = it * NT + tid, r = q >> 2, c = img_dma_chunk(r, q & 3);
        int m = m0 + r;
        m = m < g.M ? m : g.M - 1;
        a_src[it] = (unsigned)m * 64u + c * 16u;
    }
#pragma unroll
    for (int it = 0; it < W_IT; ++it) {
        const int q = it * NT + tid, r = q >> 2, c = img_dma_chunk(r, q & 3);
        int n = n0 + r;
        n = n < g.N ? n : g.N - 1;
        w_src[it] = (unsigned)n * 64u + c * 16u;
    }
    // DMA piece idx of tile kt into stage buffer sb (idx is a compile-time constant after unrolling)
    auto piece = [&](int idx, int kt, char* sb) {
        ptrdiff_t ka = (ptrdiff_t)kt * g.a_rows * 64;
        if constexpr (EPI == 2) {   // temporal convolution as one GEMM: k-block -> (tap, channel block), the tap shifts the rows
            if (g.a_taps > 0) {
                const int cb = kt / g.a_taps;
                ka = (ptrdiff_t)cb * g.a_rows * 64 + (ptrdiff_t)g.a_tap[kt - cb * g.a_taps];
            }
        }
        const size_t kw = (size_t)kt * g.N * 64;
        if (idx < NPL * A_IT) {
            const int it = idx / NPL, pl = idx % NPL;
            const int lo = (it * NT + (tid & ~63)) * 16;   // wave-uniform LDS byte offset of this 1 KiB piece
            const char* base = reinterpret_cast<const char*>(pl ? g.Alo : g.Ahi) + ka;
            __builtin_amdgcn_global_load_lds((const RGN_AS1 void*)(base + a_src[it]), (RGN_AS3 void*)(sb + pl * A_BYTES + lo), 16, 0, 0);
        } else {
            const int j = idx - NPL * A_IT, it = j / NPL, pl = j % NPL;
            const int lo = (it * NT + (tid & ~63)) * 16;
            const char* base = reinterpret_cast<const char*>(pl ? g.Wlo : g.Whi) + kw;
            __builtin_amdgcn_global_load_lds((const RGN_AS1 void*)(base + w_src[it]), (RGN_AS3 void*)(sb + NPL * A_BYTES + pl * W_BYTES + lo), 16, 0, 0);
        }
    };
    auto issue = [&](int kt, int stage) {
#pragma unroll
        for (int idx = 0; idx < LPT; ++idx) piece(idx, kt, smem + stage * STAGE);
    };

    f32x16 acc[TM][TN];
    dg_zero(acc);
    // fragment read offsets of this wave's rows within the block tile
    const int l31 = lane & 31, kh = lane >> 5;
    int a_off[TM][2], w_off[TN][2];
    dg_frag_off(a_off, wm * (BM / WM), l31, kh);
    dg_frag_off(w_off, wn * (BN / WN), l31, kh);

#ifdef RGN_GEMM_PROF
    const bool prof = ((int)blockIdx.x == RGN_GEMM_PROF) && (tid == 0 || tid == NT - 64);
    long long* pp = g_prof + (tid ? 512 : 0);
#define RGN_T(i) if (prof) pp[kt * 6 + i] = clock64();
#else
#define RGN_T(i)
#endif
    const int nk = g.Kp / 32;
    if constexpr (ILV) {
        constexpr int PPG = (LPT + TN - 1) / TN;                 // DMA pieces after each MFMA group of the first K half
        auto step = [&](int kt, bool more) {
            const char* sb = smem + (kt & 1) * STAGE;
            char* nb = smem + ((kt + 1) & 1) * STAGE;
            auto a_frag = [&](int ks, bf16x8 (&ah)[2][TM], bf16x8 (&al)[2][TM]) {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    ah[ks][i] = *reinterpret_cast<const bf16x8*>(sb + a_off[i][ks]);
                    if (X3) al[ks][i] = *reinterpret_cast<const bf16x8*>(sb + A_BYTES + a_off[i][ks]);
                }
            };
            dg_kstep<TM, TN, false, X3>(acc, sb + NPL * A_BYTES, W_BYTES, w_off, a_frag, [&](int grp) {
                if (grp < TN && more) {
#pragma unroll
                    for (int q = 0; q < PPG; ++q)
                        if (grp * PPG + q < LPT) piece(grp * PPG + q, kt + 1, nb);
                }
            });
        };
        issue(0, 0);
        for (int kt = 0; kt < nk; ++kt) {
            RGN_T(0)
            wait_vmcnt<0>();                      // my pieces of tile kt landed
            RGN_T(1)
            __builtin_amdgcn_s_barrier();         // ... everyone's did, and everyone is done reading tile kt-1's stage
            RGN_T(2)
            step(kt, kt + 1 < nk);
            RGN_T(3)
            RGN_T(4)
            RGN_T(5)
        }
    } else {
        auto compute = [&](const char* sb) {
            bf16x8 ah[2][TM], al[2][TM], wh[2][TN], wl[2][TN];
            auto frags = [&](int ks, int buf) {
#pragma unroll
                for (int t = 0; t < TM; ++t) {
                    ah[buf][t] = *reinterpret_cast<const bf16x8*>(sb + a_off[t][ks]);
                    if (X3) al[buf][t] = *reinterpret_cast<const bf16x8*>(sb + A_BYTES + a_off[t][ks]);
                }
#pragma unroll
                for (int t = 0; t < TN; ++t) {
                    wh[buf][t] = *reinterpret_cast<const bf16x8*>(sb + NPL * A_BYTES + w_off[t][ks]);
                    if (X3) wl[buf][t] = *reinterpret_cast<const bf16x8*>(sb + NPL * A_BYTES + W_BYTES + w_off[t][ks]);
                }
            };
            frags(0, 0);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                if (ks == 0) frags(1, 1);
#pragma unroll
                for (int ta = 0; ta < TM; ++ta)
#pragma unroll
                    for (int tb = 0; tb < TN; ++tb) dg_mma<false, X3>(acc[ta][tb], ah[ks][ta], al[ks][ta], wh[ks][tb], wl[ks][tb]);
            }
        };
        issue(0, 0);
        for (int kt = 0; kt < nk; ++kt) {
            RGN_T(0)
            if (kt + 1 < nk) {
                issue(kt + 1, (kt + 1) & 1);
                RGN_T(1)
                wait_vmcnt<LPT>();                // tile kt landed, tile kt+1 stays in flight
            } else {
                RGN_T(1)
                wait_vmcnt<0>();
            }
            RGN_T(2)
            __builtin_amdgcn_s_barrier();
            RGN_T(3)
            compute(smem + (kt & 1) * STAGE);
            wait_lgkmcnt<0>();
            RGN_T(4)
            __builtin_amdgcn_s_barrier();         // stage (kt&1) may now be overwritten by tile kt+2
            RGN_T(5)
        }
    }
#undef RGN_T

    const bool interior = (m0 + BM <= g.M) && (n0 + BN <= g.N);   // (= dg_close, spelled out: through its visitor the 128 x 128 forms take 4 more SGPRs, the 256 x 256 plain form 3 fewer VGPRs)
    if (interior) x3_epilogue<TM, TN, EPI, false>(g, acc, m0 + wm * (BM / WM), n0 + wn * (BN / WN), lane);
    else x3_epilogue<TM, TN, EPI, true>(g, acc, m0 + wm * (BM / WM), n0 + wn * (BN / WN), lane);
}

// k_gemm_x3's forms for one tile shape, named once: fn(kernel, planes per operand) for (arithmetic, attention-ready scatter). The scatter exists for the
// default tile only
template <int BM, int BN, int WM, int WN, bool ILV>
constexpr bool x3_form_exists(bool qkv) { return !qkv || (BM == 128 && !ILV); }
template <int BM, int BN, int WM, int WN, bool ILV, class Fn>
static hipError_t x3_form(bool x3, bool qkv, Fn fn) {
    return dispatch_bools([&](auto X, auto Q) {
        if constexpr (x3_form_exists<BM, BN, WM, WN, ILV>(decltype(Q)::value))
            return fn(k_gemm_x3<BM, BN, WM, WN, decltype(X)::value, ILV, decltype(Q)::value ? 1 : 0>, decltype(X)::value ? 2 : 1);
        else
            return hipErrorInvalidValue;
    }, x3, qkv);
}
template <int BM, int BN, int WM, int WN, bool ILV>
static hipError_t x3_launch(const GemmX3Args& g, bool x3, hipStream_t s, bool configure_only) {
    if (configure_only) {
        hipError_t e = hipSuccess;
        for (int m = 0; m < 4 && e == hipSuccess; ++m)
            if (x3_form_exists<BM, BN, WM, WN, ILV>(m & 2))
                e = x3_form<BM, BN, WM, WN, ILV>(m & 1, m & 2, [](auto kern, int npl) {
                    return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * npl * (BM * 64 + BN * 64));
                });
        return e;
    }
    return x3_form<BM, BN, WM, WN, ILV>(x3, g.Qhi != nullptr, [&](auto kern, int npl) {
        const int nbx = (g.N + BN - 1) / BN, nby = (g.M + BM - 1) / BM;
        hipLaunchKernelGGL(kern, dim3(nbx * nby), dim3(64 * WM * WN), 2 * npl * (BM * 64 + BN * 64), s, g, nbx, nby);
        return hipGetLastError();
    });
}

// ---- the ST-GCN evaluator's GEMMs (rgn_stgcn.hip): millions of rows x 64 / 128 / 256 channels, split-bf16 throughout. 256-row tiles with
//      the interleaved one-barrier loop; the tile is as wide as the layer (a 64-channel layer on a 128-wide tile would idle half its MFMAs).
//      256 channels: two 128-wide column blocks. The 256-wide tile (123 spilled SGPRs + 576 B of scratch in this form) was measured anyway: 23.2 / 53.2 ms
//      per forward at 60 / 150 frames against 23.0 / 53.2 - the wide blocks are not bound by operand bytes per MFMA (profiles/r05/sg_tile256.txt)
template <class Fn>
static hipError_t x3_sg_form(bool narrow, Fn fn) {           // the two forms, named once: fn(kernel, BN, threads)
    return narrow ? fn(k_gemm_x3<256, 64, 4, 1, true, true, 2>, 64, 256) : fn(k_gemm_x3<256, 128, 4, 2, true, true, 2>, 128, 512);
}
hipError_t launch_gemm_x3_sg(const GemmX3Args& g, hipStream_t s) {
    return x3_sg_form(g.N <= 64, [&](auto kern, int BN, int threads) {
        const int nbx = (g.N + BN - 1) / BN, nby = (g.M + 255) / 256;
        hipLaunchKernelGGL(kern, dim3(nbx * nby), dim3(threads), 2 * 2 * (256 * 64 + BN * 64), s, g, nbx, nby);
        return hipGetLastError();
    });
}
hipError_t configure_gemm_x3_sg() {
    hipError_t e = hipSuccess;
    for (int narrow = 0; narrow < 2 && e == hipSuccess; ++narrow)
        e = x3_sg_form(narrow, [](auto kern, int BN, int) { return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 2 * (256 * 64 + BN * 64)); });
    return e;
}

// variant 0 = 128x128 / 4 waves (two workgroups per CU): the default. variant 1 = 256x256 / 8 waves / interleaved DMA (one
// workgroup per CU): its loop is ~1.45x faster per output but it needs several tiles per CU to hide its 256 KiB-per-tile
// epilogue, so the engine picks it only for launches of >= 7000 rows per chain (rgn_plan.cpp). tools/gemm_bench builds
// with RGN_GEMM_TOOLS and can also time 2 = 256x256 with the two-barrier loop, 3 = 128x128 with the interleaved loop,
// 4 / 5 = 128x256 / 256x128 interleaved.
hipError_t launch_gemm_x3(const GemmX3Args& g, bool x3, int variant, hipStream_t s) {
    if (variant == 1) return x3_launch<256, 256, 4, 2, true>(g, x3, s, false);
#ifdef RGN_GEMM_TOOLS
    if (variant == 2) return x3_launch<256, 256, 4, 2, false>(g, x3, s, false);
    if (variant == 3) return x3_launch<128, 128, 2, 2, true>(g, x3, s, false);
    if (variant == 4) return x3_launch<128, 256, 2, 4, true>(g, x3, s, false);
    if (variant == 5) return x3_launch<256, 128, 4, 2, true>(g, x3, s, false);
#endif
    return x3_launch<128, 128, 2, 2, false>(g, x3, s, false);
}
hipError_t configure_gemm_x3() {
    GemmX3Args g{};
    hipError_t e = x3_launch<128, 128, 2, 2, false>(g, true, nullptr, true);
    if (e != hipSuccess) return e;
#ifdef RGN_GEMM_TOOLS
    e = x3_launch<256, 256, 4, 2, false>(g, true, nullptr, true);
    if (e != hipSuccess) return e;
    e = x3_launch<128, 128, 2, 2, true>(g, true, nullptr, true);
    if (e != hipSuccess) return e;
    e = x3_launch<128, 256, 2, 4, true>(g, true, nullptr, true);
    if (e != hipSuccess) return e;
    e = x3_launch<256, 128, 4, 2, true>(g, true, nullptr, true);
#endif
    if (e != hipSuccess) return e;
    return x3_launch<256, 256, 4, 2, true>(g, true, nullptr, true);
}

#ifdef RGN_GEMM_PROF
void gemm_prof_read(long long* out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), sizeof(long long) * 1024); }
#endif

}  // namespace rgn
