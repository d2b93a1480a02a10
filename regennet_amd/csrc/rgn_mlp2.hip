// Row-persistent decoder-layer tail for the plain-bf16 phase (second build: round 2's k_mlp is gone, its measurements are DESIGN.md 4.0b): for a tile of R
// complete token rows ONE workgroup runs
//
//   h' = LN2( LN1( att . Wo^T + bo + h ) + call_time[step] + call_cond[sample] )        out_proj, norm1, folded cross-attn, norm2
//   y  = LN3( gelu( h' . W1^T + b1 ) . W2^T + b2 + h' )                                 linear1, GELU, linear2, norm3
//
// (nn.TransformerDecoderLayer post-norm blocks constructed at model/cmdm.py:75-81, called at :227) with every intermediate on chip.
// R = 64 rows, 8 waves, wave w = output columns [64 w, 64 w + 64) (MT x NT = 2 x 2 accumulator tiles of 32 x 32), one workgroup per
// CU - a weight fragment feeds two MFMAs. (A 32-row form with two workgroups per CU streams twice the weights per row and lost
// wherever the 64-row tiles fill the chip: DESIGN.md 4.0b2.)
// What changed against round 2's k_mlp (all measured in the sampling loop):
//   * the layer input tile h (residual of norm1) never touches LDS: every lane loads the 64 values it will add straight into
//     registers BEHIND the att DMA and the first weight fragments, and the first MFMA waits for the att tile only
//   * ONE continuous weight stream: buffer loads (scalar resource + compile-time offsets, the lane contributes lane * 16), a ring of
//     half-k-step granules that never drains between the five GEMM passes - the tail of a pass requests the head of the next one, so
//     the epilogues run with the next pass's first fragments in flight
//   * per-column vectors: every wave stages ITS OWN column slices (wave-private LDS, no barrier); phase A (out_proj bias, norm1 /
//     norm2, per-sample vectors) is overwritten by phase B (linear1 / linear2 biases, norm3) once the wave is past norm2
//   * LayerNorm statistics as sum and sum of squares in ONE exchange (fp32; plain-bf16 phase only - the split-bf16 tail keeps the
//     two-pass kernels), mean folded into the final FMA; exchange layout [stat][wave][token]: conflict-free both ways
// The machinery of all that - tile geometry, weight ring and GEMM pass, LayerNorm, epilogue sweeps, the FFN stage - is rgn_tail.h, shared with
// k_layers (rgn_layers.hip); this file keeps the kernel's own stage 1 (att DMA, residual tile in registers, per-sample vectors, ENC) and stage 3.
//   LDS X: att tile image (A operand of out_proj) -> GELU(hidden half) image (A operand of linear2) -> output image
//   LDS Y: h' image (A operand of linear1, residual of norm3)
#include "rgn_internal.h"
#include "rgn_tail.h"

#include <hip/hip_runtime.h>

#include <type_traits>

namespace rgn {

#ifndef RGN_M2_HRES
#define RGN_M2_HRES 0      // where the residual tile is requested: 0 = in the prologue behind the att DMA, 1 = behind the att barrier
#endif
#ifndef RGN_M2_ST_AUX
#define RGN_M2_ST_AUX 16   // output stores write-through (sc1): nothing left dirty in the XCD L2s for the end-of-kernel write-back
#endif

struct M2 {
    static constexpr int MT = 2;                      // row tiles of 32 per workgroup
    static constexpr int R = 32 * MT, NW = 4 * MT, NTH = 64 * NW, NT = 4 / MT, CW = 512 / NW;   // rows, waves, threads, column blocks and columns per wave
    static constexpr int RD = 4 * MT;                 // weight ring depth in granules (half k-steps of NT fragments): 64 registers
    static constexpr int KB = R * 64, IMG = 16 * KB;  // bytes of one k-block [R rows][64 B] and of an image
    static constexpr int NSAMP = 4;                   // samples a tile can touch (mlp_supported)
    // LDS map: X | Y | statistics exchange (2 buffers x [2 stats][NW waves][R tokens]) | NW wave-private vector regions
    static constexpr int X = 0, Y = IMG, RED = 2 * IMG, REDF = 2 * NW * R, VEC = RED + 2 * REDF * 4, VECW = (4 + NSAMP) * CW, LDS = VEC + NW * VECW * 4;
    // wave-private vector region (floats): phase A (stage 1) and phase B (stages 2, 3)
    static constexpr int A_BO = 0, A_G1 = CW, A_G2 = 2 * CW, A_B2 = 3 * CW, A_SPV = 4 * CW /* NSAMP x CW */;
    static constexpr int B_BF1 = 0 /* 2 x CW: hidden halves */, B_BF2 = 2 * CW, B_G3 = 3 * CW, B_B3 = 4 * CW;
    static_assert(32 % RD == 0, "ring slots continue across passes");
    static_assert(LDS == 152 * 1024, "LDS map");
};

#ifdef RGN_M2_STAMPS
// tools/mlp_bench -DRGN_M2_STAMPS: wave 0 of EVERY workgroup stamps s_memtime at the phase boundaries, plus where it runs
// (HW_ID: SIMD / CU / SE, XCC_ID), so that the host can put the workgroups of one CU next to each other
__device__ long long g_m2_st[1024][12];
#define RGN_M2T(i)                                                                                                  \
    {                                                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                                          \
        if (threadIdx.x == 0 && blockIdx.x < 1024) {                                                                \
            g_m2_st[blockIdx.x][i] = __builtin_readcyclecounter();                                                  \
            if (i == 0) {                                                                                           \
                unsigned hw, xcc;                                                                                   \
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));                                    \
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));                                  \
                g_m2_st[blockIdx.x][10] = hw;                                                                       \
                g_m2_st[blockIdx.x][11] = xcc;                                                                       \
            }                                                                                                       \
        }                                                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                                          \
    }
#else
#define RGN_M2T(i)
#endif

// ENC = true: the encoder-layer tail of arch='offline' (as k_mlp_x3<true>): h' = LN1(att . Wo^T + bo + h), final norm from g3 / b3; g2, b2,
// pervec and stepvec are not read.
template <bool F16 = false, bool ENC = false>
__global__ __launch_bounds__(M2::NTH, 2) void k_mlp2(MlpArgs g) {
    using C = M2;
    using OP = OpFmt<F16>;                // bf16 or fp16 operands (rgn_device.h): planes in, planes out, weight planes
    using op8 = typename OP::v8;
    using op4 = typename OP::v4;
    constexpr int MT = C::MT, NT = C::NT, NW = C::NW, R = C::R, CW = C::CW, RD = C::RD, KB = C::KB, NSAMP = C::NSAMP, VK = CW / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, kh = lane >> 5;
    const int m0 = xcd_affine(blockIdx.x, gridDim.x) * R;
    float* vec = reinterpret_cast<float*>(smem + C::VEC) + wave * C::VECW;   // this wave's private region
    RGN_M2T(0)
    // ---- att tile -> X by DMA: 16 k-blocks x R/16 pieces of 1 KiB (16 rows x 64 B), wave w issues the pieces w, w + NW, ...
    static_assert(R == 64, "tile_dma_in: tiles of 64 rows");
    tile_dma_in<0, 16, NW>(smem + C::X, g.att, g.rows, m0, g.M - m0, lane, wave);
    // ---- the layer tail's shared machinery (rgn_tail.h): accumulator <-> image map, weight ring, GEMM pass, LayerNorm, epilogue sweeps, FFN stage
    using Pass = TailPass;
    const TailLane tl = tail_lane<C>(smem, lane, wave);
    int a_offx[2], a_offy[2];                                        // B-operand fragment offsets into the images X and Y
    static_assert(C::X == 0, "a_offx addresses the image at byte 0");
    tail_a_off(a_offx, lane);
    tail_a_off(a_offy, a_offx, C::Y);
    op8 wf[RD][NT];                                                  // the weight ring

    // =============== stage 1: out_proj + residual + norm1 + folded cross-attention + norm2 -> h' (Y) ====================
    const Pass p_wo{tail_wrs(g.w.Wo, NT * wave, 512 * 512 * 2), 16 * 2048, 0}, p_w1a{tail_wrs(g.w.W1, NT * wave, 1024 * 512 * 2), 32 * 2048, 0},
        p_w1b{tail_wrs(g.w.W1, 16 + NT * wave, 1024 * 512 * 2), 32 * 2048, 0}, p_w2a{tail_wrs(g.w.W2, NT * wave, 512 * 1024 * 2), 16 * 2048, 0},
        p_w2b{p_w2a.rs, 16 * 2048, 32};
    f32x16 acc[NT][MT];
#pragma unroll
    for (int s = 0; s < RD - 1; ++s) tail_load_g<OP, C>(wf, tl, p_wo, s, s);           // right behind the att DMA: the first MFMA needs both, and nothing else
    RGN_M2T(6)
    const int cw = CW * wave + lane;                                 // this lane's column(s) of every vector slice: cw (+ 64)
    // phase A vectors of the wave's columns: requested now, staged to the wave's LDS region after the out_proj loop - nothing
    // before the first MFMA depends on them (the accumulators start from zero; out_proj's bias is added with the residual)
    float va[4][VK], sv[VK], pv[NSAMP][VK];
    int step = 0;
    {
        const float* srcA[4] = {g.w.bo, g.w.g1, g.w.g2, g.w.b2};
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int k = 0; k < VK; ++k) va[v][k] = (ENC && v >= 2) ? 0.f : srcA[v][cw + 64 * k];
        if (!ENC && g.stepvec) step = *g.d_step;
        const int s0 = m0 / g.Tq, slast = (g.M - 1) / g.Tq;
#pragma unroll
        for (int k = 0; k < VK; ++k) {
            sv[k] = g.w.b1[cw + 64 * k];                             // norm1's beta, folded into the per-sample vector
#pragma unroll
            for (int j = 0; j < NSAMP; ++j) {
                const int sidx = s0 + j < slast ? s0 + j : slast;
                pv[j][k] = (!ENC && g.pervec) ? g.pervec[(size_t)sidx * g.ldper + cw + 64 * k] : 0.f;
            }
        }
    }
    asm volatile("" ::: "memory");
    // the residual tile straight into registers (needed after the loop: NOT waited for before the first MFMA), then phase B
    op4 hres[NT][MT][4];
    auto load_hres = [&]() {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            int m = m0 + 32 * mt + l31;
            m = m < g.M ? m : g.M - 1;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int i4 = 0; i4 < 4; ++i4)
                    hres[nt][mt][i4] = *reinterpret_cast<const op4*>(g.h + plane_off(g.rows, m, 32 * (NT * wave + nt) + 8 * i4 + 4 * kh));
        }
    };
#if RGN_M2_HRES == 0
    load_hres();
#endif
    float vb[5][VK];                                                 // phase B, held in registers until the wave is past norm2
#pragma unroll
    for (int k = 0; k < VK; ++k) {
        vb[0][k] = g.w.bf1[cw + 64 * k];
        vb[1][k] = g.w.bf1[512 + cw + 64 * k];
        vb[2][k] = g.w.bf2[cw + 64 * k];
        vb[3][k] = g.w.g3[cw + 64 * k];
        vb[4][k] = g.w.b3[cw + 64 * k];
    }
    asm volatile("" ::: "memory");
    constexpr int EXTRA = 16 + 6 * VK;                               // residual + phase B + step vector loads
    // the att image is complete once EVERY wave's DMA pieces have landed: they are the oldest vector-memory operations of this
    // wave, so the count below leaves everything younger than the first weight fragments in flight
    wait_vmcnt<(RGN_M2_HRES == 0 ? 16 : 0) + 5 * VK>();
    RGN_M2T(7)
    __builtin_amdgcn_s_barrier();
#if RGN_M2_HRES == 1
    load_hres();
#endif
    float tv[VK];
#pragma unroll
    for (int k = 0; k < VK; ++k) tv[k] = (!ENC && g.stepvec) ? g.stepvec[(size_t)step * g.ldstep + cw + 64 * k] : 0.f;   // (the loop index landed long ago)
    asm volatile("" ::: "memory");
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[nt][mt][i] = 0.f;
    RGN_M2T(1)
    tail_gemm<OP, C, 32, true, EXTRA>(acc, wf, tl, a_offx, p_wo, p_w1a);   // (EXTRA may stay in flight behind the ring)
    RGN_M2T(2)
    // phase A vectors -> the wave's LDS region (wave-private: no barrier, the exchange barrier of norm1 is far behind the writes)
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int k = 0; k < VK; ++k) vec[CW * v + 64 * k + lane] = va[v][k];
#pragma unroll
    for (int j = 0; j < NSAMP; ++j)
#pragma unroll
        for (int k = 0; k < VK; ++k) vec[C::A_SPV + CW * j + 64 * k + lane] = (tv[k] + sv[k]) + pv[j][k];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(vec + C::A_BO + tail_col4(tl, nt, i4));
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[nt][mt][4 * i4 + e] += (float)hres[nt][mt][i4][e] + b[e];
        }
    {   // norm1 (gamma only) + norm1.beta + call_time[step] + call_cond[sample of the token] (pre-summed per sample in LDS)
        const float* spv[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int m = m0 + 32 * mt + l31;
            spv[mt] = vec + C::A_SPV + ((m < g.M ? m : g.M - 1) / g.Tq - m0 / g.Tq) * CW;
        }
        tail_layernorm<C, 0>(acc, tl, vec + C::A_G1, [&](int nt, int i4, int mt) { return *reinterpret_cast<const f32x4*>(spv[mt] + tail_col4(tl, nt, i4)); });
    }
    if constexpr (!ENC) tail_layernorm<C, 1>(acc, tl, vec + C::A_G2, tail_rowvec(tl, vec + C::A_B2));
    tail_store_img<OP, C>(acc, tl, C::Y);
    // phase B vectors over phase A (wave-private: program order suffices)
#pragma unroll
    for (int v = 0; v < 5; ++v)
#pragma unroll
        for (int k = 0; k < VK; ++k) vec[CW * v + 64 * k + lane] = vb[v][k];
    wait_lgkmcnt<0>();
    __builtin_amdgcn_s_barrier();                                     // h' image complete
    RGN_M2T(3)

    // =============== stage 2: linear1 + GELU + linear2: reads h' from Y, the hidden halves go through X (the att tile is dead since stage 1) ====
    f32x16 acc2[NT][MT];
    tail_ffn<OP, C>(acc2, wf, tl, a_offy, a_offx, C::X, p_w1a, p_w1b, p_w2a, p_w2b, vec + C::B_BF1, vec + C::B_BF2);
    RGN_M2T(4)

    // =============== stage 3: + residual h' + norm3 -> output planes =====================================================
    tail_add_resid<OP, C>(acc2, tl, C::Y);
    tail_layernorm<C, 0>(acc2, tl, vec + C::B_G3, tail_rowvec(tl, vec + C::B_B3));   // (its barrier also fences the last reads of X)
    tail_store_img<OP, C>(acc2, tl, C::X);
    wait_lgkmcnt<0>();
    __builtin_amdgcn_s_barrier();
    {
        const __amdgpu_buffer_rsrc_t o_rs = __builtin_amdgcn_make_buffer_rsrc(g.out, 0, (int)((size_t)g.rows * 512 * 2), 0x00020000);
        const int r16 = lane >> 2, c = lane & 3;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int p = wave * 8 + j, blk = p / (R / 16), r = (p % (R / 16)) * 16 + r16;
            const int m = m0 + r;
            if (m < g.M)
                __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4*>(smem + C::X + blk * KB + img_chunk(r, c)), o_rs,
                                                       (int)(plane_chunk(g.rows, m, blk, c) * 2), 0, RGN_M2_ST_AUX);
        }
    }
    RGN_M2T(5)
}

#ifdef RGN_M2_STAMPS
void m2_stamps_read(long long* out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_m2_st), sizeof(long long) * 1024 * 12); }
#endif

// a 64-row tile must not touch more samples than it has per-sample vector slots for
bool mlp_supported(int d, int ff, int Tq) { return d == 512 && ff == 1024 && 63 / Tq + 2 <= M2::NSAMP; }
hipError_t configure_mlp() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_mlp2<true>), hipFuncAttributeMaxDynamicSharedMemorySize, M2::LDS);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_mlp2<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, M2::LDS);
    return e != hipSuccess ? e : hipFuncSetAttribute(reinterpret_cast<const void*>(k_mlp2<false>), hipFuncAttributeMaxDynamicSharedMemorySize, M2::LDS);
}
hipError_t launch_mlp(const MlpArgs& g, hipStream_t s, bool enc) {
    if (enc && g.f16) return hipErrorInvalidValue;                  // (encoder handles have no fp16 phase)
    if (enc) hipLaunchKernelGGL((k_mlp2<false, true>), dim3((g.M + 63) / 64), dim3(M2::NTH), M2::LDS, s, g);
    else if (g.f16) hipLaunchKernelGGL((k_mlp2<true>), dim3((g.M + 63) / 64), dim3(M2::NTH), M2::LDS, s, g);
    else hipLaunchKernelGGL((k_mlp2<false>), dim3((g.M + 63) / 64), dim3(M2::NTH), M2::LDS, s, g);
    return hipGetLastError();
}

}  // namespace rgn
