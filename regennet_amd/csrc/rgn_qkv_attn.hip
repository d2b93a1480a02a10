// Fused in_proj GEMM + self-attention (Tq <= 64 tokens, head dim 128): q, k, v never leave the register file. Causal for the decoder layers,
// and every kernel here also has a full-attention instantiation (CAUSAL = false) for the encoder layers of arch='offline' (cmdm.py:228-238).
//
// Replaces, per decoder layer, the packed in_proj Linear of nn.MultiheadAttention and the attention itself
// (model/cmdm.py:227 -> TransformerDecoderLayer._sa_block with generate_square_subsequent_mask :168-171).
// For each of its heads a workgroup computes [q_h | k_h | v_h] = x . W_h^T (64 tokens per sample x 384, operand layouts: rgn_layout.h) and then runs
// the attention straight from the accumulators: an MFMA contraction does not care in which order the reduction index is fed as long as both
// operands agree, and the C/D layouts of q^T, k^T (accumulated transposed: W fragment as the MFMA A operand), v and the
// softmaxed scores agree by construction, so S^T = K.Q^T and O^T = V^T.P^T take the accumulator registers as operands
// with no LDS staging, no transposes and no fragment reads. The only exchange is the sum of the four dh-tile partials
// of S^T through an fp32 LDS buffer. The head's output is stored as split planes in the K32-blocked layout the out_proj GEMM consumes.
// The C/D map the register-resident attention relies on is mfma32_row / mfma32_col there. That attention, qa_attention, is one function;
// what differs between the THREE FORMS is how the in_proj GEMM gets its operands (qkv_attn_form at the foot of the file decides which one runs):
//
//   k_qkv_attn<X3>          DMA-fed: both operands by direct-to-LDS DMA from the K32-blocked planes into swizzled images, as in k_gemm_x3. 8 waves,
//                           a workgroup owns TWO samples and H/2 heads (grid = ceil(Bm/2) x 2; one head each for small launches). Split-bf16
//                           (X3: three MFMAs per product) or plain bf16. Every width but 512, a mode that packs no fragment-ordered weight planes,
//                           and the split phase under the engine option QKV_X3_DMA = 1.
//   k_qkv_attn_rs<false>    register-streamed, plain phase at d = 512 (bf16 or fp16 operands): the weights go from the fragment-ordered plane straight
//                           into a register ring; 4 waves, ONE sample and H/2 heads per workgroup (all heads' workgroups apart while the evaluation is small).
//   k_qkv_attn_rs<true>     the same loop in the split arithmetic (plan_query reports it as k_qkv_attn_rs_x3), split phase at d = 512: hi and lo
//                           fragment planes side by side. Bit-equal to k_qkv_attn<true>.
//
// The DMA-fed form. Why two samples x half the heads instead of one sample x all heads: the kernel is bound by the ~20 B/clk a CU pulls
// from L2 into LDS (see rgn_gemm_x3.hip), and almost all of that is the in_proj weight stream. Pairing samples halves
// the weight bytes per sample (2.0 MiB of DMA per workgroup instead of 3.5 MiB) at the same workgroup count.
// 8 waves; wave = (sample wm, dh tile wn): wave tile 64 x 96 = both token tiles x the 32 columns wn of each of q, k, v;
// two 64 KiB LDS stages [A 128x32 | W_h 384x32] x {hi, lo}; tile rows 0-63 / 64-127 are the tokens of sample 0 / 1
// (padding rows replicate the last token and are masked). The S^T exchange buffer aliases the dead pipeline stages.
#include "rgn_internal.h"
#include "rgn_device.h"

#include <hip/hip_runtime.h>

namespace rgn {

#ifndef RGN_QA_ST_AUX
#define RGN_QA_ST_AUX 16   // cache policy of the plain-bf16 build's output stores: 16 = sc1 (write-through)
#endif

constexpr int QA_ROWS = 64, QA_NS = 2, QA_DH = 128, QA_WROWS = 3 * QA_DH, QA_NT = 512;

#ifdef RGN_QA_LIFE
__device__ long long g_qa_life[2048 * 3];   // tools only: wall_clock64() (10 ns) at start / first MFMA operands landed / end of every workgroup
#define RGN_QL(i) if (tid == 0) g_qa_life[(blockIdx.y * gridDim.x + blockIdx.x) * 3 + i] = wall_clock64();
#else
#define RGN_QL(i)
#endif
#ifdef RGN_QA_PROF
__device__ long long g_qa_prof[64];   // tools only: phase cycle stamps of one workgroup (wave 0)
#define RGN_QT(i) if (blockIdx.x == RGN_QA_PROF && blockIdx.y == 0 && tid == 0) g_qa_prof[i] = clock64();
#else
#define RGN_QT(i)
#endif

// Sum of the four dh-tile partials of the S^T tiles T0 .. T0 + NT - 1 over the sample's waves, through slots 0 .. NT - 1 of the exchange buffer
// [sample][slot 3][wave wn][i/4][lane] float4: every wave writes its partials, barrier, every wave sums the sample's four
template <int T0, int NT, int N>
__device__ __forceinline__ void qa_exchange_sum(f32x16 (&st)[N], f32x4* sred, int wm, int wn, int lane, int hslot, int tid) {
    (void)hslot; (void)tid;
#pragma unroll
    for (int sl = 0; sl < NT; ++sl)
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4) {
            const f32x4 v = {st[T0 + sl][4 * i4], st[T0 + sl][4 * i4 + 1], st[T0 + sl][4 * i4 + 2], st[T0 + sl][4 * i4 + 3]};
            sred[(((wm * 3 + sl) * 4 + wn) * 4 + i4) * 64 + lane] = v;
        }
    wait_lgkmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (T0 == 0) { RGN_QT(hslot * 8 + 2) }
#pragma unroll
    for (int sl = 0; sl < NT; ++sl)
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4) {
            f32x4 v = sred[(((wm * 3 + sl) * 4 + 0) * 4 + i4) * 64 + lane];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const f32x4 u = sred[(((wm * 3 + sl) * 4 + w) * 4 + i4) * 64 + lane];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += u[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) st[T0 + sl][4 * i4 + e] = v[e];
        }
}

// Attention straight from the in_proj accumulators of one head (see the file header); shared by the DMA-fed and the
// register-streamed GEMM phases. acc[token tile][q | k | v]; smem: the 96 KiB fp32 exchange buffer for the S^T partials.
// CAUSAL = false (encoder layers, arch='offline'): all four S^T tiles, keys >= Tq masked. The fourth tile (keys 32-63, queries 0-31)
// is reduced in a second pass through the first tile's slot of the same exchange buffer, so the LDS budget is the causal one.
template <bool X3, bool F16 = false, bool CAUSAL = true>
__device__ __forceinline__ void qa_attention(f32x16 (&acc)[2][3], const QkvAttnArgs& g, char* smem, const float* bias_h, int hd, int hslot,
                                             int wm, int wn, int nsamp, int b0, int lane, int tid) {
    static_assert(!(X3 && F16), "the split form is bf16 (hi, lo) pairs");
    using OP = OpFmt<F16>;                // plain form: bf16 or fp16 operands (rgn_device.h)
    using op_t = typename OP::t;
    using op8 = typename OP::v8;
    using op4 = typename OP::v4;
    const int l31 = lane & 31, kh = lane >> 5, Tq = g.Tq;
    (void)tid; (void)hslot;
    // ---------------- attention straight from the accumulators: q, k, v never leave the register file --------------
    // Wave (wm, wn) holds, for its sample and the 32 dh columns of tile wn: q and k transposed (lane = token, the 16
    // registers = dh (i&3) + 8(i>>2) + 4*kh) and v plain (lane = dh, registers = tokens in the same pattern), for both
    // token tiles. An MFMA contraction does not care in which order the reduction index is fed as long as both
    // operands agree, and here they do by construction: register i of lane half kh means the same dh in q and in k,
    // and the same token in v and in p. So
    //   S^T[keys, queries] (partial over this wave's 32 dh) = K-regs (A operand) x Q-regs (B operand),
    //   O^T[dh tile, queries] = V-regs (A) x P^T-regs (B, the softmaxed S^T accumulators)
    // need no LDS staging, no transposes and no ds_reads. The only exchange is the sum of the four dh-tile partials of
    // S^T, done through an fp32 LDS buffer that aliases the dead pipeline stages (96 KiB: 2 samples x 3 causal tiles
    // x 4 waves x 4 KiB). Both samples proceed at the same time on their own four waves.
    const bool live = wm < nsamp;                               // (an odd batch: the second sample of the last pair is a dummy)
    const size_t row0 = (size_t)(b0 + (live ? wm : 0)) * Tq;
        op8 qh[2][2], ql[2][2], kfh[2][2], kfl[2][2], vh[2][2], vl[2][2];   // [token tile][16-slice of the register index]
    {
        const float bv = bias_h[2 * QA_DH + l31];
        const float qs2 = g.qscale * 1.44269504088896340736f;   // scores in log2 units: softmax = exp2(s - max), one mul less per score
#pragma unroll
        for (int ta = 0; ta < 2; ++ta)
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {
                const f32x4 bq0 = *reinterpret_cast<const f32x4*>(bias_h + 16 * sl + 4 * kh);
                const f32x4 bq1 = *reinterpret_cast<const f32x4*>(bias_h + 16 * sl + 8 + 4 * kh);
                const f32x4 bk0 = *reinterpret_cast<const f32x4*>(bias_h + QA_DH + 16 * sl + 4 * kh);
                const f32x4 bk1 = *reinterpret_cast<const f32x4*>(bias_h + QA_DH + 16 * sl + 8 + 4 * kh);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int i = 8 * sl + j;
                    const float xq = (acc[ta][0][i] + (j < 4 ? bq0[j] : bq1[j - 4])) * qs2;
                    const float xk = acc[ta][1][i] + (j < 4 ? bk0[j] : bk1[j - 4]);
                    const float xv = acc[ta][2][i] + bv;
                    qh[ta][sl][j] = (op_t)xq;
                    kfh[ta][sl][j] = (op_t)xk;
                    vh[ta][sl][j] = (op_t)xv;
                    if (X3) {
                        ql[ta][sl][j] = (op_t)(xq - (float)qh[ta][sl][j]);
                        kfl[ta][sl][j] = (op_t)(xk - (float)kfh[ta][sl][j]);
                        vl[ta][sl][j] = (op_t)(xv - (float)vh[ta][sl][j]);
                    }
                }
            }
    }
    // causal tiles of S^T: 0 = (keys 0-31, queries 0-31), 1 = (keys 0-31, queries 32-63), 2 = (keys 32-63, queries 32-63);
    // the full form adds 3 = (keys 32-63, queries 0-31)
    constexpr int NTL = CAUSAL ? 3 : 4;
    f32x16 st[NTL];
#pragma unroll
    for (int tl = 0; tl < NTL; ++tl) {
        const int kj = tl >> 1, qtile = CAUSAL ? (tl ? 1 : 0) : ((tl == 1 || tl == 2) ? 1 : 0);
#pragma unroll
        for (int i = 0; i < 16; ++i) st[tl][i] = 0.f;
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            if (X3) {
                st[tl] = OP::mfma(kfl[kj][sl], qh[qtile][sl], st[tl]);
                st[tl] = OP::mfma(kfh[kj][sl], ql[qtile][sl], st[tl]);
            }
            st[tl] = OP::mfma(kfh[kj][sl], qh[qtile][sl], st[tl]);
        }
    }
    f32x4* sred = reinterpret_cast<f32x4*>(smem);
    qa_exchange_sum<0, 3>(st, sred, wm, wn, lane, hslot, tid);
    if constexpr (!CAUSAL) {   // second pass: tile 3 through tile 0's slot, once every wave's reads of it have landed
        wait_lgkmcnt<0>();
        __builtin_amdgcn_s_barrier();
        qa_exchange_sum<3, 1>(st, sred, wm, wn, lane, hslot, tid);
    }
    RGN_QT(hslot * 8 + 4)
    // softmax over keys for the lane's two queries (l31 and 32 + l31); every wave of the sample does the same work
    float inv[2];
#pragma unroll
    for (int qtile = 0; qtile < 2; ++qtile) {
        const int q = 32 * qtile + l31;
        float mx = -INFINITY;
        // tiles {0} for query tile 0, {1, 2} for query tile 1 (the full form: {0, 3}, {1, 2}; the causal bounds fold to tl = qtile .. 2 qtile)
#define RGN_QA_TILES(tl) for (int tl = qtile; tl <= (CAUSAL ? 2 * qtile : (qtile ? 2 : 3)); tl += (CAUSAL ? 1 : (qtile ? 1 : 3)))
#pragma unroll
        RGN_QA_TILES(tl) {
            const int kj = tl >> 1;
            // key of register i = 32 kj + 4 kh + c_i, c_i = (i & 3) + 8 (i >> 2); visible iff key <= min(q, Tq - 1) (tile 1 - keys 0-31,
            // queries 32-63 - lies below the diagonal: only key < Tq; the full form: key < Tq everywhere). ONE per-lane limit, made opaque
            // here: written as 48 compares of loop-invariant values they are hoisted out of the head loop and their lane masks live in
            // ~70 SGPRs spilled to VGPR lanes
            int lim = ((CAUSAL ? tl == 1 : true) ? Tq - 1 : (q < Tq - 1 ? q : Tq - 1)) - 32 * kj - 4 * kh;
            asm volatile("" : "+v"(lim));
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                st[tl][i] = (mfma32_row(i, 0) <= lim) ? st[tl][i] : -INFINITY;
                mx = fmaxf(mx, st[tl][i]);
            }
        }
        mx = half_max(mx);
        float sum = 0.f;
#pragma unroll
        RGN_QA_TILES(tl)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float e = __builtin_amdgcn_exp2f(st[tl][i] - mx);
                st[tl][i] = e;
                sum += e;
            }
        sum = half_sum(sum);
        inv[qtile] = 1.0f / sum;
    }
    RGN_QT(hslot * 8 + 5)
    // O^T[dh tile wn, queries] = V (A operand, registers = keys) x P^T (B operand, registers = keys)
#pragma unroll
    for (int qtile = 0; qtile < 2; ++qtile) {
        f32x16 oa;
#pragma unroll
        for (int i = 0; i < 16; ++i) oa[i] = 0.f;
#pragma unroll
        RGN_QA_TILES(tl) {
            const int kj = tl >> 1;
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {
                op8 ph, pl;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float x = st[tl][8 * sl + j];
                    ph[j] = (op_t)x;
                    pl[j] = (op_t)(x - (float)ph[j]);
                }
                if (X3) {
                    oa = OP::mfma(vl[kj][sl], ph, oa);
                    oa = OP::mfma(vh[kj][sl], pl, oa);
                }
                oa = OP::mfma(vh[kj][sl], ph, oa);
            }
        }
        // O^T tile: lane = query (column), registers = 16 dh indices -> 4 runs of 4 consecutive dh = 8-byte plane
        // stores; the 32 x 32 tile is one contiguous 2 KiB run of the K32-blocked plane
        const int q = 32 * qtile + l31;
        if constexpr (!X3) {
            // plain-bf16 phase (hi plane only): the lane pair (l31, kh = 0 / 1) holds the two 8-byte halves of every 16-byte chunk of the
            // row - one v_permlane32_swap per register pairs them up, and the row goes out as two 16-byte WRITE-THROUGH stores per lane
            // (sc1: nothing of the plane stays dirty in L2 for the end-of-kernel write-back; an 8-byte sc1 store costs 2.7x per byte)
            u32x2 run[4];
#pragma unroll
            for (int i4 = 0; i4 < 4; ++i4) {
                op4 hv;
#pragma unroll
                for (int e = 0; e < 4; ++e) hv[e] = (op_t)(oa[4 * i4 + e] * inv[qtile]);
                run[i4] = __builtin_bit_cast(u32x2, hv);
            }
            const __amdgpu_buffer_rsrc_t o_rs = __builtin_amdgcn_make_buffer_rsrc(g.out.hi, 0, (int)((size_t)g.out.rows * g.d * 2), 0x00020000);
            const size_t o = plane_chunk(g.out.rows, row0 + q, hd * (QA_DH / 32) + wn, kh);
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {          // runs (2 pr, 2 pr + 1) = elements 16 pr + 4 kh + {0..3} and 16 pr + 8 + 4 kh + {0..3}
                u32x4 v;
#pragma unroll
                for (int w = 0; w < 2; ++w) {
                    // after the swap: lanes kh = 0 hold (own even run, partner's even run), lanes kh = 1 (partner's odd run, own odd run)
                    const auto sw = __builtin_amdgcn_permlane32_swap(run[2 * pr][w], run[2 * pr + 1][w], false, false);
                    v[w] = sw[0];
                    v[2 + w] = sw[1];
                }
                if (live && q < Tq) __builtin_amdgcn_raw_buffer_store_b128(v, o_rs, (int)((o + 16 * pr) * 2), 0, RGN_QA_ST_AUX);
            }
        } else if (live && q < Tq) {
            const size_t o = plane_chunk(g.out.rows, row0 + q, hd * (QA_DH / 32) + wn, 0) + 4 * kh;
#pragma unroll
            for (int i4 = 0; i4 < 4; ++i4) {
                op4 hv, lv;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x = oa[4 * i4 + e] * inv[qtile];
                    hv[e] = (op_t)x;
                    lv[e] = (op_t)(x - (float)hv[e]);
                }
                *reinterpret_cast<op4*>(reinterpret_cast<op_t*>(g.out.hi) + o + 8 * i4) = hv;
                if (g.out.lo) *reinterpret_cast<op4*>(reinterpret_cast<op_t*>(g.out.lo) + o + 8 * i4) = lv;
            }
        }
    }
}

#undef RGN_QA_TILES

// ---- the prologue the DMA-fed and the register-streamed kernels share (k_qkv_attn_long has a tile shape and wave roles of its own) ----
// Plane row of tile row r (sample r / 64 of the workgroup's nsamp, token r % 64): padding rows replicate the last token (masked later), and
// the rows of a dummy second sample (an odd batch leaves the last pair half empty) those of the first
__device__ __forceinline__ int qa_plane_row(int r, int b0, int nsamp, int Tq) {
    const int sm = (r >> 6) < nsamp ? (r >> 6) : 0, tk = r & 63;
    return (b0 + sm) * Tq + (tk < Tq ? tk : Tq - 1);
}
// byte offsets of the wave's A fragments in an activation image: [token tile][k half] of sample wm
__device__ __forceinline__ void qa_frag_offsets(int (&a_off)[2][2], int wm, int l31, int kh) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) a_off[t][ks] = img_frag(wm * 64 + t * 32 + l31, ks, kh);
}
// in_proj biases of the workgroup's hpb heads from hd0 on -> LDS [hpb][q | k | v][128] (visible to every wave after the first barrier of the k-loop)
__device__ __forceinline__ void qa_stage_bias(float* bias_s, const QkvAttnArgs& g, int hd0, int hpb, int tid, int nt) {
    for (int i = tid; i < hpb * QA_WROWS; i += nt) {
        const int hh = i / QA_WROWS, r = i - hh * QA_WROWS;
        bias_s[i] = g.bias[(r >> 7) * g.d + (hd0 + hh) * QA_DH + (r & 127)];
    }
}
__device__ __forceinline__ void qa_zero(f32x16 (&acc)[2][3]) {
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[ta][t][i] = 0.f;
}

template <bool X3, bool CAUSAL = true>
__global__ __launch_bounds__(QA_NT, 1) void k_qkv_attn(QkvAttnArgs g) {
    constexpr int NPL = X3 ? 2 : 1;
    constexpr int A_BYTES = QA_NS * QA_ROWS * 64, W_BYTES = QA_WROWS * 64;
    constexpr int STAGE = NPL * (A_BYTES + W_BYTES);                 // 64 KiB (x3), 32 KiB (plain bf16)
    // pipeline depth: the same 128 KiB hold two split-bf16 stages or four plain-bf16 ones; what a CU pulls from L2 is set by
    // the bytes it keeps in flight (tools/l2_paths_bench), so the plain-bf16 build prefetches three tiles ahead
    constexpr int NSTG = X3 ? 2 : 4;
    constexpr int W_IT = QA_WROWS * 4 / QA_NT;                       // 3
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;                         // GEMM phase roles: wm = sample of the pair
    const int l31 = lane & 31, kh = lane >> 5;
    const int b0 = xcd_affine(blockIdx.x, gridDim.x) * QA_NS, Tq = g.Tq, d = g.d;   // (gridDim.x = sample pairs; id = y * gridDim.x + x)
    const int hpb = g.H / (int)gridDim.y, hd0 = blockIdx.y * hpb;    // heads of this workgroup
    const int nsamp = g.Bm - b0 < QA_NS ? g.Bm - b0 : QA_NS;         // an odd batch leaves the last pair half empty

    // this thread's 16 bytes of every activation k-block (elements): chunk c of tile row tid / 4
    const size_t a_src = (size_t)qa_plane_row(tid >> 2, b0, nsamp, Tq) * 32 + img_dma_chunk(tid >> 2, tid & 3) * 8;
    int a_off[2][2], w_off[3][2];
    qa_frag_offsets(a_off, wm, l31, kh);
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int rr = t * QA_DH + wn * 32 + l31;                    // t = 0 / 1 / 2: the wave's 32 columns of q / k / v
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) w_off[t][ks] = img_frag(rr, ks, kh);
    }
    const int nk = g.Kp / 32;
    float* bias_s = reinterpret_cast<float*>(smem + 4 * (A_BYTES + W_BYTES));   // [hpb][3][128] in_proj biases, past the stages / operand buffers
    qa_stage_bias(bias_s, g, hd0, hpb, tid, QA_NT);

    for (int hd = hd0; hd < hd0 + hpb; ++hd) {
        // ---------------- GEMM: [128 x Kp] . W_h[384 x Kp]^T ----------------------------------------------------
        size_t w_src[W_IT];
#pragma unroll
        for (int it = 0; it < W_IT; ++it) {
            const int q = it * QA_NT + tid, r = q >> 2, c = img_dma_chunk(r, q & 3);
            const int which = r >> 7, j = r & 127;
            w_src[it] = ((size_t)which * d + hd * QA_DH + j) * 32 + c * 8;
        }
        // DMA piece idx (compile-time after unrolling) of tile kt into stage buffer sb: A hi/lo, then the 3 W pieces hi/lo
        auto piece = [&](int idx, int kt, char* sb) {
            const size_t ka = (size_t)kt * g.a_rows * 32, kw = (size_t)kt * 3 * d * 32;
            if (idx < NPL) {
                const int lo = (tid & ~63) * 16;
                __builtin_amdgcn_global_load_lds((const RGN_AS1 void*)((idx ? g.Alo : g.Ahi) + a_src + ka), (RGN_AS3 void*)(sb + idx * A_BYTES + lo), 16, 0, 0);
            } else {
                const int j = idx - NPL, it = j / NPL, pl = j % NPL;
                const int lo = (it * QA_NT + (tid & ~63)) * 16;
                __builtin_amdgcn_global_load_lds((const RGN_AS1 void*)((pl ? g.Wlo : g.Whi) + w_src[it] + kw),
                                                 (RGN_AS3 void*)(sb + NPL * A_BYTES + pl * W_BYTES + lo), 16, 0, 0);
            }
        };
        constexpr int LPT = NPL * (1 + W_IT);                        // 8 (x3)
        f32x16 acc[2][3];
        qa_zero(acc);
        RGN_QT((hd - hd0) * 8 + 0)
#pragma unroll
        for (int t0 = 0; t0 < NSTG - 1; ++t0)
#pragma unroll
            for (int idx = 0; idx < LPT; ++idx) piece(idx, t0, smem + t0 * STAGE);   // nk >= NSTG - 1 (host-checked)
        // One barrier per k-step: tile kt+1's pieces are issued two at a time behind the MFMA groups of the first K half of
        // tile kt (a back-to-back burst would stall the in-order wave for the whole queue of the CU's vector-memory
        // path), into the stage every wave finished reading before this step's barrier; fragments are fetched one MFMA
        // group (one W tile x both A tiles) ahead.
        for (int kt = 0; kt < nk; ++kt) {
            // my pieces of tile kt landed; tiles kt+1 .. kt+NSTG-2 stay in flight (fewer near the end of the loop)
            if (NSTG == 2 || kt + 1 >= nk) wait_vmcnt<0>();
            else if (kt + 2 >= nk) wait_vmcnt<4>();     // LPT = 4 in the plain-bf16 build
            else wait_vmcnt<8>();
            __builtin_amdgcn_s_barrier();                          // ... everyone's did, and everyone left step kt-1
            const char* sb = smem + (kt % NSTG) * STAGE;
            char* nb = smem + ((kt + NSTG - 1) % NSTG) * STAGE;
            const bool more = kt + NSTG - 1 < nk;
            bf16x8 ah[2][2], al[2][2], wh[2], wl[2];
            auto fetch = [&](int grp) {                             // grp = ks * 3 + t
                const int ks = grp / 3, t = grp % 3;
                if (t == 0) {
#pragma unroll
                    for (int ta = 0; ta < 2; ++ta) {
                        ah[ks][ta] = *reinterpret_cast<const bf16x8*>(sb + a_off[ta][ks]);
                        if (X3) al[ks][ta] = *reinterpret_cast<const bf16x8*>(sb + A_BYTES + a_off[ta][ks]);
                    }
                }
                wh[grp & 1] = *reinterpret_cast<const bf16x8*>(sb + NPL * A_BYTES + w_off[t][ks]);
                if (X3) wl[grp & 1] = *reinterpret_cast<const bf16x8*>(sb + NPL * A_BYTES + W_BYTES + w_off[t][ks]);
            };
            fetch(0);
#pragma unroll
            for (int grp = 0; grp < 6; ++grp) {
                if (grp + 1 < 6) fetch(grp + 1);
                const int ks = grp / 3, t = grp % 3;
#pragma unroll
                for (int ta = 0; ta < 2; ++ta) {
                    if (t < 2) {   // q, k tiles transposed (lane = token, registers = dh): 8-byte LDS writes below
                        if (X3) {
                            acc[ta][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[grp & 1], al[ks][ta], acc[ta][t], 0, 0, 0);
                            acc[ta][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[grp & 1], ah[ks][ta], acc[ta][t], 0, 0, 0);
                        }
                        acc[ta][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[grp & 1], ah[ks][ta], acc[ta][t], 0, 0, 0);
                    } else {       // v tile: lane = dh, registers = tokens (v goes to LDS transposed)
                        if (X3) {
                            acc[ta][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[ks][ta], wh[grp & 1], acc[ta][t], 0, 0, 0);
                            acc[ta][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[ks][ta], wl[grp & 1], acc[ta][t], 0, 0, 0);
                        }
                        acc[ta][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[ks][ta], wh[grp & 1], acc[ta][t], 0, 0, 0);
                    }
                }
                if (more && grp < 4) {
#pragma unroll
                    for (int q = 0; q < LPT / 4; ++q) piece(grp * (LPT / 4) + q, kt + NSTG - 1, nb);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        wait_lgkmcnt<0>();
        __builtin_amdgcn_s_barrier();                              // every wave is done reading the last stage
        RGN_QT((hd - hd0) * 8 + 1)
        qa_attention<X3, false, CAUSAL>(acc, g, smem, bias_s + (hd - hd0) * QA_WROWS + wn * 32, hd, hd - hd0, wm, wn, nsamp, b0, lane, tid);
        RGN_QT((hd - hd0) * 8 + 6)
        wait_lgkmcnt<0>();
        __builtin_amdgcn_s_barrier();      // the next head's DMA overwrites the reduction buffer
        RGN_QT((hd - hd0) * 8 + 3)
    }
}

// ---- d = 512: the same kernel with the in_proj weights streamed into REGISTERS, k_qkv_attn_rs<X3, F16, CAUSAL> -------------------------
// The scheme (both arithmetics). The DMA-fed loop above moves 112 KiB through LDS per k-step in the plain-bf16 build (32 KiB of DMA writes +
// 80 KiB of fragment reads, of which 48 KiB are the W fragments) against the 128 B/clk the LDS delivers: ~1400 clk per k-step for 768 clk of
// MFMA work (tools/qkv_attn_bench -DRGN_QA_PROF). Here every wave loads its own q/k/v weight fragments straight from the
// fragment-ordered plane ([Kp/32][3d/32][2 ks][64 lanes][8] of rgn_layout.h, one contiguous 1 KiB run per wave-load, as in k_rowgemm)
// into a register ring, WQ fragments ahead; only the activation tile (8 KiB per plane and k-step, loaded to registers DA steps
// ahead and written to a 2-stage LDS ring one step ahead) still passes through LDS. No direct-to-LDS DMA in the
// loop, and the 16 k-steps are fully unrolled: the compiler's own s_waitcnt bookkeeping then stays exact (it drains
// vmcnt at loop back-edges and before the first LDS read behind a DMA).
// QR_NS = 1 sample per workgroup (4 waves). LDS: [exchange buffer 48 KiB | activation ring [2 stages][planes][64 rows][64 B] | biases].
// Two INDEPENDENT 4-wave workgroups per CU (one wave each per SIMD) instead of one 8-wave workgroup of two samples whose two waves per
// SIMD move through the phases in lockstep - the attention phase and the ring fill of one workgroup (no MFMA work, no weight requests)
// then run under the other's k-loop: 36.4 -> 35.4 us alone at B = 256, 28 -> 21 us at B = 128, +3 - 4.5 % on
// the whole step, same results bit for bit.
//
// What the split form (X3; round 6) changes: two planes - the hi and lo fragment planes side by side in the weight ring, the activation stage = hi | lo
// (16 KiB per pair of stages) - three MFMAs per product, and rings half as deep in k-steps (the registers are the same: 72 for the weights). Its
// DMA-fed twin k_qkv_attn<true> moves 64 KiB of operands per k-step through the ~20 B/clk direct-to-LDS path against 2304 cycles of MFMA (3400
// measured). Every accumulator sees the MFMAs of k_qkv_attn<true> in the same order (k-block, k half; lo x hi, hi x lo, hi x hi): the two forms agree
// bit for bit (tests/test_hip_parity.py), "QKV_X3_DMA" = 1 keeps the direct-to-LDS form. The kernel itself runs 53 us where the direct-to-LDS form ran
// 73 (rocprofv3, the evaluation schedule at B = 256) - and the CALL gains 1 - 3 %: the split steps run three kernel chains side by side and are short
// of L2 bandwidth chip-wide (k_mlp_x3 streams 5.2 MB of weight fragments per 32-row tile), so time a chain's in_proj gives back is taken by its
// neighbours' layer tails. One sample per workgroup: 5.71 ms per ddim5 call at B = 256 against 5.79 with two (whose sample halves request the same
// weight fragments at the same time) and 5.78 with the direct-to-LDS form, 3.04 / 3.06 / 3.14 at B = 64 (profiles/r06_qkv_x3_forms.txt).
constexpr int QR_NK = 16;
constexpr int QR_NS = 1, QR_NT = QR_NS * 256;
constexpr int QR_ABUF = QR_NS * 48 * 1024;
template <bool X3> struct QrRing {                                // ring depths and LDS bytes of the two arithmetics
    static constexpr int NPL = X3 ? 2 : 1;                        // planes: hi (| lo)
    static constexpr int WQ = X3 ? 9 : 18;                        // weight fragment ring (6 fragments - X3: (hi, lo) pairs - per k-step): 3 / 1.5 k-steps' worth
    static constexpr int DA = X3 ? 2 : 4, ARING = DA + 1;         // activation pieces: DA ahead (they must be in LDS one step early)
    static constexpr int LDS = QR_ABUF + 2 * NPL * QR_NS * QA_ROWS * 64 + 8 * QA_WROWS * 4;
};
constexpr int QR_LDS = QrRing<false>::LDS, QX_LDS = QrRing<true>::LDS;
// (Wfr: g.Wfr as an argument of its own; the lo plane is g.Wfr_lo)
template <bool X3, bool F16 = false, bool CAUSAL = true>
__global__ __launch_bounds__(QR_NT, 2) void k_qkv_attn_rs(QkvAttnArgs g, const __bf16* __restrict__ Wfr) {
    static_assert(!(X3 && F16), "the split form is bf16 (hi, lo) pairs");
    using OP = OpFmt<F16>;                // bf16 or fp16 operands (rgn_device.h): input plane, weight plane, q / k / v / p, output plane
    using op8 = typename OP::v8;
    using R = QrRing<X3>;
    constexpr int NS = QR_NS, NT = QR_NT, NPL = R::NPL, STAGE = NS * QA_ROWS * 64;   // STAGE: one plane of one stage; a stage = hi (| lo)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int l31 = lane & 31, kh = lane >> 5;
    const int b0 = xcd_affine(blockIdx.x, gridDim.x) * NS, Tq = g.Tq, d = g.d;   // (gridDim.x = sample groups; id = y * gridDim.x + x)
    const int hpb = g.H / (int)gridDim.y, hd0 = blockIdx.y * hpb;
    const int nsamp = g.Bm - b0 < NS ? g.Bm - b0 : NS;
    RGN_QL(0)
    constexpr int nb_all = 3 * 512 / 32;                             // d = 512 (qkv_attn_form): compile-time weight offsets - as run-time
                                                                     // values the 96 k-step offsets of a head live in SGPRs and spill to VGPR lanes
    // this thread's 16 bytes of every activation k-block (elements): chunk c of tile row tid / 4
    const unsigned a_voff = (unsigned)qa_plane_row(tid >> 2, b0, nsamp, Tq) * 32u + img_dma_chunk(tid >> 2, tid & 3) * 8;
    // buffer loads: descriptor + uniform k-step offset in SGPRs, one 32-bit VGPR per lane address (with flat addresses the
    // compiler materialises a 64-bit address pair per unrolled k-step and spills)
    const __bf16* const a_pl[2] = {g.Ahi, g.Alo};
    const __bf16* const w_pl[2] = {Wfr, g.Wfr_lo};
    __amdgpu_buffer_rsrc_t a_rs[NPL], w_rs[NPL];
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) {
        a_rs[pl] = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(a_pl[pl]), 0, (int)((size_t)g.a_rows * g.Kp * 2), 0x00020000);
        w_rs[pl] = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(w_pl[pl]), 0, 3 * d * g.Kp * 2, 0x00020000);
    }
    const unsigned a_kbytes = (unsigned)g.a_rows * 64u;
    int a_off[2][2];
    qa_frag_offsets(a_off, wm, l31, kh);
    char* abuf = smem + QR_ABUF;                                     // [stage 2][plane NPL][64 rows][64 B]
    float* bias_s = reinterpret_cast<float*>(abuf + 2 * NPL * STAGE);
    qa_stage_bias(bias_s, g, hd0, hpb, tid, NT);

    for (int hd = hd0; hd < hd0 + hpb; ++hd) {
        unsigned wofs[3];                                            // fragment block of this wave's 32 columns of q / k / v (elements)
#pragma unroll
        for (int t = 0; t < 3; ++t) wofs[t] = (unsigned)((t * d + hd * QA_DH) / 32 + wn) * 1024u + lane * 8;
        f32x16 acc[2][3];
        qa_zero(acc);
        RGN_QT((hd - hd0) * 8 + 0)
        // Weight fragments: a ring of WQ fragments per plane (plain: 18 = 3 k-steps' worth) recycled ONE AT A TIME: fragment q = 6 kt + 3 ks + t
        // is consumed by its MFMAs and its registers immediately take fragment q + WQ - the same 72 VGPRs as three whole-step
        // slots, but every load is issued three k-steps (not two) ahead of its use and the loads are spread between the MFMAs.
        op8 wq[NPL][R::WQ];
        u32x4 areg[NPL][R::ARING];
        auto issue_a = [&](int kt) {
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl)
                areg[pl][kt % R::ARING] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rs[pl], a_voff * 2, kt * a_kbytes, 0));
        };
        auto issue_q = [&](int q) {                                  // q compile-time after unrolling
            const int kt = q / 6, ks = (q % 6) / 3, t = q % 3;
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl)
                wq[pl][q % R::WQ] = __builtin_bit_cast(op8, __builtin_amdgcn_raw_buffer_load_b128(w_rs[pl], wofs[t] * 2, (kt * nb_all * 1024 + ks * 512) * 2, 0));
        };
        auto stage_a = [&](int kt) {                                 // k-block kt of the activation tile: registers -> its stage
#pragma unroll
            for (int pl = 0; pl < NPL; ++pl) *reinterpret_cast<u32x4*>(abuf + ((kt & 1) * NPL + pl) * STAGE + tid * 16) = areg[pl][kt % R::ARING];
        };
#pragma unroll
        for (int kt = 0; kt < R::DA; ++kt) issue_a(kt);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < R::WQ; ++q) issue_q(q);
        __builtin_amdgcn_sched_barrier(0);
        stage_a(0);
#pragma unroll
        for (int kt = 0; kt < QR_NK; ++kt) {
            wait_lgkmcnt<0>();
            __builtin_amdgcn_s_barrier();                            // k-block kt is in its stage; everyone left stage (kt + 1) % 2
            const char* sb = abuf + (kt & 1) * NPL * STAGE;
            op8 af[NPL][2][2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                    for (int pl = 0; pl < NPL; ++pl) af[pl][ks][ta] = *reinterpret_cast<const op8*>(sb + pl * STAGE + a_off[ta][ks]);
            __builtin_amdgcn_sched_barrier(0);
            if (kt + R::DA < QR_NK) issue_a(kt + R::DA);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int grp = 0; grp < 6; ++grp) {
                const int ks = grp / 3, t = grp % 3, q = kt * 6 + grp, s = q % R::WQ;
#ifdef RGN_QA_LIFE
                if (kt == 0 && grp == 1 && hd == hd0) { RGN_QL(1) }
#endif
#pragma unroll
                for (int ta = 0; ta < 2; ++ta) {
                    if (t < 2) {   // q, k tiles transposed (lane = token, registers = dh)
                        if constexpr (X3) {
                            acc[ta][t] = OP::mfma(wq[0][s], af[1][ks][ta], acc[ta][t]);
                            acc[ta][t] = OP::mfma(wq[1][s], af[0][ks][ta], acc[ta][t]);
                        }
                        acc[ta][t] = OP::mfma(wq[0][s], af[0][ks][ta], acc[ta][t]);
                    } else {       // v tile: lane = dh, registers = tokens
                        if constexpr (X3) {
                            acc[ta][t] = OP::mfma(af[1][ks][ta], wq[0][s], acc[ta][t]);
                            acc[ta][t] = OP::mfma(af[0][ks][ta], wq[1][s], acc[ta][t]);
                        }
                        acc[ta][t] = OP::mfma(af[0][ks][ta], wq[0][s], acc[ta][t]);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                if (q + R::WQ < 6 * QR_NK) issue_q(q + R::WQ);
                if (grp == 2 && kt + 1 < QR_NK) stage_a(kt + 1);     // next k-block of the activation tile -> the other stage
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if constexpr (X3) {
            wait_lgkmcnt<0>();
            __builtin_amdgcn_s_barrier();                            // (the exchange buffer does not alias the ring, but every wave must have left the k-loop's last stage reads)
        }
        RGN_QT((hd - hd0) * 8 + 1)
        qa_attention<X3, F16, CAUSAL>(acc, g, smem, bias_s + (hd - hd0) * QA_WROWS + wn * 32, hd, hd - hd0, wm, wn, nsamp, b0, lane, tid);
        RGN_QT((hd - hd0) * 8 + 6)
        wait_lgkmcnt<0>();
        __builtin_amdgcn_s_barrier();
        RGN_QT((hd - hd0) * 8 + 3)
    }
    RGN_QL(2)
}

bool qkv_attn_supported(int Tq, int dh, int d) { return Tq <= QA_ROWS && dh == QA_DH && d % 32 == 0 && d / dh <= 8 && d >= 128; }
static int qa_lds(bool x3) { return 2 * (x3 ? 2 : 1) * (QA_NS * QA_ROWS * 64 + QA_WROWS * 64) + 8 * QA_WROWS * 4 /* biases of <= 8 heads (odd H: one workgroup runs them all) */; }
hipError_t configure_qkv_attn() {
    // every instantiation (the full-attention forms take the causal allocations: the fourth S^T tile passes through the causal exchange buffer;
    // the plain-bf16 DMA-fed build is given the split one's: its operand buffers, one plane each, alias its 64 KiB of stages)
    const struct { const void* kernel; int lds; } forms[] = {
        {reinterpret_cast<const void*>(k_qkv_attn<true, true>), qa_lds(true)},          {reinterpret_cast<const void*>(k_qkv_attn<true, false>), qa_lds(true)},
        {reinterpret_cast<const void*>(k_qkv_attn<false, true>), qa_lds(true)},         {reinterpret_cast<const void*>(k_qkv_attn<false, false>), qa_lds(true)},
        {reinterpret_cast<const void*>(k_qkv_attn_rs<false, false, true>), QR_LDS},     {reinterpret_cast<const void*>(k_qkv_attn_rs<false, false, false>), QR_LDS},
        {reinterpret_cast<const void*>(k_qkv_attn_rs<false, true, true>), QR_LDS},
        {reinterpret_cast<const void*>(k_qkv_attn_rs<true, false, true>), QX_LDS},      {reinterpret_cast<const void*>(k_qkv_attn_rs<true, false, false>), QX_LDS}};
    for (const auto& f : forms)
        if (hipError_t e = hipFuncSetAttribute(f.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, f.lds); e != hipSuccess) return e;
    return hipSuccess;
}
// THE form rule: launch_qkv_attn dispatches on it and rgn_plan_query reports it.
QkvAttnForm qkv_attn_form(const QkvAttnArgs& g, bool x3) {
    // register-streamed: d = 512 instantiations (compile-time weight offsets, 16 k-steps) that read fragment-ordered weight planes - the split one both of
    // them and the lo activation plane - through 32-bit buffer offsets; every other width, and a mode that packs no fragment planes, runs the DMA-fed form
    const bool rs = g.Wfr && (!x3 || (g.Wfr_lo && g.Alo)) && g.Kp == 32 * QR_NK && g.d == 512 && (size_t)g.a_rows * g.Kp * 2 < (1ull << 31);
    if (rs) {
        // Heads per workgroup: two (half the in_proj weight requests per sample) once the evaluation alone fills the chip with 4-wave
        // workgroups - >= 256 samples over all chains: 512 workgroups, two per CU - and ONE head per workgroup below that (B = 64 / 128 /
        // 192 at 60 frames: 116.9 / 131.0 / 154.1 vs 135.6 / 139.7 / 158.0 ms per 250-step call; B = 256: 360 vs 369 motions/s the other way)
        const int beval = g.Bm_eval > 0 ? g.Bm_eval : g.Bm;
        return {x3 ? QF_RS_X3 : QF_RS, (beval < 256 || g.H % 2) ? g.H : 2};
    }
    // DMA-fed: half of the heads (the weight stream per sample is what bounds the kernel), but one head each while
    // the launch is small (<= 64 workgroups): a small batch is latency-bound and the heads of a workgroup run back to back
    const int pairs = (g.Bm + QA_NS - 1) / QA_NS;
    return {QF_DMA, (pairs * g.H <= 64) ? g.H : (g.H % 2 == 0 ? 2 : 1)};
}
hipError_t launch_qkv_attn(const QkvAttnArgs& g, bool x3, hipStream_t s, bool causal) {
    const QkvAttnForm f = qkv_attn_form(g, x3);
    // fp16 operands (the schedule's fp16 sub-phase): only the register-streamed plain form has the instantiation, and encoder handles have no fp16 phase
    if (g.f16 && (f.form != QF_RS || !causal)) return hipErrorInvalidValue;
    if (f.form == QF_DMA)
        dispatch_bools([&](auto X, auto C) {
            hipLaunchKernelGGL((k_qkv_attn<decltype(X)::value, decltype(C)::value>), dim3((g.Bm + QA_NS - 1) / QA_NS, f.hsplit), dim3(QA_NT), qa_lds(true), s, g);
        }, x3, causal);
    else
        dispatch_bools([&](auto X, auto F, auto C) {
            constexpr bool X3 = decltype(X)::value, F16 = decltype(F)::value, CAUSAL = decltype(C)::value;
            if constexpr (!F16 || (!X3 && CAUSAL))
                hipLaunchKernelGGL((k_qkv_attn_rs<X3, F16, CAUSAL>), dim3(g.Bm, f.hsplit), dim3(QR_NT), QrRing<X3>::LDS, s, g, g.Wfr);
        }, f.form == QF_RS_X3, g.f16 != 0, causal);
    return hipGetLastError();
}

#ifdef RGN_QA_LIFE
void qa_life_read(long long* out, int n) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_qa_life), sizeof(long long) * n); }
#endif
#ifdef RGN_QA_PROF
void qa_prof_read(long long* out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_qa_prof), sizeof(long long) * 64); }
#endif

}  // namespace rgn
