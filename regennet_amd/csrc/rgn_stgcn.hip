// ST-GCN feature extractor / action classifier of the evaluation harness on MI355X.
//
// Replaces eval/a2m/recognition/models/stgcn.py:76-123 (STGCN.forward, eval mode) with its ten st_gcn blocks (:145-228)
// and ConvTemporalGraphical (stgcnutils/tgcn.py:61-71). What runs per block, all BatchNorms folded at load time (fp64):
//
//   g  = relu((sum_v A'_k[v,w] x[(n,t,v),ci]) . W1'^T + b1'[w])            k_sg_gcn      graph aggregation first (the 1x1 conv and the vertex mixing
//                                                                            commute; A' = A * edge_importance keeps the skeleton's sparsity -
//                                                                            166 of 3 x 56 x 56 entries for SMPL-X), formed in registers in MFMA
//                                                                            fragment layout, then ONE split-bf16 GEMM over K = 3 C_in
//   x' = relu(sum_dt g[t + dt - 4] . W2'_dt^T + b2' + residual)             k_sg_tconv    ONE split-bf16 GEMM over K = 9 C_out on an LDS-resident window
//                                                                            of the time-PADDED activation (tap dt = rows shifted by (dt - 4) V:
//                                                                            no im2col buffer), the block's tail in the epilogue; output as the
//                                                                            next block's planes - polyphase (even | odd frames) in front of a
//   (stride 2: taps on the even / odd frame regions, + the 1x1 shortcut)    k_sg_tconv_s2 stride-2 block, which then runs at the output rate
//
// The blocks follow the handle's PLAN (rgn_stgcn_set_blocks; default: the ten above; the unconstrained evaluation's extractor, eval/unconstrained/models/stgcn.py, has six),
// and a graph of fewer than 28 nodes runs on a padded vertex count with isolated pad vertices (rgn_sg_plan.h; finalize and forward below; k_sg_tconv_pre).
// The kernels live in rgn_sg_kernels.hip (what they share with each other and with k_gemm_x3: rgn_dma_gemm.h); this file holds the load-time folding, the plane geometry and the block loop, plus the small kernels around
// them (input layout + data_bn, pad zeroing, pooling) and the forms the fused kernels replaced (k_sg_agg + row-shifted k_gemm_x3 + k_sg_post), which
// still serve graphs and shapes the fused kernels do not take and can be selected per handle (rgn_stgcn_set_option; every form is tested).
//
// Activations are split-bf16 operand planes (hi = rne(x), lo = rne(x - hi)) in the K32-blocked layout of rgn_gemm_x3.hip,
// [C/32][R][32] with rows (n m, frame, vertex): 4 zero pad frames behind every sequence (= in front of the next one) and 4 V zero guard rows
// at both ends of a plane block, so the temporal convolution is plain row-shifted operand reads. Products are formed as a_lo w_hi + a_hi w_lo +
// a_hi w_hi (fp32 accumulate): ~2^-16 per product, measured <= 2e-5 relative on the reference's features (the fp32-MFMA build this replaces
// measured the same parity at 173 ms per 256 two-person motions of 60 frames; profiles/r05).
#include "../../include/regennet_hip.h"
#include "rgn_internal.h"
#include "rgn_device.h"
#include "rgn_sg_plan.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

using namespace rgn;

namespace {

constexpr int SG_PAD = 4;                      // temporal kernel 9 -> 4 zero frames BEHIND every sequence: they are also the pad in front of the next
                                               // one (the guard rows in front of the first), so a sequence costs T + 4 frames of rows, not T + 8
struct SgBlock {
    int ci = 0, co = 0, stride = 1, kp1 = 0, kpr = 0;
    unsigned slot_k = 0;                             // the same lists as 8 slots per vertex for k_sg_gcn (rgn_internal.h); sl_v == nullptr: they do not fit
    int* sl_v = nullptr;
    float* sl_a = nullptr;
    bool res_conv = false, res_id = false;
    int *nz_ptr = nullptr, *nz_v = nullptr;          // nonzeros of A'_k[:, w]: list (k V + w) = [nz_ptr[k V + w], nz_ptr[k V + w + 1])
    float* nz_a = nullptr;
    __bf16 *W1h = nullptr, *W1l = nullptr, *W2h = nullptr, *W2l = nullptr, *Wrh = nullptr, *Wrl = nullptr;   // K32-blocked weight planes [Kp/32][co][32]
    __bf16 *W1f = nullptr, *W2f = nullptr, *Wrf = nullptr;   // the same planes as ONE IEEE fp16 plane each (SG_F16: the single-plane form, rgn_sg_kernels.hip)
    float* W1s = nullptr;                                    // first block only: W1' dense fp32 [co][K ci] (k_sg_block0)
    float *b1 = nullptr, *b2 = nullptr, *br = nullptr, *b2r = nullptr;   // b2r = b2' + br' (the stride-2 kernel adds the shortcut into the same accumulators)
};

// split-bf16 activation planes [C/32][R][32]; hi / lo point at row 0 (behind the leading guard rows), R = block stride in rows
struct SgPl {
    __bf16* hi;
    __bf16* lo;
    long long R;
};

}  // namespace

struct rgn_stgcn_ctx {
    rgn_stgcn_config cfg{};
    std::string err;
    std::map<std::string, std::vector<float>> sd;
    std::map<std::string, std::vector<int64_t>> shapes;
    bool finalized = false;
    std::string f16_refused;                     // why SG_F16 cannot be served by this checkpoint (a folded weight beyond the fp16 range); empty: it can
    std::map<std::string, int> opts;             // rgn_stgcn_set_option: kernel-selection switches of this handle (they take precedence over REGENNET_<KEY>)
    int V = 0, K = 0, C0 = 0;
    int Vp = 0, P = 0;                           // vertices per frame of the planes (V < 28: padded, rgn_sg_plan.h) and the period of the vertex bias table
    std::vector<SgBlockDef> plan = sg_default_plan();   // rgn_stgcn_set_blocks
    std::vector<SgBlock> blocks;
    float *bn_s = nullptr, *bn_t = nullptr, *Wf = nullptr, *bf = nullptr;
    __bf16 *xa[2] = {nullptr, nullptr}, *xb[2] = {nullptr, nullptr}, *z[2] = {nullptr, nullptr}, *g[2] = {nullptr, nullptr};   // (hi, lo) plane buffers
    float *conv = nullptr, *rfull = nullptr, *pooled = nullptr;
    size_t guard = 0;                            // guard rows at both ends of every plane block (the temporal taps' reach: 4 V)
    std::vector<void*> allocs;
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    int fail(int code, const std::string& m) {
        err = m;
        return code;
    }
};

namespace {

thread_local std::string g_sg_create_error;

#define SG_HIP(h, expr)                                                                                 \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) return (h)->fail(RGN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// The kernel-selection switches (rgn_stgcn_set_option; every selectable form meets the same parity bound - tests/test_eval_gpu.py runs them all):
// SG_F16 selects the ARITHMETIC, not a kernel form: blocks 1-9 (and block 0's temporal convolution) on single fp16 operand planes, one MFMA per product instead of
// three - 2^-12 per operand (the level of the TF32 convolutions the reference's own GPU run uses by default) instead of ~2^-16 per product; measured 1e-3-class
// relative feature differences instead of 1e-5-class (tests/test_eval_gpu.py states both bounds). Off unless asked for.
const char* const kSgOptions[] = {"SG_NO_WINDOW", "SG_NO_GCN_FUSE", "SG_NO_TAIL_FUSE", "SG_NO_POLY_TAIL", "SG_NO_S2_WINDOW", "SG_TCONV_SMALL", "SG_GCN_BN", "SG_GCN_STEP32", "SG_F16", "SG_NO_BLOCK0_FUSE"};
// value of a switch: the handle's option if given, else the environment variable REGENNET_<KEY>, else `dflt`
int sg_opt(const rgn_stgcn_ctx* c, const char* key, int dflt) {
    auto it = c->opts.find(key);
    if (it != c->opts.end()) return it->second;
    const std::string env = std::string("REGENNET_") + key;
    if (const char* e = getenv(env.c_str())) return atoi(e);
    return dflt;
}

// data_bn + layout: output [N, V, M*C, T] (batch['output'], stgcn.py:83-101) -> x planes, rows (n M + m, t, v) with t < T + SG_PAD, channels c < C (the
// rest of the 32-channel block zero), BatchNorm1d channel index (m*V + v)*C + c; pad frames are written as zeros. One thread per row.
__global__ void k_sg_in(const float* __restrict__ out, SgPl x, const float* __restrict__ s, const float* __restrict__ t, int N, int V, int M, int C, int T) {
    const int Tp = T + SG_PAD;
    const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= (size_t)N * M * Tp * V) return;
    const int v = (int)(row % V);
    const int tp = (int)((row / V) % Tp);
    const int nm = (int)(row / ((size_t)V * Tp));
    const int tt = tp;
    float val[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) val[c] = 0.f;
    if (tt >= 0 && tt < T) {
        const int n = nm / M, m = nm % M;
        for (int c = 0; c < C && c < 32; ++c) {
            const int ch = (m * V + v) * C + c;
            val[c] = out[(((size_t)n * V + v) * (M * C) + m * C + c) * T + tt] * s[ch] + t[ch];
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float v8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v8[j] = val[8 * q + j];
        bf16x8 h, l;
        split_bf16(v8, h, l);
        *reinterpret_cast<bf16x8*>(x.hi + row * 32 + 8 * q) = h;
        *reinterpret_cast<bf16x8*>(x.lo + row * 32 + 8 * q) = l;
    }
}

// ... for a small graph (V < 28): the input keeps its V real vertices, [N, V, M*C, T], the planes carry Vp >= V rows per frame; a pad vertex's row is
// zero in every frame (data_bn's scale and shift are taken as zero there). Rows (n M + m, t, v < Vp).
__global__ void k_sg_in_pad(const float* __restrict__ out, SgPl x, const float* __restrict__ s, const float* __restrict__ t, int N, int V, int Vp, int M, int C, int T) {
    const int Tp = T + SG_PAD;
    const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= (size_t)N * M * Tp * Vp) return;
    const int v = (int)(row % Vp);
    const int tt = (int)((row / Vp) % Tp);
    const int nm = (int)(row / ((size_t)Vp * Tp));
    float val[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) val[c] = 0.f;
    if (tt < T && v < V) {
        const int n = nm / M, m = nm % M;
        for (int c = 0; c < C && c < 32; ++c) {
            const int ch = (m * V + v) * C + c;
            val[c] = out[(((size_t)n * V + v) * (M * C) + m * C + c) * T + tt] * s[ch] + t[ch];
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float v8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v8[j] = val[8 * q + j];
        bf16x8 h, l;
        split_bf16(v8, h, l);
        *reinterpret_cast<bf16x8*>(x.hi + row * 32 + 8 * q) = h;
        *reinterpret_cast<bf16x8*>(x.lo + row * 32 + 8 * q) = l;
    }
}

// z[(frame, w), k C + ci] = sum_v A'_k[v, w] x[(frame, v), ci] over the nonzeros of A'_k[:, w]. C % 32 == 0: one thread per (row, k, run of 8
// channels); the output channel k C + ci lies in plane block k C / 32 + ci / 32.
constexpr int SG_NZ_LDS = 1024;                // nonzero lists up to this many entries are staged in LDS (the SMPL-X skeleton has 166)
__global__ __launch_bounds__(256) void k_sg_agg(SgPl x, SgPl z, const int* __restrict__ nz_ptr, const int* __restrict__ nz_v, const float* __restrict__ nz_a, size_t rows, int V, int K, int C) {
    // lanes run along (16-byte quarter of a 64-byte plane row, row): a wave reads and writes contiguous 1 KiB runs of one plane block
    __shared__ int s_ptr[513], s_v[SG_NZ_LDS];
    __shared__ float s_a[SG_NZ_LDS];
    const int nlists = K * V, nnz = nz_ptr[nlists];
    const bool staged = nlists <= 512 && nnz <= SG_NZ_LDS;     // (uniform)
    if (staged) {
        for (int i = threadIdx.x; i <= nlists; i += 256) s_ptr[i] = nz_ptr[i];
        for (int i = threadIdx.x; i < nnz; i += 256) {
            s_v[i] = nz_v[i];
            s_a[i] = nz_a[i];
        }
        __syncthreads();
    }
    // grid: x over (row, quarter), y = output plane block (k, channel block): 32-bit index arithmetic only (64-bit div / mod per thread cost more than the
    // 64 bytes the thread moves)
    const int cbn = C / 32;
    const unsigned gx = blockIdx.x * 256u + threadIdx.x, row = gx >> 2;
    if (row >= (unsigned)rows) return;
    const int kb = blockIdx.y, k = kb / cbn, c8 = (kb - k * cbn) * 4 + (int)(gx & 3);
    const unsigned frame = row / (unsigned)V;
    const int w = (int)(row - frame * (unsigned)V);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const size_t in_off = plane_chunk(x.R, 0, c8 >> 2, c8 & 3);
    const int j0 = staged ? s_ptr[k * V + w] : nz_ptr[k * V + w], j1 = staged ? s_ptr[k * V + w + 1] : nz_ptr[k * V + w + 1];
    for (int j = j0; j < j1; ++j) {
        const size_t src = in_off + (size_t)(frame * (unsigned)V + (unsigned)(staged ? s_v[j] : nz_v[j])) * 32;
        const float a = staged ? s_a[j] : nz_a[j];
        const bf16x8 h = *reinterpret_cast<const bf16x8*>(x.hi + src), l = *reinterpret_cast<const bf16x8*>(x.lo + src);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(a, (float)h[e] + (float)l[e], acc[e]);
    }
    bf16x8 h, l;
    split_bf16(acc, h, l);
    const size_t dst = plane_chunk(z.R, row, k * (C / 32) + (c8 >> 2), c8 & 3);
    *reinterpret_cast<bf16x8*>(z.hi + dst) = h;
    *reinterpret_cast<bf16x8*>(z.lo + dst) = l;
}
// the first block (C = in_channels / persons = 6, K C <= 32): one thread per row writes the whole 32-channel output row
__global__ void k_sg_agg_small(SgPl x, SgPl z, const int* __restrict__ nz_ptr, const int* __restrict__ nz_v, const float* __restrict__ nz_a, size_t rows, int V, int K, int C) {
    const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const size_t frame = row / V;
    const int w = (int)(row - frame * V);
    float val[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) val[c] = 0.f;
    for (int k = 0; k < K; ++k)
        for (int j = nz_ptr[k * V + w]; j < nz_ptr[k * V + w + 1]; ++j) {
            const size_t src = (frame * V + nz_v[j]) * 32;
            const float a = nz_a[j];
            for (int c = 0; c < C; ++c) val[k * C + c] = fmaf(a, (float)x.hi[src + c] + (float)x.lo[src + c], val[k * C + c]);
        }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float v8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v8[j] = val[8 * q + j];
        bf16x8 h, l;
        split_bf16(v8, h, l);
        *reinterpret_cast<bf16x8*>(z.hi + row * 32 + 8 * q) = h;
        *reinterpret_cast<bf16x8*>(z.lo + row * 32 + 8 * q) = l;
    }
}

// ... and for the shapes the evaluation uses (C = 6 rot6d channels per person, K = 3 partitions; any C <= 8) with everything static: the sums stay in
// registers (the form above indexes val[k C + c] with run-time C: private memory) and a neighbour's channels are ONE 16-byte load per plane
template <int C, int K>
__global__ __launch_bounds__(256) void k_sg_agg_small_t(SgPl x, SgPl z, const int* __restrict__ nz_ptr, const int* __restrict__ nz_v, const float* __restrict__ nz_a, size_t rows, int V) {
    static_assert(C <= 8 && K * C <= 32, "one 16-byte chunk per neighbour, one 32-channel block out");
    const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const size_t frame = row / V;
    const int w = (int)(row - frame * V);
    float val[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) val[c] = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int j = nz_ptr[k * V + w]; j < nz_ptr[k * V + w + 1]; ++j) {
            const size_t src = (frame * V + nz_v[j]) * 32;
            const float a = nz_a[j];
            const bf16x8 h = *reinterpret_cast<const bf16x8*>(x.hi + src), l = *reinterpret_cast<const bf16x8*>(x.lo + src);
#pragma unroll
            for (int c = 0; c < C; ++c) val[k * C + c] = fmaf(a, (float)h[c] + (float)l[c], val[k * C + c]);
        }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float v8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v8[j] = val[8 * q + j];
        bf16x8 h, l;
        split_bf16(v8, h, l);
        *reinterpret_cast<bf16x8*>(z.hi + row * 32 + 8 * q) = h;
        *reinterpret_cast<bf16x8*>(z.lo + row * 32 + 8 * q) = l;
    }
}

// The whole graph convolution of the FIRST block for the evaluation's shapes (C = 6 channels per person, K = 3 partitions, 64 output channels) as one kernel: the
// aggregation above, then g = relu(z . W1'^T + b1'[w]) on the VALU in fp32 - 18 x 64 fmas per row with the weights as scalar operands (uniform addresses: s_load) -
// written as the temporal convolution's operand planes, split bf16 or (F16) one fp16 plane. Replaces k_sg_agg_small_t + k_gemm_x3<256, 64> (K = 18 padded to a
// 32-deep k-block, three MFMAs per product, z written and read back) [+ k_sg_to_f16]: 0.28 (0.39) -> 0.1 ms per 256 motions, and exact fp32 products.
template <int C, int K, int CO, bool F16>
__global__ __launch_bounds__(256) void k_sg_block0(SgPl x, SgPl g, const int* __restrict__ nz_ptr, const int* __restrict__ nz_v, const float* __restrict__ nz_a,
                                                   const float* __restrict__ W, const float* __restrict__ b1, size_t rows, int V) {
    static_assert(C <= 8 && CO % 32 == 0, "one 16-byte chunk per neighbour, whole 32-channel output blocks");
    const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const size_t frame = row / V;
    const int w = (int)(row - frame * V);
    float z[K * C];
#pragma unroll
    for (int q = 0; q < K * C; ++q) z[q] = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int j = nz_ptr[k * V + w]; j < nz_ptr[k * V + w + 1]; ++j) {
            const size_t src = (frame * V + nz_v[j]) * 32;
            const float a = nz_a[j];
            const bf16x8 h = *reinterpret_cast<const bf16x8*>(x.hi + src), l = *reinterpret_cast<const bf16x8*>(x.lo + src);
#pragma unroll
            for (int c = 0; c < C; ++c) z[k * C + c] = fmaf(a, (float)h[c] + (float)l[c], z[k * C + c]);
        }
    const float* bw = b1 + (size_t)w * CO;
#pragma unroll
    for (int og = 0; og < CO / 8; ++og) {
        const float4 ba = *reinterpret_cast<const float4*>(bw + 8 * og), bb = *reinterpret_cast<const float4*>(bw + 8 * og + 4);
        float acc[8] = {ba.x, ba.y, ba.z, ba.w, bb.x, bb.y, bb.z, bb.w};
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int q = 0; q < K * C; ++q) acc[j] = fmaf(z[q], W[(og * 8 + j) * (K * C) + q], acc[j]);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaxf(acc[j], 0.f);
        const size_t o = plane_chunk(g.R, row, og >> 2, og & 3);
        if constexpr (F16) {
            f16x8 f;
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = (_Float16)acc[j];
            *reinterpret_cast<f16x8*>(g.hi + o) = f;
        } else {
            bf16x8 h, l;
            split_bf16(acc, h, l);
            *reinterpret_cast<bf16x8*>(g.hi + o) = h;
            *reinterpret_cast<bf16x8*>(g.lo + o) = l;
        }
    }
}

// zero the pad frames and the guard rows of padded planes with `cb` channel blocks: sequences of Tr real + (Tp - Tr) pad frames starting at row
// `base` of every plane block, `lead` / `trail` guard rows in front of / behind the NM sequences (0: that side borders another region)
__global__ void k_sg_zero(SgPl g, long long base, int NM, int Tr, int Tp, int V, int cb, int lead, int trail) {
    const int npf = Tp - Tr;
    const size_t npad = (size_t)NM * npf * V, per = npad + (size_t)lead + (size_t)trail;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per * cb * 4) return;
    const int q = (int)(idx & 3);
    const size_t e = (idx >> 2) % per;
    const int b = (int)((idx >> 2) / per);
    long long row;
    if (e < npad) {
        const int nm = (int)(e / ((size_t)npf * V));
        const int r = (int)(e % ((size_t)npf * V));
        row = ((long long)nm * Tp + Tr + r / V) * V + (r % V);
    } else {
        const long long j = (long long)(e - npad);
        row = j < lead ? j - lead : (long long)NM * Tp * V + (j - lead);
    }
    bf16x8 zero;
#pragma unroll
    for (int j = 0; j < 8; ++j) zero[j] = (__bf16)0.f;
    const long long o = plane_chunk<long long>(g.R, base + row, b, q);
    *reinterpret_cast<bf16x8*>(g.hi + o) = zero;
    *reinterpret_cast<bf16x8*>(g.lo + o) = zero;
}

// split-bf16 planes -> the single fp16 plane of SG_F16, in place in the hi plane (block 0's graph convolution stays on the split GEMM: K = 32, 2 % of the forward):
// one thread per run of 8 channels of `cb` channel blocks x `rows` rows
__global__ void k_sg_to_f16(SgPl g, size_t rows, int cb) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * cb * 4) return;
    const size_t row = (idx >> 2) % rows;
    const size_t o = ((idx >> 2) / rows * (size_t)g.R + row) * 32 + 8 * (idx & 3);
    const bf16x8 h = *reinterpret_cast<const bf16x8*>(g.hi + o), l = *reinterpret_cast<const bf16x8*>(g.lo + o);
    f16x8 f;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (_Float16)((float)h[e] + (float)l[e]);
    *reinterpret_cast<f16x8*>(g.hi + o) = f;
}

// x'[nm][t'][v][co] = relu(conv[nm][t'][v][co] + b2[co] + res) as planes, pads of x' zero. conv / rfull rows run (nm, frame < Tpi, v): the block's own
// rate (a stride-2 block computes its convolution at the OUTPUT rate from polyphase planes: nothing is subsampled here).
//   res: none | identity x[nm][t'][v][co] (planes, same geometry) | rfull[nm][t'][v][co] + br[co] (the strided 1x1 convolution + BN)
// Output geometry: sequences of To real + 4 pad frames - or, when the NEXT block has stride 2 (opoly), polyphase: the even frames of all sequences as one
// region (Te = ceil(To / 2) real frames + 4 pads each), the odd frames as a second region of the SAME geometry (floor(To / 2) real frames, the rest pads)
// one thread per (output row, run of 8 channels)
__global__ void k_sg_post(const float* __restrict__ conv, const float* __restrict__ b2, SgPl xin, int res_id, const float* __restrict__ rfull,
                          const float* __restrict__ br, SgPl xout, int NM, int Tpi, int To, int opoly, int V, int C) {
    const int Te = (To + 1) >> 1, Tpo = opoly ? Te + SG_PAD : To + SG_PAD;
    const unsigned region = (unsigned)NM * Tpo * V, orows = opoly ? 2 * region : region;       // (32-bit index arithmetic: rows < 2^26)
    const unsigned gx = blockIdx.x * 256u + threadIdx.x, orow = gx >> 2;                       // lanes along (quarter of a plane row, row): contiguous 1 KiB plane stores per wave
    if (orow >= orows) return;
    const int c8 = blockIdx.y * 4 + (int)(gx & 3);                                             // grid y = channel block
    const unsigned rr = orow >= region ? orow - region : orow;
    const int odd = orow >= region ? 1 : 0;
    const unsigned fr = rr / (unsigned)V;
    const int v = (int)(rr - fr * (unsigned)V);
    const int nm = (int)(fr / (unsigned)Tpo);
    const int tpo = (int)(fr - (unsigned)nm * (unsigned)Tpo);
    const int to = opoly ? 2 * tpo + odd : tpo;               // the frame this output row holds (pads: beyond the real frames of its region)
    const bool real = opoly ? (tpo < (odd ? (To >> 1) : Te)) : (tpo < To);
    float val[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (real) {
        const size_t srow = ((size_t)nm * Tpi + (size_t)to) * V + v;
        const float4 c0 = *reinterpret_cast<const float4*>(conv + srow * C + 8 * c8), c1 = *reinterpret_cast<const float4*>(conv + srow * C + 8 * c8 + 4);
        const float4 bb0 = *reinterpret_cast<const float4*>(b2 + 8 * c8), bb1 = *reinterpret_cast<const float4*>(b2 + 8 * c8 + 4);
        val[0] = c0.x + bb0.x; val[1] = c0.y + bb0.y; val[2] = c0.z + bb0.z; val[3] = c0.w + bb0.w;
        val[4] = c1.x + bb1.x; val[5] = c1.y + bb1.y; val[6] = c1.z + bb1.z; val[7] = c1.w + bb1.w;
        if (rfull) {
            const float4 r0 = *reinterpret_cast<const float4*>(rfull + srow * C + 8 * c8), r1 = *reinterpret_cast<const float4*>(rfull + srow * C + 8 * c8 + 4);
            const float4 q0 = *reinterpret_cast<const float4*>(br + 8 * c8), q1 = *reinterpret_cast<const float4*>(br + 8 * c8 + 4);
            val[0] += r0.x + q0.x; val[1] += r0.y + q0.y; val[2] += r0.z + q0.z; val[3] += r0.w + q0.w;
            val[4] += r1.x + q1.x; val[5] += r1.y + q1.y; val[6] += r1.z + q1.z; val[7] += r1.w + q1.w;
        } else if (res_id) {                       // identity residual: stride 1, same channel count, same geometry as conv
            const size_t o = plane_chunk(xin.R, srow, c8 >> 2, c8 & 3);
            const bf16x8 h = *reinterpret_cast<const bf16x8*>(xin.hi + o), l = *reinterpret_cast<const bf16x8*>(xin.lo + o);
#pragma unroll
            for (int e = 0; e < 8; ++e) val[e] += (float)h[e] + (float)l[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) val[e] = fmaxf(val[e], 0.f);
    }
    bf16x8 h, l;
    split_bf16(val, h, l);
    const size_t o = plane_chunk(xout.R, orow, c8 >> 2, c8 & 3);
    *reinterpret_cast<bf16x8*>(xout.hi + o) = h;
    *reinterpret_cast<bf16x8*>(xout.lo + o) = l;
}

// global average pool over (t, v) and mean over the M persons (stgcn.py:113-114): pooled[n][c]. One workgroup per motion: thread = (run of 8 channels,
// slice of the rows), 16-byte plane loads, the slices summed through LDS
template <bool F16>
__global__ __launch_bounds__(256) void k_sg_pool(SgPl x, float* __restrict__ pooled, int M, int T, int V, int C) {
    __shared__ float part[8][256];
    const int n = blockIdx.x, Tp = T + SG_PAD, c8n = C / 8;                      // C <= 256: c8n <= 32
    const int c8 = threadIdx.x % 32, sl = threadIdx.x / 32;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c8 < c8n)
        for (int m = 0; m < M; ++m) {
            const size_t o = plane_chunk(x.R, ((size_t)(n * M + m) * Tp) * V, c8 >> 2, c8 & 3);
            for (int i = sl; i < T * V; i += 8) {
                if constexpr (F16) {
                    const f16x8 h = *reinterpret_cast<const f16x8*>(x.hi + o + (size_t)i * 32);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += (float)h[e];
                } else {
                    const bf16x8 h = *reinterpret_cast<const bf16x8*>(x.hi + o + (size_t)i * 32), l = *reinterpret_cast<const bf16x8*>(x.lo + o + (size_t)i * 32);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += (float)h[e] + (float)l[e];
                }
            }
        }
#pragma unroll
    for (int e = 0; e < 8; ++e) part[sl][(8 * c8 + e) & 255] = acc[e];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float a = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) a += part[q][c];
        pooled[(size_t)n * C + c] = a / (float)(T * V) / (float)M;
    }
}

// ... of a small graph: the planes hold Vp rows per frame of which the first V are vertices. Behind a temporal convolution a pad row holds relu(b2' ...),
// not zero: the pool SKIPS the pad rows (no producer zeroes them) and divides by the T V real ones.
__global__ __launch_bounds__(256) void k_sg_pool_pad(SgPl x, float* __restrict__ pooled, int M, int T, int V, int Vp, int C) {
    __shared__ float part[8][256];
    const int n = blockIdx.x, Tp = T + SG_PAD, c8n = C / 8;                      // C <= 256: c8n <= 32
    const int c8 = threadIdx.x % 32, sl = threadIdx.x / 32;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c8 < c8n)
        for (int m = 0; m < M; ++m) {
            const size_t o = plane_chunk(x.R, ((size_t)(n * M + m) * Tp) * Vp, c8 >> 2, c8 & 3);
            for (int i = sl; i < T * Vp; i += 8) {
                if (i % Vp >= V) continue;
                const bf16x8 h = *reinterpret_cast<const bf16x8*>(x.hi + o + (size_t)i * 32), l = *reinterpret_cast<const bf16x8*>(x.lo + o + (size_t)i * 32);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += (float)h[e] + (float)l[e];
            }
        }
#pragma unroll
    for (int e = 0; e < 8; ++e) part[sl][(8 * c8 + e) & 255] = acc[e];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float a = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) a += part[q][c];
        pooled[(size_t)n * C + c] = a / (float)(T * V) / (float)M;
    }
}

template <typename T>
int sg_alloc(rgn_stgcn_ctx* c, T** p, size_t count) {
    void* q = nullptr;
    SG_HIP(c, hipMalloc(&q, count * sizeof(T) + 256));
    SG_HIP(c, hipMemset(q, 0, count * sizeof(T) + 256));
    c->allocs.push_back(q);
    *p = reinterpret_cast<T*>(q);
    return RGN_OK;
}
int sg_upload(rgn_stgcn_ctx* c, float** p, const std::vector<float>& v) {
    int rc = sg_alloc(c, p, v.size());
    if (rc) return rc;
    SG_HIP(c, hipMemcpy(*p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    return RGN_OK;
}
inline size_t up32(size_t x) { return (x + 31) / 32 * 32; }
// physical rows of a block's planes for `seqs` sequences of T frames: T + 4 frames each - or, in front of a stride-2 block, the POLYPHASE form: two regions
// (even / odd frames) of ceil(T / 2) + 4 frames per sequence each, so that the block's temporal convolution runs at the OUTPUT rate
inline size_t sg_plane_rows(size_t seqs, int T, bool poly, int V) { return seqs * (poly ? 2 * ((size_t)(T + 1) / 2 + SG_PAD) : (size_t)T + SG_PAD) * V; }
// W [N][Kp] (row-major fp32, Kp % 32 == 0) -> split-bf16 weight planes [Kp/32][N][32] (the B operand layout of k_gemm_x3)
// ... and, with `f16`, the same layout as one IEEE fp16 plane (rne); a weight beyond the fp16 range is recorded in c->f16_refused under `name`
int sg_upload_planes(rgn_stgcn_ctx* c, const std::vector<float>& W, int N, int Kp, __bf16** hi, __bf16** lo, __bf16** f16 = nullptr, const char* name = "") {
    std::vector<uint16_t> h((size_t)N * Kp), l((size_t)N * Kp), f(f16 ? (size_t)N * Kp : 0);
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < Kp; ++k) {
            const float v = W[(size_t)n * Kp + k];
            const size_t o = plane_off(N, n, k);
            h[o] = f2bf(v);
            l[o] = f2bf(v - bf2f(h[o]));
            if (f16) {
                if (!(std::fabs(v) < 6.0e4f) && c->f16_refused.empty()) c->f16_refused = std::string(name) + " (folded with its BatchNorm) holds " + std::to_string(v);
                const _Float16 hv = (_Float16)v;
                memcpy(&f[o], &hv, 2);
            }
        }
    int rc;
    if ((rc = sg_alloc(c, hi, h.size())) || (rc = sg_alloc(c, lo, l.size()))) return rc;
    SG_HIP(c, hipMemcpy(*hi, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    SG_HIP(c, hipMemcpy(*lo, l.data(), l.size() * 2, hipMemcpyHostToDevice));
    if (f16) {
        if ((rc = sg_alloc(c, f16, f.size()))) return rc;
        SG_HIP(c, hipMemcpy(*f16, f.data(), f.size() * 2, hipMemcpyHostToDevice));
    }
    return RGN_OK;
}
int sg_upload_ints(rgn_stgcn_ctx* c, int** p, const std::vector<int>& v) {
    int rc = sg_alloc(c, p, v.size());
    if (rc) return rc;
    SG_HIP(c, hipMemcpy(*p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
    return RGN_OK;
}

GemmArgs sg_gemm(const float* A, int lda, const float* W, int Kp, int K, const float* bias, float* C, int ldc, int M, int N) {
    GemmArgs g{};
    g.A = A; g.lda = lda; g.W = W; g.bias = bias; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.Kp = Kp;
    return g;
}
// split-bf16 GEMM over activation planes A (kblocks x [R][32]) and weight planes [Kp/32][N][32]
GemmX3Args sg_gemm_x3(const SgPl& A, const __bf16* Wh, const __bf16* Wl, int M, int N, int Kp) {
    GemmX3Args g{};
    g.Ahi = A.hi; g.Alo = A.lo; g.a_rows = (int)A.R;
    g.Whi = Wh; g.Wlo = Wl;
    g.M = M; g.N = N; g.Kp = Kp;
    return g;
}

int sg_boundary_error(rgn_stgcn_ctx* h, const char* fn, const char* what) noexcept {
    try {
        std::string m = std::string(fn) + ": C++ exception at the boundary: " + what;
        if (h) h->err.swap(m);
        else g_sg_create_error.swap(m);
    } catch (...) {
    }
    return RGN_ERR_INTERNAL;
}
// no C++ exception crosses the C boundary (see rgn_guard in rgn_abi.cpp)
template <class F>
int sg_guard(rgn_stgcn_ctx* h, const char* fn, F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return sg_boundary_error(h, fn, "std::bad_alloc (host memory)");
    } catch (const std::exception& e) {
        return sg_boundary_error(h, fn, e.what());
    } catch (...) {
        return sg_boundary_error(h, fn, "unknown exception");
    }
}

}  // namespace

extern "C" {

const char* rgn_stgcn_last_error(rgn_stgcn_handle h) { return h ? h->err.c_str() : g_sg_create_error.c_str(); }

int rgn_stgcn_create(const rgn_stgcn_config* cfg, rgn_stgcn_handle* out) {
    return sg_guard(static_cast<rgn_stgcn_ctx*>(nullptr), "rgn_stgcn_create", [&]() -> int {
        if (!cfg || !out) {
            g_sg_create_error = "rgn_stgcn_create: null argument";
            return RGN_ERR_INVALID_ARG;
        }
        *out = nullptr;
        if (cfg->in_channels <= 0 || cfg->num_person <= 0 || cfg->in_channels % cfg->num_person || cfg->num_class <= 0 || cfg->num_nodes <= 0 ||
            cfg->num_frames <= 0 || cfg->max_batch <= 0) {
            g_sg_create_error = "rgn_stgcn_create: non-positive dimension or in_channels % num_person != 0";
            return RGN_ERR_INVALID_ARG;
        }
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) {
            g_sg_create_error = "rgn_stgcn_create: no such HIP device";
            return RGN_ERR_HIP;
        }
        rgn_stgcn_ctx* c = new rgn_stgcn_ctx();
        c->cfg = *cfg;
        c->V = cfg->num_nodes;
        c->Vp = sg_padded_nodes(c->V);
        c->P = sg_bias_period(c->V);
        c->C0 = cfg->in_channels / cfg->num_person;
        *out = c;
        return RGN_OK;
    });
}

int rgn_stgcn_destroy(rgn_stgcn_handle h) {
    return sg_guard(h, "rgn_stgcn_destroy", [&]() -> int {
        if (!h) return RGN_ERR_INVALID_ARG;
        (void)hipSetDevice(h->cfg.device);
        (void)hipDeviceSynchronize();
        if (h->ev_in) (void)hipEventDestroy(h->ev_in);
        if (h->ev_out) (void)hipEventDestroy(h->ev_out);
        if (h->stream) (void)hipStreamDestroy(h->stream);
        for (void* p : h->allocs) (void)hipFree(p);
        delete h;
        return RGN_OK;
    });
}

int rgn_stgcn_load_weight(rgn_stgcn_handle h, const char* key, const float* host, const int64_t* shape, int32_t ndim) {
    return sg_guard(h, "rgn_stgcn_load_weight", [&]() -> int {
        if (!h) return RGN_ERR_INVALID_ARG;
        if (!key || !host || ndim < 0 || (ndim > 0 && !shape)) return h->fail(RGN_ERR_INVALID_ARG, "rgn_stgcn_load_weight: null/empty argument");
        if (h->finalized) return h->fail(RGN_ERR_STATE, "rgn_stgcn_load_weight: already finalized");
        size_t n = 1;
        for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
        h->sd[key].assign(host, host + n);
        h->shapes[key].assign(shape, shape + ndim);
        return RGN_OK;
    });
}

int rgn_stgcn_check_blocks(int32_t n_blocks, const int32_t* out_channels, const int32_t* strides, char* err, int32_t cap) {
    return sg_guard(static_cast<rgn_stgcn_ctx*>(nullptr), "rgn_stgcn_check_blocks", [&]() -> int {
        std::string m;
        const bool ok = sg_plan_check(n_blocks, out_channels, strides, nullptr, &m);
        if (err && cap > 0) {
            const size_t n = std::min(m.size(), (size_t)cap - 1);
            memcpy(err, m.data(), n);
            err[n] = 0;
        }
        return ok ? RGN_OK : RGN_ERR_INVALID_ARG;
    });
}

int rgn_stgcn_set_blocks(rgn_stgcn_handle h, int32_t n_blocks, const int32_t* out_channels, const int32_t* strides) {
    return sg_guard(h, "rgn_stgcn_set_blocks", [&]() -> int {
        if (!h) return RGN_ERR_INVALID_ARG;
        if (h->finalized) return h->fail(RGN_ERR_STATE, "rgn_stgcn_set_blocks: already finalized");
        std::string m;
        std::vector<SgBlockDef> plan;
        if (!sg_plan_check(n_blocks, out_channels, strides, &plan, &m)) return h->fail(RGN_ERR_INVALID_ARG, "rgn_stgcn_set_blocks: " + m);
        h->plan.swap(plan);
        return RGN_OK;
    });
}

int rgn_stgcn_finalize(rgn_stgcn_handle h) {
    return sg_guard(h, "rgn_stgcn_finalize", [&]() -> int {
        if (!h) return RGN_ERR_INVALID_ARG;
        rgn_stgcn_ctx* c = h;
        if (c->finalized) return c->fail(RGN_ERR_STATE, "rgn_stgcn_finalize: already finalized");
        SG_HIP(c, hipSetDevice(c->cfg.device));
        std::string missing;
        auto need = [&](const std::string& k, size_t n) -> const float* {
            auto it = c->sd.find(k);
            if (it == c->sd.end()) {
                missing += (missing.empty() ? "" : ", ") + k;
                return nullptr;
            }
            if (it->second.size() != n) {
                missing += (missing.empty() ? "" : ", ") + k + " (size " + std::to_string(it->second.size()) + " != " + std::to_string(n) + ")";
                return nullptr;
            }
            return it->second.data();
        };
        auto itA = c->sd.find("A");
        if (itA == c->sd.end() || c->shapes["A"].size() != 3 || c->shapes["A"][1] != c->V || c->shapes["A"][2] != c->V)
            return c->fail(RGN_ERR_MISSING_KEY, "rgn_stgcn_finalize: adjacency buffer 'A' [K, V, V] missing or of the wrong shape");
        c->K = (int)c->shapes["A"][0];
        const int V = c->V, K = c->K, M = c->cfg.num_person, C0 = c->C0;
        // Small graphs: the planes run on Vp >= V vertices per frame (rgn_sg_plan.h). A pad vertex is ISOLATED - it has no entry in any aggregation list and
        // b1' = 0, so it is zero behind every graph convolution - and the vertex bias table is replicated to P rows (add_mod). V >= 28: Vp = P = V.
        const int Vp = c->Vp, P = c->P, nb = (int)c->plan.size();
        for (const auto& kv : c->sd)
            if (sg_key_block(kv.first) >= nb)
                return c->fail(RGN_ERR_BAD_KEY, "rgn_stgcn_finalize: the checkpoint holds '" + kv.first + "' but the block plan has " + std::to_string(nb) + " blocks (rgn_stgcn_set_blocks)");
        const float* A0 = itA->second.data();
        // BatchNorm (eval): y = x * s + t with s = gamma / sqrt(var + eps), t = beta - mean * s
        auto bn_fold = [&](const std::string& p, int n, std::vector<double>& s, std::vector<double>& t) -> bool {
            const float *w = need(p + ".weight", n), *b = need(p + ".bias", n), *mu = need(p + ".running_mean", n), *var = need(p + ".running_var", n);
            if (!w || !b || !mu || !var) return false;
            s.resize(n);
            t.resize(n);
            for (int i = 0; i < n; ++i) {
                s[i] = (double)w[i] / std::sqrt((double)var[i] + 1e-5);
                t[i] = (double)b[i] - (double)mu[i] * s[i];
            }
            return true;
        };
        int rc;
        {
            std::vector<double> s, t;
            if (bn_fold("data_bn", M * V * C0, s, t)) {
                std::vector<float> sf(s.begin(), s.end()), tf(t.begin(), t.end());
                if ((rc = sg_upload(c, &c->bn_s, sf)) || (rc = sg_upload(c, &c->bn_t, tf))) return rc;
            }
        }
        c->blocks.resize(nb);
        for (int i = 0; i < nb; ++i) {
            SgBlock& b = c->blocks[i];
            const std::string p = "st_gcn_networks." + std::to_string(i) + ".";
            b.ci = i == 0 ? C0 : c->plan[i].ci;
            b.co = c->plan[i].co;
            b.stride = c->plan[i].stride;
            b.res_conv = c->plan[i].res_conv;
            b.res_id = c->plan[i].res_id;
            const int ci = b.ci, co = b.co, K1 = K * ci;
            const float* imp = need("edge_importance." + std::to_string(i), (size_t)K * V * V);
            const float *wg = need(p + "gcn.conv.weight", (size_t)K * co * ci), *bg = need(p + "gcn.conv.bias", (size_t)K * co);
            const float *wt = need(p + "tcn.2.weight", (size_t)co * co * 9), *bt = need(p + "tcn.2.bias", co);
            std::vector<double> s1, t1, s2, t2, sr, tr;
            const bool ok1 = bn_fold(p + "tcn.0", co, s1, t1), ok2 = bn_fold(p + "tcn.3", co, s2, t2);
            const float *wr = nullptr, *brs = nullptr;
            bool okr = true;
            if (b.res_conv) {
                wr = need(p + "residual.0.weight", (size_t)co * ci);
                brs = need(p + "residual.0.bias", co);
                okr = bn_fold(p + "residual.1", co, sr, tr);
            }
            if (!imp || !wg || !bg || !wt || !bt || !ok1 || !ok2 || !okr || (b.res_conv && (!wr || !brs))) continue;
            std::vector<float> Ak((size_t)K * V * V);
            for (size_t j = 0; j < Ak.size(); ++j) Ak[j] = A0[j] * imp[j];                       // stgcn.py:105 (fp32 product, as there)
            // nonzero lists of A'_k[:, w] (the skeleton graph is sparse; a dense A simply gives V entries per list)
            std::vector<int> nzp((size_t)K * Vp + 1, 0), nzv;     // (lists run over the Vp plane vertices; a pad vertex's are empty)
            std::vector<float> nza;
            for (int k = 0; k < K; ++k)
                for (int w = 0; w < Vp; ++w) {
                    for (int v = 0; v < V && w < V; ++v)
                        if (Ak[((size_t)k * V + v) * V + w] != 0.f) {
                            nzv.push_back(v);
                            nza.push_back(Ak[((size_t)k * V + v) * V + w]);
                        }
                    nzp[(size_t)k * Vp + w + 1] = (int)nzv.size();
                }
            if (nzv.empty()) { nzv.push_back(0); nza.push_back(0.f); }
            // W1'[co][(k, ci)] = s1[co] * Wg[k*co_n + co][ci];  b1'[w][co] = s1 * sum_k bg[k*co_n + co] * colsum_k[w] + t1
            b.kp1 = (int)up32((size_t)K1);
            std::vector<float> W1((size_t)co * b.kp1, 0.f), b1((size_t)P * co, 0.f);    // b1': P rows, row r = vertex r % Vp (zero for a pad vertex)
            for (int o = 0; o < co; ++o)
                for (int k = 0; k < K; ++k)
                    for (int q = 0; q < ci; ++q) W1[(size_t)o * b.kp1 + k * ci + q] = (float)(s1[o] * (double)wg[((size_t)k * co + o) * ci + q]);
            for (int w = 0; w < V; ++w)
                for (int o = 0; o < co; ++o) {
                    double acc = 0.0;
                    for (int k = 0; k < K; ++k) {
                        double cs = 0.0;
                        for (int v = 0; v < V; ++v) cs += (double)Ak[((size_t)k * V + v) * V + w];
                        acc += (double)bg[(size_t)k * co + o] * cs;
                    }
                    b1[(size_t)w * co + o] = (float)(s1[o] * acc + t1[o]);
                }
            for (int r = Vp; r < P; ++r) std::copy(b1.begin() + (size_t)(r % Vp) * co, b1.begin() + (size_t)(r % Vp + 1) * co, b1.begin() + (size_t)r * co);
            // W2'[co][(channel block, dt, channel in block)] = s2[co] * Wt[co][ci][dt] (K = 9 co in the order the shifted-row GEMM walks: taps innermost
            // per 32-channel block, so that consecutive k-steps re-read one channel block of the activation 56 rows further on);  b2' = s2 * bt + t2
            std::vector<float> W2((size_t)co * 9 * co, 0.f), b2(co);
            for (int dt = 0; dt < 9; ++dt)
                for (int o = 0; o < co; ++o)
                    for (int q = 0; q < co; ++q)
                        W2[(size_t)o * 9 * co + ((size_t)(q / 32) * 9 + dt) * 32 + q % 32] = (float)(s2[o] * (double)wt[((size_t)o * co + q) * 9 + dt]);
            for (int o = 0; o < co; ++o) b2[o] = (float)(s2[o] * (double)bt[o] + t2[o]);
            {   // slot form of the lists: partition k owns as many slots as its longest list
                std::vector<int> cnt(K, 0);
                int total = 0;
                for (int k = 0; k < K; ++k) {
                    for (int w = 0; w < Vp; ++w) cnt[k] = std::max(cnt[k], nzp[(size_t)k * Vp + w + 1] - nzp[(size_t)k * Vp + w]);
                    total += cnt[k];
                }
                if (total <= 8 && K <= 8) {
                    std::vector<int> sv((size_t)Vp * 8);
                    std::vector<float> sa((size_t)Vp * 8, 0.f);
                    b.slot_k = 0xFFFFFFFFu;
                    for (int w = 0; w < Vp; ++w) {
                        int sidx = 0;
                        for (int k = 0; k < K; ++k)
                            for (int i = 0; i < cnt[k]; ++i, ++sidx) {
                                const int j = nzp[(size_t)k * Vp + w] + i;
                                const bool real = j < nzp[(size_t)k * Vp + w + 1];
                                sv[(size_t)w * 8 + sidx] = real ? nzv[j] : w;
                                sa[(size_t)w * 8 + sidx] = real ? nza[j] : 0.f;
                                b.slot_k = (b.slot_k & ~(15u << (4 * sidx))) | ((unsigned)k << (4 * sidx));
                            }
                        for (; sidx < 8; ++sidx) sv[(size_t)w * 8 + sidx] = w;
                    }
                    if ((rc = sg_upload_ints(c, &b.sl_v, sv)) || (rc = sg_upload(c, &b.sl_a, sa))) return rc;
                }
            }
            if ((rc = sg_upload_ints(c, &b.nz_ptr, nzp)) || (rc = sg_upload_ints(c, &b.nz_v, nzv)) || (rc = sg_upload(c, &b.nz_a, nza)) ||
                (rc = sg_upload_planes(c, W1, co, b.kp1, &b.W1h, &b.W1l, &b.W1f, (p + "gcn.conv.weight").c_str())) || (rc = sg_upload(c, &b.b1, b1)) ||
                (rc = sg_upload_planes(c, W2, co, 9 * co, &b.W2h, &b.W2l, &b.W2f, (p + "tcn.2.weight").c_str())) || (rc = sg_upload(c, &b.b2, b2)))
                return rc;
            if (i == 0) {
                std::vector<float> Ws((size_t)co * K1);
                for (int o = 0; o < co; ++o)
                    for (int q = 0; q < K1; ++q) Ws[(size_t)o * K1 + q] = W1[(size_t)o * b.kp1 + q];
                if ((rc = sg_upload(c, &b.W1s, Ws))) return rc;
            }
            if (b.res_conv) {
                b.kpr = (int)up32((size_t)ci);
                std::vector<float> Wr((size_t)co * b.kpr, 0.f), br(co);
                for (int o = 0; o < co; ++o) {
                    for (int q = 0; q < ci; ++q) Wr[(size_t)o * b.kpr + q] = (float)(sr[o] * (double)wr[(size_t)o * ci + q]);
                    br[o] = (float)(sr[o] * (double)brs[o] + tr[o]);
                }
                std::vector<float> b2r(co);
                for (int o = 0; o < co; ++o) b2r[o] = b2[o] + br[o];
                if ((rc = sg_upload_planes(c, Wr, co, b.kpr, &b.Wrh, &b.Wrl, &b.Wrf, (p + "residual.0.weight").c_str())) || (rc = sg_upload(c, &b.br, br)) || (rc = sg_upload(c, &b.b2r, b2r))) return rc;
            }
        }
        {
            const int nc = c->cfg.num_class;
            const float *wf = need("fcn.weight", (size_t)nc * 256), *bf = need("fcn.bias", nc);
            if (wf && bf) {
                std::vector<float> W(wf, wf + (size_t)nc * 256), B(bf, bf + nc);
                if ((rc = sg_upload(c, &c->Wf, W)) || (rc = sg_upload(c, &c->bf, B))) return rc;
            }
        }
        if (!missing.empty()) return c->fail(RGN_ERR_MISSING_KEY, "missing / mis-shaped keys in the ST-GCN state_dict: " + missing);
        c->sd.clear();
        // The plane kernels assume: channel counts of the blocks are multiples of 32 (64 / 128 / 256) behind a first block whose K C_in fits one
        // 32-channel block, and the vertex bias row (row % P) wraps at most once inside a 32-row MFMA tile (P >= 28: a small graph's table is replicated)
        if (K * C0 > 32 || C0 > 32) return c->fail(RGN_ERR_UNSUPPORTED, "rgn_stgcn_finalize: needs K * (in_channels / persons) <= 32");
        // workspace: padded activation planes sized for the largest block (the 8 pad frames make the late, short blocks the big ones),
        // with guard rows at both ends of every plane block so that the +-4-frame row shifts of the temporal convolution never leave it
        c->guard = (size_t)SG_PAD * Vp;
        size_t xmax = 0, zmax = 0, gmax = 0, cmax = 0;     // elements per plane / fp32 tensor
        {
            auto phys = [&](int T, bool poly) { return sg_plane_rows((size_t)c->cfg.max_batch * M, T, poly, Vp); };
            int T = c->cfg.num_frames;
            for (int i = 0; i < nb; ++i) {
                const SgBlock& b = c->blocks[i];
                const size_t rows = phys(T, b.stride == 2), R = rows + 2 * c->guard;
                if (rows >= ((size_t)1 << 26)) return c->fail(RGN_ERR_UNSUPPORTED, "rgn_stgcn_finalize: max_batch x persons x frames x nodes beyond 2^26 rows");
                if (b.stride != 1 && b.stride != 2) return c->fail(RGN_ERR_UNSUPPORTED, "rgn_stgcn_finalize: temporal stride other than 1 or 2");
                xmax = std::max(xmax, up32((size_t)b.ci) * R);
                zmax = std::max(zmax, (size_t)b.kp1 * R);
                gmax = std::max(gmax, (size_t)b.co * R);
                cmax = std::max(cmax, rows * b.co);
                T = (T + b.stride - 1) / b.stride;
                const size_t rows_o = phys(T, i + 1 < nb && c->blocks[i + 1].stride == 2);
                xmax = std::max(xmax, (size_t)b.co * (rows_o + 2 * c->guard));
            }
        }
        for (int pl = 0; pl < 2; ++pl)
            if ((rc = sg_alloc(c, &c->xa[pl], xmax)) || (rc = sg_alloc(c, &c->xb[pl], xmax)) || (rc = sg_alloc(c, &c->z[pl], zmax)) || (rc = sg_alloc(c, &c->g[pl], gmax)))
                return rc;
        if ((rc = sg_alloc(c, &c->conv, cmax))) return rc;
        if ((rc = sg_alloc(c, &c->rfull, cmax))) return rc;
        if ((rc = sg_alloc(c, &c->pooled, (size_t)c->cfg.max_batch * 256))) return rc;
        SG_HIP(c, configure_gemm_x3_sg());
        SG_HIP(c, configure_sg_tconv());
        SG_HIP(c, configure_sg_tconv_pre());
        SG_HIP(c, configure_sg_gcn());
        SG_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        SG_HIP(c, hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming));
        SG_HIP(c, hipEventCreateWithFlags(&c->ev_out, hipEventDisableTiming));
        c->finalized = true;
        return RGN_OK;
    });
}

int rgn_stgcn_set_option(rgn_stgcn_handle h, const char* key, int32_t value) {
    return sg_guard(h, "rgn_stgcn_set_option", [&]() -> int {
        if (!h) return RGN_ERR_INVALID_ARG;
        if (!key) return h->fail(RGN_ERR_INVALID_ARG, "rgn_stgcn_set_option: null key");
        for (const char* k : kSgOptions)
            if (!strcmp(k, key)) {
                h->opts[key] = value;
                return RGN_OK;
            }
        return h->fail(RGN_ERR_BAD_KEY, std::string("rgn_stgcn_set_option: unknown switch '") + key + "'");
    });
}

int rgn_stgcn_forward(rgn_stgcn_handle h, int32_t N, const float* output, float* features, float* yhat, void* stream) {
    return sg_guard(h, "rgn_stgcn_forward", [&]() -> int {
        if (!h) return RGN_ERR_INVALID_ARG;
        rgn_stgcn_ctx* c = h;
        if (!c->finalized) return c->fail(RGN_ERR_STATE, "rgn_stgcn_forward: weights not finalized");
        if (N <= 0 || N > c->cfg.max_batch) return c->fail(RGN_ERR_INVALID_ARG, "rgn_stgcn_forward: N outside (0, max_batch]");
        if (!output || (!features && !yhat)) return c->fail(RGN_ERR_INVALID_ARG, "rgn_stgcn_forward: null pointer");
        SG_HIP(c, hipSetDevice(c->cfg.device));
        hipStream_t us = reinterpret_cast<hipStream_t>(stream), s = c->stream;
        SG_HIP(c, hipEventRecord(c->ev_in, us));
        SG_HIP(c, hipStreamWaitEvent(s, c->ev_in, 0));
        // V: vertices per frame of the PLANES (a small graph's padded count; the input and the pool know the real c->V), nb: blocks of the handle's plan
        const int V = c->Vp, K = c->K, M = c->cfg.num_person, NM = N * M, nb = (int)c->blocks.size();
        const bool small_graph = c->V < 28;
        const int guard = (int)c->guard;
        int T = c->cfg.num_frames;
        auto planes = [&](__bf16* const (&buf)[2], size_t rows) { return SgPl{buf[0] + (size_t)guard * 32, buf[1] + (size_t)guard * 32, (long long)(rows + 2 * (size_t)guard)}; };
        auto blocks1d = [](size_t n) { return dim3((unsigned)((n + 255) / 256)); };
        {
            const size_t rows = (size_t)NM * (T + SG_PAD) * V;
            if (small_graph) hipLaunchKernelGGL(k_sg_in_pad, blocks1d(rows), dim3(256), 0, s, output, planes(c->xa, rows), c->bn_s, c->bn_t, N, c->V, V, M, c->C0, T);
            else hipLaunchKernelGGL(k_sg_in, blocks1d(rows), dim3(256), 0, s, output, planes(c->xa, rows), c->bn_s, c->bn_t, N, V, M, c->C0, T);
        }
        // kernel forms (defaults: everything fused; the switches exist for tools and for the tests that run every form against the goldens)
        const bool no_window = sg_opt(c, "SG_NO_WINDOW", 0) != 0;        // the row-shifted GEMM for every temporal convolution
        const bool no_fuse = sg_opt(c, "SG_NO_GCN_FUSE", 0) != 0;        // aggregation and 1x1 GEMM as two launches
        const bool no_tail = sg_opt(c, "SG_NO_TAIL_FUSE", 0) != 0;       // k_sg_post for every block
        const bool no_poly = sg_opt(c, "SG_NO_POLY_TAIL", 0) != 0;       // ... only for the blocks whose output is polyphase
        const bool no_s2 = sg_opt(c, "SG_NO_S2_WINDOW", 0) != 0;         // row-shifted GEMM + shortcut GEMM + k_sg_post for the stride-2 blocks
        const bool small_tiles = sg_opt(c, "SG_TCONV_SMALL", 0) != 0;    // 256-row, <= 128-wide temporal-convolution tiles
        const int gcn_bn = sg_opt(c, "SG_GCN_BN", 256);                  // widest k_sg_gcn tile
        const bool gcn_step32 = sg_opt(c, "SG_GCN_STEP32", 0) != 0;      // 64-wide k_sg_gcn: one barrier per 32-deep k-block (default: per channel block)
        const bool f16 = sg_opt(c, "SG_F16", 0) != 0;                    // single fp16 operand planes (above): the fused kernels only
        const bool no_block0 = sg_opt(c, "SG_NO_BLOCK0_FUSE", 0) != 0;   // first block's graph convolution as aggregation + split GEMM (+ conversion)
        if (f16 && !c->f16_refused.empty()) return c->fail(RGN_ERR_UNSUPPORTED, "rgn_stgcn_forward: SG_F16 - a weight lies beyond the fp16 range: " + c->f16_refused);
        auto f16_unserved = [&](int blk, const char* what) {
            return c->fail(RGN_ERR_UNSUPPORTED, std::string("rgn_stgcn_forward: SG_F16 exists for the fused kernels only; block ") + std::to_string(blk) + " would take " + what +
                                                    " (this graph / shape, or an SG_NO_* switch)");
        };
        __bf16 *(*x)[2] = &c->xa, *(*xn)[2] = &c->xb;
        auto phys = [&](int Tf, bool poly) { return sg_plane_rows((size_t)NM, Tf, poly, V); };
        for (int i = 0; i < nb; ++i) {
            const SgBlock& b = c->blocks[i];
            // a stride-2 block reads POLYPHASE planes (written so by the block in front of it): region E = the even frames of every sequence, region O = the odd
            // ones, Te + 4 frames per sequence in both - its 9-tap stride-2 convolution is then five row-shifted taps on E and four on O at the OUTPUT rate
            const bool ipoly = b.stride == 2, opoly = i + 1 < nb && c->blocks[i + 1].stride == 2;
            const int To = (T + b.stride - 1) / b.stride, Te = (T + 1) / 2;   // Conv2d(9x1, pad 4, stride s): ceil(T / s) frames
            const int Tpi = ipoly ? Te + SG_PAD : T + SG_PAD;                 // frames per sequence of the rows the convolution is computed on
            const size_t rows = phys(T, ipoly), rows_c = (size_t)NM * Tpi * V, rows_o = phys(To, opoly);
            const SgPl xp = planes(*x, rows), zp = planes(c->z, rows), gp = planes(c->g, rows), xo = planes(*xn, rows_o);
            // graph aggregation on the input channels (sparse A'), then the 1x1 convolution over K C_in (+ folded BN, vertex bias, ReLU): frame-local, any row order
            const bool fused = !no_fuse && b.sl_v && b.ci % 32 == 0 && b.kp1 == K * b.ci && sg_gcn_supported(b.co, b.kp1, V, K);
            if (f16 && !fused && i > 0) return f16_unserved(i, "the two-launch graph convolution");
            const bool gf16 = f16 && fused;                      // (block 0, K C_in = 18 of one 32-deep k-block, keeps the split GEMM: its planes come from k_sg_in)
            GemmX3Args g1 = sg_gemm_x3(fused ? xp : zp, gf16 ? b.W1f : b.W1h, b.W1l, (int)rows, b.co, b.kp1);
            g1.add = b.b1; g1.ldadd = b.co; g1.add_mod = c->P; g1.act = 3;                       // + b1'[row % P], ReLU (P = V unless the graph is small)
            g1.Chi = gp.hi; g1.Clo = gp.lo; g1.c_rows = (int)gp.R;
            g1.f16 = gf16 ? 1 : 0;
            if (fused) SG_HIP(c, launch_sg_gcn(g1, V, K, b.slot_k, b.sl_v, b.sl_a, gcn_bn, gcn_step32, s));   // z is formed in registers, fragment by fragment
            else if (i == 0 && !no_block0 && b.ci == 6 && K == 3 && b.co == 64 && b.W1s) {
                dispatch_bools([&](auto F) { hipLaunchKernelGGL((k_sg_block0<6, 3, 64, decltype(F)::value>), blocks1d(rows), dim3(256), 0, s, xp, gp, b.nz_ptr, b.nz_v, b.nz_a, b.W1s, b.b1, rows, V); }, f16);
            } else if (small_graph && i == 0 && !no_block0 && !f16 && b.ci == 3 && K == 3 && b.co == 64 && b.W1s) {   // the 3-channel first block of the unconstrained evaluator
                hipLaunchKernelGGL((k_sg_block0<3, 3, 64, false>), blocks1d(rows), dim3(256), 0, s, xp, gp, b.nz_ptr, b.nz_v, b.nz_a, b.W1s, b.b1, rows, V);
            } else {
                if (b.ci % 32 == 0) hipLaunchKernelGGL(k_sg_agg, dim3((unsigned)((rows * 4 + 255) / 256), (unsigned)(K * (b.ci / 32))), dim3(256), 0, s, xp, zp, b.nz_ptr, b.nz_v, b.nz_a, rows, V, K, b.ci);
                else if (b.ci == 6 && K == 3) hipLaunchKernelGGL((k_sg_agg_small_t<6, 3>), blocks1d(rows), dim3(256), 0, s, xp, zp, b.nz_ptr, b.nz_v, b.nz_a, rows, V);
                else hipLaunchKernelGGL(k_sg_agg_small, blocks1d(rows), dim3(256), 0, s, xp, zp, b.nz_ptr, b.nz_v, b.nz_a, rows, V, K, b.ci);
                SG_HIP(c, launch_gemm_x3_sg(g1, s));
                if (f16) hipLaunchKernelGGL(k_sg_to_f16, blocks1d(rows * (b.co / 32) * 4), dim3(256), 0, s, gp, rows, b.co / 32);
            }
            // pad frames and guard rows back to zero: what the temporal taps read beyond a sequence
            auto zero = [&](const SgPl& pl, long long base, int Tr, int Tp, int lead, int trail) {
                const size_t n = ((size_t)NM * (Tp - Tr) * V + (size_t)lead + (size_t)trail) * (b.co / 32) * 4;
                hipLaunchKernelGGL(k_sg_zero, blocks1d(n), dim3(256), 0, s, pl, base, NM, Tr, Tp, V, b.co / 32, lead, trail);
            };
            if (!ipoly) zero(gp, 0, T, T + SG_PAD, guard, guard);
            else {
                zero(gp, 0, Te, Te + SG_PAD, guard, 0);
                zero(gp, (long long)rows_c, T / 2, Te + SG_PAD, 0, guard);
            }
            // 9x1 temporal convolution: ONE GEMM over K = 9 C_out; tap dt of k-block (channel block, dt) is a byte offset into g
            GemmX3Args g2 = sg_gemm_x3(gp, f16 ? b.W2f : b.W2h, b.W2l, (int)rows_c, b.co, 9 * b.co);
            g2.a_taps = 9;
            g2.f16 = f16 ? 1 : 0;
            for (int dt = 0; dt < 9; ++dt) {
                if (!ipoly) g2.a_tap[dt] = (long long)(dt - 4) * V * 64;                                  // frame t + dt - 4
                else if ((dt & 1) == 0) g2.a_tap[dt] = (long long)((dt - 4) / 2) * V * 64;                  // frame 2 t' + dt - 4 = even frame t' + (dt - 4) / 2
                else g2.a_tap[dt] = ((long long)rows_c + (long long)((dt - 5) / 2) * V) * 64;               // ... = odd frame t' + (dt - 5) / 2
            }
            // activation window resident in LDS: refilled strip by strip behind the taps (k_sg_tconv, 8 V >= 256) or, on a small graph, whole and double-buffered
            // (k_sg_tconv_pre, 16 <= V <= 28; split bf16 only - SG_F16 falls through to f16_unserved below)
            const bool pre = small_graph && !ipoly && !no_window && !f16 && sg_tconv_pre_supported(b.co, 9 * b.co, V);
            const bool window = pre || (!ipoly && !no_window && sg_tconv_supported(b.co, 9 * b.co, V));
            auto launch_window = [&](const GemmX3Args& ga, int tail) { return pre ? launch_sg_tconv_pre(ga, V, tail, s) : launch_sg_tconv(ga, V, tail, small_tiles, s); };
            if (ipoly && !opoly && b.res_conv && !no_s2 && !no_window && b.kpr == b.ci && sg_tconv_s2_supported(b.co, 9 * b.co, V)) {
                // stride-2 block: two resident windows (even / odd frames), the convolved shortcut as extra k-steps, the tail in the epilogue
                g2.bias = b.b2r;
                g2.Chi = xo.hi; g2.Clo = xo.lo; g2.c_rows = (int)xo.R;
                g2.A2hi = xp.hi; g2.A2lo = xp.lo; g2.a2_rows = (int)xp.R;
                g2.W2hi = f16 ? b.Wrf : b.Wrh; g2.W2lo = b.Wrl; g2.k2 = b.kpr / 32;
                SG_HIP(c, launch_sg_tconv_s2(g2, V, (long long)rows_c, s));
                zero(xo, 0, To, To + SG_PAD, guard, guard);
            } else if (window && opoly && b.res_id && !no_tail && !no_poly) {
                // ... and for the block in front of a stride-2 block the same tail, written polyphase (even frames | odd frames)
                g2.bias = b.b2;
                g2.Chi = xo.hi; g2.Clo = xo.lo; g2.c_rows = (int)xo.R;
                g2.Rhi = xp.hi; g2.Rlo = xp.lo; g2.r_rows = (int)xp.R;
                const int Teo = (To + 1) / 2;
                g2.poly_T = T; g2.poly_V = V; g2.poly_region = (int)((size_t)NM * (Teo + SG_PAD) * V);
                SG_HIP(c, launch_window(g2, 3));
                zero(xo, 0, Teo, Teo + SG_PAD, guard, 0);
                zero(xo, (long long)g2.poly_region, To / 2, Teo + SG_PAD, 0, guard);
            } else if (window && !opoly && !b.res_conv && !no_tail) {
                // the block's tail in the convolution's epilogue: x' = relu(conv + b2' [+ x]) straight into the next block's planes (same row geometry)
                g2.bias = b.b2;
                g2.Chi = xo.hi; g2.Clo = xo.lo; g2.c_rows = (int)xo.R;
                g2.Rhi = xp.hi; g2.Rlo = xp.lo; g2.r_rows = (int)xp.R;
                SG_HIP(c, launch_window(g2, b.res_id ? 2 : 1));
                zero(xo, 0, To, To + SG_PAD, guard, guard);
            } else {
                if (f16) return f16_unserved(i, "the unfused temporal convolution + k_sg_post");
                g2.C = c->conv; g2.ldc = b.co;
                if (window) SG_HIP(c, launch_window(g2, 0));
                else SG_HIP(c, launch_gemm_x3_sg(g2, s));
                if (b.res_conv) {   // strided 1x1 convolution of the block input: the even frames = region E of the polyphase planes (all rows for a stride-1 block)
                    GemmX3Args gr = sg_gemm_x3(xp, b.Wrh, b.Wrl, (int)rows_c, b.co, b.kpr);
                    gr.C = c->rfull; gr.ldc = b.co;
                    SG_HIP(c, launch_gemm_x3_sg(gr, s));
                }
                hipLaunchKernelGGL(k_sg_post, dim3((unsigned)((rows_o * 4 + 255) / 256), (unsigned)(b.co / 32)), dim3(256), 0, s, c->conv, b.b2, xp, b.res_id ? 1 : 0, b.res_conv ? c->rfull : nullptr, b.br,
                                   xo, NM, Tpi, To, opoly ? 1 : 0, V, b.co);
            }
            std::swap(x, xn);
            T = To;
        }
        if (small_graph) hipLaunchKernelGGL(k_sg_pool_pad, dim3(N), dim3(256), 0, s, planes(*x, phys(T, false)), c->pooled, M, T, c->V, V, 256);   // (f16: refused above)
        else dispatch_bools([&](auto F) { hipLaunchKernelGGL(k_sg_pool<decltype(F)::value>, dim3(N), dim3(256), 0, s, planes(*x, phys(T, false)), c->pooled, M, T, V, 256); }, f16);
        if (features) SG_HIP(c, hipMemcpyAsync(features, c->pooled, (size_t)N * 256 * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (yhat) {
            GemmArgs gf = sg_gemm(c->pooled, 256, c->Wf, 256, 256, c->bf, yhat, c->cfg.num_class, N, c->cfg.num_class);
            SG_HIP(c, launch_gemm(gf, RGN_PREC_F32, s));
        }
        SG_HIP(c, hipGetLastError());
        SG_HIP(c, hipEventRecord(c->ev_out, s));
        SG_HIP(c, hipStreamWaitEvent(us, c->ev_out, 0));
        return RGN_OK;
    });
}

}  // extern "C"
