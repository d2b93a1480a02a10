// The DMA-fed split-bf16 GEMM family, defined once for the kernels that run it: k_gemm_x3 (rgn_gemm_x3.hip) and the recogniser's three persistent
// kernels k_sg_tconv, k_sg_tconv_s2 and k_sg_gcn (rgn_sg_kernels.hip), each grown from k_gemm_x3's interleaved loop. What is shared is everything that
// is not a kernel's window management: the fragment pair's product, the weight-tile DMA, the MFMA groups of a k-step, the persistent tile walk with the
// close of a tile, and the paired-column plane store. Device code, internal linkage. The family's contract:
//
// STAGE. A k-step reads one stage of LDS, [A hi | A lo | W hi | W lo], every part the swizzled operand image of rgn_layout.h, filled by direct-to-LDS DMA
// (global_load_lds_dwordx4: 16 rows x 64 B per wave-instruction). The window kernels keep A resident instead (their windows), and their stage is
// [W hi | W lo]. F16, the single-plane fp16 form: what was the lo image of channel block cb is the fp16 image of channel block cb + 1.
//
// PRODUCT ORDER. a.w ~ al.wh + ah.wl + ah.wh: the two small terms first, so that they meet in the accumulator before the large term's rounding can
// swallow either (al.wl, ~2^-16 of the product, is dropped). fp16: this channel block, then the next. dg_mma is that order and nothing else.
//
// DMA BEHIND THE FIRST GROUP. A k-step's loads - the next weight tile and whatever else the vector-memory path carries for the kernel - are issued behind
// the step's FIRST MFMA group (dg_kstep's `behind`), never in front of it: the matrix pipe is busy before the address arithmetic starts, and the
// fragments of a group are fetched one group ahead so that no MFMA waits on LDS.
//
// STORES_BEHIND. The counted wait behind an epilogue (dg_step_wait: vmcnt <= the stores of one tile) is an upper bound on what may stay outstanding, not
// the guarantee that the next k-step's DMA has landed: a wave whose 32 rows are all pad rows SKIPS its polyphase stores (s_cbranch_execz in the ISA). The
// guarantee there is the in-order retirement of vmcnt: SGE_POLY (the only mode with conditional stores on the counted path) always comes with
// SGE_RES_PLANES, whose residual loads are issued AFTER that DMA and consumed BEFORE the first store - the DMA has retired by then whatever the number
// of stores. The other modes issue exactly the counted stores on the interior path (CHECK = false); edge tiles (CHECK = true) are followed by a full
// wait. What a 32 x 32 tile needs from memory is requested one tile AHEAD of its use: vmcnt retires in order, so a load queued behind the previous
// tile's stores would wait for their acknowledgements - 2 TM TN round trips to memory per workgroup tile in x3_epilogue's order.
#pragma once
#include "rgn_internal.h"
#include "rgn_device.h"

namespace rgn {
namespace {

// ---- 1. the product of one fragment pair into one C tile. X3 = false: the plain form, hi planes only
template <bool F16, bool X3 = true, class V>
__device__ __forceinline__ void dg_mma(f32x16& c, const V& a_h, const V& a_l, const V& w_h, const V& w_l) {
    if constexpr (F16) {                                         // (a_l, w_l: the next channel block's fragments)
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a_h), __builtin_bit_cast(f16x8, w_h), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a_l), __builtin_bit_cast(f16x8, w_l), c, 0, 0, 0);
    } else {
        if constexpr (X3) {
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a_l), __builtin_bit_cast(bf16x8, w_h), c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a_h), __builtin_bit_cast(bf16x8, w_l), c, 0, 0, 0);
        }
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a_h), __builtin_bit_cast(bf16x8, w_h), c, 0, 0, 0);
    }
}

// ---- 2. accumulators; fragment read offsets of T 32-row tiles whose first row inside the image is row0 (l31 = lane & 31, kh = lane >> 5)
template <int TM, int TN>
__device__ __forceinline__ void dg_zero(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;
}
template <int T>
__device__ __forceinline__ void dg_frag_off(int (&off)[T][2], int row0, int l31, int kh) {
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) off[t][ks] = img_frag(row0 + t * 32 + l31, ks, kh);
}

// ---- 3. the weight-tile DMA of the 512-thread window kernels: BN rows x 64 B of both planes into a stage [W hi | W lo], BN / 64 instructions per
// thread. dg_w_lanes: a thread's 16 bytes inside a plane tile (k-invariant; N is a multiple of BN, so no column clamp). dg_w_tile: the tile whose first
// row is `row` (= k-block * N + first column) of the planes whi / wlo
template <int BN>
__device__ __forceinline__ void dg_w_lanes(unsigned (&w_lane)[BN / 64], int tid) {
#pragma unroll
    for (int it = 0; it < BN / 64; ++it) {
        const int q = it * 512 + tid, pl = (it * 512 + (tid & ~63)) / (BN * 4), qq = q - pl * (BN * 4), r = qq >> 2, c = img_dma_chunk(r, qq & 3);
        w_lane[it] = (unsigned)r * 64u + c * 16u;
    }
}
template <int BN>
__device__ __forceinline__ void dg_w_tile(const char* whi, const char* wlo, size_t row, const unsigned (&w_lane)[BN / 64], char* stage, int tid) {
#pragma unroll
    for (int it = 0; it < BN / 64; ++it) {
        const int pl = (it * 512 + (tid & ~63)) / (BN * 4);
        __builtin_amdgcn_global_load_lds((const RGN_AS1 void*)((pl ? wlo : whi) + row * 64 + w_lane[it]),
                                         (RGN_AS3 void*)(stage + pl * (BN * 64) + (it * 512 + (tid & ~63) - pl * (BN * 4)) * 16), 16, 0, 0);
    }
}

// ---- 4. the MFMA groups of one k-step: group grp = (k half ks, column tile tb), TM products each, its fragments fetched one group ahead. wimg: the W hi
// image of the stage, W lo w_bytes behind it. a_frag(ks, ah, al) supplies the A fragments of k half ks (from a stage, a window row, or registers);
// behind(grp) is what the kernel issues behind group grp: the vector-memory path's loads of this k-step, behind group 0
template <int TM, int TN, bool F16, bool X3 = true, class AFrag, class Behind>
__device__ __forceinline__ void dg_kstep(f32x16 (&acc)[TM][TN], const char* wimg, int w_bytes, const int (&w_off)[TN][2], AFrag&& a_frag, Behind&& behind) {
    bf16x8 ah[2][TM], al[2][TM], wh[2], wl[2];
    auto fetch = [&](int grp) {
        const int ks = grp / TN, tb = grp % TN;
        if (tb == 0) a_frag(ks, ah, al);
        wh[grp & 1] = *reinterpret_cast<const bf16x8*>(wimg + w_off[tb][ks]);
        if (X3) wl[grp & 1] = *reinterpret_cast<const bf16x8*>(wimg + w_bytes + w_off[tb][ks]);
    };
    fetch(0);
#pragma unroll
    for (int grp = 0; grp < 2 * TN; ++grp) {
        if (grp + 1 < 2 * TN) fetch(grp + 1);
#pragma unroll
        for (int ta = 0; ta < TM; ++ta) dg_mma<F16, X3>(acc[ta][grp % TN], ah[grp / TN][ta], al[grp / TN][ta], wh[grp & 1], wl[grp & 1]);
        behind(grp);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- 5. the persistent tile walk: workgroup b starts at tile xcd_affine(b, gridDim.x) - workgroups of one XCD take neighbouring tiles, whose windows
// overlap and then come from that XCD's L2 - and steps by gridDim.x. The close of a tile: dg_close picks the interior (CHECK = false) or the edge
// epilogue, epi(std::bool_constant<CHECK>), and returns `interior` = the caller's stores_behind; dg_step_wait is the wait in front of every k-step's
// barrier (STORES = dg_tile_stores x the wave's 32 x 32 tiles; see STORES_BEHIND above)
struct DgTile { int tile, m0, n0; };
template <int BM, int BN>
__device__ __forceinline__ DgTile dg_tile(int tile, int nbx) { return DgTile{tile, (tile / nbx) * BM, (tile % nbx) * BN}; }
template <int BM, int BN, class Epi>
__device__ __forceinline__ bool dg_close(const GemmX3Args& g, int m0, int n0, Epi&& epi) {
    const bool interior = (m0 + BM <= g.M) && (n0 + BN <= g.N);
    if (interior) epi(std::false_type{});
    else epi(std::true_type{});
    return interior;
}
constexpr int dg_tile_stores(bool planes, bool f16) { return (f16 && planes) ? 8 : 16; }   // per 32 x 32 tile: planes hi [+ lo] of 8 column pairs, or 16 fp32 rows
template <int STORES>
__device__ __forceinline__ void dg_step_wait(bool& stores_behind) {
    if (stores_behind) wait_vmcnt<STORES>();                     // this k-step's DMA is older than the stores of the tile just written
    else wait_vmcnt<0>();                                        // everything this thread requested up to the last k-step has landed
    stores_behind = false;
}

// ---- 6. adjacent columns paired across lane ^ 1, so that every plane store is a packed pair (4 B): even lanes store the rows of registers 0..7, odd
// lanes those of registers 8..15 (row dg_pair_row(i, odd) of the tile); c0 / c1 = columns (n & ~1, + 1) of that row
__device__ __forceinline__ void dg_pair_exchange(float mine, float give, bool odd, float& c0, float& c1) {   // mine: for this lane's store; give: what the partner needs
    const float got = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, give), 0xB1, 0xf, 0xf, true));   // lane ^ 1: quad_perm [1, 0, 3, 2]
    c0 = odd ? got : mine;
    c1 = odd ? mine : got;
}
__device__ __forceinline__ void dg_pair_columns(const float (&r)[16], int i, bool odd, float& c0, float& c1) {
    dg_pair_exchange(odd ? r[i + 8] : r[i], odd ? r[i] : r[i + 8], odd, c0, c1);
}
__device__ __forceinline__ int dg_pair_row(int i, bool odd) { return mfma32_row(odd ? i + 8 : i, 0); }
// the pair at element offset o of the planes: split bf16 hi / lo (LO_OPTIONAL: lo only where the plane exists) or one fp16 plane
template <bool F16, bool LO_OPTIONAL = false>
__device__ __forceinline__ void dg_store_pair(__bf16* hi, __bf16* lo, size_t o, float c0, float c1) {
    if constexpr (F16) {
        f16x2 hv = {(_Float16)c0, (_Float16)c1};
        *reinterpret_cast<f16x2*>(hi + o) = hv;
    } else {
        const __bf16 h0 = (__bf16)c0, h1 = (__bf16)c1;
        bf16x2 hv = {h0, h1};
        *reinterpret_cast<bf16x2*>(hi + o) = hv;
        if (!LO_OPTIONAL || lo) {
            bf16x2 lv = {(__bf16)(c0 - (float)h0), (__bf16)(c1 - (float)h1)};
            *reinterpret_cast<bf16x2*>(lo + o) = lv;
        }
    }
}

// ---- the per-vertex addend of the graph convolution: row % add_mod of g.add (rows run (frame, vertex); add_mod >= 28, so a 32-row tile wraps at most
// once), for the 16 rows of column n a lane holds from row mb on, as bits
__device__ __forceinline__ void dg_vertex_addend(const GemmX3Args& g, int mb, int n, bool n_ok, unsigned (&f)[16]) {
    const int base = (int)((unsigned)mb % (unsigned)g.add_mod);
    const float* ap = g.add + n;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        int rr = base + mfma32_row(i, 0);
        rr = rr >= g.add_mod ? rr - g.add_mod : rr;
        f[i] = n_ok ? __builtin_bit_cast(unsigned, ap[rr * g.ldadd]) : 0u;
    }
}

}  // namespace
}  // namespace rgn
