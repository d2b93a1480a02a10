// The five data layouts the MFMA kernels of this directory stand on, defined ONCE: the index arithmetic of the packer (rgn_pack.cpp, host), of
// the kernels (device) and of the stand-alone check tests/layout_check.cpp (host, no GPU) is this text. Nothing of HIP is included; every layout function
// is constexpr, so the static_asserts at the foot travel with every build. (A few sites spell an expression out, with a comment naming the function
// it equals, where the register allocation moved with the text: profiles/layout_refactor_resources.txt lists them.)
//
// 1. The K32-blocked PLANE [K / 32][rows][32] of 16-bit elements: element (row, col) lives in k-block col / 32, at column col % 32 of its row. A
//    row's 64 bytes inside a k-block are four 16-byte CHUNKS of 8 elements. The activations (xin, h, att, ffn), the row-major weight hi / lo planes
//    of the split-bf16 GEMMs and the ST-GCN planes have this layout: a 32-wide k-step of a GEMM reads one contiguous [rows][32] slab.
//
// 2. The LDS operand IMAGE [k-block][R rows][64 B]: a row tile of a plane, k-block by k-block, with the four chunks of a row permuted - logical
//    chunk c of row r sits at chunk position c ^ swz(r), swz(r) = (r >> 2) & 3. With the XOR both accesses of an image are conflict-free: the
//    16-byte operand reads of an MFMA (32 lanes = 32 rows, the same logical chunk) and the 8-byte accumulator stores. Four roles of one map:
//      img_dma_chunk  which plane chunk the lane that fills chunk position `slot` of row r must fetch (the DMA writes lanes in order)
//      img_frag       the operand fragment of (row, ks, kh): k = 16 ks + 8 kh + 0 .. 7 of the k-block, logical chunk 2 ks + kh
//      img_run        the 8-byte run of an accumulator: columns 8 i4 + 4 kh + 0 .. 3 of the k-block
//      img_chunk      a plain 16-byte copy-in / copy-out of logical chunk c
//
// 3. The FRAGMENT-ORDERED weight plane [K / 32][N / 32][2 ks][64 lanes][8]: W[n][k] stored so that the 16 bytes lane l of a wave loads for the
//    32 x 32 x 16 MFMA's A operand are contiguous and a wave's load is one 1 KiB line: lane = 32 ((k % 16) / 8) + n % 32 holds k % 8 = 0 .. 7.
//    A GRANULE is half a k-block (ks) of one 32-column block: 1 KiB; the register-streamed kernels address granule hs = 2 kt + ks.
//
// 4. The 32 x 32 MFMA C/D map: register i of lane l holds row (i & 3) + 8 (i >> 2) + 4 (l >> 5), column l & 31 of the tile.
//
// 5. The ATTENTION-READY slab [sample * H + head][Tqp][dh] of 16-bit elements: q, k and v of one (sample, head) as Tqp = 32 ceil(Tq / 32) token rows of
//    dh contiguous elements, one contiguous slab per head. The in_proj epilogues (rgn_gemm_x3.hip, rgn_rowgemm.hip, rgn_sb.hip) scatter into it,
//    k_attn_x3 (rgn_attn.hip) stages a head's slab through LDS; rows Tq .. Tqp - 1 are never written and never read.
//
// ... and the element the host packers (rgn_pack.cpp, rgn_stgcn.hip) put into the bf16 planes: f2bf / bf2f.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIP__) || defined(__CUDACC__)
#define RGN_HD __attribute__((host)) __attribute__((device))
#else
#define RGN_HD
#endif

namespace rgn {

template <class T> struct layout_index { typedef T type; };   // (keeps the index type I out of deduction: size_t unless named)

// ---- 1. plane [K / 32][rows][32]; offsets in ELEMENTS, in the index type I
template <class I = size_t>
RGN_HD constexpr inline I plane_chunk(typename layout_index<I>::type rows, typename layout_index<I>::type row, int kb, int chunk) {
    return ((I)kb * rows + row) * 32 + chunk * 8;
}
template <class I = size_t>
RGN_HD constexpr inline I plane_off(typename layout_index<I>::type rows, typename layout_index<I>::type row, int col) {
    return ((I)(col >> 5) * rows + row) * 32 + (col & 31);
}

// ---- 2. image [k-block][R rows][64 B]; offsets in BYTES inside a k-block (the k-block stride is R * 64)
RGN_HD constexpr inline int img_swz(int row) { return (row >> 2) & 3; }
RGN_HD constexpr inline int img_slot(int chunk, int swz) { return (chunk ^ swz) << 4; }                    // of a row whose swizzle is swz
RGN_HD constexpr inline int img_chunk(int row, int chunk) { return row * 64 + img_slot(chunk, img_swz(row)); }
RGN_HD constexpr inline int img_frag(int row, int ks, int kh) { return row * 64 + img_slot(2 * ks + kh, img_swz(row)); }
RGN_HD constexpr inline int img_run(int row, int i4, int kh) { return row * 64 + img_slot(i4, img_swz(row)) + 8 * kh; }
RGN_HD constexpr inline int img_dma_chunk(int row, int slot) { return slot ^ img_swz(row); }

// ---- 3. fragment plane [K / 32][nb_all = Np / 32][2][64][8]
RGN_HD constexpr inline int frag_lane(int n, int k) { return 32 * ((k % 16) / 8) + n % 32; }
RGN_HD constexpr inline int frag_elem(int k) { return k % 8; }
RGN_HD constexpr inline size_t frag_off(size_t nb_all, int n, int k) {                                   // in elements
    return ((((size_t)(k / 32) * nb_all + n / 32) * 2 + (k % 32) / 16) * 64 + frag_lane(n, k)) * 8 + frag_elem(k);
}
// byte offset of granule hs = 2 kt + ks of the first column block; kstride = nb_all * 2048 bytes per k-block, a column block further is 2048
RGN_HD constexpr inline int frag_granule(int hs, int kstride) { return (hs >> 1) * kstride + (hs & 1) * 1024; }

// ---- 4. 32 x 32 MFMA accumulator: register i of a lane in half kh = lane >> 5
RGN_HD constexpr inline int mfma32_row(int i, int kh) { return (i & 3) + 8 * (i >> 2) + 4 * kh; }
RGN_HD constexpr inline int mfma32_col(int lane) { return lane & 31; }

// ---- 5. attention-ready slab [B * H][Tqp][dh]; offsets in ELEMENTS
RGN_HD constexpr inline size_t attn_slab_base(int H, int Tqp, int dh, size_t b, int hd) { return (b * H + hd) * Tqp * dh; }
RGN_HD constexpr inline size_t attn_slab_off(int H, int Tqp, int dh, size_t b, int hd, int t, int c) { return ((b * H + hd) * Tqp + t) * dh + c; }

// ---- host: fp32 -> bf16 bits (round to nearest even; a NaN stays one) and back. A split-bf16 plane pair holds hi = f2bf(v), lo = f2bf(v - bf2f(hi))
inline uint16_t f2bf(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float bf2f(uint16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// ---- what every build checks (the exhaustive form is tests/layout_check.cpp)
namespace layout_detail {
constexpr bool chunks_permute() {
    for (int r = 0; r < 64; ++r) {
        int seen = 0;
        for (int c = 0; c < 4; ++c) {
            seen |= 1 << ((img_chunk(r, c) - r * 64) >> 4);
            if (img_chunk(r, img_dma_chunk(r, c)) != r * 64 + c * 16) return false;   // the DMA rule: slot c ends up holding the chunk it fetched
        }
        if (seen != 15) return false;
    }
    return true;
}
constexpr bool roles_agree() {
    for (int r = 0; r < 64; ++r)
        for (int ks = 0; ks < 2; ++ks)
            for (int kh = 0; kh < 2; ++kh) {
                if (img_frag(r, ks, kh) != img_chunk(r, 2 * ks + kh)) return false;
                if (img_run(r, 2 * ks + kh, 1) != img_chunk(r, 2 * ks + kh) + 8) return false;
            }
    return true;
}
constexpr bool cd_rows_permute() {
    unsigned seen = 0;
    for (int i = 0; i < 16; ++i)
        for (int kh = 0; kh < 2; ++kh) seen |= 1u << mfma32_row(i, kh);
    return seen == 0xffffffffu;
}
}  // namespace layout_detail
static_assert(layout_detail::chunks_permute(), "the chunk map permutes 0 .. 3 in every row and the DMA source rule inverts it");
static_assert(layout_detail::roles_agree(), "fragment (r, ks, kh) is logical chunk 2 ks + kh; an accumulator run is half a chunk");
static_assert(layout_detail::cd_rows_permute(), "the C/D row map covers the 32 rows of a tile");
static_assert(plane_off(300, 7, 37) == plane_chunk(300, 7, 1, 0) + 5, "a plane element lies in chunk (col % 32) / 8 of k-block col / 32");
static_assert(attn_slab_off(4, 64, 128, 3, 2, 0, 0) == attn_slab_base(4, 64, 128, 3, 2) && attn_slab_base(4, 64, 128, 3, 2) == (size_t)(3 * 4 + 2) * 64 * 128, "a head's slab is Tqp x dh elements, heads of a sample back to back");
static_assert(attn_slab_off(4, 64, 128, 3, 2, 59, 127) + 1 == attn_slab_off(4, 64, 128, 3, 2, 60, 0), "a token row of a head is dh contiguous elements");
static_assert(frag_off(16, 33, 49) * 2 == frag_granule(3, 16 * 2048) + 2048 + frag_lane(33, 49) * 16 + frag_elem(49) * 2, "granule, column block, lane, element");

}  // namespace rgn
