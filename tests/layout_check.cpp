// Exhaustive host check of regennet_amd/csrc/rgn_layout.h over small domains: c++ -std=c++17 -I regennet_amd/csrc tests/layout_check.cpp.
// Exit status 0 = every property holds; each failure prints one line. Run by tests/test_layout_cpu.py.
#include "rgn_layout.h"

#include <cstdio>
#include <vector>

using namespace rgn;

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++g_fail <= 20) {                         \
                std::printf("FAIL %s: ", #cond);          \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

// 1. (row, logical chunk) -> byte offset is a bijection onto the R x 4 chunks of a k-block
static void image_chunk_map(int R) {
    std::vector<int> hit(R * 4, 0);
    for (int r = 0; r < R; ++r)
        for (int c = 0; c < 4; ++c) {
            const int o = img_chunk(r, c);
            CHECK(o >= 0 && o < R * 64 && o % 16 == 0, "R %d row %d chunk %d -> %d", R, r, c, o);
            if (o >= 0 && o < R * 64) hit[o / 16]++;
            CHECK(o / 64 == r, "R %d row %d chunk %d leaves its row: %d", R, r, c, o);
        }
    for (int i = 0; i < R * 4; ++i) CHECK(hit[i] == 1, "R %d image chunk %d hit %d times", R, i, hit[i]);
}

// 2. the DMA writes what lane (row, slot) fetched to chunk position slot of the row: the image then holds logical chunk j at img_chunk(row, j)
static void dma_rule(int R) {
    std::vector<int> img(R * 4, -1);   // [row][position] = logical chunk held
    for (int r = 0; r < R; ++r)
        for (int slot = 0; slot < 4; ++slot) img[r * 4 + slot] = img_dma_chunk(r, slot);
    for (int r = 0; r < R; ++r)
        for (int j = 0; j < 4; ++j) CHECK(img[img_chunk(r, j) / 16] == j, "R %d row %d: chunk %d is not at its image offset", R, r, j);
}

// 3. an element written through the accumulator-run offset comes back through the fragment offset
static void writer_reader() {
    std::vector<int> img(64 * 32, -1);   // one k-block of 64 rows, 2-byte elements: [byte offset / 2] = (row << 8) | col
    for (int r = 0; r < 64; ++r)
        for (int i4 = 0; i4 < 4; ++i4)
            for (int kh = 0; kh < 2; ++kh)
                for (int e = 0; e < 4; ++e) {
                    const int o = img_run(r, i4, kh) + 2 * e;
                    CHECK(o % 2 == 0 && o >= 0 && o < 64 * 64, "run offset %d", o);
                    CHECK(img[o / 2] == -1, "row %d col %d written twice", r, 8 * i4 + 4 * kh + e);
                    img[o / 2] = (r << 8) | (8 * i4 + 4 * kh + e);
                }
    for (int r = 0; r < 64; ++r)
        for (int ks = 0; ks < 2; ++ks)
            for (int kh = 0; kh < 2; ++kh)
                for (int e8 = 0; e8 < 8; ++e8) {
                    const int got = img[(img_frag(r, ks, kh) + 2 * e8) / 2];
                    CHECK(got == ((r << 8) | (16 * ks + 8 * kh + e8)), "row %d ks %d kh %d e %d reads (%d, %d)", r, ks, kh, e8, got >> 8, got & 255);
                }
}

// 4. plane offset: bijection, and the packer's former literal
static void plane(int rows, int nb) {
    const size_t total = (size_t)rows * 32 * nb;
    std::vector<int> hit(total, 0);
    for (int row = 0; row < rows; ++row)
        for (int col = 0; col < 32 * nb; ++col) {
            const size_t o = plane_off(rows, row, col);
            const int n = row, k = col, N = rows;
            const size_t expect = ((size_t)(k / 32) * N + n) * 32 + (k % 32);
            CHECK(o == expect, "plane rows %d (%d, %d): %zu, expected %zu", rows, row, col, o, expect);
            CHECK(o < total, "plane rows %d nb %d (%d, %d) -> %zu out of range", rows, nb, row, col, o);
            if (o < total) hit[o]++;
            CHECK(plane_chunk(rows, row, col / 32, (col % 32) / 8) + col % 8 == o, "plane chunk of (%d, %d)", row, col);
        }
    for (size_t i = 0; i < total; ++i) CHECK(hit[i] == 1, "plane rows %d nb %d offset %zu hit %d times", rows, nb, i, hit[i]);
}

// 5. fragment plane: bijection, the packer's former literal, granules and the lanes' 8 consecutive k
static void fragment(int N, int K) {
    const size_t Np = (size_t)(N + 31) / 32 * 32, Kp = (size_t)(K + 31) / 32 * 32, nb_all = Np / 32, total = Np * Kp;
    std::vector<int> hit(total, 0);
    for (int n = 0; n < (int)Np; ++n)
        for (int k = 0; k < (int)Kp; ++k) {
            const size_t o = frag_off(nb_all, n, k);
            const size_t kt = k / 32, ks = (k % 32) / 16, lane = 32 * ((k % 16) / 8) + n % 32;
            const size_t expect = (((kt * nb_all + n / 32) * 2 + ks) * 64 + lane) * 8 + k % 8;
            CHECK(o == expect, "frag N %d K %d (%d, %d): %zu, expected %zu", N, K, n, k, o, expect);
            CHECK((size_t)frag_lane(n, k) == lane && frag_elem(k) == k % 8, "frag lane / element of (%d, %d)", n, k);
            CHECK(o < total, "frag N %d K %d (%d, %d) -> %zu out of range", N, K, n, k, o);
            if (o < total) hit[o]++;
        }
    for (size_t i = 0; i < total; ++i) CHECK(hit[i] == 1, "frag N %d K %d offset %zu hit %d times", N, K, i, hit[i]);
    // granule hs of column block cb: 64 lanes x 16 bytes; lane l holds n = 32 cb + (l & 31), k = 16 hs + 8 (l >> 5) + 0 .. 7
    const int kstride = (int)nb_all * 2048;
    for (int hs = 0; hs < (int)Kp / 16; ++hs)
        for (int cb = 0; cb < (int)nb_all; ++cb) {
            const size_t start = (size_t)frag_granule(hs, kstride) + (size_t)cb * 2048;
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < 8; ++e) {
                    const int n = 32 * cb + (l & 31), k = 16 * hs + 8 * (l >> 5) + e;
                    CHECK(frag_off(nb_all, n, k) * 2 == start + (size_t)l * 16 + (size_t)e * 2, "granule hs %d cb %d lane %d element %d", hs, cb, l, e);
                }
        }
}

// 6. C/D map: (i, kh) -> row is a bijection onto 0 .. 31; the column is the lane's low five bits
static void cd_map() {
    int hit[32] = {0};
    for (int i = 0; i < 16; ++i)
        for (int kh = 0; kh < 2; ++kh) {
            const int r = mfma32_row(i, kh);
            CHECK(r >= 0 && r < 32, "C/D row of (%d, %d) = %d", i, kh, r);
            if (r >= 0 && r < 32) hit[r]++;
            CHECK(r == (i & 3) + 8 * (i >> 2) + 4 * kh, "C/D row of (%d, %d)", i, kh);
        }
    for (int r = 0; r < 32; ++r) CHECK(hit[r] == 1, "C/D row %d hit %d times", r, hit[r]);
    for (int l = 0; l < 64; ++l) CHECK(mfma32_col(l) == l % 32, "C/D column of lane %d", l);
}

// 7. attention-ready slab: bijection onto B H Tqp dh elements, a token row of a head is dh contiguous elements, a head's slab Tqp dh contiguous
//    elements starting at its base, and the literal the in_proj epilogues used to spell
static void attn_slab(int B, int H, int Tqp, int dh) {
    const size_t total = (size_t)B * H * Tqp * dh;
    std::vector<int> hit(total, 0);
    for (int b = 0; b < B; ++b)
        for (int hd = 0; hd < H; ++hd) {
            const size_t base = attn_slab_base(H, Tqp, dh, b, hd);
            CHECK(base == ((size_t)b * H + hd) * Tqp * dh, "slab base of (%d, %d)", b, hd);
            for (int t = 0; t < Tqp; ++t)
                for (int c = 0; c < dh; ++c) {
                    const size_t o = attn_slab_off(H, Tqp, dh, b, hd, t, c);
                    CHECK(o == (((size_t)b * H + hd) * Tqp + t) * dh + c, "slab H %d Tqp %d dh %d (%d, %d, %d, %d): %zu", H, Tqp, dh, b, hd, t, c, o);
                    CHECK(o == base + (size_t)t * dh + c, "slab (%d, %d, %d, %d) is not row t, column c of its head's slab", b, hd, t, c);
                    CHECK(o == attn_slab_off(H, Tqp, dh, b, hd, t, 0) + c, "slab row (%d, %d, %d) is not contiguous at column %d", b, hd, t, c);
                    CHECK(o < total, "slab (%d, %d, %d, %d) -> %zu out of range", b, hd, t, c, o);
                    if (o < total) hit[o]++;
                }
        }
    for (size_t i = 0; i < total; ++i) CHECK(hit[i] == 1, "slab H %d Tqp %d dh %d offset %zu hit %d times", H, Tqp, dh, i, hit[i]);
}

int main() {
    for (int R : {32, 64}) {
        image_chunk_map(R);
        dma_rule(R);
    }
    writer_reader();
    for (int rows : {1, 44, 64, 300})
        for (int nb : {1, 11, 16}) plane(rows, nb);
    const int nk[4][2] = {{32, 32}, {352, 512}, {512, 352}, {1536, 512}};
    for (const auto& s : nk) fragment(s[0], s[1]);
    cd_map();
    const int slabs[4][4] = {{1, 1, 32, 16}, {3, 4, 64, 128}, {2, 32, 96, 16}, {5, 8, 160, 64}};   // B, H, Tqp, dh
    for (const auto& s : slabs) attn_slab(s[0], s[1], s[2], s[3]);
    if (g_fail) std::printf("%d layout checks failed\n", g_fail);
    else std::printf("layout ok\n");
    return g_fail ? 1 : 0;
}
