// Host-only check of the geometry and argument rules of the GRU denoiser's layer stack (regennet_amd/csrc/rgn_gru_stack_check.h: what
// launch_gru_stack accepts), for a sanitizer build on a machine WITHOUT a GPU. The header is pure host code, so this program links nothing else; the
// "device" pointers are never dereferenced.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer tools/gru_arch_args_check.cpp -o build/gru_arch_args_check
//   build/gru_arch_args_check
#include "../regennet_amd/csrc/rgn_gru_stack_check.h"

#include <cstdio>
#include <cstring>
#include <initializer_list>

namespace {

int failures = 0;

void expect(const char* what, const char* got, const char* want) {   // want: a word of the reason, or nullptr for "accepted"
    const bool ok = want ? (got && std::strstr(got, want)) : got == nullptr;
    std::printf("%-46s %s%s\n", what, got ? got : "accepted", ok ? "" : "   <-- UNEXPECTED");
    failures += !ok;
}

alignas(16) float dummy[64];   // stands for device memory: never read

// the 'batch' scan of the denoiser: steps = B samples (stride T d), sequences = T frames (stride d), segments B T d apart
rgn::GruStackArgs batch(int d, int L, int B, int T, int nseg) {
    rgn::GruStackArgs a{};
    a.w = dummy; a.x = dummy; a.out = dummy + 16; a.ring = L > 1 ? dummy + 32 : nullptr;
    a.d = d; a.L = L; a.S = B; a.N = T; a.nseg = nseg;
    a.x_step = a.o_step = (long long)T * d; a.x_seq = a.o_seq = d; a.x_seg = a.o_seg = (long long)B * T * d;
    return a;
}
rgn::GruStackArgs frames(int d, int L, int B, int T) {
    rgn::GruStackArgs a = batch(d, L, B, T, 1);
    a.S = T; a.N = B;
    a.x_step = a.o_step = d; a.x_seq = a.o_seq = (long long)T * d; a.x_seg = a.o_seg = 0;
    return a;
}

}  // namespace

int main() {
    using namespace rgn;
    for (int d : {16, 64, 512, 1024, 4096}) expect("geometry: a multiple of 16", gru_stack_geometry_error(d, 8), nullptr);
    for (int d : {0, -16, 8, 24, 100, 4112}) expect("geometry: hidden size refused", gru_stack_geometry_error(d, 8), "hidden size");
    for (int L : {0, -1, 65536}) expect("geometry: layer count refused", gru_stack_geometry_error(512, L), "layers");
    expect("geometry: one layer", gru_stack_geometry_error(512, 1), nullptr);

    expect("batch scan, ntu shape, guided", gru_stack_args_error(batch(512, 8, 256, 60, 2)), nullptr);
    expect("frames scan, ntu shape, 512 sequences", gru_stack_args_error(frames(512, 8, 512, 60)), nullptr);
    expect("one layer without a ring", gru_stack_args_error(batch(64, 1, 3, 8, 1)), nullptr);
    expect("one step, one sequence", gru_stack_args_error(batch(16, 3, 1, 1, 1)), nullptr);
    GruStackArgs a = batch(64, 2, 3, 8, 1); a.w = nullptr; expect("null weights", gru_stack_args_error(a), "null");
    a = batch(64, 2, 3, 8, 1); a.x = nullptr; expect("null input", gru_stack_args_error(a), "null");
    a = batch(64, 2, 3, 8, 1); a.out = nullptr; expect("null output", gru_stack_args_error(a), "null");
    a = batch(64, 2, 3, 8, 1); a.ring = nullptr; expect("null ring with two layers", gru_stack_args_error(a), "ring");
    a = batch(64, 2, 3, 8, 1); a.out = const_cast<float*>(a.x); expect("in place", gru_stack_args_error(a), "in place");
    a = batch(64, 2, 3, 8, 1); a.x = dummy + 1; expect("misaligned input", gru_stack_args_error(a), "aligned");
    a = batch(64, 2, 3, 8, 1); a.S = 0; expect("S = 0", gru_stack_args_error(a), "at least 1");
    a = batch(64, 2, 3, 8, 1); a.N = -2; expect("N = -2", gru_stack_args_error(a), "at least 1");
    a = batch(64, 2, 3, 8, 1); a.nseg = 0; expect("no segment", gru_stack_args_error(a), "at least 1");
    a = batch(64, 2, 3, 8, 1); a.N = (1 << 24) + 1; expect("N too large", gru_stack_args_error(a), "too large");
    a = batch(64, 2, 3, 8, 1); a.x_seq = 62; expect("stride not a multiple of 4", gru_stack_args_error(a), "multiples of 4");
    a = batch(64, 2, 3, 8, 1); a.o_step = -64; expect("negative stride", gru_stack_args_error(a), "non-negative");
    a = batch(64, 2, 3, 8, 1); a.x_seq = 32; expect("input rows overlap (sequence stride < d)", gru_stack_args_error(a), "input rows overlap");
    a = batch(64, 2, 3, 8, 1); a.o_step = 7 * 64; expect("output rows overlap (step stride < N rows)", gru_stack_args_error(a), "output rows overlap");
    a = batch(64, 2, 3, 8, 2); a.x_seg = 64; expect("segments overlap", gru_stack_args_error(a), "input rows overlap");
    a = frames(64, 2, 3, 8); a.x_seq = 7 * 64; expect("frames scan: sequences overlap", gru_stack_args_error(a), "input rows overlap");
    a = frames(64, 2, 3, 8); a.x_seq = a.o_seq = 1ll << 31; expect("sequence stride beyond 31 bits", gru_stack_args_error(a), "31 bits");
    a = batch(16, 2, 2, 1 << 23, 1); expect("too many sequence groups for one launch", gru_stack_args_error(a), "too many sequences");
    a = batch(16, 40000, 40000, 4, 2); expect("too many cells on a diagonal", gru_stack_args_error(a), "diagonal");

    // every diagonal of every small scan: the cells are exactly those with 0 <= l < L, 0 <= s < S, and each cell appears once
    int diagonals = 0;
    for (int S = 1; S <= 12; ++S)
        for (int L = 1; L <= 9; ++L) {
            int seen[12][9] = {};
            for (int delta = 0; delta < gru_stack_launches(S, L); ++delta, ++diagonals) {
                int lo, n;
                gru_stack_diagonal(delta, S, L, &lo, &n);
                bool ok = n >= 1 && lo >= 0 && lo + n <= L;
                for (int l = lo; ok && l < lo + n; ++l) {
                    const int s = delta - l;
                    ok = s >= 0 && s < S;
                    if (ok) ++seen[s][l];
                }
                if (!ok) { std::printf("gru_stack_diagonal(%d, %d, %d): l_lo %d cells %d   <-- UNEXPECTED\n", delta, S, L, lo, n); ++failures; }
            }
            for (int s = 0; s < S; ++s)
                for (int l = 0; l < L; ++l)
                    if (seen[s][l] != 1) { std::printf("cell (%d, %d) of S %d L %d ran %d times   <-- UNEXPECTED\n", l, s, S, L, seen[s][l]); ++failures; }
        }
    std::printf("%d diagonals checked\n", diagonals);
    const bool sizes = gru_stack_layer_floats(512) == 6u * 512 * 512 + 2048 && gru_stack_ring_floats(512, 8, 2, 60) == 7u * 2 * 2 * 60 * 512 &&
                       gru_stack_ring_floats(512, 1, 2, 60) == 0 && gru_stack_launches(256, 8) == 263;
    std::printf("sizes %s\n", sizes ? "as stated" : "   <-- UNEXPECTED");
    failures += !sizes;
    std::printf("%d unexpected\n", failures);
    return failures ? 1 : 0;
}
