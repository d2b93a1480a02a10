// The geometry and argument rules of the GRU denoiser's layer stack (rgn_gru_stack.hip: arch='gru') as pure host code: what launch_gru_stack accepts,
// decided before a kernel is launched. Shared by rgn_gru_stack.hip and tools/gru_arch_args_check.cpp (a stand-alone program built with the host
// sanitizers), so the rules have one definition.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rgn {

constexpr int GRS_TILE = 16;          // sequences per wave: the column count of the 16x16x4 fp32 MFMA
constexpr int GRS_WAVES = 4;          // waves per workgroup: four groups of 16 sequences share a unit tile's weight stream through the CU's cache
constexpr int GRS_MAX_GRID = 65535;   // gridDim.y / gridDim.z

// One scan: S steps over N independent sequences and L layers, nseg independent scans side by side (segments). Strides are in floats. Row (seg, s, n)
// of x / out starts at seg x_seg + s x_step + n x_seq and holds d floats. Everything below `nseg` is the caller's; launch_gru_stack fills the rest.
struct GruStackArgs {
    const float* w;                   // L packed layers of gru_stack_layer_floats(d) each: W_ih fragments | W_hh fragments | bias [4][d]
    const float* x;                   // layer 0's input rows (fp32)
    float* out;                       // the top layer's state of every step: the stack's output
    float* ring;                      // state of the layers below the top one: [L - 1][2][nseg][N][d] (null when L == 1)
    long long x_step, x_seq, x_seg, o_step, o_seq, o_seg;
    int d, L, S, N, nseg;
    int delta, l_lo, ncells;          // the launch's anti-diagonal l + s = delta, its first layer and its cell count
};

inline size_t gru_stack_layer_floats(int d) { return (size_t)6 * d * d + (size_t)4 * d; }
inline size_t gru_stack_ring_floats(int d, int L, int nseg, int N) { return L > 1 ? (size_t)(L - 1) * 2 * nseg * N * d : 0; }
inline int gru_stack_launches(int S, int L) { return S + L - 1; }
// the layers [l_lo, l_lo + ncells) that have a cell on diagonal delta: 0 <= l < L and 0 <= delta - l < S
inline void gru_stack_diagonal(int delta, int S, int L, int* l_lo, int* ncells) {
    const int lo = delta - (S - 1) > 0 ? delta - (S - 1) : 0, hi = delta < L - 1 ? delta : L - 1;
    *l_lo = lo;
    *ncells = hi - lo + 1;
}

// nullptr when the geometry is served; otherwise the reason
inline const char* gru_stack_geometry_error(int d, int L) {
    if (d < 16 || d % 16) return "the hidden size must be a positive multiple of 16";
    if (d > 4096) return "the hidden size must be at most 4096";
    if (L < 1) return "num_layers must be at least 1";
    if (L > GRS_MAX_GRID) return "more than 65535 layers";
    return nullptr;
}

// Distinct (seg, s, n) must address disjoint rows of d floats: with the three (stride, extent) pairs sorted by stride, every stride covers the
// whole extent of the one before it and the smallest covers a row. Extent-1 axes do not take part.
inline bool gru_stack_rows_disjoint(long long st0, int n0, long long st1, int n1, long long st2, int n2, int d) {
    long long st[3] = {st0, st1, st2};
    long long ex[3] = {n0, n1, n2};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (st[j] < st[i]) {
                const long long a = st[i], b = ex[i];
                st[i] = st[j]; ex[i] = ex[j];
                st[j] = a; ex[j] = b;
            }
    long long need = d;
    for (int i = 0; i < 3; ++i) {
        if (ex[i] <= 1) continue;
        if (st[i] < need) return false;
        if (st[i] > (1ll << 40) / ex[i]) return false;   // (keeps every product below far from overflow)
        need = st[i] * ex[i];
    }
    return true;
}

// nullptr when a scan's arguments are served
inline const char* gru_stack_args_error(const GruStackArgs& a) {
    if (const char* why = gru_stack_geometry_error(a.d, a.L)) return why;
    if (!a.w || !a.x || !a.out) return "null weights / input / output";
    if (a.L > 1 && !a.ring) return "null state ring with more than one layer";
    if (a.S < 1 || a.N < 1 || a.nseg < 1) return "S, N and the segment count must be at least 1";
    if (a.S > (1 << 24) || a.N > (1 << 24) || a.nseg > (1 << 16)) return "S, N or the segment count too large";
    if (a.x == a.out) return "the stack does not run in place";
    if ((reinterpret_cast<uintptr_t>(a.w) | reinterpret_cast<uintptr_t>(a.x) | reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.ring)) & 15)
        return "pointers must be 16-byte aligned";
    const long long st[6] = {a.x_step, a.x_seq, a.x_seg, a.o_step, a.o_seq, a.o_seg};
    for (long long v : st)
        if (v < 0 || v % 4) return "strides must be non-negative multiples of 4 floats";
    if (a.x_seq > 0x7fffffffll || a.o_seq > 0x7fffffffll) return "the sequence stride must fit 31 bits";
    if (!gru_stack_rows_disjoint(a.x_step, a.S, a.x_seq, a.N, a.x_seg, a.nseg, a.d)) return "input rows overlap";
    if (!gru_stack_rows_disjoint(a.o_step, a.S, a.o_seq, a.N, a.o_seg, a.nseg, a.d)) return "output rows overlap";
    const long long groups = (a.N + GRS_TILE - 1) / GRS_TILE;
    if ((groups + GRS_WAVES - 1) / GRS_WAVES > GRS_MAX_GRID) return "too many sequences for one launch";
    const long long cells = a.S < a.L ? a.S : a.L;
    if (cells * a.nseg > GRS_MAX_GRID) return "too many (cell, segment) pairs on one diagonal";
    return nullptr;
}

}  // namespace rgn
