// The layer stack of the GRU denoiser (arch='gru', model/cmdm.py:243-249: nn.GRU(d, d, num_layers=L)) as a wavefront over (layer, step) cells.
//
// Cell (l, s) needs cell (l - 1, s) (its input) and cell (l, s - 1) (its own previous state), so the cells of one anti-diagonal l + s = delta are
// independent. launch_gru_stack enqueues ONE launch per diagonal, S + L - 1 of them, and the stream's order is the only synchronisation: no
// workgroup waits for another, no spin loop, no atomic, no cooperative launch.
//
// A launch's grid is (d / 16 unit tiles) x (groups of 16 sequences, four to a workgroup) x (cells on the diagonal x segments). A wave owns one unit
// tile of one cell for 16 sequences: the three gate pre-activations over [input ; state] with gru_gate_kloop (rgn_gru_cell.h) on
// v_mfma_f32_16x16x4_f32 - weights as the A operand, sequences as the B operand, exact fp32 products in every precision mode of the handle - then
// the gates in the lane that holds r, z, W_in x + b_in and W_hn h + b_hn of the same (unit, sequence). Step 0 runs no state k-loop and reads no state.
// Sequences past N in the last group are clamped on read (they repeat sequence N - 1) and never stored.
//
// State. Layers below the top keep a ring of two steps, ring[l][s & 1][segment][n][d]; the top layer writes every step into `out`, which is the
// stack's result, and reads step s - 1 from there. Launch delta writes ring[l][(delta - l) & 1] for every l on the diagonal. The readers of
// ring[l][.] in the SAME launch are cell (l, delta - l), which reads its previous state from parity (delta - l - 1) & 1, and cell (l + 1, delta - l - 1),
// which reads its input from parity (delta - l - 1) & 1: both the other slot. The slot a launch overwrites was last read one launch earlier
// (by cell (l, delta - l - 1) as state and cell (l + 1, delta - l - 2) as input, both on diagonal delta - 1), and launches are ordered by the stream.
#include <hip/hip_runtime.h>

#include <vector>

#include "rgn_device.h"
#include "rgn_gru_cell.h"
#include "rgn_internal.h"

namespace rgn {
namespace {

__global__ __launch_bounds__(GRS_WAVES * 64) void k_gru_stack(const GruStackArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = blockIdx.x, grp = blockIdx.y * GRS_WAVES + wave;
    if (grp * GRS_TILE >= a.N) return;                            // (wave-uniform; the kernel has no barrier)
    const int ci = blockIdx.z % a.ncells, seg = blockIdx.z / a.ncells;
    const int l = a.l_lo + ci, s = a.delta - l;
    const int d = a.d, nt = d >> 4, L = a.L;
    const int col = lane & 15, n = grp * GRS_TILE + col, nc = n < a.N ? n : a.N - 1;
    const size_t tile = (size_t)nt * 768, slot = (size_t)a.nseg * a.N * d;

    const float* lw = a.w + (size_t)l * ((size_t)6 * d * d + (size_t)4 * d);
    const float* wx = lw + (size_t)u * tile;
    const float* wh = lw + (size_t)nt * tile + (size_t)u * tile;
    const float* bias = lw + 2 * (size_t)nt * tile;

    // the rows of this segment: the cell's input at step s, its own layer's state at s - 1 and at s
    const float* in;
    long long in_ld;
    if (l == 0) {
        in = a.x + seg * a.x_seg + s * a.x_step;
        in_ld = a.x_seq;
    } else {
        in = a.ring + ((size_t)(l - 1) * 2 + (s & 1)) * slot + (size_t)seg * a.N * d;
        in_ld = d;
    }
    float* cur;
    const float* prev = nullptr;
    long long st_ld;
    if (l == L - 1) {
        cur = a.out + seg * a.o_seg + s * a.o_step;
        if (s > 0) prev = cur - a.o_step;
        st_ld = a.o_seq;
    } else {
        float* base = a.ring + (size_t)l * 2 * slot + (size_t)seg * a.N * d;
        cur = base + (size_t)(s & 1) * slot;
        if (s > 0) prev = base + (size_t)((s - 1) & 1) * slot;
        st_ld = d;
    }

    const int unit0 = u * 16 + (lane >> 4) * 4;                   // C/D layout: column = lane & 15, row = 4 (lane >> 4) + register
    f32x4 ar = *reinterpret_cast<const f32x4*>(bias + unit0), az = *reinterpret_cast<const f32x4*>(bias + d + unit0);
    f32x4 ain = *reinterpret_cast<const f32x4*>(bias + 2 * d + unit0), ahn = *reinterpret_cast<const f32x4*>(bias + 3 * d + unit0);
    // gru_gate_kloop addresses row (lane & 15) of its operand: handing it the rows from (nc - col) on makes that row nc, the clamped sequence
    gru_gate_kloop(wx, nt, in + (long long)(nc - col) * in_ld, (int)in_ld, lane, ar, az, ain);
    f32x4 hp = {0.f, 0.f, 0.f, 0.f};
    if (s > 0) {                                                  // (uniform over the launch's cell) step 0: zero state, nothing read
        gru_gate_kloop(wh, nt, prev + (long long)(nc - col) * st_ld, (int)st_ld, lane, ar, az, ahn);
        hp = *reinterpret_cast<const f32x4*>(prev + (long long)nc * st_ld + unit0);
    }
    f32x4 hv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float r = gru_sigmoid(ar[j]), z = gru_sigmoid(az[j]);
        const float nn = gru_tanh(ain[j] + r * ahn[j]);           // r multiplies W_hn h + b_hn, bias included
        hv[j] = (1.0f - z) * nn + z * hp[j];
    }
    if (n < a.N) *reinterpret_cast<f32x4*>(cur + (long long)n * st_ld + unit0) = hv;
}

// out[b, :] = rows[b, :] + stepemb[*d_step, :] (either addend may be null): the timestep + condition embedding of every evaluation row
__global__ void k_gru_emb(const float* __restrict__ rows, const float* __restrict__ stepemb, const int* __restrict__ d_step, float* __restrict__ out, int d) {
    const int b = blockIdx.x;
    const float* se = stepemb ? stepemb + (size_t)(*d_step) * d : nullptr;
    for (int j = threadIdx.x; j < d; j += blockDim.x) out[(size_t)b * d + j] = (se ? se[j] : 0.f) + (rows ? rows[(size_t)b * d + j] : 0.f);
}

// h[b T + t, :] += e[b, :]: the emb columns of the two pose embeddings, one vector per sample
__global__ __launch_bounds__(256) void k_gru_add_rows(float* __restrict__ h, const float* __restrict__ e, int T, int d, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t row = i / d;
        h[i] += e[(row / T) * d + (i - row * d)];
    }
}

// the top layer's fp32 rows as the K32-blocked operand planes of the output projection
__global__ __launch_bounds__(256) void k_gru_planes(const float* __restrict__ src, Planes hp, int d, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        plane_put(hp, (int)(i / d), (int)(i % d), src[i]);
}

inline int ew_blocks(size_t n) { return (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096); }

}  // namespace

std::vector<float> gru_stack_pack_layer(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int d) {
    std::vector<float> p = gru_pack(w_ih, d, d);
    const std::vector<float> ph = gru_pack(w_hh, d, d);
    p.insert(p.end(), ph.begin(), ph.end());
    const size_t o = p.size();
    p.resize(o + (size_t)4 * d);
    for (int k = 0; k < d; ++k) {                                 // b_ir + b_hr, b_iz + b_hz, b_in, b_hn (the n biases stay apart)
        p[o + k] = b_ih[k] + b_hh[k];
        p[o + d + k] = b_ih[d + k] + b_hh[d + k];
        p[o + 2 * d + k] = b_ih[2 * d + k];
        p[o + 3 * d + k] = b_hh[2 * d + k];
    }
    return p;
}

hipError_t launch_gru_stack(const GruStackArgs& g, hipStream_t s) {
    if (gru_stack_args_error(g)) return hipErrorInvalidValue;
    const int groups = (g.N + GRS_TILE - 1) / GRS_TILE;
    GruStackArgs a = g;
    for (int delta = 0; delta < gru_stack_launches(g.S, g.L); ++delta) {
        a.delta = delta;
        gru_stack_diagonal(delta, g.S, g.L, &a.l_lo, &a.ncells);
        const dim3 grid(g.d / 16, (groups + GRS_WAVES - 1) / GRS_WAVES, a.ncells * g.nseg);
        hipLaunchKernelGGL(k_gru_stack, grid, dim3(GRS_WAVES * 64), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_gru_emb(const float* rows, const float* stepemb, const int* d_step, float* out, int Bm, int d, hipStream_t s) {
    if (Bm <= 0 || d <= 0 || !out || (stepemb && !d_step)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gru_emb, dim3(Bm), dim3(256), 0, s, rows, stepemb, d_step, out, d);
    return hipGetLastError();
}

hipError_t launch_gru_add_rows(float* h, const float* e, int Bm, int T, int d, hipStream_t s) {
    if (Bm <= 0 || T <= 0 || d <= 0 || !h || !e) return hipErrorInvalidValue;
    const size_t n = (size_t)Bm * T * d;
    hipLaunchKernelGGL(k_gru_add_rows, dim3(ew_blocks(n)), dim3(256), 0, s, h, e, T, d, n);
    return hipGetLastError();
}

hipError_t launch_gru_planes(const float* src, Planes hp, int M, int d, hipStream_t s) {
    if (M <= 0 || d <= 0 || !src || !hp.hi) return hipErrorInvalidValue;
    const size_t n = (size_t)M * d;
    hipLaunchKernelGGL(k_gru_planes, dim3(ew_blocks(n)), dim3(256), 0, s, src, hp, d, n);
    return hipGetLastError();
}

}  // namespace rgn
