// The text-motion co-embedding evaluator of the HumanML3D / KIT evaluation (data_loaders/humanml/networks/modules.py: MovementConvEncoder :79-98,
// TextEncoderBiGRUCo :311-350, MotionEncoderBiGRUCo :353-386, as evaluator_wrapper.py:121-187 drives them) and the matching of its embeddings
// (data_loaders/humanml/utils/metrics.py:6-56). Exact fp32 arithmetic on v_mfma_f32_16x16x4_f32; every workgroup independent (no inter-workgroup wait,
// no atomic on a result, no grid barrier).
//
// Three kinds of kernel.
//
// k_rows - every row-parallel layer: the two convolutions (k 4, s 2, p 1), the Linears in front of the recurrence, the hoisted W_ih x + b_ih of BOTH
//   directions, and the head's two Linears. A workgroup owns 16 consecutive output frames of one sequence, stages the window of input frames they read
//   ((16 - 1) stride + taps frames) into LDS once - zeros for a convolution's own padding and for frames behind the sequence's live count, which are
//   never read from memory - and runs
//       D[unit, frame] = sum_tap sum_c W[unit, tap, c] window[stride frame + tap][c]
//   with the weights as the A operand, packed at finalize in fragment order [64 units][tap][16 c][4 tiles][64 lanes][4] so a wave streams contiguous
//   KiBs from L2, four 16-unit tiles sharing each activation fragment. A convolution is a GEMM whose four taps are k-blocks of the same window: no
//   im2col array exists anywhere. A Linear is taps = 1, stride = 1. Only live frames are computed and stored (rgn_t2m_check.h states which).
//
// k_bigru<H> - the recurrence. A workgroup owns 16 sequences of ONE direction for the whole frame loop, their state [2][16][H + 4] in LDS
//   (read one copy, write the other: one barrier per step). Per step it adds W_hh h (A fragments of W_hh streamed from L2, k-loop and cell shared with rgn_gru.hip through rgn_gru_cell.h) to the gate inputs that k_rows left in
//   [N, Lmax, 2, 3 H], applies PyTorch's cell and freezes a finished sequence by a select. Forward: hidden[0], t = 0 .. L-1. Reverse: hidden[1],
//   t = L-1 .. 0 of the same L frames (pack_padded_sequence's semantics, modules.py:341-348). Even workgroups run forward, odd ones reverse: workgroups are
//   dealt to the 8 XCDs in turn, so each XCD's L2 holds one direction's W_hh.
//
// k_ln_lrelu, k_match - row-local: the head's LayerNorm + LeakyReLU, and the distance matrices of groups of up to 32 (text, motion) pairs by direct
//   differences (never -2ab + a^2 + b^2, which cancels), their diagonal and the rank of the true pair.
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "../../include/regennet_hip.h"
#include "rgn_device.h"
#include "rgn_gru_cell.h"
#include "rgn_t2m_check.h"

namespace rgn {
namespace {

constexpr int T2M_NTHR = T2M_WAVES * 64;

// one row-parallel layer: its packed weights and geometry (fixed at finalize)
struct RowsLayer {
    const float* w;        // [ngroups][taps][Cp / 16][4][64][4]
    const float* bias;     // [ngroups * 64], zero behind Nout
    int C, Cp, taps, stride, pad, Nout, ngroups, lrelu;
};
struct RowsArgs {
    RowsLayer l;
    const float* x;        // frame f of sequence n at x + n x_seq + f x_row, C channels
    int64_t x_seq, x_row;
    const int* lens;       // per sequence; null: every frame is live
    int oa, ob, ia, ib;    // live output frames min(Tout, oa len + ob), live input frames min(Tin, ia len + ib)
    const float* res;      // added behind the activation, laid out as y; nullable
    float* y;
    int64_t y_seq, y_row;
    int Tin, Tout;
};

__global__ __launch_bounds__(T2M_NTHR) void k_rows(const RowsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float t2m_win[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x, j0 = blockIdx.y * T2M_TILE;
    int out_live = a.Tout, in_live = a.Tin;
    if (a.lens) {
        const int len = a.lens[n];
        out_live = min(a.Tout, a.oa * len + a.ob);
        in_live = min(a.Tin, a.ia * len + a.ib);
    }
    if (j0 >= out_live) return;
    const RowsLayer& L = a.l;
    const int ld = L.Cp + 4, nwin = (T2M_TILE - 1) * L.stride + L.taps, f0 = j0 * L.stride - L.pad;
    const float* xs = a.x + (size_t)n * a.x_seq;
    for (int idx = tid; idx < nwin * ld; idx += T2M_NTHR) {
        const int wf = idx / ld, c = idx - wf * ld, f = f0 + wf;
        float v = 0.f;                                        // the convolution's own padding, the k pad, and everything behind the live frames
        if (f >= 0 && f < in_live && c < L.C) v = xs[(size_t)f * a.x_row + c];
        t2m_win[idx] = v;
    }
    __syncthreads();
    const int kc = L.Cp / T2M_KC, nq = L.taps * kc;
    const int row = j0 + (lane & 15);
    const float* b = t2m_win + (L.stride * (lane & 15)) * ld + 4 * (lane >> 4);
    for (int g = wave; g < L.ngroups; g += T2M_WAVES) {
        const int unit0 = g * T2M_UG + 4 * (lane >> 4);       // C/D layout: column = lane & 15 (the frame), row = 4 (lane >> 4) + register (the unit)
        f32x4 acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = *reinterpret_cast<const f32x4*>(L.bias + unit0 + 16 * i);
        const f32x4* w = reinterpret_cast<const f32x4*>(L.w + (size_t)g * nq * 1024) + lane;
        f32x4 w0 = w[0], w1 = w[64], w2 = w[128], w3 = w[192];
        int tap = 0, c = 0;
        for (int q = 0; q < nq; ++q) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(b + tap * ld + T2M_KC * c);
            const int qn = q + 1 < nq ? q + 1 : q;
            const f32x4 n0 = w[qn * 256], n1 = w[qn * 256 + 64], n2 = w[qn * 256 + 128], n3 = w[qn * 256 + 192];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0[j], bv[j], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1[j], bv[j], acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(w2[j], bv[j], acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(w3[j], bv[j], acc[3], 0, 0, 0);
            }
            w0 = n0; w1 = n1; w2 = n2; w3 = n3;
            if (++c == kc) { c = 0; ++tap; }
        }
        if (row < out_live) {
            const size_t at = (size_t)n * a.y_seq + (size_t)row * a.y_row;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int u = unit0 + 16 * i;
                if (u < L.Nout) {                             // Nout is a multiple of 4: a quad is whole or absent
                    f32x4 v = acc[i];
                    if (L.lrelu)
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = v[j] >= 0.f ? v[j] : 0.2f * v[j];
                    if (a.res) v += *reinterpret_cast<const f32x4*>(a.res + at + u);
                    *reinterpret_cast<f32x4*>(a.y + at + u) = v;
                }
            }
        }
    }
}

// lens[n] = clamp(src[n] / div, 1, maxv), flagged when the clamp acted; src null: maxv (every frame)
__global__ void k_t2m_lens(const int64_t* src, int N, int div, int maxv, int* lens, int* status) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    int len = maxv;
    if (src) {
        const int64_t v = src[n] / div;
        if (v < 1 || v > maxv) *status = 1;      // a plain store from any number of threads: all write the same 1, the flag is only ever read for != 0
        len = v < 1 ? 1 : v > maxv ? maxv : (int)v;
    }
    lens[n] = len;
}

struct BigruArgs {
    const float* wh[2];    // packed W_hh per direction [H/16][H/16][3][64][4]
    const float* bhn[2];   // b_hn per direction [H]
    const float* h0;       // hidden [2][H]
    const float* gi;       // [N, Lmax, 2, 3 H]: W_ih x + b_ih (+ b_hh for r and z)
    const int* lens;       // [N], in [1, Lmax]
    float* hcat;           // [N, 2 H] = cat(h_fwd, h_rev)
    int N, Lmax;
};

template <int H>
__global__ __launch_bounds__(T2M_NTHR) void k_bigru(const BigruArgs a) {
    extern __shared__ __attribute__((aligned(16))) float t2m_state[];
    constexpr int NT = H / 16, HLD = H + 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dir = blockIdx.x & 1, n0 = (blockIdx.x >> 1) * T2M_TILE, N = a.N;
    // two copies of the state: a step reads one and writes the other, so one barrier closes it and no new value waits in registers
    constexpr int COPY = T2M_TILE * HLD;
    int* lens = reinterpret_cast<int*>(t2m_state + 2 * T2M_TILE * HLD);
    if (tid < T2M_TILE) lens[tid] = n0 + tid < N ? a.lens[n0 + tid] : 0;      // a pad sequence of the last tile: never live, never stored
    for (int idx = tid; idx < T2M_TILE * H; idx += T2M_NTHR) {
        const int s = idx / H, k = idx - s * H;
        t2m_state[s * HLD + k] = a.h0[dir * H + k];
    }
    __syncthreads();
    int tmax = 0;
#pragma unroll
    for (int s = 0; s < T2M_TILE; ++s) tmax = max(tmax, lens[s]);
    const int seq = lane & 15, len = lens[seq];
    const float* wh = a.wh[dir];
    const float* bhn = a.bhn[dir];
    const float* girow = a.gi + ((size_t)(n0 + seq) * a.Lmax * 2 + dir) * 3 * H;

    for (int s = 0; s < tmax; ++s) {
        const bool live = s < len;
        const int t = dir ? len - 1 - s : s;
        const float* g = girow + (size_t)(live ? t : 0) * 6 * H;
        const float* hs = t2m_state + (s & 1) * COPY;
        float* hw = t2m_state + ((s & 1) ^ 1) * COPY;
#pragma unroll 1
        for (int u = wave; u < NT; u += T2M_WAVES) {          // one unit tile at a time: its three accumulators and fragments are all a wave holds
            const int unit0 = u * 16 + (lane >> 4) * 4;       // C/D layout: column = lane & 15 (the sequence), row = 4 (lane >> 4) + register
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            f32x4 ar = zero, az = zero, gin = zero;           // a finished (or pad) sequence reads no gate input: its column is discarded below
            if (live) {
                ar = *reinterpret_cast<const f32x4*>(g + unit0);
                az = *reinterpret_cast<const f32x4*>(g + H + unit0);
                gin = *reinterpret_cast<const f32x4*>(g + 2 * H + unit0);
            }
            f32x4 ahn = *reinterpret_cast<const f32x4*>(bhn + unit0);
            gru_gate_kloop(wh + (size_t)u * NT * 768, NT, hs, HLD, lane, ar, az, ahn);
            const f32x4 hp = *reinterpret_cast<const f32x4*>(hs + seq * HLD + unit0);
            f32x4 hn;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float r = gru_sigmoid(ar[j]), z = gru_sigmoid(az[j]);
                const float nn = gru_tanh(gin[j] + r * ahn[j]);
                const float hv = (1.0f - z) * nn + z * hp[j];
                hn[j] = live ? hv : hp[j];
            }
            *reinterpret_cast<f32x4*>(hw + seq * HLD + unit0) = hn;
        }
        __syncthreads();                                      // the new state is complete, and nobody reads the old one any more
    }
    const float* hs = t2m_state + (tmax & 1) * COPY;
    for (int idx = tid; idx < T2M_TILE * H; idx += T2M_NTHR) {
        const int s = idx / H, k = idx - s * H;
        if (n0 + s < N) a.hcat[(size_t)(n0 + s) * 2 * H + dir * H + k] = hs[s * HLD + k];
    }
}

template <class Fn>
bool t2m_dispatch_h(int H, Fn&& f) {
    switch (H / 64) {
#define T2M_CASE(q) case q: f(std::integral_constant<int, 64 * q>{}); return true;
        T2M_CASE(1) T2M_CASE(2) T2M_CASE(3) T2M_CASE(4) T2M_CASE(5) T2M_CASE(6) T2M_CASE(7) T2M_CASE(8)
        T2M_CASE(9) T2M_CASE(10) T2M_CASE(11) T2M_CASE(12) T2M_CASE(13) T2M_CASE(14) T2M_CASE(15) T2M_CASE(16)
#undef T2M_CASE
    }
    return false;
}

// y[row] = LeakyReLU_0.2(LayerNorm(x[row])) over H values (eps 1e-5, biased variance, two passes); one workgroup of 256 per row, sums in a fixed tree
__global__ __launch_bounds__(256) void k_ln_lrelu(const float* x, const float* gamma, const float* beta, float* y, int H) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    const float* xr = x + (size_t)blockIdx.x * H;
    float s = 0.f;
    for (int k = tid; k < H; k += 256) s += xr[k];
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    const float mean = red[0] / (float)H;
    __syncthreads();
    s = 0.f;
    for (int k = tid; k < H; k += 256) {
        const float d = xr[k] - mean;
        s = fmaf(d, d, s);
    }
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    const float rstd = 1.0f / sqrtf(red[0] / (float)H + 1e-5f);
    for (int k = tid; k < H; k += 256) {
        const float v = (xr[k] - mean) * rstd * gamma[k] + beta[k];
        y[(size_t)blockIdx.x * H + k] = v >= 0.f ? v : 0.2f * v;
    }
}

// One workgroup per group of up to 32 pairs: d[i, j] = || text_i - motion_j || by direct differences, four fp32 fma chains in k order; diag[i] = d[i, i];
// rank[i] = #{ j : d[i, j] < d[i, i] } - the number of motions STRICTLY nearer to text i than its own. A tie with the true pair does not count against
// it (the reference's argsort would break it by position).
__global__ __launch_bounds__(256) void k_match(const float* text, const float* motion, int N, int D, int group, float* diag, int* rank) {
    __shared__ float d[T2M_MAX_GROUP][T2M_MAX_GROUP + 1];
    const int tid = threadIdx.x, g0 = blockIdx.x * group, gs = min(group, N - g0);
    for (int p = tid; p < gs * gs; p += 256) {
        const int i = p / gs, j = p - i * gs;
        const f32x4* ti = reinterpret_cast<const f32x4*>(text + (size_t)(g0 + i) * D);
        const f32x4* mj = reinterpret_cast<const f32x4*>(motion + (size_t)(g0 + j) * D);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};                     // four chains, one per position in the quad: a quarter of the terms each
        for (int k = 0; k < D / 4; ++k) {
            const f32x4 df = ti[k] - mj[k];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = fmaf(df[q], df[q], acc[q]);
        }
        d[i][j] = sqrtf((acc[0] + acc[1]) + (acc[2] + acc[3]));
    }
    __syncthreads();
    if (tid < gs) {
        const float own = d[tid][tid];
        int r = 0;
        for (int j = 0; j < gs; ++j) r += d[tid][j] < own ? 1 : 0;
        diag[g0 + tid] = own;
        rank[g0 + tid] = r;
    }
}

// W(unit, tap, c) -> [ngroups][taps][Cp / 16][4 tiles][64 lanes][4], zero behind Nout and behind C
template <class Get>
std::vector<float> t2m_pack_rows(Get&& W, int Nout, int taps, int C) {
    const int Cp = t2m_pad(C, T2M_KC), kc = Cp / T2M_KC, ng = t2m_pad(Nout, T2M_UG) / T2M_UG;
    std::vector<float> p((size_t)ng * taps * kc * 1024, 0.f);
    for (int g = 0; g < ng; ++g)
        for (int tap = 0; tap < taps; ++tap)
            for (int c = 0; c < kc; ++c)
                for (int i = 0; i < 4; ++i)
                    for (int l = 0; l < 64; ++l)
                        for (int j = 0; j < 4; ++j) {
                            const int k = c * T2M_KC + 4 * (l >> 4) + j, u = g * T2M_UG + 16 * i + (l & 15);
                            if (k < C && u < Nout) p[((((size_t)g * taps + tap) * kc + c) * 4 + i) * 256 + l * 4 + j] = W(u, tap, k);
                        }
    return p;
}

struct T2mEncoder {       // one bidirectional encoder behind its gate-input layer
    RowsLayer gi, head0, head3;
    BigruArgs ru{};
    const float *ln_g = nullptr, *ln_b = nullptr;
    int H = 0;
};

thread_local std::string g_t2m_create_error;

}  // namespace
}  // namespace rgn

struct rgn_t2m_ctx {
    rgn_t2m_config cfg{};
    rgn::T2mGeom geom{};
    std::string err;
    std::map<std::string, std::vector<float>> sd;
    std::map<std::string, std::vector<int64_t>> want;
    bool finalized = false;
    std::vector<void*> allocs;
    rgn::RowsLayer conv1{}, conv2{}, outnet{}, memb{}, pos{}, temb{};
    rgn::T2mEncoder menc{}, tenc{};
    int* status = nullptr;
    int fail(int code, const std::string& m) {
        err = m;
        return code;
    }
};

namespace rgn {
namespace {

int t2m_boundary_error(rgn_t2m_ctx* h, const char* fn, const char* what) noexcept {
    try {
        std::string m = std::string(fn) + ": C++ exception at the boundary: " + what;
        if (h) h->err.swap(m);
        else g_t2m_create_error.swap(m);
    } catch (...) {
    }
    return RGN_ERR_INTERNAL;
}
template <class F>
int t2m_guard(rgn_t2m_ctx* h, const char* fn, F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return t2m_boundary_error(h, fn, "std::bad_alloc (host memory)");
    } catch (const std::exception& e) {
        return t2m_boundary_error(h, fn, e.what());
    } catch (...) {
        return t2m_boundary_error(h, fn, "unknown exception");
    }
}
int t2m_hip_fail(rgn_t2m_ctx* c, const char* what, hipError_t e) { return c->fail(RGN_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
#define T2M_HIP(c, call)                                                  \
    do {                                                                  \
        hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) return rgn::t2m_hip_fail(c, #call, e_);     \
    } while (0)

int t2m_upload(rgn_t2m_ctx* c, const float** dst, const std::vector<float>& v) {
    void* p = nullptr;
    T2M_HIP(c, hipMalloc(&p, v.size() * sizeof(float)));
    c->allocs.push_back(p);
    T2M_HIP(c, hipMemcpy(p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    *dst = static_cast<const float*>(p);
    return RGN_OK;
}

std::string t2m_shape_text(const std::vector<int64_t>& s) {
    std::string t = "[";
    for (size_t i = 0; i < s.size(); ++i) t += (i ? ", " : "") + std::to_string(s[i]);
    return t + "]";
}

// a row layer from a [Nout, C] Linear weight (taps == 1) or a [Nout, C, 4] Conv1d weight (taps == 4: k 4, s 2, p 1)
int t2m_make_layer(rgn_t2m_ctx* c, RowsLayer* L, const std::vector<float>& W, const std::vector<float>& bias, int Nout, int C, int taps, int lrelu) {
    L->C = C; L->Cp = t2m_pad(C, T2M_KC); L->taps = taps; L->stride = taps == 4 ? 2 : 1; L->pad = taps == 4 ? 1 : 0;
    L->Nout = Nout; L->ngroups = t2m_pad(Nout, T2M_UG) / T2M_UG; L->lrelu = lrelu;
    std::vector<float> b((size_t)L->ngroups * T2M_UG, 0.f);
    for (int u = 0; u < Nout; ++u) b[u] = bias[u];
    int rc;
    if ((rc = t2m_upload(c, &L->w, t2m_pack_rows([&](int u, int tap, int k) { return W[((size_t)u * C + k) * taps + tap]; }, Nout, taps, C)))) return rc;
    return t2m_upload(c, &L->bias, b);
}

// the part of an encoder behind input_emb: W_ih of both directions as ONE row layer (b_ih, + b_hh for r and z), W_hh packed per direction, the head
int t2m_make_encoder(rgn_t2m_ctx* c, T2mEncoder* e, const std::string& pre, int H, int D) {
    e->H = H;
    std::vector<float> W((size_t)6 * H * H), b((size_t)6 * H);
    int rc;
    for (int d = 0; d < 2; ++d) {
        const std::string s = d ? "_l0_reverse" : "_l0";
        const std::vector<float>&wi = c->sd[pre + "gru.weight_ih" + s], &bi = c->sd[pre + "gru.bias_ih" + s], &bh = c->sd[pre + "gru.bias_hh" + s];
        std::memcpy(W.data() + (size_t)d * 3 * H * H, wi.data(), (size_t)3 * H * H * sizeof(float));
        std::vector<float> bhn(H);
        for (int k = 0; k < H; ++k) {
            b[(size_t)d * 3 * H + k] = bi[k] + bh[k];
            b[(size_t)d * 3 * H + H + k] = bi[H + k] + bh[H + k];
            b[(size_t)d * 3 * H + 2 * H + k] = bi[2 * H + k];
            bhn[k] = bh[2 * H + k];
        }
        if ((rc = t2m_upload(c, &e->ru.wh[d], gru_pack(c->sd[pre + "gru.weight_hh" + s].data(), H, H)))) return rc;
        if ((rc = t2m_upload(c, &e->ru.bhn[d], bhn))) return rc;
    }
    if ((rc = t2m_make_layer(c, &e->gi, W, b, 6 * H, H, 1, 0))) return rc;
    if ((rc = t2m_upload(c, &e->ru.h0, c->sd[pre + "hidden"]))) return rc;
    if ((rc = t2m_make_layer(c, &e->head0, c->sd[pre + "output_net.0.weight"], c->sd[pre + "output_net.0.bias"], H, 2 * H, 1, 0))) return rc;
    if ((rc = t2m_upload(c, &e->ln_g, c->sd[pre + "output_net.1.weight"])) || (rc = t2m_upload(c, &e->ln_b, c->sd[pre + "output_net.1.bias"]))) return rc;
    return t2m_make_layer(c, &e->head3, c->sd[pre + "output_net.3.weight"], c->sd[pre + "output_net.3.bias"], D, H, 1, 0);
}

void t2m_want_encoder(rgn_t2m_ctx* c, const std::string& pre, int64_t H, int64_t D) {
    for (const char* s : {"_l0", "_l0_reverse"}) {
        c->want[pre + "gru.weight_ih" + s] = {3 * H, H};
        c->want[pre + "gru.weight_hh" + s] = {3 * H, H};
        c->want[pre + "gru.bias_ih" + s] = {3 * H};
        c->want[pre + "gru.bias_hh" + s] = {3 * H};
    }
    c->want[pre + "hidden"] = {2, 1, H};
    c->want[pre + "output_net.0.weight"] = {H, 2 * H};
    c->want[pre + "output_net.0.bias"] = {H};
    c->want[pre + "output_net.1.weight"] = {H};
    c->want[pre + "output_net.1.bias"] = {H};
    c->want[pre + "output_net.3.weight"] = {D, H};
    c->want[pre + "output_net.3.bias"] = {D};
}

// one k_rows launch. nseq sequences of Tin -> Tout frames; lens null: a flat [Tout] list of rows, all live
void t2m_rows(const RowsLayer& L, const float* x, int64_t x_seq, int64_t x_row, int nseq, int Tin, int Tout, const int* lens, int oa, int ob, int ia, int ib,
              const float* res, float* y, int64_t y_seq, int64_t y_row, hipStream_t st) {
    RowsArgs a{};
    a.l = L; a.x = x; a.x_seq = x_seq; a.x_row = x_row; a.lens = lens; a.oa = oa; a.ob = ob; a.ia = ia; a.ib = ib; a.res = res; a.y = y;
    a.y_seq = y_seq; a.y_row = y_row; a.Tin = Tin; a.Tout = Tout;
    const dim3 grid(nseq, (Tout - 1) / T2M_TILE + 1), block(T2M_NTHR);
    hipLaunchKernelGGL(k_rows, grid, block, t2m_rows_lds_bytes(L.C, L.taps, L.stride), st, a);
}

// gate inputs -> recurrence -> head, for N sequences of up to Lmax frames whose input_emb rows are at p.emb
void t2m_encode(const T2mEncoder& e, const T2mPlan& p, char* work, int N, int Lmax, float* emb_out, int D, hipStream_t st) {
    const int H = e.H;
    const int* lens = reinterpret_cast<const int*>(work + p.lens);
    float *emb = reinterpret_cast<float*>(work + p.emb), *gi = reinterpret_cast<float*>(work + p.gi), *hcat = reinterpret_cast<float*>(work + p.hcat);
    float *y1 = reinterpret_cast<float*>(work + p.y1), *y2 = reinterpret_cast<float*>(work + p.y2);
    t2m_rows(e.gi, emb, (int64_t)Lmax * H, H, N, Lmax, Lmax, lens, 1, 0, 1, 0, nullptr, gi, (int64_t)Lmax * 6 * H, 6 * H, st);
    BigruArgs r = e.ru;
    r.gi = gi; r.lens = lens; r.hcat = hcat; r.N = N; r.Lmax = Lmax;
    const dim3 grid(2 * ((N - 1) / T2M_TILE + 1)), block(T2M_NTHR);
    const size_t lds = (size_t)t2m_bigru_lds_bytes(H);
    t2m_dispatch_h(H, [&](auto HH) { hipLaunchKernelGGL(k_bigru<decltype(HH)::value>, grid, block, lds, st, r); });
    t2m_rows(e.head0, hcat, 0, 2 * H, 1, N, N, nullptr, 1, 0, 1, 0, nullptr, y1, 0, H, st);
    hipLaunchKernelGGL(k_ln_lrelu, dim3(N), dim3(256), 0, st, y1, e.ln_g, e.ln_b, y2, H);
    t2m_rows(e.head3, y2, 0, H, 1, N, N, nullptr, 1, 0, 1, 0, nullptr, emb_out, 0, D, st);
}

void t2m_lens(rgn_t2m_ctx* c, const int64_t* src, int N, int div, int maxv, char* work, size_t off, hipStream_t st) {
    hipLaunchKernelGGL(k_t2m_lens, dim3((N + 255) / 256), dim3(256), 0, st, src, N, div, maxv, reinterpret_cast<int*>(work + off), c->status);
}

// the movement encoder for N motions of T frames (in_stride floats per frame, the first dim_pose - 4 of them read) into mov [N, T2, Dm]; lens at p.lens
void t2m_movements(rgn_t2m_ctx* c, const T2mPlan& p, char* work, int N, int T, int in_stride, const float* x, float* mov, hipStream_t st) {
    const int T1 = t2m_t1(T), T2 = t2m_t2(T), Hm = c->geom.Hm, Dm = c->geom.Dm;
    const int* lens = reinterpret_cast<const int*>(work + p.lens);
    float *a = reinterpret_cast<float*>(work + p.a), *b = reinterpret_cast<float*>(work + p.b);
    t2m_rows(c->conv1, x, (int64_t)T * in_stride, in_stride, N, T, T1, lens, 2, 1, 4, 3, nullptr, a, (int64_t)T1 * Hm, Hm, st);
    t2m_rows(c->conv2, a, (int64_t)T1 * Hm, Hm, N, T1, T2, lens, 1, 0, 2, 1, nullptr, b, (int64_t)T2 * Dm, Dm, st);
    t2m_rows(c->outnet, b, (int64_t)T2 * Dm, Dm, N, T2, T2, lens, 1, 0, 1, 0, nullptr, mov, (int64_t)T2 * Dm, Dm, st);
}

int t2m_call_error(rgn_t2m_ctx* h, const char* fn, const char* why) {
    const std::string m = std::string(fn) + ": " + why;
    if (h) h->err = m;
    else g_t2m_create_error = m;
    return RGN_ERR_INVALID_ARG;
}

}  // namespace
}  // namespace rgn

extern "C" {

const char* rgn_t2m_last_error(rgn_t2m_handle h) { return h ? h->err.c_str() : rgn::g_t2m_create_error.c_str(); }

int rgn_t2m_create(const rgn_t2m_config* cfg, rgn_t2m_handle* out) {
    using namespace rgn;
    return t2m_guard(nullptr, "rgn_t2m_create", [&]() -> int {
        if (!cfg || !out) {
            g_t2m_create_error = "rgn_t2m_create: null argument";
            return RGN_ERR_INVALID_ARG;
        }
        *out = nullptr;
        if (const char* why = t2m_geometry_error(cfg->dim_pose, cfg->movement_hidden, cfg->movement_latent, cfg->motion_hidden, cfg->dim_word, cfg->dim_pos_ohot,
                                                 cfg->text_hidden, cfg->coemb, cfg->unit_length)) {
            g_t2m_create_error = std::string("rgn_t2m_create: ") + why;
            return RGN_ERR_UNSUPPORTED;
        }
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) {
            g_t2m_create_error = "rgn_t2m_create: no HIP device visible, or no such device";
            return RGN_ERR_HIP;
        }
        rgn_t2m_ctx* c = new rgn_t2m_ctx();
        c->cfg = *cfg;
        c->geom = T2mGeom{cfg->dim_pose, cfg->movement_hidden, cfg->movement_latent, cfg->motion_hidden, cfg->dim_word, cfg->dim_pos_ohot, cfg->text_hidden,
                          cfg->coemb};
        const int64_t C = cfg->dim_pose - 4, Hm = cfg->movement_hidden, Dm = cfg->movement_latent, H = cfg->motion_hidden, W = cfg->dim_word,
                      P = cfg->dim_pos_ohot, Ht = cfg->text_hidden, D = cfg->coemb;
        c->want["movement_encoder.main.0.weight"] = {Hm, C, 4};
        c->want["movement_encoder.main.0.bias"] = {Hm};
        c->want["movement_encoder.main.3.weight"] = {Dm, Hm, 4};
        c->want["movement_encoder.main.3.bias"] = {Dm};
        c->want["movement_encoder.out_net.weight"] = {Dm, Dm};
        c->want["movement_encoder.out_net.bias"] = {Dm};
        c->want["motion_encoder.input_emb.weight"] = {H, Dm};
        c->want["motion_encoder.input_emb.bias"] = {H};
        t2m_want_encoder(c, "motion_encoder.", H, D);
        c->want["text_encoder.pos_emb.weight"] = {W, P};
        c->want["text_encoder.pos_emb.bias"] = {W};
        c->want["text_encoder.input_emb.weight"] = {Ht, W};
        c->want["text_encoder.input_emb.bias"] = {Ht};
        t2m_want_encoder(c, "text_encoder.", Ht, D);
        *out = c;
        return RGN_OK;
    });
}

int rgn_t2m_destroy(rgn_t2m_handle h) {
    return rgn::t2m_guard(h, "rgn_t2m_destroy", [&]() -> int {
        if (!h) return RGN_ERR_INVALID_ARG;
        (void)hipSetDevice(h->cfg.device);
        (void)hipDeviceSynchronize();
        for (void* p : h->allocs) (void)hipFree(p);
        delete h;
        return RGN_OK;
    });
}

int rgn_t2m_load_weight(rgn_t2m_handle h, const char* key, const float* host, const int64_t* shape, int32_t ndim) {
    using namespace rgn;
    return t2m_guard(h, "rgn_t2m_load_weight", [&]() -> int {
        if (!h) return RGN_ERR_INVALID_ARG;
        if (!key || !host || ndim < 1 || !shape) return h->fail(RGN_ERR_INVALID_ARG, "rgn_t2m_load_weight: null/empty argument");
        if (h->finalized) return h->fail(RGN_ERR_STATE, "rgn_t2m_load_weight: already finalized");
        auto it = h->want.find(key);
        if (it == h->want.end()) return h->fail(RGN_ERR_BAD_KEY, std::string("rgn_t2m_load_weight: unexpected key '") + key + "'");
        if (h->sd.count(key)) return h->fail(RGN_ERR_BAD_KEY, std::string("rgn_t2m_load_weight: key '") + key + "' loaded twice");
        const std::vector<int64_t> got(shape, shape + ndim);
        if (got != it->second)
            return h->fail(RGN_ERR_BAD_SHAPE, std::string("rgn_t2m_load_weight: '") + key + "' has shape " + t2m_shape_text(got) + ", expected " + t2m_shape_text(it->second));
        size_t n = 1;
        for (int64_t d : got) n *= (size_t)d;
        h->sd[key].assign(host, host + n);
        return RGN_OK;
    });
}

int rgn_t2m_finalize(rgn_t2m_handle h) {
    using namespace rgn;
    return t2m_guard(h, "rgn_t2m_finalize", [&]() -> int {
        if (!h) return RGN_ERR_INVALID_ARG;
        rgn_t2m_ctx* c = h;
        if (c->finalized) return c->fail(RGN_ERR_STATE, "rgn_t2m_finalize: already finalized");
        std::string missing;
        for (const auto& kv : c->want)
            if (!c->sd.count(kv.first)) missing += (missing.empty() ? "" : ", ") + kv.first;
        if (!missing.empty()) return c->fail(RGN_ERR_MISSING_KEY, "rgn_t2m_finalize: missing " + missing);
        T2M_HIP(c, hipSetDevice(c->cfg.device));
        const T2mGeom& g = c->geom;
        auto& sd = c->sd;
        int rc;
        if ((rc = t2m_make_layer(c, &c->conv1, sd["movement_encoder.main.0.weight"], sd["movement_encoder.main.0.bias"], g.Hm, g.dim_pose - 4, 4, 1))) return rc;
        if ((rc = t2m_make_layer(c, &c->conv2, sd["movement_encoder.main.3.weight"], sd["movement_encoder.main.3.bias"], g.Dm, g.Hm, 4, 1))) return rc;
        if ((rc = t2m_make_layer(c, &c->outnet, sd["movement_encoder.out_net.weight"], sd["movement_encoder.out_net.bias"], g.Dm, g.Dm, 1, 0))) return rc;
        if ((rc = t2m_make_layer(c, &c->memb, sd["motion_encoder.input_emb.weight"], sd["motion_encoder.input_emb.bias"], g.H, g.Dm, 1, 0))) return rc;
        if ((rc = t2m_make_encoder(c, &c->menc, "motion_encoder.", g.H, g.D))) return rc;
        if ((rc = t2m_make_layer(c, &c->pos, sd["text_encoder.pos_emb.weight"], sd["text_encoder.pos_emb.bias"], g.W, g.P, 1, 0))) return rc;
        if ((rc = t2m_make_layer(c, &c->temb, sd["text_encoder.input_emb.weight"], sd["text_encoder.input_emb.bias"], g.Ht, g.W, 1, 0))) return rc;
        if ((rc = t2m_make_encoder(c, &c->tenc, "text_encoder.", g.Ht, g.D))) return rc;
        void* st = nullptr;
        T2M_HIP(c, hipMalloc(&st, sizeof(int)));
        c->allocs.push_back(st);
        T2M_HIP(c, hipMemset(st, 0, sizeof(int)));
        c->status = static_cast<int*>(st);
        T2M_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_rows), hipFuncAttributeMaxDynamicSharedMemorySize, T2M_LDS_LIMIT));
        for (int H : {g.H, g.Ht}) {
            hipError_t e = hipSuccess;
            t2m_dispatch_h(H, [&](auto HH) {
                e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_bigru<decltype(HH)::value>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        t2m_bigru_lds_bytes(H));
            });
            T2M_HIP(c, e);
        }
        c->sd.clear();
        c->finalized = true;
        return RGN_OK;
    });
}

int rgn_t2m_workspace(rgn_t2m_handle h, int32_t N, int32_t T, int32_t Lw, size_t* bytes) {
    using namespace rgn;
    return t2m_guard(h, "rgn_t2m_workspace", [&]() -> int {
        if (!h) {
            g_t2m_create_error = "rgn_t2m_workspace: null handle";
            return RGN_ERR_INVALID_ARG;
        }
        if (!bytes) return h->fail(RGN_ERR_INVALID_ARG, "rgn_t2m_workspace: null argument");
        if (const char* why = t2m_shape_error(N, T, Lw)) return t2m_call_error(h, "rgn_t2m_workspace", why);
        *bytes = t2m_workspace_bytes(h->geom, N, T, Lw);
        return RGN_OK;
    });
}

int rgn_t2m_movements(rgn_t2m_handle h, int32_t N, int32_t T, int32_t in_stride, const float* x_dev, const int64_t* m_lens_dev, float* mov_dev, void* work,
                      size_t work_bytes, void* stream) {
    using namespace rgn;
    return t2m_guard(h, "rgn_t2m_movements", [&]() -> int {
        const size_t need = h && !t2m_shape_error(N, T, 1) ? t2m_motion_plan(h->geom, N, T).total : 0;
        if (const char* why = t2m_motion_error(N, T, x_dev, m_lens_dev, mov_dev, work, work_bytes, need, true)) return t2m_call_error(h, "rgn_t2m_movements", why);
        if (!h) return t2m_call_error(h, "rgn_t2m_movements", "null handle");
        if (in_stride < h->geom.dim_pose - 4) return t2m_call_error(h, "rgn_t2m_movements", "in_stride below dim_pose - 4");
        if (!h->finalized) return h->fail(RGN_ERR_STATE, "rgn_t2m_movements: weights not finalized");
        T2M_HIP(h, hipSetDevice(h->cfg.device));
        const T2mPlan p = t2m_motion_plan(h->geom, N, T);
        hipStream_t st = static_cast<hipStream_t>(stream);
        t2m_lens(h, m_lens_dev, N, h->cfg.unit_length, t2m_t2(T), static_cast<char*>(work), p.lens, st);
        t2m_movements(h, p, static_cast<char*>(work), N, T, in_stride, x_dev, mov_dev, st);
        T2M_HIP(h, hipGetLastError());
        return RGN_OK;
    });
}

int rgn_t2m_encode_movements(rgn_t2m_handle h, int32_t N, int32_t T2, const float* mov_dev, const int64_t* lens_dev, float* emb_dev, void* work,
                             size_t work_bytes, void* stream) {
    using namespace rgn;
    return t2m_guard(h, "rgn_t2m_encode_movements", [&]() -> int {
        const int64_t T = 4 * (int64_t)T2;
        const bool shape_ok = T2 >= 1 && !t2m_shape_error(N, T, 1);
        const size_t need = h && shape_ok ? t2m_motion_plan(h->geom, N, T).total : 0;
        if (T2 < 1 || T2 > T2M_MAX_T / 4) return t2m_call_error(h, "rgn_t2m_encode_movements", "T2 outside [1, 1024]");
        if (const char* why = t2m_motion_error(N, T, mov_dev, lens_dev, emb_dev, work, work_bytes, need)) return t2m_call_error(h, "rgn_t2m_encode_movements", why);
        if (!h) return t2m_call_error(h, "rgn_t2m_encode_movements", "null handle");
        if (!h->finalized) return h->fail(RGN_ERR_STATE, "rgn_t2m_encode_movements: weights not finalized");
        T2M_HIP(h, hipSetDevice(h->cfg.device));
        const T2mPlan p = t2m_motion_plan(h->geom, N, T);
        hipStream_t st = static_cast<hipStream_t>(stream);
        char* w = static_cast<char*>(work);
        const int Dm = h->geom.Dm, H = h->geom.H;
        t2m_lens(h, lens_dev, N, 1, T2, w, p.lens, st);
        t2m_rows(h->memb, mov_dev, (int64_t)T2 * Dm, Dm, N, T2, T2, reinterpret_cast<const int*>(w + p.lens), 1, 0, 1, 0, nullptr,
                 reinterpret_cast<float*>(w + p.emb), (int64_t)T2 * H, H, st);
        t2m_encode(h->menc, p, w, N, T2, emb_dev, h->geom.D, st);
        T2M_HIP(h, hipGetLastError());
        return RGN_OK;
    });
}

int rgn_t2m_motion_embeddings(rgn_t2m_handle h, int32_t N, int32_t T, const float* motions_dev, const int64_t* m_lens_dev, float* emb_dev, void* work,
                              size_t work_bytes, void* stream) {
    using namespace rgn;
    return t2m_guard(h, "rgn_t2m_motion_embeddings", [&]() -> int {
        const size_t need = h && !t2m_shape_error(N, T, 1) ? t2m_motion_plan(h->geom, N, T).total : 0;
        if (const char* why = t2m_motion_error(N, T, motions_dev, m_lens_dev, emb_dev, work, work_bytes, need)) return t2m_call_error(h, "rgn_t2m_motion_embeddings", why);
        if (!h) return t2m_call_error(h, "rgn_t2m_motion_embeddings", "null handle");
        if (!h->finalized) return h->fail(RGN_ERR_STATE, "rgn_t2m_motion_embeddings: weights not finalized");
        T2M_HIP(h, hipSetDevice(h->cfg.device));
        const T2mPlan p = t2m_motion_plan(h->geom, N, T);
        hipStream_t st = static_cast<hipStream_t>(stream);
        char* w = static_cast<char*>(work);
        const int T2 = t2m_t2(T), Dm = h->geom.Dm, H = h->geom.H;
        t2m_lens(h, m_lens_dev, N, h->cfg.unit_length, T2, w, p.lens, st);
        float* mov = reinterpret_cast<float*>(w + p.c);
        t2m_movements(h, p, w, N, T, h->geom.dim_pose, motions_dev, mov, st);
        t2m_rows(h->memb, mov, (int64_t)T2 * Dm, Dm, N, T2, T2, reinterpret_cast<const int*>(w + p.lens), 1, 0, 1, 0, nullptr,
                 reinterpret_cast<float*>(w + p.emb), (int64_t)T2 * H, H, st);
        t2m_encode(h->menc, p, w, N, T2, emb_dev, h->geom.D, st);
        T2M_HIP(h, hipGetLastError());
        return RGN_OK;
    });
}

int rgn_t2m_text_embeddings(rgn_t2m_handle h, int32_t N, int32_t Lw, const float* word_embs_dev, const float* pos_ohot_dev, const int64_t* cap_lens_dev,
                            float* emb_dev, void* work, size_t work_bytes, void* stream) {
    using namespace rgn;
    return t2m_guard(h, "rgn_t2m_text_embeddings", [&]() -> int {
        const size_t need = h && !t2m_shape_error(N, 4, Lw) ? t2m_text_plan(h->geom, N, Lw).total : 0;
        if (const char* why = t2m_text_error(N, Lw, word_embs_dev, pos_ohot_dev, cap_lens_dev, emb_dev, work, work_bytes, need))
            return t2m_call_error(h, "rgn_t2m_text_embeddings", why);
        if (!h) return t2m_call_error(h, "rgn_t2m_text_embeddings", "null handle");
        if (!h->finalized) return h->fail(RGN_ERR_STATE, "rgn_t2m_text_embeddings: weights not finalized");
        T2M_HIP(h, hipSetDevice(h->cfg.device));
        const T2mPlan p = t2m_text_plan(h->geom, N, Lw);
        hipStream_t st = static_cast<hipStream_t>(stream);
        char* w = static_cast<char*>(work);
        const int W = h->geom.W, P = h->geom.P, Ht = h->geom.Ht;
        const int* lens = reinterpret_cast<const int*>(w + p.lens);
        float *x1 = reinterpret_cast<float*>(w + p.a), *emb = reinterpret_cast<float*>(w + p.emb);
        t2m_lens(h, cap_lens_dev, N, 1, Lw, w, p.lens, st);
        t2m_rows(h->pos, pos_ohot_dev, (int64_t)Lw * P, P, N, Lw, Lw, lens, 1, 0, 1, 0, word_embs_dev, x1, (int64_t)Lw * W, W, st);
        t2m_rows(h->temb, x1, (int64_t)Lw * W, W, N, Lw, Lw, lens, 1, 0, 1, 0, nullptr, emb, (int64_t)Lw * Ht, Ht, st);
        t2m_encode(h->tenc, p, w, N, Lw, emb_dev, h->geom.D, st);
        T2M_HIP(h, hipGetLastError());
        return RGN_OK;
    });
}

int rgn_t2m_length_status(rgn_t2m_handle h, int32_t* clamped) {
    using namespace rgn;
    return t2m_guard(h, "rgn_t2m_length_status", [&]() -> int {
        if (!h) return RGN_ERR_INVALID_ARG;
        if (!clamped) return h->fail(RGN_ERR_INVALID_ARG, "rgn_t2m_length_status: null argument");
        if (!h->finalized) return h->fail(RGN_ERR_STATE, "rgn_t2m_length_status: weights not finalized");
        T2M_HIP(h, hipSetDevice(h->cfg.device));
        T2M_HIP(h, hipDeviceSynchronize());
        int v = 0;
        T2M_HIP(h, hipMemcpy(&v, h->status, sizeof(int), hipMemcpyDeviceToHost));
        T2M_HIP(h, hipMemset(h->status, 0, sizeof(int)));
        *clamped = v;
        return RGN_OK;
    });
}

int rgn_t2m_match(int32_t device, const float* text_dev, const float* motion_dev, int32_t N, int32_t D, int32_t group, float* diag_dev, int32_t* rank_dev,
                  void* stream) {
    using namespace rgn;
    return t2m_guard(nullptr, "rgn_t2m_match", [&]() -> int {
        if (const char* why = t2m_match_error(text_dev, motion_dev, N, D, group, diag_dev, rank_dev)) return t2m_call_error(nullptr, "rgn_t2m_match", why);
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
            g_t2m_create_error = "rgn_t2m_match: no HIP device visible, or no such device";
            return RGN_ERR_HIP;
        }
        if (hipSetDevice(device) != hipSuccess) {
            g_t2m_create_error = "rgn_t2m_match: hipSetDevice failed";
            return RGN_ERR_HIP;
        }
        hipLaunchKernelGGL(k_match, dim3((N - 1) / group + 1), dim3(256), 0, static_cast<hipStream_t>(stream), text_dev, motion_dev, N, D, group, diag_dev, rank_dev);
        if (hipGetLastError() != hipSuccess) {
            g_t2m_create_error = "rgn_t2m_match: launch failed";
            return RGN_ERR_HIP;
        }
        return RGN_OK;
    });
}

}  // extern "C"
