// The GRU action classifier of the action2motion evaluation (eval/a2m/action2motion/models.py:6-61: MotionDiscriminator / MotionDiscriminatorForFID):
// nn.GRU(I, H, L) over the frames of N sequences, the state after each sequence's last valid frame, tanh(linear1) and linear2 - ONE launch, every workgroup
// independent (no inter-workgroup wait, no atomic).
//
// A workgroup owns GRU_TILE = 16 sequences for the whole frame loop; its 8 waves split the hidden units in tiles of 16. The gate pre-activations are
//   D[unit, sequence] = sum_k W[unit, k] act[k, sequence]          on v_mfma_f32_16x16x4_f32: exact fp32 products, a k-ordered fp32 fma chain
// with the weights as the A operand and the activations (the frame of x, or a layer's state) as B, so one lane ends up with r, z, W_in x and W_hn h of the
// same (unit, sequence) and the gate arithmetic needs no exchange. A result column depends on the B column of its own sequence alone: a sequence's rows
// are the same bits whatever else sits in the tile, and a NaN in a frame past a sequence's length never leaves its column, where the state is frozen by a
// select (never by arithmetic).
//
// Where things live. The state h [L][16][H] stays in LDS across the loop. The weights do not fit on a CU (3 x 384 x 128 floats at the reference geometry):
// they are packed at finalize in A-fragment order - per (unit tile, k granule of 16, gate) 64 lanes x 4 floats, so a wave's load of a fragment is one
// contiguous KiB - and streamed from L2 every frame, one granule ahead of the MFMAs that use it. x [N, I, T] is read as it lies: up to 8 frames at a
// time are staged into LDS transposed to [frame][sequence][I].
//
// The frame loop's critical path: per frame and layer, 3 (Kin + H) / 4 MFMAs of 32 cycles per unit tile (two waves share a SIMD's matrix pipe), the gate
// transcendentals, and two workgroup barriers (all reads of the old state | its overwrite). The loop is bound by the MFMA pipe, not by a dependent
// chain: the four accumulators of a tile (r, z, W_in x, W_hn h) are independent. The layers of one frame run one after the other.
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "../../include/regennet_hip.h"
#include "rgn_device.h"
#include "rgn_gru_cell.h"
#include "rgn_gru_check.h"

namespace rgn {
namespace {

struct GruLayerW {
    const float* wx;      // packed W_ih [H/16][kxc][3][64][4]
    const float* wh;      // packed W_hh [H/16][H/16][3][64][4]
    const float* bias;    // [4][H]: b_ir + b_hr, b_iz + b_hz, b_in, b_hn (r multiplies W_hn h + b_hn, so the n biases stay apart)
    int kxc;              // k granules of the input part
};
struct GruArgs {
    GruLayerW layer[GRU_MAX_LAYERS];
    const float *w1, *b1, *w2, *b2;       // the head, row-major as the checkpoint stores it
    const float* x;                       // [N, I, T]
    const int64_t* lengths;               // [N]
    const float* h0;                      // [L, N, H]
    float *features, *logits;             // [N, F], [N, C]; either may be null
    int* status;                          // set to 1 when a length outside [1, T] was clamped
    int N, T, I, L, F, C;
    GruLds lds;
};

// One frame of one GRU layer (PyTorch's form, gate order r, z, n) for the workgroup's 16 sequences: hl [16][H + 4] in LDS is replaced by
//   h' = (1 - z) n + z h,  r = s(W_ir x + W_hr h + b_r), z likewise, n = tanh(W_in x + b_in + r (W_hn h + b_hn))
// for the sequences with t < lens[seq]; the others keep their state bit for bit. xin [16][x_ld] in LDS is the layer's input (a staged frame of x, or the
// state of the layer below, already at this frame). Called by all 8 waves; ends behind a barrier, so hl is complete on return.
template <int H>
__device__ __forceinline__ void gru_layer_step(const GruLayerW& w, const float* xin, int x_ld, float* hl, const int* lens, int t, int lane, int wave) {
    constexpr int NT = H / 16, TPW = (NT + GRU_WAVES - 1) / GRU_WAVES, HLD = H + 4;
    const int seq = lane & 15;
    const bool live = t < lens[seq];
    f32x4 hn[TPW];
    static_for<TPW>([&](auto I) {
        constexpr int i = decltype(I)::value;
        const int u = wave + GRU_WAVES * i;
        if (u < NT) {
            const int unit0 = u * 16 + (lane >> 4) * 4;      // C/D layout: column = lane & 15, row = 4 (lane >> 4) + register
            f32x4 ar = *reinterpret_cast<const f32x4*>(w.bias + unit0), az = *reinterpret_cast<const f32x4*>(w.bias + H + unit0);
            f32x4 ain = *reinterpret_cast<const f32x4*>(w.bias + 2 * H + unit0), ahn = *reinterpret_cast<const f32x4*>(w.bias + 3 * H + unit0);
            gru_gate_kloop(w.wx + (size_t)u * w.kxc * 768, w.kxc, xin, x_ld, lane, ar, az, ain);
            gru_gate_kloop(w.wh + (size_t)u * NT * 768, NT, hl, HLD, lane, ar, az, ahn);
            const f32x4 hp = *reinterpret_cast<const f32x4*>(hl + seq * HLD + unit0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float r = gru_sigmoid(ar[j]), z = gru_sigmoid(az[j]);
                const float n = gru_tanh(ain[j] + r * ahn[j]);
                const float hv = (1.0f - z) * n + z * hp[j];
                hn[i][j] = live ? hv : hp[j];
            }
        }
    });
    __syncthreads();                                          // every wave has read the old state
    static_for<TPW>([&](auto I) {
        constexpr int i = decltype(I)::value;
        const int u = wave + GRU_WAVES * i;
        if (u < NT) *reinterpret_cast<f32x4*>(hl + seq * HLD + u * 16 + (lane >> 4) * 4) = hn[i];
    });
    __syncthreads();
}

template <int H>
__global__ __launch_bounds__(GRU_WAVES * 64) void k_gru(const GruArgs a) {
    extern __shared__ __attribute__((aligned(16))) float gru_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NTHR = GRU_WAVES * 64, HLD = H + 4;
    const int n0 = blockIdx.x * GRU_TILE, N = a.N, T = a.T, I = a.I, L = a.L;
    float* hs = gru_smem + a.lds.h_off;
    float* feat = gru_smem + a.lds.feat_off;
    int* lens = reinterpret_cast<int*>(gru_smem + a.lds.len_off);
    float* xs = gru_smem + a.lds.x_off;
    const int x_ld = a.lds.x_ld, TC = a.lds.tc;

    if (tid < GRU_TILE) {
        int len = 0;                                          // a pad sequence of the last tile: never live, never stored
        if (n0 + tid < N) {
            const int64_t v = a.lengths[n0 + tid];
            if (v < 1 || v > T) *a.status = 1;                // clamped and flagged: nothing outside x is read
            len = v < 1 ? 1 : v > T ? T : (int)v;
        }
        lens[tid] = len;
    }
    for (int idx = tid; idx < L * GRU_TILE * H; idx += NTHR) {
        const int l = idx / (GRU_TILE * H), r = idx - l * GRU_TILE * H, s = r / H, k = r - s * H;
        hs[(l * GRU_TILE + s) * HLD + k] = n0 + s < N ? a.h0[((size_t)l * N + n0 + s) * H + k] : 0.f;
    }
    for (int idx = tid; idx < TC * GRU_TILE * x_ld; idx += NTHR) xs[idx] = 0.f;     // the k pad of the staged frames stays 0
    __syncthreads();
    int tmax = 0;
#pragma unroll
    for (int s = 0; s < GRU_TILE; ++s) tmax = max(tmax, lens[s]);

    for (int t = 0; t < tmax; ++t) {
        const int tc = t % TC;
        if (tc == 0) {
            // frames t .. t + TC - 1 of the tile's sequences, frames innermost in memory -> [frame][sequence][I] (the previous chunk's readers are behind
            // the barrier that closed the last layer step)
            for (int idx = tid; idx < GRU_TILE * I * TC; idx += NTHR) {
                const int f = idx % TC, q = idx / TC, i = q % I, s = q / I;
                const int fr = t + f;
                float v = 0.f;
                if (fr < T && n0 + s < N) v = a.x[((size_t)(n0 + s) * I + i) * T + fr];
                xs[(f * GRU_TILE + s) * x_ld + i] = v;
            }
            __syncthreads();
        }
        const float* xin = xs + tc * GRU_TILE * x_ld;
        int ld = x_ld;
        for (int l = 0; l < L; ++l) {
            float* hl = hs + l * GRU_TILE * HLD;
            gru_layer_step<H>(a.layer[l], xin, ld, hl, lens, t, lane, wave);
            xin = hl;
            ld = HLD;
        }
    }

    // the head on the top layer's state, frozen since frame lengths - 1: features = tanh(linear1(out)), logits = linear2(features); fp32 fma chains in k order
    const float* htop = hs + (L - 1) * GRU_TILE * HLD;
    const int F = a.F, C = a.C;
    for (int idx = tid; idx < GRU_TILE * F; idx += NTHR) {
        const int s = idx / F, f = idx - s * F;
        float acc = a.b1[f];
        for (int k = 0; k < H; ++k) acc = fmaf(a.w1[f * H + k], htop[s * HLD + k], acc);
        const float v = gru_tanh(acc);
        feat[s * 64 + f] = v;
        if (a.features && n0 + s < N) a.features[(size_t)(n0 + s) * F + f] = v;
    }
    __syncthreads();
    if (a.logits)
        for (int idx = tid; idx < GRU_TILE * C; idx += NTHR) {
            const int s = idx / C, c = idx - s * C;
            float acc = a.b2[c];
            for (int k = 0; k < F; ++k) acc = fmaf(a.w2[c * F + k], feat[s * 64 + k], acc);
            if (n0 + s < N) a.logits[(size_t)(n0 + s) * C + c] = acc;
        }
}

template <class Fn>
bool gru_dispatch_h(int H, Fn&& f) {
    switch (H) {
        case 32: f(std::integral_constant<int, 32>{}); return true;
        case 64: f(std::integral_constant<int, 64>{}); return true;
        case 96: f(std::integral_constant<int, 96>{}); return true;
        case 128: f(std::integral_constant<int, 128>{}); return true;
        case 160: f(std::integral_constant<int, 160>{}); return true;
        case 192: f(std::integral_constant<int, 192>{}); return true;
        case 224: f(std::integral_constant<int, 224>{}); return true;
        case 256: f(std::integral_constant<int, 256>{}); return true;
    }
    return false;
}

thread_local std::string g_gru_create_error;

}  // namespace
}  // namespace rgn

struct rgn_gru_ctx {
    rgn_gru_config cfg{};
    std::string err;
    std::map<std::string, std::vector<float>> sd;
    std::map<std::string, std::vector<int64_t>> want;        // every key of the reference's state dict, with its shape
    bool finalized = false;
    std::vector<void*> allocs;
    rgn::GruArgs args{};
    int fail(int code, const std::string& m) {
        err = m;
        return code;
    }
};

namespace rgn {
namespace {

int gru_boundary_error(rgn_gru_ctx* h, const char* fn, const char* what) noexcept {
    try {
        std::string m = std::string(fn) + ": C++ exception at the boundary: " + what;
        if (h) h->err.swap(m);
        else g_gru_create_error.swap(m);
    } catch (...) {
    }
    return RGN_ERR_INTERNAL;
}
template <class F>
int gru_guard(rgn_gru_ctx* h, const char* fn, F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return gru_boundary_error(h, fn, "std::bad_alloc (host memory)");
    } catch (const std::exception& e) {
        return gru_boundary_error(h, fn, e.what());
    } catch (...) {
        return gru_boundary_error(h, fn, "unknown exception");
    }
}
int gru_hip_fail(rgn_gru_ctx* c, const char* what, hipError_t e) { return c->fail(RGN_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
#define GRU_HIP(c, call)                                                  \
    do {                                                                  \
        hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) return rgn::gru_hip_fail(c, #call, e_);     \
    } while (0)

int gru_upload(rgn_gru_ctx* c, const float** dst, const std::vector<float>& v) {
    void* p = nullptr;
    GRU_HIP(c, hipMalloc(&p, v.size() * sizeof(float)));
    c->allocs.push_back(p);
    GRU_HIP(c, hipMemcpy(p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    *dst = static_cast<const float*>(p);
    return RGN_OK;
}

std::string gru_shape_text(const std::vector<int64_t>& s) {
    std::string t = "[";
    for (size_t i = 0; i < s.size(); ++i) t += (i ? ", " : "") + std::to_string(s[i]);
    return t + "]";
}

}  // namespace
}  // namespace rgn

extern "C" {

const char* rgn_gru_last_error(rgn_gru_handle h) { return h ? h->err.c_str() : rgn::g_gru_create_error.c_str(); }

int rgn_gru_create(const rgn_gru_config* cfg, rgn_gru_handle* out) {
    using namespace rgn;
    return gru_guard(nullptr, "rgn_gru_create", [&]() -> int {
        if (!cfg || !out) {
            g_gru_create_error = "rgn_gru_create: null argument";
            return RGN_ERR_INVALID_ARG;
        }
        *out = nullptr;
        if (const char* why = gru_geometry_error(cfg->input_size, cfg->hidden_size, cfg->num_layers, cfg->lin1_size, cfg->output_size)) {
            g_gru_create_error = std::string("rgn_gru_create: ") + why;
            return RGN_ERR_UNSUPPORTED;
        }
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) {
            g_gru_create_error = "rgn_gru_create: no HIP device visible, or no such device";
            return RGN_ERR_HIP;
        }
        rgn_gru_ctx* c = new rgn_gru_ctx();
        c->cfg = *cfg;
        const int64_t H = cfg->hidden_size, F = cfg->lin1_size, C = cfg->output_size;
        for (int l = 0; l < cfg->num_layers; ++l) {
            const std::string s = "_l" + std::to_string(l);
            c->want["recurrent.weight_ih" + s] = {3 * H, l ? H : (int64_t)cfg->input_size};
            c->want["recurrent.weight_hh" + s] = {3 * H, H};
            c->want["recurrent.bias_ih" + s] = {3 * H};
            c->want["recurrent.bias_hh" + s] = {3 * H};
        }
        c->want["linear1.weight"] = {F, H};
        c->want["linear1.bias"] = {F};
        c->want["linear2.weight"] = {C, F};
        c->want["linear2.bias"] = {C};
        *out = c;
        return RGN_OK;
    });
}

int rgn_gru_destroy(rgn_gru_handle h) {
    return rgn::gru_guard(h, "rgn_gru_destroy", [&]() -> int {
        if (!h) return RGN_ERR_INVALID_ARG;
        (void)hipSetDevice(h->cfg.device);
        (void)hipDeviceSynchronize();
        for (void* p : h->allocs) (void)hipFree(p);
        delete h;
        return RGN_OK;
    });
}

int rgn_gru_load_weight(rgn_gru_handle h, const char* key, const float* host, const int64_t* shape, int32_t ndim) {
    using namespace rgn;
    return gru_guard(h, "rgn_gru_load_weight", [&]() -> int {
        if (!h) return RGN_ERR_INVALID_ARG;
        if (!key || !host || ndim < 1 || !shape) return h->fail(RGN_ERR_INVALID_ARG, "rgn_gru_load_weight: null/empty argument");
        if (h->finalized) return h->fail(RGN_ERR_STATE, "rgn_gru_load_weight: already finalized");
        auto it = h->want.find(key);
        if (it == h->want.end()) return h->fail(RGN_ERR_BAD_KEY, std::string("rgn_gru_load_weight: unexpected key '") + key + "'");
        if (h->sd.count(key)) return h->fail(RGN_ERR_BAD_KEY, std::string("rgn_gru_load_weight: key '") + key + "' loaded twice");
        const std::vector<int64_t> got(shape, shape + ndim);
        if (got != it->second)
            return h->fail(RGN_ERR_BAD_SHAPE, std::string("rgn_gru_load_weight: '") + key + "' has shape " + gru_shape_text(got) + ", expected " + gru_shape_text(it->second));
        size_t n = 1;
        for (int64_t d : got) n *= (size_t)d;
        h->sd[key].assign(host, host + n);
        return RGN_OK;
    });
}

int rgn_gru_finalize(rgn_gru_handle h) {
    using namespace rgn;
    return gru_guard(h, "rgn_gru_finalize", [&]() -> int {
        if (!h) return RGN_ERR_INVALID_ARG;
        rgn_gru_ctx* c = h;
        if (c->finalized) return c->fail(RGN_ERR_STATE, "rgn_gru_finalize: already finalized");
        std::string missing;
        for (const auto& kv : c->want)
            if (!c->sd.count(kv.first)) missing += (missing.empty() ? "" : ", ") + kv.first;
        if (!missing.empty()) return c->fail(RGN_ERR_MISSING_KEY, "rgn_gru_finalize: missing " + missing);
        GRU_HIP(c, hipSetDevice(c->cfg.device));
        const int H = c->cfg.hidden_size, I = c->cfg.input_size, L = c->cfg.num_layers;
        GruArgs& a = c->args;
        int rc;
        for (int l = 0; l < L; ++l) {
            const std::string s = "_l" + std::to_string(l);
            const int K = l ? H : I;
            a.layer[l].kxc = gru_pad_k(K) / GRU_KC;
            if ((rc = gru_upload(c, &a.layer[l].wx, gru_pack(c->sd["recurrent.weight_ih" + s].data(), H, K)))) return rc;
            if ((rc = gru_upload(c, &a.layer[l].wh, gru_pack(c->sd["recurrent.weight_hh" + s].data(), H, H)))) return rc;
            const std::vector<float>&bi = c->sd["recurrent.bias_ih" + s], &bh = c->sd["recurrent.bias_hh" + s];
            std::vector<float> b(4 * (size_t)H);
            for (int k = 0; k < H; ++k) {
                b[k] = bi[k] + bh[k];
                b[H + k] = bi[H + k] + bh[H + k];
                b[2 * H + k] = bi[2 * H + k];
                b[3 * H + k] = bh[2 * H + k];
            }
            if ((rc = gru_upload(c, &a.layer[l].bias, b))) return rc;
        }
        if ((rc = gru_upload(c, &a.w1, c->sd["linear1.weight"])) || (rc = gru_upload(c, &a.b1, c->sd["linear1.bias"])) ||
            (rc = gru_upload(c, &a.w2, c->sd["linear2.weight"])) || (rc = gru_upload(c, &a.b2, c->sd["linear2.bias"])))
            return rc;
        void* st = nullptr;
        GRU_HIP(c, hipMalloc(&st, sizeof(int)));
        c->allocs.push_back(st);
        GRU_HIP(c, hipMemset(st, 0, sizeof(int)));
        a.status = static_cast<int*>(st);
        a.I = I; a.L = L; a.F = c->cfg.lin1_size; a.C = c->cfg.output_size;
        a.lds = gru_lds_plan(I, H, L);
        hipError_t e = hipSuccess;
        gru_dispatch_h(H, [&](auto HH) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_gru<decltype(HH)::value>), hipFuncAttributeMaxDynamicSharedMemorySize, a.lds.bytes);
        });
        GRU_HIP(c, e);
        c->sd.clear();
        c->finalized = true;
        return RGN_OK;
    });
}

int rgn_gru_forward(rgn_gru_handle h, int32_t N, int32_t T, const float* x_dev, const int64_t* lengths_dev, const float* h0_dev, float* features_dev,
                    float* logits_dev, void* stream) {
    using namespace rgn;
    return gru_guard(h, "rgn_gru_forward", [&]() -> int {
        if (const char* why = gru_forward_error(N, T, x_dev, lengths_dev, h0_dev, features_dev, logits_dev)) {
            const std::string m = std::string("rgn_gru_forward: ") + why;
            if (h) h->err = m;
            else g_gru_create_error = m;
            return RGN_ERR_INVALID_ARG;
        }
        if (!h) {
            g_gru_create_error = "rgn_gru_forward: null handle";
            return RGN_ERR_INVALID_ARG;
        }
        rgn_gru_ctx* c = h;
        if (!c->finalized) return c->fail(RGN_ERR_STATE, "rgn_gru_forward: weights not finalized");
        GRU_HIP(c, hipSetDevice(c->cfg.device));
        GruArgs a = c->args;
        a.x = x_dev; a.lengths = lengths_dev; a.h0 = h0_dev; a.features = features_dev; a.logits = logits_dev;
        a.N = N; a.T = T;
        const dim3 grid((N - 1) / GRU_TILE + 1), block(GRU_WAVES * 64);
        gru_dispatch_h(c->cfg.hidden_size, [&](auto HH) {
            hipLaunchKernelGGL(k_gru<decltype(HH)::value>, grid, block, a.lds.bytes, static_cast<hipStream_t>(stream), a);
        });
        GRU_HIP(c, hipGetLastError());
        return RGN_OK;
    });
}

int rgn_gru_length_status(rgn_gru_handle h, int32_t* clamped) {
    using namespace rgn;
    return gru_guard(h, "rgn_gru_length_status", [&]() -> int {
        if (!h) return RGN_ERR_INVALID_ARG;
        if (!clamped) return h->fail(RGN_ERR_INVALID_ARG, "rgn_gru_length_status: null argument");
        if (!h->finalized) return h->fail(RGN_ERR_STATE, "rgn_gru_length_status: weights not finalized");
        GRU_HIP(h, hipSetDevice(h->cfg.device));
        GRU_HIP(h, hipDeviceSynchronize());
        int v = 0;
        GRU_HIP(h, hipMemcpy(&v, h->args.status, sizeof(int), hipMemcpyDeviceToHost));
        GRU_HIP(h, hipMemset(h->args.status, 0, sizeof(int)));
        *clamped = v;
        return RGN_OK;
    });
}

}  // extern "C"
