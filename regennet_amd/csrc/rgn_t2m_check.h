// The geometry and argument rules of the text-to-motion evaluator (rgn_t2m_*) as pure host code: what the kernels of rgn_t2m.hip accept, decided before
// the device is touched, and the workspace plan both entry points share. Included by rgn_t2m.hip and by tools/t2m_args_check.cpp (a stand-alone program
// built with the host sanitizers), so the rules have one definition. No HIP in here.
//
// What a movement frame reads. T1 = T / 2 frames leave the first convolution (k 4, s 2, p 1), T2 = T1 / 2 the second. Movement frame j reads first-layer
// frames 2j-1 .. 2j+2 and those read input frames 4j-3 .. 4j+6, each convolution padding with zeros at ITS OWN ends (frame -1 and frame T1 of the first
// layer's output are zeros, not convolutions of padding). A sequence of L4 = m_lens / unit_length movement frames therefore looks at input frames
// 0 .. min(T, 4 L4 + 3) - 1 - up to three past 4 L4, exactly as the reference does - and at first-layer frames 0 .. min(T1, 2 L4 + 1) - 1. Nothing
// behind those counts is read.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rgn {

constexpr int T2M_TILE = 16;          // rows (sequence frames) or sequences per workgroup: the column count of the 16x16x4 fp32 MFMA
constexpr int T2M_WAVES = 8;
constexpr int T2M_KC = 16;            // k granule of the packed weights
constexpr int T2M_UG = 64;            // output units a wave carries at once (four 16-unit tiles share one activation fragment)
constexpr int T2M_MAX_T = 4096;
constexpr int T2M_MAX_LW = 256;
constexpr int T2M_MAX_GROUP = 32;
constexpr int T2M_LDS_LIMIT = 160 * 1024;

inline int t2m_pad(int v, int q) { return (v + q - 1) / q * q; }
inline int t2m_t1(int T) { return (T - 2) / 2 + 1; }
inline int t2m_t2(int T) { return (t2m_t1(T) - 2) / 2 + 1; }

inline bool t2m_hidden_ok(int h) { return h >= 64 && h <= 1024 && h % 64 == 0; }

// nullptr when the geometry is served; otherwise the reason
inline const char* t2m_geometry_error(int dim_pose, int movement_hidden, int movement_latent, int motion_hidden, int dim_word, int dim_pos_ohot,
                                      int text_hidden, int coemb, int unit_length) {
    if (dim_pose < 5 || dim_pose > 1024) return "dim_pose must be in [5, 1024]";
    if (!t2m_hidden_ok(movement_hidden)) return "movement_hidden must be a multiple of 64 in [64, 1024]";
    if (!t2m_hidden_ok(movement_latent)) return "movement_latent must be a multiple of 64 in [64, 1024]";
    if (!t2m_hidden_ok(motion_hidden)) return "motion_hidden must be a multiple of 64 in [64, 1024]";
    if (!t2m_hidden_ok(text_hidden)) return "text_hidden must be a multiple of 64 in [64, 1024]";
    if (dim_word < 4 || dim_word > 1024 || dim_word % 4) return "dim_word must be a multiple of 4 in [4, 1024]";
    if (dim_pos_ohot < 1 || dim_pos_ohot > 1024) return "dim_pos_ohot must be in [1, 1024]";
    if (coemb < 4 || coemb > 1024 || coemb % 4) return "coemb must be a multiple of 4 in [4, 1024]";
    if (unit_length != 4) return "unit_length must be 4 (two stride-2 convolutions)";
    return nullptr;
}

// LDS bytes of one workgroup of the row GEMM: the window of (TILE - 1) stride + taps frames of `channels` (padded to the k granule, + 4 against bank
// conflicts)
inline int t2m_rows_lds_bytes(int channels, int taps, int stride) {
    return ((T2M_TILE - 1) * stride + taps) * (t2m_pad(channels, T2M_KC) + 4) * 4;
}
static_assert(((T2M_TILE - 1) * 2 + 4) * (1024 + 4) * 4 <= T2M_LDS_LIMIT, "the widest convolution window must fit");
static_assert(T2M_TILE * (2048 + 4) * 4 <= T2M_LDS_LIMIT, "the head's 2 H rows must fit");
// LDS bytes of one workgroup of the recurrence: two copies of the state of 16 sequences (a step reads one and writes the other), and their lengths
inline int t2m_bigru_lds_bytes(int hidden) { return (2 * T2M_TILE * (hidden + 4) + T2M_TILE) * 4; }
static_assert((2 * T2M_TILE * (1024 + 4) + T2M_TILE) * 4 <= T2M_LDS_LIMIT, "the recurrence's two state copies must fit");

inline const char* t2m_shape_error(int64_t N, int64_t T, int64_t Lw) {
    if (N < 1) return "N < 1";
    if (N > (1 << 19)) return "N above 2^19";
    if (T < 4 || T > T2M_MAX_T) return "T outside [4, 4096]";
    if (Lw < 1 || Lw > T2M_MAX_LW) return "Lw outside [1, 256]";
    return nullptr;
}

struct T2mGeom {
    int dim_pose, Hm, Dm, H, W, P, Ht, D;
};

// The workspace of one call, in bytes: offsets of each stage's buffer (all multiples of 16 bytes). One plan serves the motion and the text side; the
// query returns the larger total, so a buffer of rgn_t2m_workspace(N, T, Lw) bytes serves either call at up to that N, T, Lw.
struct T2mPlan {
    size_t lens, a, b, c, emb, gi, hcat, y1, y2, total;
};
inline size_t t2m_align(size_t v) { return (v + 15) / 16 * 16; }
inline T2mPlan t2m_motion_plan(const T2mGeom& g, int64_t N, int64_t T) {
    const size_t n = (size_t)N, T1 = (size_t)t2m_t1((int)T), T2 = (size_t)t2m_t2((int)T);
    T2mPlan p{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += t2m_align(bytes); return at; };
    p.lens = take(n * 4);
    p.a = take(n * T1 * g.Hm * 4);        // first convolution
    p.b = take(n * T2 * g.Dm * 4);        // second convolution
    p.c = take(n * T2 * g.Dm * 4);        // movements
    p.emb = take(n * T2 * g.H * 4);       // input_emb
    p.gi = take(n * T2 * 6 * g.H * 4);    // gate inputs [N, T2, 2, 3 H]
    p.hcat = take(n * 2 * g.H * 4);
    p.y1 = take(n * g.H * 4);
    p.y2 = take(n * g.H * 4);
    p.total = o;
    return p;
}
inline T2mPlan t2m_text_plan(const T2mGeom& g, int64_t N, int64_t Lw) {
    const size_t n = (size_t)N, L = (size_t)Lw;
    T2mPlan p{};
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += t2m_align(bytes); return at; };
    p.lens = take(n * 4);
    p.a = take(n * L * g.W * 4);          // word_embs + pos_emb(pos_ohot)
    p.b = p.c = 0;
    p.emb = take(n * L * g.Ht * 4);
    p.gi = take(n * L * 6 * g.Ht * 4);
    p.hcat = take(n * 2 * g.Ht * 4);
    p.y1 = take(n * g.Ht * 4);
    p.y2 = take(n * g.Ht * 4);
    p.total = o;
    return p;
}
inline size_t t2m_workspace_bytes(const T2mGeom& g, int64_t N, int64_t T, int64_t Lw) {
    const size_t m = t2m_motion_plan(g, N, T).total, t = t2m_text_plan(g, N, Lw).total;
    return m > t ? m : t;
}

// lens_optional: rgn_t2m_movements takes a null m_lens (every frame)
inline const char* t2m_motion_error(int64_t N, int64_t T, const void* motions, const void* m_lens, const void* out, const void* work, size_t work_bytes,
                                    size_t need, bool lens_optional = false) {
    if (const char* why = t2m_shape_error(N, T, 1)) return why;
    if (!motions || (!m_lens && !lens_optional) || !out) return "null motions / m_lens / output";
    if (!work) return "null workspace";
    if (work_bytes < need) return "workspace smaller than rgn_t2m_workspace asks for";
    return nullptr;
}
inline const char* t2m_text_error(int64_t N, int64_t Lw, const void* word_embs, const void* pos_ohot, const void* cap_lens, const void* out, const void* work,
                                  size_t work_bytes, size_t need) {
    if (const char* why = t2m_shape_error(N, 4, Lw)) return why;
    if (!word_embs || !pos_ohot || !cap_lens || !out) return "null word_embs / pos_ohot / cap_lens / output";
    if (!work) return "null workspace";
    if (work_bytes < need) return "workspace smaller than rgn_t2m_workspace asks for";
    return nullptr;
}
inline const char* t2m_match_error(const void* text, const void* motion, int64_t N, int64_t D, int64_t group, const void* diag, const void* rank) {
    if (!text || !motion || !diag || !rank) return "null text / motion / diag / rank";
    if (N < 1) return "N < 1";
    if (N > (1 << 24)) return "N above 2^24";
    if (D < 4 || D > 1024 || D % 4) return "D must be a multiple of 4 in [4, 1024]";
    if (group < 1 || group > T2M_MAX_GROUP) return "group outside [1, 32]";
    return nullptr;
}

}  // namespace rgn
