// The sampler step (p_sample / ddim_sample, gaussian_diffusion.py:265-276, 319-323, 419-423, 508-560, 785-793), written ONCE for the three kernels
// that run it: k_update (rgn_kernels.hip), k_step (rgn_step.hip) and the step boundary of k_layers<true> (rgn_layers.hip). Each kernel keeps its
// loops, layouts, prefetch batching, LDS images and barriers; what an element's next state IS comes from here:
//
//   x0   = guide(c, u, scale)                        classifier-free guidance                              cfg_sampler.py:31
//   x0   = pred_x0<INPAINT>(x0, mask, target, clip)  in-painting select, then the clamp                    gaussian_diffusion.py:319-323
//   eps  = step_eps(...) | quad_or_step_eps(...)     the noise tape's entry, or the Philox draw            gaussian_diffusion.py:544-557
//   x'   = sampler_next(k, sampler, x0, x, eps)      DDPM / DDIM                                           gaussian_diffusion.py:265-276,559 | 419-423,785-793
//   step_ticket(...)                                 the last workgroup of a step moves the device-side loop index on
//
// and the Philox4x32-10 + Box-Muller stream itself, shared with k_randn. Device code only; every helper has internal linkage.
#pragma once
#include "rgn_internal.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#ifndef RGN_PHILOX_ROUNDS
#define RGN_PHILOX_ROUNDS 10
#endif

namespace rgn {
namespace {

// ---- Philox4x32-10 + Box-Muller: counter = (element/4, loop index, sample lo, sample hi), key = seed
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < RGN_PHILOX_ROUNDS; ++r) {
        // one 32 x 32 -> 64 multiply (v_mad_u64_u32) per product instead of a v_mul_hi + v_mul_lo pair: the integer multiplies are
        // quarter-rate instructions and were most of the draw's cost
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// Box-Muller on the hardware transcendentals: -2 ln u1 = -2 ln 2 * v_log_f32(u1) (log2), v_sqrt_f32, and v_sin_f32 / v_cos_f32, which
// take their argument in REVOLUTIONS (sin(2 pi u2) = v_sin_f32(u2)): 6 instructions per pair of normals instead of the ~80 of
// logf / sqrtf / sincospif (the draw is ~10 us of the 47 us step boundary at B = 256: 5.2 M normals per step). ~1 ulp transforms of
// uniform 24-bit inputs; one definition for every kernel that draws, so all of them see one stream.
__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& n0, float& n1) {
    const float u1 = ((ra >> 8) + 1u) * 5.9604644775390625e-08f;   // (0,1]
    const float u2 = (rb >> 8) * 5.9604644775390625e-08f;          // [0,1)
    const float rad = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));
    n0 = rad * __builtin_amdgcn_cosf(u2);
    n1 = rad * __builtin_amdgcn_sinf(u2);
}
__device__ __forceinline__ float philox_normal(unsigned long long seed, unsigned long long sample, uint32_t stream,
                                               uint32_t elem) {
    uint32_t r[4];
    philox4x32_10(elem >> 2, stream, (uint32_t)sample, (uint32_t)(sample >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const int pair = (elem >> 1) & 1;
    float n0, n1;
    box_muller(r[2 * pair], r[2 * pair + 1], n0, n1);
    return (elem & 1) ? n1 : n0;
}
// The element counter is (feature * 4096 + frame), not the flat index: the draw for (sample, step, feature, frame) does
// not depend on the sequence length, so a run truncated to the first frames (auto_regressive evaluation: frame f only
// needs tokens 0..f of a causal decoder) sees the same noise as the full-length run.
__device__ __forceinline__ uint32_t noise_elem(int f, int t) { return (uint32_t)(f * 4096 + t); }

// ---- classifier-free guidance: x0 = x0_u + scale_b (x0_c - x0_u), cfg_sampler.py:31.
// Here and below products and sums are rounded separately (no FMA contraction) to follow the reference's op order.
__device__ __forceinline__ float guide(float c, float u, float scale) { return __fadd_rn(u, __fmul_rn(scale, __fsub_rn(c, u))); }

// ---- pred_xstart: the in-painting select (rgn_set_inpainting; gaussian_diffusion.py:319-323: x0 = mask ? motion : x0) sits between the
// guidance combination and the clamp, so a target outside [-1, 1] is clamped like a prediction
template <bool INPAINT>
__device__ __forceinline__ float pred_x0(float x0, unsigned char mask_byte, float target, int clip) {
    if constexpr (INPAINT) x0 = mask_byte ? target : x0;
    if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    return x0;
}

// ---- the step's noise for element (feature f, frame t) of motion b at loop index `step`. Whose draw a motion takes is bn = noise_motion(sp, b),
// wave-uniform in every kernel and so formed once by the caller: const_noise gives every motion the draw of motion 0 (gaussian_diffusion.py:546-547)
__device__ __forceinline__ int noise_motion(const SampleParams& sp, int b) { return sp.const_noise ? 0 : b; }
__device__ __forceinline__ float tape_eps(const SampleParams& sp, int step, int B, size_t FT, int bn, int f, int T, int t) {
    return sp.noise[(size_t)(sp.first_index - step) * B * FT + (size_t)bn * FT + (size_t)f * T + t];   // tape entry 0 belongs to first_index
}
__device__ __forceinline__ float step_eps(const SampleParams& sp, int step, int B, size_t FT, int bn, int f, int T, int t) {
    if (sp.noise) return tape_eps(sp, step, B, FT, bn, f, T, t);
    return philox_normal(sp.seed, sp.sample_offset + bn, (uint32_t)step, noise_elem(f, t));
}
// ... for the kernels that may hold the element's Philox draw already (quads: eps_quad comes from quad_normals below). The tape is tested first
// and the draw second, in that order: k_layers<true> sits at its 256 VGPRs, and `quads ? eps_quad : step_eps(...)` at the call site costs it
// up to 11 more spilled SGPRs per form
__device__ __forceinline__ float quad_or_step_eps(bool quads, float eps_quad, const SampleParams& sp, int step, int B, size_t FT, int bn, int f, int T,
                                                  int t) {
    if (sp.noise) return tape_eps(sp, step, B, FT, bn, f, T, t);
    if (!quads) return philox_normal(sp.seed, sp.sample_offset + bn, (uint32_t)step, noise_elem(f, t));
    return eps_quad;
}
// ... and the same draw for a whole quad of lanes at once. One Philox4x32-10 call yields the four normals of frames 4j .. 4j+3 of a (sample,
// step, feature): where the lanes of a quad hold exactly such a run (first frame tq, tq % 4 == 0), lane q draws feature 4 fg + q for the
// quad's four frames and the quad transposes - a quarter of the Philox rounds and half of the Box-Muller work of step_eps, bit-identical values.
// eps4[j] = this lane's (frame tq + q) normal of feature 4 fg + j.
__device__ __forceinline__ void quad_normals(const SampleParams& sp, int step, int bn, int fg, int q, int tq, float (&eps4)[4]) {
    const uint32_t elem = noise_elem(4 * fg + q, tq);
    const unsigned long long sample = sp.sample_offset + bn;
    uint32_t r[4];
    philox4x32_10(elem >> 2, (uint32_t)step, (uint32_t)sample, (uint32_t)(sample >> 32), (uint32_t)sp.seed, (uint32_t)(sp.seed >> 32), r);
#pragma unroll
    for (int pair = 0; pair < 2; ++pair) box_muller(r[2 * pair], r[2 * pair + 1], eps4[2 * pair], eps4[2 * pair + 1]);
    // 4 x 4 transpose inside the quad (this lane needs, for feature 4 fg + j, element q of lane j's four): two butterfly stages of a
    // conditional swap with the lane q ^ 1, then q ^ 2 (DPP quad_perm): 16 operations where a broadcast-and-select of every element takes 32
    auto stage = [&](float& lo_r, float& hi_r, bool bit, auto ctrl) {
        const float send = bit ? lo_r : hi_r;
        const float recv = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, send), decltype(ctrl)::value, 0xf, 0xf, true));
        lo_r = bit ? recv : lo_r;
        hi_r = bit ? hi_r : recv;
    };
    const bool b0 = (q & 1) != 0, b1 = (q & 2) != 0;
    stage(eps4[0], eps4[1], b0, std::integral_constant<int, 0xB1>{});   // quad_perm [1, 0, 3, 2]
    stage(eps4[2], eps4[3], b0, std::integral_constant<int, 0xB1>{});
    stage(eps4[0], eps4[2], b1, std::integral_constant<int, 0x4E>{});   // quad_perm [2, 3, 0, 1]
    stage(eps4[1], eps4[3], b1, std::integral_constant<int, 0x4E>{});
}

// ---- the update itself
//   DDPM  x' = (c1*x0 + c2*x) + sig*eps                          gaussian_diffusion.py:265-276,559
//   DDIM  e = (sr*x - x0)/srm1 ; x' = (x0*ca + cb*e) + sig*eps   gaussian_diffusion.py:419-423,785-793
__device__ __forceinline__ float sampler_next(const StepCoef& k, int sampler, float x0, float x, float eps) {
    if (sampler == 0) {
        const float mean = __fadd_rn(__fmul_rn(k.c1, x0), __fmul_rn(k.c2, x));
        return __fadd_rn(mean, __fmul_rn(k.sig_ddpm, eps));
    }
    const float e = __fdiv_rn(__fsub_rn(__fmul_rn(k.sr, x), x0), k.srm1);
    const float mean = __fadd_rn(__fmul_rn(x0, k.ca), __fmul_rn(k.cb, e));
    return __fadd_rn(mean, __fmul_rn(k.sig_ddim, eps));
}

// ---- in-painting operands through buffer loads: ONE descriptor per array over the `n` elements from element `first` of the bound mask / motion
// ([B,F,T], the layout of x), the lane's element as the vector offset, the feature row as a wave-uniform scalar offset - flat addresses for the
// 88 features of a lane cost ~330 spilled SGPRs. The descriptors are sized by the pointer (wave-uniform: nothing bound, zero records, every load
// returns 0 untouched by memory) and bound what a surplus row or a padding feature may touch; the callers never use those values.
struct InpaintRsrc { __amdgpu_buffer_rsrc_t mask, motion; };
__device__ __forceinline__ InpaintRsrc inpaint_rsrc(const SampleParams& sp, size_t first, size_t n) {
    const unsigned nrec = sp.inpaint_mask ? (unsigned)n : 0u;
    return {__builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(sp.inpaint_mask) + first, 0, (int)nrec, 0x00020000),
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(sp.inpaint_motion) + first, 0, (int)(nrec * 4u), 0x00020000)};
}
__device__ __forceinline__ void inpaint_load(const InpaintRsrc& rs, int lane_elem, int row_elem, unsigned char& mask_byte, float& target) {
    mask_byte = __builtin_amdgcn_raw_buffer_load_b8(rs.mask, lane_elem, row_elem, 0);
    target = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs.motion, lane_elem * 4, row_elem * 4, 0));
}

// ---- the ticket that moves the device-side loop index on: the last of `total` arrivals at *tick resets the counter for the next step and
// writes `next`. One thread per workgroup calls it, after the workgroup's last read of *d_step; every other reader of *d_step precedes the
// step's boundary kernels in stream order. (One address takes ~88 atomics per us: 5632 arrivals on one counter cost 60 us - k_update, with a
// block per 32 x 32 tile, counts per sample first.)
__device__ __forceinline__ void step_ticket(int* tick, int total, int* d_step, int next) {
    if (atomicAdd(tick, 1) == total - 1) {
        tick[0] = 0;
        d_step[0] = next;
    }
}

}  // namespace
}  // namespace rgn
