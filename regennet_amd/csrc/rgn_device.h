// Primitives shared by the kernel sources (every .hip under csrc/): vector types, address spaces, counted waits, DPP and shuffle
// reductions, the compile-time loop, the split-bf16 conversion, the GELU / erf forms, the 16-bit operand format of the plain phase (OpFmt), the
// XCD-affine workgroup order, the half-wave exchange and the row-tile DMA loop from the planes into an LDS image (layouts: rgn_layout.h). All of that
// is device code. One host-only section closes the file: dispatch_bools, which
// the launchers at the foot of the .hip sources use to pick a template form. Every helper has internal linkage.
// Forms whose arithmetic differs (the GELU / erf variants, the DPP and the shuffle wave sums) are kept apart and named for what they compute.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "rgn_internal.h"
#include "rgn_layout.h"

#define RGN_AS1 __attribute__((address_space(1)))   // global
#define RGN_AS3 __attribute__((address_space(3)))   // LDS

namespace rgn {
namespace {

template <class T, int N>
using vec_t = T __attribute__((ext_vector_type(N)));
typedef vec_t<float, 2> f32x2;
typedef vec_t<float, 4> f32x4;
typedef vec_t<float, 16> f32x16;
typedef vec_t<__bf16, 2> bf16x2;
typedef vec_t<__bf16, 4> bf16x4;
typedef vec_t<__bf16, 8> bf16x8;
typedef vec_t<_Float16, 2> f16x2;
typedef vec_t<_Float16, 8> f16x8;
typedef vec_t<unsigned int, 2> u32x2;
typedef vec_t<unsigned int, 4> u32x4;

// ---- counted waits: at most N vector-memory (vmcnt) / LDS, GDS, constant and message (lgkmcnt) operations of this wave still outstanding
template <int N>
__device__ __forceinline__ void wait_vmcnt() {   // (the six-bit counter saturates at 63)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N > 63 ? 63 : N) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_lgkmcnt() {
    static_assert(N >= 0 && N <= 15, "lgkmcnt is a four-bit counter");
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}

// ---- cross-lane reductions ----
// v from the lane CTRL names (DPP control word; bound_ctrl: a lane with no source reads 0)
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// sum over the 16-lane DPP row, in every lane of the row: 4 DPP adds, no cross-row traffic, no SGPR round trips
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp<0xB1>(v);     // quad_perm [1,0,3,2]: lane ^ 1
    v += dpp<0x4E>(v);     // quad_perm [2,3,0,1]: lane ^ 2
    v += dpp<0x141>(v);    // row_half_mirror: sums of 8
    v += dpp<0x140>(v);    // row_mirror: sums of 16
    return v;
}
// wave-wide sum on the VALU (DPP within rows of 16 lanes, then the four row totals through SGPRs): ~15 instructions with no LDS round trip;
// the ds_bpermute butterflies of wave_sum_shfl cost ~1.4 k cycles per row in rgn_rowgemm.hip's LayerNorm epilogue
__device__ __forceinline__ float wave_sum_dpp(float v) {
    const int b = __builtin_bit_cast(int, row16_sum(v));
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16)) +
           __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)) + __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
}
// wave-wide sum / max by a __shfl_xor butterfly (ds_bpermute): the result in every lane, summed in a different order than wave_sum_dpp
__device__ __forceinline__ float wave_sum_shfl(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max_shfl(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- compile-time loop: f(std::integral_constant<int, 0>{}) ... f(std::integral_constant<int, N - 1>{}) (for bodies too large for `#pragma unroll`
// to be honoured whose operands must live in registers, i.e. be indexed by constants)
template <int... Is, class F>
__device__ __forceinline__ void static_for_seq(std::integer_sequence<int, Is...>, F&& f) { (f(std::integral_constant<int, Is>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_seq(std::make_integer_sequence<int, N>{}, static_cast<F&&>(f)); }

// ---- split-bf16: hi = bf16(v), lo = bf16(v - hi) (round to nearest even both times: hi + lo holds ~16 significant bits of v)
__device__ __forceinline__ void split_bf16(const f32x4 v, bf16x4& hi, bf16x4& lo) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const __bf16 h = (__bf16)v[j];
        hi[j] = h;
        lo[j] = (__bf16)(v[j] - (float)h);
    }
}
__device__ __forceinline__ void split_bf16(const float (&v)[8], bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        hi[j] = (__bf16)v[j];
        lo[j] = (__bf16)(v[j] - (float)hi[j]);
    }
}
// ... and one element (row, col) into split planes of the K32-blocked layout (lo may be absent)
__device__ __forceinline__ void plane_put(const Planes& p, int row, int col, float v) {
    const size_t o = plane_off(p.rows, row, col);
    const __bf16 h = (__bf16)v;
    p.hi[o] = h;
    if (p.lo) p.lo[o] = (__bf16)(v - (float)h);
}

// ---- GELU (erf form) and erf ----
// erf via Abramowitz-Stegun 7.1.26 (|abs err| <= 1.5e-7) on fast exp / rcp: ~12 VALU instead of ~30 for erff(); far inside the fp32 noise of
// the surrounding GEMMs and of the 1e-3 tolerance. erf_as divides with __frcp_rn, erf_as_rcpf with v_rcp_f32 (1 ulp: below the fit's own 1.5e-7).
__device__ __forceinline__ float erf_as(float x) {
    const float ax = fabsf(x);
    const float t = __frcp_rn(fmaf(0.3275911f, ax, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = 1.0f - p * t * __expf(-ax * ax);
    return copysignf(e, x);
}
__device__ __forceinline__ float erf_as_rcpf(float x) {
    const float ax = fabsf(x);
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = 1.0f - p * t * __expf(-ax * ax);
    return copysignf(e, x);
}
__device__ __forceinline__ float gelu_as(float v) { return v * 0.5f * (1.0f + erf_as(v * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_as_rcpf(float v) { return v * 0.5f * (1.0f + erf_as_rcpf(v * 0.70710678118654752440f)); }

// GELU of two elements with packed fp32 FMAs and no transcendental instruction (v_exp / v_rcp issue at quarter rate; the A&S form spends
// ~40 % of k_gemm_x3's epilogue VALU time in them).
// gelu2_p13: x (0.5 + t Q(t^2)) with t = clamp(x, +-3.9) and t Q(t^2) ~ Phi(t) - 0.5: an odd degree-13 minimax polynomial on [0, 3.9] (max abs
// error 8.3e-5 in Phi with the clamp's 4.8e-5 beyond it; max abs error of the GELU < 3.3e-4 over [-8, 8]: 3.21e-4 in fp64, 3.22e-4 evaluated in fp32 (tests/test_plain_stage_cpu.py) - the
// degree-15 fit of gelu2_p15 had 8.1e-5 and 6.4e-4: the wider interval bought nothing the bf16 rounding of the result does not hide 10x over),
// the 1/sqrt 2 and the 0.5 folded into the coefficients: 11 instructions per pair
__device__ __forceinline__ f32x2 gelu2_p13(f32x2 x) {
    const f32x2 t = {__builtin_amdgcn_fmed3f(x[0], -3.9f, 3.9f), __builtin_amdgcn_fmed3f(x[1], -3.9f, 3.9f)};   // (no canonicalising v_max in front, unlike min(max()))
    const f32x2 z = t * t;
    f32x2 p = f32x2{3.214928057e-08f, 3.214928057e-08f};
    p = __builtin_elementwise_fma(p, z, f32x2{-2.075321845e-06f, -2.075321845e-06f});
    p = __builtin_elementwise_fma(p, z, f32x2{5.740237248e-05f, 5.740237248e-05f});
    p = __builtin_elementwise_fma(p, z, f32x2{-9.056383278e-04f, -9.056383278e-04f});
    p = __builtin_elementwise_fma(p, z, f32x2{9.218782187e-03f, 9.218782187e-03f});
    p = __builtin_elementwise_fma(p, z, f32x2{-6.556465477e-02f, -6.556465477e-02f});
    p = __builtin_elementwise_fma(p, z, f32x2{3.986084461e-01f, 3.986084461e-01f});
    return x * __builtin_elementwise_fma(t, p, f32x2{0.5f, 0.5f});
}
// gelu2_p15: 0.5 x (1 + erf(u)) with erf an odd degree-15 polynomial in u = clamp(x / sqrt 2, +-3.2) (weighted least-squares fit, max abs
// error 1.6e-4 -> GELU error relative to |x| < 8.7e-5 over [-8, 8]: 8.2e-5 in fp64, 8.6e-5 evaluated in fp32; 20x below the bf16 rounding of the result)
__device__ __forceinline__ f32x2 gelu2_p15(f32x2 x) {
    f32x2 u = x * 0.70710678118654752440f;
    u = __builtin_elementwise_min(__builtin_elementwise_max(u, f32x2{-3.2f, -3.2f}), f32x2{3.2f, 3.2f});
    const f32x2 z = u * u;
    f32x2 p = f32x2{-2.6911866e-07f, -2.6911866e-07f};
    p = __builtin_elementwise_fma(p, z, f32x2{1.2661994e-05f, 1.2661994e-05f});
    p = __builtin_elementwise_fma(p, z, f32x2{-2.5566161e-04f, -2.5566161e-04f});
    p = __builtin_elementwise_fma(p, z, f32x2{2.9286479e-03f, 2.9286479e-03f});
    p = __builtin_elementwise_fma(p, z, f32x2{-2.1317327e-02f, -2.1317327e-02f});
    p = __builtin_elementwise_fma(p, z, f32x2{1.0528564e-01f, 1.0528564e-01f});
    p = __builtin_elementwise_fma(p, z, f32x2{-3.7135834e-01f, -3.7135834e-01f});
    p = __builtin_elementwise_fma(p, z, f32x2{1.1274883e+00f, 1.1274883e+00f});
    const f32x2 hx = x * 0.5f;
    return __builtin_elementwise_fma(hx, p * u, hx);   // 0.5 x (1 + erf)
}

// ---- the 16-bit operand format of the plain phase's MFMAs (weights, activation images / planes, q / k / v / p): bf16 (8 mantissa bits) or IEEE fp16
// (11). Both instructions are 8 passes of 4 cycles per 32 x 32 x 16 tile and take 16 bytes per lane and operand, so a kernel's structure - rings,
// images, waits - does not depend on the format; what changes is every operand's rounding (2^-9 -> 2^-12 relative) and its range (fp16: 6.1e-5 ..
// 65504 normal; LayerNorm outputs, GELU values, softmax probabilities and the weights of a transformer sit well inside, and rgn_finalize_weights
// refuses a checkpoint that does not). Accumulation, LayerNorm statistics, softmax and the sampler update are fp32 either way. Nominally the same
// rate - but the chip is power-managed under a matrix load and a pure f16 MFMA loop sustains 7.5 - 8 % less than the bf16 one
// (tools/experiments/mfma_sustained.hip), which is why fp16 is a PHASE of the precision schedule (rgn_set_f16_steps), not its plain format.
template <bool F16> struct OpFmt;
template <> struct OpFmt<false> {
    typedef __bf16 t;
    typedef __bf16 v8 __attribute__((ext_vector_type(8)));
    typedef __bf16 v4 __attribute__((ext_vector_type(4)));
    typedef float acc16 __attribute__((ext_vector_type(16)));
    static __device__ __forceinline__ acc16 mfma(v8 a, v8 b, acc16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct OpFmt<true> {
    typedef _Float16 t;
    typedef _Float16 v8 __attribute__((ext_vector_type(8)));
    typedef _Float16 v4 __attribute__((ext_vector_type(4)));
    typedef float acc16 __attribute__((ext_vector_type(16)));
    static __device__ __forceinline__ acc16 mfma(v8 a, v8 b, acc16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

// ---- XCD-affine workgroup order: the hardware places workgroup id b on XCD b % 8. Remapping the id so that every XCD gets one
// CONTIGUOUS range of tiles / samples makes the rows a kernel reads the rows the previous kernel of the chain wrote on the
// same XCD (k_qkv_attn -> k_mlp -> k_qkv_attn ...): they are still in that XCD's L2 instead of behind the fabric.
__device__ __forceinline__ int xcd_affine(int bid, int nwg) {
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

// ---- the other half-wave's value (lane ^ 32): v_permlane32_swap_b32 a, b gives a' = [a.lo | b.lo], b' = [a.hi | b.hi], so with b a copy of a in a
// register of its own b' and a' are the two halves' values in every lane - one VALU instruction where __shfl_xor(v, 32) is a ds_bpermute round trip.
// (inline asm: the builtin's second result is miscompiled by ROCm 7.2's clang, it adds a' to itself; tools/permlane_check.hip)
__device__ __forceinline__ void half_swap(float& a, float& b) { asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ float half_max(float v) {
    float o = v;
    asm volatile("" : "+v"(o));
    half_swap(v, o);
    return fmaxf(v, o);
}
__device__ __forceinline__ float half_sum(float v) {
    float o = v;
    asm volatile("" : "+v"(o));
    half_swap(v, o);
    return v + o;
}

// ---- plane -> LDS image (rgn_layout.h) of a tile of 64 rows x 32 NKB columns by DMA (global_load_lds, 16 bytes per lane), issued by a workgroup of NW
// waves: 4 NKB pieces of 1 KiB (16 rows x 64 B of a k-block), wave w issues the pieces w, w + NW, ... Tile row r is plane row row0 + r; `live` rows of
// the tile exist (the rows of a sample, or what is left of M): a row past the last live one replicates it (row-local everywhere, never stored).
// AUX: the loads' cache policy. Completion is the caller's vmcnt wait
template <int AUX = 0, int NKB = 16, int NW = 8, class T>
__device__ __forceinline__ void tile_dma_in(char* img, const T* plane, int rows, size_t row0, int live, int lane, int wave) {
    const int r16 = lane >> 2, c = lane & 3;
#pragma unroll
    for (int j = 0; j < 4 * NKB / NW; ++j) {
        const int p = wave + NW * j, kb = p >> 2, r = (p & 3) * 16 + r16;
        const int rr = r < live ? r : live - 1;
        const size_t src = plane_chunk(rows, row0 + rr, kb, img_dma_chunk(r, c));
        __builtin_amdgcn_global_load_lds((const RGN_AS1 void*)(plane + src), (RGN_AS3 void*)(img + p * 1024), 16, 0, AUX);
    }
}

// ---- rotation_6d_to_matrix (utils/rotation_conversions.py:513-534): Gram-Schmidt of the two 3-vectors a1, a2, F.normalize semantics
// (v / max(||v||, 1e-12)); m[0..8] = the matrix, row-major (global memory or a local array). The one definition k_rot6d (rgn_kernels.hip) and
// k_fk (rgn_fk.hip) share, so the two agree bit for bit.
__device__ __forceinline__ void rot6d_to_matrix(float a1x, float a1y, float a1z, float a2x, float a2y, float a2z, float* m) {
    float n1 = fmaxf(sqrtf(a1x * a1x + a1y * a1y + a1z * a1z), 1e-12f);
    const float b1x = a1x / n1, b1y = a1y / n1, b1z = a1z / n1;
    const float dot = b1x * a2x + b1y * a2y + b1z * a2z;
    float b2x = a2x - dot * b1x, b2y = a2y - dot * b1y, b2z = a2z - dot * b1z;
    const float n2 = fmaxf(sqrtf(b2x * b2x + b2y * b2y + b2z * b2z), 1e-12f);
    b2x /= n2; b2y /= n2; b2z /= n2;
    m[0] = b1x; m[1] = b1y; m[2] = b1z;
    m[3] = b2x; m[4] = b2y; m[5] = b2z;
    m[6] = b1y * b2z - b1z * b2y;
    m[7] = b1z * b2x - b1x * b2z;
    m[8] = b1x * b2y - b1y * b2x;
}

// =================================================== HOST ONLY ===================================================
// ---- run-time flags -> template arguments, for launch_* / configure_*. dispatch_bools(f, a, b, ...) returns f(std::bool_constant<a>{}, std::bool_constant<b>{}, ...):
// a launcher and its configure_* name a kernel's forms once, as k<decltype(A)::value, ...> inside f, instead of an if ladder each
template <class F>
auto dispatch_bools(F&& f) { return f(); }
template <class F, class... Rest>
auto dispatch_bools(F&& f, bool b, Rest... rest) {
    auto bind = [&](auto B) { return dispatch_bools([&](auto... bs) { return f(B, bs...); }, rest...); };
    return b ? bind(std::true_type{}) : bind(std::false_type{});
}

}  // namespace
}  // namespace rgn
