// The likelihood evaluation of GaussianDiffusion.calc_bpd_loop (diffusion/gaussian_diffusion.py:1546-1601) for MANY (timestep, motion) rows at once.
// The reference walks the S timesteps of a motion one after the other; they do not depend on one another, so here they are the rows of larger
// evaluations: row r = (timestep index, motion b = r % B), with its own loop index and its own schedule coefficients.
//
//   k_q_sample_rows   x_t[r] = a_r * x_start[b] + s_r * noise_r (q_sample, :245-263): two separately rounded fp32 products and one add, the
//                     bits of the torch expression. noise_r is read, or drawn from the Philox stream of rgn_sampler.h exactly as k_randn draws
//                     rgn_randn_step(seed, sample_offset + b, loop_index = t_r): (seed; sample_offset + b, t_r, feature * 4096 + frame).
//   k_vb_terms        per row (vb, xstart_mse, mse):
//                       vb, t != 0   mean(normal_kl(mean_q, lv_q, mean_m, lv_m)) / ln 2       losses.py:12-39, :265-276, :386, :1217-1226
//                       vb, t == 0   mean(-discretized_gaussian_log_likelihood(x0, mean_m, 0.5 lv_m)) / ln 2      losses.py:42-77, :1228-1232
//                       xstart_mse   mean((p - x0)^2)                                         :1585
//                       mse          mean((eps - noise)^2), eps = (sr x_t - p) / srm1         :419-423, :1586-1587
//                     with mean_q = c1 x0 + c2 x_t, mean_m = c1 p + c2 x_t and p the model's output, clamped to [-1, 1] under RGN_VB_CLIP.
//
// Arithmetic of k_vb_terms: the convention of rgn_loss.hip - fp64 from the fp32 inputs and the fp32 coefficients, every output rounded to fp32
// once. ONE WORKGROUP PER ROW: thread i takes elements i, i + 256, ... in order, the threads are combined by a butterfly inside each wave and the
// four waves in index order. No atomics; a row's numbers depend on that row alone and are the same on every run.
#include "rgn_sampler.h"

#include "../../include/regennet_hip.h"

namespace rgn {

constexpr int VB_THREADS = 256;

__global__ __launch_bounds__(VB_THREADS) void k_q_sample_rows(const float* __restrict__ x_start, const float* __restrict__ noise_in,
                                                              const float* __restrict__ coef, const int* __restrict__ t_idx, float* __restrict__ x_t,
                                                              float* __restrict__ noise_out, int B, int n, int T, int chunks,
                                                              unsigned long long seed, unsigned long long sample_offset) {
    // a flat grid of N x chunks workgroups, a row's chunks side by side: no limit on the rows of a call but the grid's 2^31 - 1
    const int r = blockIdx.x / chunks, b = r % B;
    const int e = (blockIdx.x % chunks) * VB_THREADS + threadIdx.x;
    if (e >= n) return;
    const size_t at = (size_t)r * n + e;
    const float a = coef[2 * r], s = coef[2 * r + 1];
    const float nz = noise_in ? noise_in[at] : philox_normal(seed, sample_offset + (unsigned long long)b, (uint32_t)t_idx[r], noise_elem(e / T, e % T));
    if (noise_out) noise_out[at] = nz;
    x_t[at] = __fadd_rn(__fmul_rn(a, x_start[(size_t)b * n + e]), __fmul_rn(s, nz));
}

__device__ __forceinline__ double vb_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// approx_standard_normal_cdf (losses.py:42-47)
__device__ __forceinline__ double vb_cdf(double x) { return 0.5 * (1.0 + tanh(0.7978845608028654 /* sqrt(2 / pi) */ * (x + 0.044715 * (x * x * x)))); }

__global__ __launch_bounds__(VB_THREADS) void k_vb_terms(const float* __restrict__ x_start, const float* __restrict__ x_t,
                                                         const float* __restrict__ output, const float* __restrict__ noise,
                                                         const int* __restrict__ t_idx, const float* __restrict__ coef, float* __restrict__ terms, int B,
                                                         int n, int flags) {
    __shared__ double red[VB_THREADS / 64][3];
    const int r = blockIdx.x, b = r % B;
    const float* x0r = x_start + (size_t)b * n;
    const float* xtr = x_t + (size_t)r * n;
    const float* pr = output + (size_t)r * n;
    const float* nr = noise ? noise + (size_t)r * n : nullptr;
    const double c1 = coef[6 * r], c2 = coef[6 * r + 1], lv_q = coef[6 * r + 2], lv_m = coef[6 * r + 3], sr = coef[6 * r + 4], srm1 = coef[6 * r + 5];
    const bool first = t_idx[r] == 0;
    const bool clip = flags & RGN_VB_CLIP;
    // what every element of the row shares: the variance part of the KL, or the decoder's inverse scale
    const double kl_var = -1.0 + lv_m - lv_q + exp(lv_q - lv_m), inv_var_m = exp(-lv_m), inv_stdv = exp(-(0.5 * lv_m));

    double s_vb = 0.0, s_x0 = 0.0, s_eps = 0.0;
    for (int e = threadIdx.x; e < n; e += VB_THREADS) {
        const double x0 = x0r[e], xt = xtr[e];
        double p = pr[e];
        if (clip) p = fmin(fmax(p, -1.0), 1.0);
        const double mean_m = c1 * p + c2 * xt;
        if (!first) {
            const double mean_q = c1 * x0 + c2 * xt, d = mean_q - mean_m;
            s_vb += 0.5 * (kl_var + d * d * inv_var_m);
        } else {
            const double centered = x0 - mean_m;
            const double cdf_plus = vb_cdf(inv_stdv * (centered + 1.0 / 255.0)), cdf_min = vb_cdf(inv_stdv * (centered - 1.0 / 255.0));
            const double lp = x0 < -0.999 ? log(fmax(cdf_plus, 1e-12)) : x0 > 0.999 ? log(fmax(1.0 - cdf_min, 1e-12)) : log(fmax(cdf_plus - cdf_min, 1e-12));
            s_vb -= lp;
        }
        const double dx = p - x0;
        s_x0 += dx * dx;
        if (nr) {
            const double de = (sr * xt - p) / srm1 - (double)nr[e];
            s_eps += de * de;
        }
    }
    const int wave = threadIdx.x >> 6;
    s_vb = vb_wave_sum(s_vb);
    s_x0 = vb_wave_sum(s_x0);
    s_eps = vb_wave_sum(s_eps);
    if ((threadIdx.x & 63) == 0) {
        red[wave][0] = s_vb;
        red[wave][1] = s_x0;
        red[wave][2] = s_eps;
    }
    __syncthreads();
    if (threadIdx.x < RGN_VB_NTERMS) {
        const int k = threadIdx.x;
        double v = 0.0;
        for (int w = 0; w < VB_THREADS / 64; ++w) v += red[w][k];
        v /= (double)n;
        if (k == RGN_VB_VB) v /= 0.6931471805599453 /* ln 2 */;
        terms[(size_t)r * RGN_VB_NTERMS + k] = (float)v;
    }
}

int q_sample_chunks(int n) { return (int)(((long long)n + VB_THREADS - 1) / VB_THREADS); }

hipError_t launch_q_sample_rows(const float* x_start, const float* noise_in, const float* coef, const int* t_idx, float* x_t, float* noise_out, int B,
                                int N, int n, int T, unsigned long long seed, unsigned long long sample_offset, hipStream_t s) {
    if (N <= 0 || n <= 0) return hipSuccess;
    const int chunks = q_sample_chunks(n);
    hipLaunchKernelGGL(k_q_sample_rows, dim3((unsigned)((long long)N * chunks)), dim3(VB_THREADS), 0, s, x_start, noise_in, coef, t_idx, x_t, noise_out, B,
                       n, T, chunks, seed, sample_offset);
    return hipGetLastError();
}

hipError_t launch_vb_terms(const float* x_start, const float* x_t, const float* output, const float* noise, const int* t_idx, const float* coef,
                           float* terms, int B, int N, int n, int flags, hipStream_t s) {
    if (N <= 0 || n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_vb_terms, dim3((unsigned)N), dim3(VB_THREADS), 0, s, x_start, x_t, output, noise, t_idx, coef, terms, B, n, flags);
    return hipGetLastError();
}

}  // namespace rgn
