// The terms of GaussianDiffusion.training_losses (diffusion/gaussian_diffusion.py:1239-1403) for a predicted reaction `output` against the
// ground truth `target` and the actor `cmotion`, one row of seven numbers per motion (rgn_loss_terms): rot_mse, rcxyz_mse, vel_mse, fc, orient,
// body, transl - each a masked_l2 (:213-225), i.e. sum(mask * (a - b)^2) / (sum(mask) * a.shape[1] * a.shape[2]) of the tensor handed in.
//
// Work split. ONE WORKGROUP PER MOTION walks the motion's frames in tiles of LOSS_FRAMES; the threads are dealt like k_fk's (rgn_fk.hip):
// lane = frame, group of LOSS_FRAMES lanes = a share of the joints / rows. Per tile
//   rows      rot_mse, vel_mse (rows 0 .. R-2), transl and orient straight from the three inputs
//   chain x 3 the chain of rgn_fk.h for target, output and cmotion in the one LDS image g; the posed joints (joint 0 subtracted) of target and
//             output stay in the planes pT / pO, so rcxyz_mse falls out of the output's chain and body out of cmotion's. No xyz tensor is written.
//   fc        between the output's and cmotion's chain, from pT / pO
// The velocity terms pair frame t with frame t - 1 (the pair's mask is that of frame t: mask[..., 1:]); lane 0 takes frame t - 1 of the foot
// joints from the four positions the previous tile left in `carry`, the rows are read from memory again.
//
// Arithmetic: fp64 from the fp32 inputs, the row rounded to fp32 at the end. Every output is ONE number per motion, so there is no maximum over
// many elements to steady the comparison with an fp32 evaluation of the reference: an fp32 form of this kernel sat at 1 - 3 times the fp32
// reference's own distance from fp64 on the chain terms and at 9 times on orient (a difference of two angles of ~2 rad each, squared), where the
// project's rule allows 4. In fp64 the kernel's only error is the final rounding. That halves the tile (16 frames: the image of one chain is
// J x 13 x 16 x 8 B, 91.5 KB at J = 55, the two position planes 21 KB each, of the CU's 160 KB) and costs nothing that shows: the kernel waits on
// its barriers (one per tree depth and chain), not on its arithmetic.
// The threads are combined in a fixed order (a butterfly inside each wave, then the four waves in index order): no atomics, the same bits on
// every run, and a motion's row depends on that motion alone.
#include "rgn_fk.h"

namespace rgn {

constexpr int LOSS_FRAMES = 16;                         // frames per tile = lanes of a group
constexpr int LOSS_WORKERS = FK_THREADS / LOSS_FRAMES;  // groups per workgroup
constexpr int LOSS_JSTRIDE = 13 * LOSS_FRAMES;          // doubles per joint in the chain image (fk_chain<LOSS_FRAMES>)
constexpr int LOSS_PSTRIDE = 3 * LOSS_FRAMES;           // doubles per joint in pT / pO
constexpr int LOSS_NACC = 9;                            // the seven sums, sum(mask), sum(mask[1:])

size_t loss_lds_bytes(int J) { return ((size_t)J * (LOSS_JSTRIDE + 2 * LOSS_PSTRIDE) + 2 * 4 * 3 + (FK_THREADS / 64) * LOSS_NACC) * sizeof(double); }

// rotation_6d_to_matrix (utils/rotation_conversions.py:513-534; F.normalize's floor of 1e-12 on the norms), rows b1, b2, b1 x b2
__device__ __forceinline__ void rot6d_to_matrix_f64(const float* __restrict__ xp, long long T, double (&m)[9]) {
    const double a1x = xp[0], a1y = xp[T], a1z = xp[2 * T], a2x = xp[3 * T], a2y = xp[4 * T], a2z = xp[5 * T];
    const double n1 = fmax(sqrt(a1x * a1x + a1y * a1y + a1z * a1z), 1e-12);
    const double b1x = a1x / n1, b1y = a1y / n1, b1z = a1z / n1;
    const double dot = b1x * a2x + b1y * a2y + b1z * a2z;
    double b2x = a2x - dot * b1x, b2y = a2y - dot * b1y, b2z = a2z - dot * b1z;
    const double n2 = fmax(sqrt(b2x * b2x + b2y * b2y + b2z * b2z), 1e-12);
    b2x /= n2; b2y /= n2; b2z /= n2;
    m[0] = b1x; m[1] = b1y; m[2] = b1z;
    m[3] = b2x; m[4] = b2y; m[5] = b2z;
    m[6] = b1y * b2z - b1z * b2y;
    m[7] = b1z * b2x - b1x * b2z;
    m[8] = b1x * b2y - b1y * b2x;
}

// theta = || matrix_to_axis_angle(Rc^T Rx) || (utils/rotation_conversions.py:98-120 matrix_to_quaternion, :482-510 quaternion_to_axis_angle)
__device__ __forceinline__ double relative_angle(const double (&c)[9], const double (&x)[9]) {
    // M = Rc^T Rx, M[i][j] = sum_k c[k][i] x[k][j]: its diagonal and its three antisymmetric differences
    auto M = [&](int i, int j) { return c[i] * x[j] + c[3 + i] * x[3 + j] + c[6 + i] * x[6 + j]; };
    const double m00 = M(0, 0), m11 = M(1, 1), m22 = M(2, 2);
    auto sqrt_pos = [](double v) { return v > 0.0 ? sqrt(v) : 0.0; };
    auto copysign_ = [](double a, double b) { return ((a < 0.0) != (b < 0.0)) ? -a : a; };
    const double o0 = 0.5 * sqrt_pos(1.0 + m00 + m11 + m22);
    const double qx = 0.5 * sqrt_pos(1.0 + m00 - m11 - m22);
    const double qy = 0.5 * sqrt_pos(1.0 - m00 + m11 - m22);
    const double qz = 0.5 * sqrt_pos(1.0 - m00 - m11 + m22);
    const double o1 = copysign_(qx, M(2, 1) - M(1, 2)), o2 = copysign_(qy, M(0, 2) - M(2, 0)), o3 = copysign_(qz, M(1, 0) - M(0, 1));
    const double norms = sqrt(o1 * o1 + o2 * o2 + o3 * o3);
    const double half = atan2(norms, o0), angle = 2.0 * half;
    const double s = fabs(angle) < 1e-6 ? 0.5 - (angle * angle) / 48.0 : sin(half) / angle;
    const double ax = o1 / s, ay = o2 / s, az = o3 / s;
    return sqrt(ax * ax + ay * ay + az * az);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// phase 1 of a chain: rows 0 .. J-1 of motion `xb` at frame tc -> 3x3 matrices, planes 0..8 of g[i] (the fp64 counterpart of fk_local_matrices for rot6d rows)
__device__ __forceinline__ void loss_local_matrices(double* g, const float* __restrict__ xb, int T, int J, int tc, int fl, int w) {
    for (int i = w; i < J; i += LOSS_WORKERS) {
        double m[9];
        rot6d_to_matrix_f64(xb + ((long long)i * 6) * T + tc, T, m);
        double* gi = g + i * LOSS_JSTRIDE + fl;
#pragma unroll
        for (int k = 0; k < 9; ++k) gi[k * LOSS_FRAMES] = m[k];
    }
}

__global__ __launch_bounds__(FK_THREADS) void k_loss_terms(const float* __restrict__ target, const float* __restrict__ output,
                                                           const float* __restrict__ cmotion, const uint8_t* __restrict__ mask,
                                                           float* __restrict__ terms, int T, int J, int4 foot, int transl_row, float vel_threshold,
                                                           int flags, const FkSkel sk) {
    extern __shared__ __attribute__((aligned(16))) double g[];      // [J][13][16] chain image | pT [J][3][16] | pO [J][3][16] | carry [2][4][3] | red [4][9]
    double* pT = g + J * LOSS_JSTRIDE;
    double* pO = pT + J * LOSS_PSTRIDE;
    double* carry = pO + J * LOSS_PSTRIDE;
    double* red = carry + 24;
    const int fl = threadIdx.x & (LOSS_FRAMES - 1), w = threadIdx.x / LOSS_FRAMES;
    const int R = J + 1;
    const long long b = blockIdx.x, mstride = (long long)R * 6 * T;
    const float* tb = target + b * mstride;
    const float* ob = output + b * mstride;
    const float* cb = cmotion + b * mstride;
    const uint8_t* mb = mask + b * T;
    const int fjw = w == 0 ? foot.x : w == 1 ? foot.y : w == 2 ? foot.z : foot.w;      // the foot joint of groups 0 .. 3
    const double thr = vel_threshold;

    double acc[LOSS_NACC];
#pragma unroll
    for (int k = 0; k < LOSS_NACC; ++k) acc[k] = 0.0;

    const int ntiles = (T + LOSS_FRAMES - 1) / LOSS_FRAMES;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int t = tile * LOSS_FRAMES + fl;
        const bool live = t < T, pair = live && t >= 1;             // pair: (t - 1, t)
        const int tc = live ? t : T - 1;                            // a lane past the end runs the chains on the last frame again (every address stays in bounds) and adds nothing
        const double mk = live && mb[t] != 0 ? 1.0 : 0.0;
        if (w == 0 && live) {
            acc[7] += mk;
            if (pair) acc[8] += mk;
        }
        // ---- the rows themselves: rot_mse over all R rows, vel_mse over rows 0 .. R-2
        if (live) {
            double s_rot = 0.0, s_vel = 0.0;
            for (int r = w; r < R; r += LOSS_WORKERS) {
                const long long o = ((long long)r * 6) * T + t;
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    const double tv = tb[o + (long long)c * T], ov = ob[o + (long long)c * T];
                    const double d = tv - ov;
                    s_rot += d * d;
                    if (pair && r < R - 1) {
                        const double dv = (tv - (double)tb[o + (long long)c * T - 1]) - (ov - (double)ob[o + (long long)c * T - 1]);
                        s_vel += dv * dv;
                    }
                }
            }
            acc[0] += s_rot * mk;
            if (pair) acc[2] += s_vel * mk;
            if (w == LOSS_WORKERS - 1) {            // transl: distance of the translation row's first three channels to the actor's
                const long long o = ((long long)transl_row * 6) * T + t;
                double dt = 0.0, dq = 0.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double cv = cb[o + (long long)c * T], a = cv - (double)tb[o + (long long)c * T], q = cv - (double)ob[o + (long long)c * T];
                    dt += a * a;
                    dq += q * q;
                }
                const double d = sqrt(dt) - sqrt(dq);
                acc[6] += d * d * mk;
            }
            if (w == LOSS_WORKERS - 2) {            // orient: row 0 as matrices, the angle of Rc^T Rx
                double mc[9], mt[9], mo[9];
                rot6d_to_matrix_f64(cb + t, T, mc);
                rot6d_to_matrix_f64(tb + t, T, mt);
                rot6d_to_matrix_f64(ob + t, T, mo);
                const double d = relative_angle(mc, mt) - relative_angle(mc, mo);
                acc[4] += d * d * mk;
            }
        }

        // ---- target's chain: posed joints (joint 0 subtracted, as rot2xyz does) -> pT
        loss_local_matrices(g, tb, T, J, tc, fl, w);
        __syncthreads();
        fk_chain<LOSS_FRAMES>(g, sk, fl, w, [&](int i, const double (&pos)[3], const double*) {
#pragma unroll
            for (int c = 0; c < 3; ++c) pT[i * LOSS_PSTRIDE + c * LOSS_FRAMES + fl] = pos[c] - (double)sk.rel[0][c];
        });
        // ---- output's chain -> pO, rcxyz_mse
        {
            loss_local_matrices(g, ob, T, J, tc, fl, w);
            __syncthreads();
            double s = 0.0;
            fk_chain<LOSS_FRAMES>(g, sk, fl, w, [&](int i, const double (&pos)[3], const double*) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double po = pos[c] - (double)sk.rel[0][c];
                    pO[i * LOSS_PSTRIDE + c * LOSS_FRAMES + fl] = po;
                    const double d = pT[i * LOSS_PSTRIDE + c * LOSS_FRAMES + fl] - po;
                    s += d * d;
                }
            });
            if (live) acc[1] += s * mk;
        }
        // ---- fc: where the ground truth's foot joint moves at most vel_threshold from frame t - 1 to t, the prediction's velocity is penalised
        if ((flags & RGN_LOSS_FC) && w < 4 && pair) {
            double gt = 0.0, pv = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int at = fjw * LOSS_PSTRIDE + c * LOSS_FRAMES + fl;
                const double t0 = fl > 0 ? pT[at - 1] : carry[w * 3 + c], o0 = fl > 0 ? pO[at - 1] : carry[12 + w * 3 + c];
                const double dg = pT[at] - t0, dp = pO[at] - o0;
                gt += dg * dg;
                pv += dp * dp;
            }
            if (sqrt(gt) <= thr) acc[3] += pv * mk;
        }
        // ---- cmotion's chain: body = (|c - target| - |c - output|)^2 per joint
        {
            loss_local_matrices(g, cb, T, J, tc, fl, w);
            __syncthreads();                        // (also: every lane 0 has read `carry` before a last lane replaces it below)
            double s = 0.0;
            fk_chain<LOSS_FRAMES>(g, sk, fl, w, [&](int i, const double (&pos)[3], const double*) {
                double dt = 0.0, dq = 0.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double pc = pos[c] - (double)sk.rel[0][c];
                    const double a = pc - pT[i * LOSS_PSTRIDE + c * LOSS_FRAMES + fl], q = pc - pO[i * LOSS_PSTRIDE + c * LOSS_FRAMES + fl];
                    dt += a * a;
                    dq += q * q;
                }
                const double d = sqrt(dt) - sqrt(dq);
                s += d * d;
            });
            if (live) acc[5] += s * mk;
        }
        if ((flags & RGN_LOSS_FC) && w < 4 && fl == LOSS_FRAMES - 1) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                carry[w * 3 + c] = pT[fjw * LOSS_PSTRIDE + c * LOSS_FRAMES + fl];
                carry[12 + w * 3 + c] = pO[fjw * LOSS_PSTRIDE + c * LOSS_FRAMES + fl];
            }
        }
        __syncthreads();                            // g / pT / pO / carry are free for the next tile
    }

    // ---- combine: butterfly inside each wave, then the waves in index order
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < LOSS_NACC; ++k) {
        const double v = wave_sum_f64(acc[k]);
        if ((threadIdx.x & 63) == 0) red[wave * LOSS_NACC + k] = v;
    }
    __syncthreads();
    if (threadIdx.x < RGN_LOSS_NTERMS) {
        const int k = threadIdx.x;
        auto total = [&](int q) {
            double v = 0.0;
            for (int x = 0; x < FK_THREADS / 64; ++x) v += red[x * LOSS_NACC + q];
            return v;
        };
        const double n = total(7), n1 = total(8);
        // n_entries = a.shape[1] * a.shape[2] of the tensor masked_l2 was handed: orient / transl [B,1,T] and body [B,J,T] carry the frame count
        const double entries = k == RGN_LOSS_ROT_MSE ? (double)R * 6 : k == RGN_LOSS_RCXYZ_MSE ? (double)J * 3 : k == RGN_LOSS_VEL_MSE ? (double)(R - 1) * 6
                               : k == RGN_LOSS_FC_TERM ? 12.0 : k == RGN_LOSS_BODY ? (double)J * T : (double)T;
        const double den = (k == RGN_LOSS_VEL_MSE || k == RGN_LOSS_FC_TERM ? n1 : n) * entries;
        const double v = (k == RGN_LOSS_FC_TERM && !(flags & RGN_LOSS_FC)) ? 0.0 : total(k) / den;      // 0 / 0: NaN, as the reference gives
        terms[b * RGN_LOSS_NTERMS + k] = (float)v;
    }
}

hipError_t launch_loss_terms(const float* target, const float* output, const float* cmotion, const uint8_t* mask, float* terms, int B, int T, int J,
                             const int* foot, int transl_row, float vel_threshold, int flags, const FkSkel& sk, hipStream_t s) {
    if (B <= 0 || T <= 0) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_loss_terms), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_loss_terms, dim3((unsigned)B), dim3(FK_THREADS), loss_lds_bytes(J), s, target, output, cmotion, mask, terms, T, J,
                       make_int4(foot[0], foot[1], foot[2], foot[3]), transl_row, vel_threshold, flags, sk);
    return hipGetLastError();
}

}  // namespace rgn
