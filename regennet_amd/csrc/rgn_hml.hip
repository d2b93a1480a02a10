// Joint positions of a HumanML3D / KIT feature vector: what the reference does after every sampling call of a data_rep='hml_vec' model
// (sample/cgenerate.py:147-152, sample/edit.py:117-120, :153-155, sample/predict.py:114-117) - inv_transform with the dataset's Mean / Std
// (data_loaders/humanml/data/dataset.py:132), then recover_from_ric (data_loaders/humanml/scripts/motion_process.py:362-381, :415-430) - in ONE
// launch on the sample's own layout: x [B, D, 1, T] -> xyz [B, J, 3, T] (the view / permute of cgenerate.py:152 is the output layout).
//
// Per motion, with f_k[t] the de-normalised feature k of frame t (rows: rgn_hml_check.h):
//   a[t] = sum_{s < t} f_0[s]                                     r_rot_ang: the cumsum of the velocities SHIFTED by one frame (:364-367), a[0] = 0
//   q[t] = (cos a[t], 0, sin a[t], 0)                             a goes in as it stands, NOT halved (:369-371): the frame turns by 2 a
//   u[t] = qrot(qinv(q[t]), (f_1[t-1], 0, f_2[t-1])), u[0] = 0    the velocity of frame t-1 under the angle of frame t (:373-376); the INVERSE rotates
//   r[t] = sum_{s <= t} u[s], r[t].y = f_3[t]                     (:378-380)
//   joint 0 = r[t]; joint j >= 1 = qrot(qinv(q[t]), f_{4+3(j-1) ..}[t]) + (r[t].x, 0, r[t].z)     (:417-428)
// qrot is quaternion.py:54-73 as written, v + 2 (w uv + uuv) with uv = qvec x v and uuv = qvec x uv; only the products with the two zero
// components of qvec = (0, -sin a, 0) are left out, which changes no value.
//
// Arithmetic: the convention of rgn_loss.hip / rgn_vb.hip. The de-normalisation is x * std + mean in fp32, two separately rounded operations and no
// fma - the bits of the reference's expression on fp32 statistics; with NULL statistics the feature is taken as it is. Everything after that - both
// sums, sincos, the rotations - is fp64 from those fp32 values, and every output is rounded to fp32 once.
//
// ONE WORKGROUP PER MOTION, frames in chunks of HML_CHUNK = 256 (one frame per thread). The two recurrences are prefix scans: a shuffle scan inside
// each wave, the four wave totals combined through LDS in index order, and the chunk's last frame carried into the next chunk. The order of every
// sum is fixed by T alone and there are no atomics: a motion's result depends neither on B nor on its neighbours and is the same on every run.
// The per-frame quadruple (cos a, sin a, r.x, r.z) of the chunk stays in LDS; the joint phase then walks (joint, frame) with the frame fastest, so
// the three reads of x and the three writes of xyz per item are contiguous along frames. Only rows 0 .. 3 (J-1) + 3 of x, mean and std are read.
// LDS: 8 KiB + a few carries, independent of T.
#include "rgn_device.h"

#include "../../include/regennet_hip.h"

namespace rgn {

constexpr int HML_CHUNK = 256;                 // frames per chunk = threads per workgroup
constexpr int HML_WAVES = HML_CHUNK / 64;

// inclusive prefix sum over the 64 lanes of a wave, lane order
__device__ __forceinline__ double hml_wave_scan(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    return v;
}

__global__ __launch_bounds__(HML_CHUNK) void k_hml_joints(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ stdv,
                                                          float* __restrict__ xyz, int T, int D, int J) {
    __shared__ double quad[HML_CHUNK][4];      // (cos a, sin a, r.x, r.z) of the chunk's frames
    __shared__ double wtot[3][HML_WAVES];      // wave totals of the three scans (a, u.x, u.z)
    __shared__ double last[3];                 // the chunk's last frame: the carry into the next chunk
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* xb = x + (size_t)blockIdx.x * D * T;
    float* ob = xyz + (size_t)blockIdx.x * J * 3 * T;
    // feature k of frame t, de-normalised as the reference's fp32 expression data * std + mean
    auto feat = [&](int k, int t) -> double {
        const float v = xb[(size_t)k * T + t];
        return (double)(mean ? __fadd_rn(__fmul_rn(v, stdv[k]), mean[k]) : v);
    };
    double ca = 0.0, cx = 0.0, cz = 0.0;       // carries: a, r.x, r.z at the last frame of the previous chunk

    for (int t0 = 0; t0 < T; t0 += HML_CHUNK) {
        const int t = t0 + tid, len = min(HML_CHUNK, T - t0);
        const bool prev = t >= 1 && t < T;     // frame t has a frame before it
        // ---- a[t]: inclusive scan of the velocities shifted by one frame
        double a = hml_wave_scan(prev ? feat(0, t - 1) : 0.0, lane);
        if (lane == 63) wtot[0][wave] = a;
        __syncthreads();
        double base = ca;
        for (int w = 0; w < wave; ++w) base += wtot[0][w];
        a += base;
        double sn, cs;
        sincos(a, &sn, &cs);
        // ---- u[t] = qrot(qinv(q), (f_1[t-1], 0, f_2[t-1])): qvec = (0, -sn, 0), uv = qvec x v, uuv = qvec x uv
        const double vx = prev ? feat(1, t - 1) : 0.0, vz = prev ? feat(2, t - 1) : 0.0;
        const double uvx = -sn * vz, uvz = sn * vx;
        const double uuvx = -sn * uvz, uuvz = sn * uvx;
        double rx = hml_wave_scan(vx + 2.0 * (cs * uvx + uuvx), lane);
        double rz = hml_wave_scan(vz + 2.0 * (cs * uvz + uuvz), lane);
        if (lane == 63) {
            wtot[1][wave] = rx;
            wtot[2][wave] = rz;
        }
        __syncthreads();
        double bx = cx, bz = cz;
        for (int w = 0; w < wave; ++w) {
            bx += wtot[1][w];
            bz += wtot[2][w];
        }
        rx += bx;
        rz += bz;
        quad[tid][0] = cs;
        quad[tid][1] = sn;
        quad[tid][2] = rx;
        quad[tid][3] = rz;
        if (tid == HML_CHUNK - 1) {
            last[0] = a;
            last[1] = rx;
            last[2] = rz;
        }
        __syncthreads();
        ca = last[0];
        cx = last[1];
        cz = last[2];
        // ---- joints: (joint, frame) with the frame fastest
        for (int i = tid; i < J * len; i += HML_CHUNK) {
            const int j = i / len, tl = i - j * len, tt = t0 + tl;
            const double c = quad[tl][0], s = quad[tl][1], px = quad[tl][2], pz = quad[tl][3];
            double ox, oy, oz;
            if (j == 0) {
                ox = px;
                oy = feat(3, tt);
                oz = pz;
            } else {
                const int k = 4 + 3 * (j - 1);
                const double jx = feat(k, tt), jy = feat(k + 1, tt), jz = feat(k + 2, tt);
                const double wx = -s * jz, wz = s * jx;            // uv
                const double yx = -s * wz, yz = s * wx;            // uuv
                ox = (jx + 2.0 * (c * wx + yx)) + px;
                oy = jy;
                oz = (jz + 2.0 * (c * wz + yz)) + pz;
            }
            float* o = ob + (size_t)j * 3 * T + tt;
            o[0] = (float)ox;
            o[T] = (float)oy;
            o[2 * (size_t)T] = (float)oz;
        }
        // (the next chunk writes quad only after its two barriers, which every thread reaches after this loop)
    }
}

hipError_t launch_hml_joints(const float* x, const float* mean, const float* stdv, float* xyz, int B, int T, int D, int J, hipStream_t s) {
    hipLaunchKernelGGL(k_hml_joints, dim3((unsigned)B), dim3(HML_CHUNK), 0, s, x, mean, stdv, xyz, T, D, J);
    return hipGetLastError();
}

}  // namespace rgn
