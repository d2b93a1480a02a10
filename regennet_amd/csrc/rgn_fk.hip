// Forward kinematics of a skeleton: the posed joints of the body layer behind Rotation2xyz / Rotation2xyz_x (model/rotation2xyz.py:11-155 / :158-324),
// i.e. the rigid-transform chain of linear blend skinning   G_0 = [R_0 | j_0],  G_i = G_parent(i) . [R_i | j_i - j_parent(i)],  joint i = translation of G_i,
// straight from the sampler's [B, rows, feats, T] layout to [B, J, 3 P, T] joint positions (rgn_rot2xyz). Nothing vertex-related is computed.
//
// Work split. A frame is one (motion b, person p, time t); frames are the innermost axis of x and of the output, so ADJACENT LANES TAKE ADJACENT
// FRAMES and every global access of a half-wave is one run of consecutive floats. A workgroup owns 32 consecutive frames and splits the joints over
// its 8 half-waves:
//   phase 1   rows -> 3x3 matrices (rot6d | rotvec | rotquat | rotmat), every (joint, frame) independent, into LDS
//   phase 2   the chain, depth by depth: the joints of one depth are independent, so they are dealt to the 8 half-waves; a barrier per depth.
//             A joint's transform replaces its local matrix in LDS in place (only its own thread touches it before the barrier).
// Joint 0's posed position is j_0 itself, so the root subtraction needs no second pass and every joint is written as soon as it is known.
// No atomics, no cross-workgroup traffic; a frame's result depends on that frame alone (and, for one person, on frame 0's translation row).
#include "../../include/regennet_hip.h"
#include "rgn_internal.h"
#include "rgn_device.h"

#include <hip/hip_runtime.h>
#include <math.h>

namespace rgn {

constexpr int FK_FRAMES = 32;                       // frames per workgroup = lanes of a half-wave
constexpr int FK_WORKERS = 8;                       // half-waves per workgroup
constexpr int FK_THREADS = FK_FRAMES * FK_WORKERS;
constexpr int FK_JSTRIDE = 13 * FK_FRAMES;          // floats per joint in LDS: 9 matrix + 3 position planes of 32 frames, + 1 plane so that the two
                                                    // half-waves of a wave (neighbouring joints) fall on different halves of the 64 banks

// quaternion_to_matrix (utils/rotation_conversions.py:38-66), real part first
__device__ __forceinline__ void quat_to_matrix(float r, float i, float j, float k, float (&m)[9]) {
    const float two_s = 2.0f / (r * r + i * i + j * j + k * k);
    m[0] = 1.0f - two_s * (j * j + k * k);
    m[1] = two_s * (i * j - k * r);
    m[2] = two_s * (i * k + j * r);
    m[3] = two_s * (i * j + k * r);
    m[4] = 1.0f - two_s * (i * i + k * k);
    m[5] = two_s * (j * k - i * r);
    m[6] = two_s * (i * k - j * r);
    m[7] = two_s * (j * k + i * r);
    m[8] = 1.0f - two_s * (i * i + j * j);
}

// one rotation of C channels, channel stride T floats, -> row-major 3x3
__device__ __forceinline__ void fk_rotation(const float* __restrict__ xp, long long T, int rep, float (&m)[9]) {
    if (rep == RGN_POSE_ROT6D) {
        rot6d_to_matrix(xp[0], xp[T], xp[2 * T], xp[3 * T], xp[4 * T], xp[5 * T], m);
    } else if (rep == RGN_POSE_ROTVEC) {            // axis_angle_to_matrix goes through the quaternion (rotation_conversions.py:418-479)
        const float ax = xp[0], ay = xp[T], az = xp[2 * T];
        const float angle = sqrtf(ax * ax + ay * ay + az * az), half = 0.5f * angle;
        const float s = angle < 1e-6f ? 0.5f - (angle * angle) / 48.0f : sinf(half) / angle;
        quat_to_matrix(cosf(half), ax * s, ay * s, az * s, m);
    } else if (rep == RGN_POSE_ROTQUAT) {
        quat_to_matrix(xp[0], xp[T], xp[2 * T], xp[3 * T], m);
    } else {                                        // rotmat: taken as is
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = xp[k * T];
    }
}

__global__ __launch_bounds__(FK_THREADS) void k_fk(const float* __restrict__ x, const uint8_t* __restrict__ mask, float* __restrict__ xyz,
                                                   float* __restrict__ rotmat, int B, int T, int P, int J, int C, int rep, int flags, const FkSkel sk) {
    extern __shared__ __attribute__((aligned(16))) float g[];       // [J][13][32]
    const int fl = threadIdx.x & (FK_FRAMES - 1), w = threadIdx.x / FK_FRAMES;
    const long long NF = (long long)B * P * T, f = (long long)blockIdx.x * FK_FRAMES + fl;
    const bool live = f < NF;
    const long long fc = live ? f : NF - 1;          // a lane past the end computes the last frame again (every address stays in bounds) and stores nothing
    const int t = (int)(fc % T), p = (int)((fc / T) % P);
    const long long b = fc / ((long long)T * P);
    const bool glob = flags & RGN_R2X_GLOB, trans = flags & RGN_R2X_TRANSLATION;
    const int R = (glob ? J : J - 1) + (trans ? 1 : 0);
    const long long rowstride = (long long)C * P * T;
    const float* __restrict__ xb = x + (b * R * rowstride + (long long)p * C * T + t);      // + row * rowstride + channel * T

    for (int i = w; i < J; i += FK_WORKERS) {       // ---- phase 1
        float m[9];
        const int row = glob ? i : i - 1;
        if (row < 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) m[k] = sk.glob[k];
        } else {
            fk_rotation(xb + row * rowstride, T, rep, m);
        }
        float* gi = g + i * FK_JSTRIDE + fl;
#pragma unroll
        for (int k = 0; k < 9; ++k) gi[k * FK_FRAMES] = m[k];
        if (rotmat && live) {
            float* rm = rotmat + (f * J + i) * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) rm[k] = m[k];
        }
    }
    // what is added after the root subtraction (rotation2xyz.py:247-249, :316-321): the translation row, for one person relative to frame 0
    float tr[3] = {0.f, 0.f, 0.f};
    const bool addtr = trans && (flags & RGN_R2X_VERTSTRANS);
    if (addtr) {
        const float* xt = xb + (R - 1) * rowstride;
#pragma unroll
        for (int c = 0; c < 3; ++c) tr[c] = P == 1 ? xt[c * (long long)T] - xt[c * (long long)T - t] : xt[c * (long long)T];
    }
    const bool keep = mask ? mask[b * T + t] != 0 : true;
    float* __restrict__ ob = xyz + ((b * J * 3 * P + 3 * p) * (long long)T + t);             // + joint * 3 P T + channel * T
    __syncthreads();

    for (int l = 0; l < sk.nlevels; ++l) {          // ---- phase 2
        for (int q = sk.level[l] + w; q < sk.level[l + 1]; q += FK_WORKERS) {
            const int i = sk.order[q], par = sk.parent[i];
            float* gi = g + i * FK_JSTRIDE + fl;
            float pos[3];
            if (par < 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) pos[c] = sk.rel[0][c];
            } else {
                const float* gp = g + par * FK_JSTRIDE + fl;
                float a[9], m[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) { a[k] = gp[k * FK_FRAMES]; m[k] = gi[k * FK_FRAMES]; }
                const float r0 = sk.rel[i][0], r1 = sk.rel[i][1], r2 = sk.rel[i][2];
#pragma unroll
                for (int r = 0; r < 3; ++r) {       // the 4x4 product of the chain, row r: rotation part and translation column
#pragma unroll
                    for (int c = 0; c < 3; ++c) gi[(3 * r + c) * FK_FRAMES] = a[3 * r] * m[c] + a[3 * r + 1] * m[3 + c] + a[3 * r + 2] * m[6 + c];
                    pos[r] = a[3 * r] * r0 + a[3 * r + 1] * r1 + a[3 * r + 2] * r2 + gp[(9 + r) * FK_FRAMES];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) gi[(9 + c) * FK_FRAMES] = pos[c];
            if (live) {
                float* o = ob + (long long)i * 3 * P * T;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float v = keep ? pos[c] - sk.rel[0][c] : 0.f;       // masked frames are 0, then joint 0 is subtracted (:305-314)
                    if (addtr) v += tr[c];
                    o[c * (long long)T] = v;
                }
            }
        }
        __syncthreads();
    }
}

hipError_t launch_fk(const float* x, const uint8_t* mask, float* xyz, float* rotmat, int B, int T, int P, int J, int pose_rep, int flags,
                     const FkSkel& sk, hipStream_t s) {
    const long long NF = (long long)B * P * T;
    if (NF <= 0) return hipSuccess;
    const int C = pose_rep == RGN_POSE_ROT6D ? 6 : pose_rep == RGN_POSE_ROTVEC ? 3 : pose_rep == RGN_POSE_ROTQUAT ? 4 : 9;
    const size_t lds = (size_t)J * FK_JSTRIDE * sizeof(float);      // <= 64 * 1664 B = 104 KB of the CU's 160 KB
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_fk), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fk, dim3((unsigned)((NF + FK_FRAMES - 1) / FK_FRAMES)), dim3(FK_THREADS), lds, s, x, mask, xyz, rotmat, B, T, P, J, C, pose_rep,
                       flags, sk);
    return hipGetLastError();
}

}  // namespace rgn
