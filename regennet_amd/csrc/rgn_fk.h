// The device side of forward kinematics that k_fk (rgn_fk.hip: posed joints) and k_lbs_chain (rgn_lbs.hip: skinning transforms) share: the frame a lane
// owns, the conversion of its rows to 3x3 matrices into LDS (phase 1) and the rigid-transform chain down the parent table (phase 2). The work split is
// described at the top of rgn_fk.hip; what a kernel does with a joint's matrix or its posed transform goes in through a callable.
#pragma once
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

// The frame (motion b, person p, time t) of lane `fl` in the workgroup's tile of FK_FRAMES frames, with what the wrappers' tail needs of it.
struct FkFrame {
    long long f, b;                 // frame index (b P + p) T + t, motion
    int t, p, R;                    // R: rows of x
    bool live, keep, addtr;         // inside the batch; mask != 0; the translation row is added
    long long rowstride;            // floats between two rows of x
    const float* xb;                // x + this frame's offset: + row * rowstride + channel * T
    float tr[3];                    // what is added after masking (rotation2xyz.py:247-249, :316-321): the translation row, for one person relative to frame 0
};

__device__ __forceinline__ FkFrame fk_frame(const float* __restrict__ x, const uint8_t* __restrict__ mask, long long tile, int fl, int B, int T, int P, int J,
                                            int C, int flags) {
    FkFrame fr;
    const long long NF = (long long)B * P * T;
    fr.f = tile * FK_FRAMES + fl;
    fr.live = fr.f < NF;
    const long long fc = fr.live ? fr.f : NF - 1;   // a lane past the end computes the last frame again (every address stays in bounds) and stores nothing
    fr.t = (int)(fc % T);
    fr.p = (int)((fc / T) % P);
    fr.b = fc / ((long long)T * P);
    const bool glob = flags & RGN_R2X_GLOB, trans = flags & RGN_R2X_TRANSLATION;
    fr.R = (glob ? J : J - 1) + (trans ? 1 : 0);
    fr.rowstride = (long long)C * P * T;
    fr.xb = x + (fr.b * fr.R * fr.rowstride + (long long)fr.p * C * T + fr.t);
    fr.tr[0] = fr.tr[1] = fr.tr[2] = 0.f;
    fr.addtr = trans && (flags & RGN_R2X_VERTSTRANS);
    if (fr.addtr) {
        const float* xt = fr.xb + (fr.R - 1) * fr.rowstride;
#pragma unroll
        for (int c = 0; c < 3; ++c) fr.tr[c] = P == 1 ? xt[c * (long long)T] - xt[c * (long long)T - fr.t] : xt[c * (long long)T];
    }
    fr.keep = mask ? mask[fr.b * T + fr.t] != 0 : true;
    return fr;
}

// phase 1: joint i's rows -> its 3x3 matrix, planes 0..8 of g[i]; each(i, m) sees (and may replace) the matrix before it is stored
template <class Each>
__device__ __forceinline__ void fk_local_matrices(float* g, const FkFrame& fr, long long T, int J, int rep, bool glob, const FkSkel& sk, int fl, int w,
                                                  Each&& each) {
    for (int i = w; i < J; i += FK_WORKERS) {
        float m[9];
        const int row = glob ? i : i - 1;
        if (row < 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) m[k] = sk.glob[k];
        } else {
            fk_rotation(fr.xb + row * fr.rowstride, T, rep, m);
        }
        each(i, m);
        float* gi = g + i * FK_JSTRIDE + fl;
#pragma unroll
        for (int k = 0; k < 9; ++k) gi[k * FK_FRAMES] = m[k];
    }
}

// Joint i's parent-relative rest offset as fk_chain asks for it, rel(i, r): the call's one rest skeleton, from the by-value table ...
struct FkRestRel {
    const FkSkel& sk;
    template <class S>
    __device__ __forceinline__ void operator()(int i, S (&r)[3]) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = sk.rel[i][c];
    }
};

// ... or this lane's own (rgn_rot2xyz_shaped / rgn_rot2verts_shaped): rel[i] + sum_k (shape_joints[i] - shape_joints[parent(i)])[.][k] beta[k], the
// frame's betas in registers, shape_joints [J][3][nb] read from global memory at an address the half-wave shares. Nothing of it goes through LDS.
// (FkShape: rgn_internal.h)

// The betas of the lane's frame. A masked frame, or a lane past the end, reads none and counts as shape 0.
__device__ __forceinline__ void fk_load_betas(const FkShape& sh, const FkFrame& fr, float (&be)[FK_MAX_BETAS]) {
    const bool rd = fr.live && fr.keep;
    const float* bp = sh.betas + (fr.b * sh.sb + fr.p * sh.sp + fr.t * sh.st);
#pragma unroll
    for (int k = 0; k < FK_MAX_BETAS; ++k) be[k] = (rd && k < sh.nb) ? bp[k] : 0.f;
}

// r += sum_k (shape_joints[i] - shape_joints[par])[.][k] be[k] in k order; par < 0: joint i's own shape directions (the absolute rest position)
__device__ __forceinline__ void fk_shape_add(const FkShape& sh, int i, int par, const float (&be)[FK_MAX_BETAS], float (&r)[3]) {
    const float* si = sh.sj + (size_t)i * 3 * sh.nb;
    const float* sp = sh.sj + (size_t)(par < 0 ? 0 : par) * 3 * sh.nb;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < FK_MAX_BETAS; ++k)
            if (k < sh.nb) r[c] = fmaf(par < 0 ? si[c * sh.nb + k] : si[c * sh.nb + k] - sp[c * sh.nb + k], be[k], r[c]);
}

struct FkShapedRel {
    const FkSkel& sk;
    const FkShape& sh;
    const float (&be)[FK_MAX_BETAS];
    __device__ __forceinline__ void operator()(int i, float (&r)[3]) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = sk.rel[i][c];
        fk_shape_add(sh, i, sk.parent[i], be, r);
    }
};

// phase 2: the chain, depth by depth (a barrier per depth). Joint i's transform replaces its local matrix in g[i] (planes 0..8 rotation, 9..11 posed
// position); emit(i, pos, gi) runs on the thread that formed it, gi = g[i] + this lane. The image's scalar type follows g and its tile width is FRAMES
// (13 planes of FRAMES per joint, FK_THREADS / FRAMES workers): k_fk and k_lbs_chain run float x FK_FRAMES, k_loss_terms (rgn_loss.hip) double x 16.
// rel(i, r) gives joint i's offset from its parent's rest position (joint 0: its rest position) for this lane.
template <int FRAMES = FK_FRAMES, class S, class Rel, class Emit>
__device__ __forceinline__ void fk_chain_rel(S* g, const FkSkel& sk, int fl, int w, Rel&& rel, Emit&& emit) {
    constexpr int JSTRIDE = 13 * FRAMES, WORKERS = FK_THREADS / FRAMES;
    for (int l = 0; l < sk.nlevels; ++l) {
        for (int q = sk.level[l] + w; q < sk.level[l + 1]; q += WORKERS) {
            const int i = sk.order[q], par = sk.parent[i];
            S* gi = g + i * JSTRIDE + fl;
            S pos[3];
            if (par < 0) {
                rel(0, pos);
            } else {
                const S* gp = g + par * JSTRIDE + fl;
                S a[9], m[9], rl[3];
#pragma unroll
                for (int k = 0; k < 9; ++k) { a[k] = gp[k * FRAMES]; m[k] = gi[k * FRAMES]; }
                rel(i, rl);
                const S r0 = rl[0], r1 = rl[1], r2 = rl[2];
#pragma unroll
                for (int r = 0; r < 3; ++r) {       // the 4x4 product of the chain, row r: rotation part and translation column
#pragma unroll
                    for (int c = 0; c < 3; ++c) gi[(3 * r + c) * FRAMES] = a[3 * r] * m[c] + a[3 * r + 1] * m[3 + c] + a[3 * r + 2] * m[6 + c];
                    pos[r] = a[3 * r] * r0 + a[3 * r + 1] * r1 + a[3 * r + 2] * r2 + gp[(9 + r) * FRAMES];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) gi[(9 + c) * FRAMES] = pos[c];
            emit(i, pos, gi);
        }
        __syncthreads();
    }
}

template <int FRAMES = FK_FRAMES, class S, class Emit>
__device__ __forceinline__ void fk_chain(S* g, const FkSkel& sk, int fl, int w, Emit&& emit) {
    fk_chain_rel<FRAMES>(g, sk, fl, w, FkRestRel{sk}, emit);
}

}  // namespace rgn
