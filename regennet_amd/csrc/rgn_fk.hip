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
//
// k_fk<true> (rgn_rot2xyz_shaped) is the same kernel with the frame's body shape: the lane reads its betas into registers after phase 1 and takes
// every joint's rest offset - and joint 0's rest position, which is what the root subtraction removes - from them (rgn_fk.h: FkShapedRel). The LDS
// image is the same; k_fk<false> does not look at `sh`.
#include "rgn_fk.h"

namespace rgn {

template <bool SHAPED>
__global__ __launch_bounds__(FK_THREADS) void k_fk(const float* __restrict__ x, const uint8_t* __restrict__ mask, float* __restrict__ xyz,
                                                   float* __restrict__ rotmat, int B, int T, int P, int J, int C, int rep, int flags, const FkSkel sk,
                                                   const FkShape sh) {
    extern __shared__ __attribute__((aligned(16))) float g[];       // [J][13][32]
    const int fl = threadIdx.x & (FK_FRAMES - 1), w = threadIdx.x / FK_FRAMES;
    const FkFrame fr = fk_frame(x, mask, blockIdx.x, fl, B, T, P, J, C, flags);

    fk_local_matrices(g, fr, T, J, rep, flags & RGN_R2X_GLOB, sk, fl, w, [&](int i, float (&m)[9]) {      // ---- phase 1 (shared: rgn_fk.h)
        if (rotmat && fr.live) {
            float* rm = rotmat + (fr.f * J + i) * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) rm[k] = m[k];
        }
    });
    float* __restrict__ ob = xyz + ((fr.b * J * 3 * P + 3 * fr.p) * (long long)T + fr.t);       // + joint * 3 P T + channel * T
    __syncthreads();

    if constexpr (!SHAPED) {
        fk_chain(g, sk, fl, w, [&](int i, const float (&pos)[3], const float*) {                    // ---- phase 2
            if (fr.live) {
                float* o = ob + (long long)i * 3 * P * T;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float v = fr.keep ? pos[c] - sk.rel[0][c] : 0.f;        // masked frames are 0, then joint 0 is subtracted (:305-314)
                    if (fr.addtr) v += fr.tr[c];
                    o[c * (long long)T] = v;
                }
            }
        });
    } else {
        float be[FK_MAX_BETAS], j0[3];
        fk_load_betas(sh, fr, be);
        const FkShapedRel rel{sk, sh, be};
        rel(0, j0);                                                         // joint 0 as this frame's shape places it: the chain's own value
        fk_chain_rel(g, sk, fl, w, rel, [&](int i, const float (&pos)[3], const float*) {
            if (fr.live) {
                float* o = ob + (long long)i * 3 * P * T;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float v = fr.keep ? pos[c] - j0[c] : 0.f;
                    if (fr.addtr) v += fr.tr[c];
                    o[c * (long long)T] = v;
                }
            }
        });
    }
}

template <bool SHAPED>
static hipError_t launch_fk_form(const float* x, const uint8_t* mask, float* xyz, float* rotmat, int B, int T, int P, int J, int pose_rep, int flags,
                                 const FkSkel& sk, const FkShape& sh, hipStream_t s) {
    const long long NF = (long long)B * P * T;
    if (NF <= 0) return hipSuccess;
    const int C = pose_rep == RGN_POSE_ROT6D ? 6 : pose_rep == RGN_POSE_ROTVEC ? 3 : pose_rep == RGN_POSE_ROTQUAT ? 4 : 9;
    const size_t lds = (size_t)J * FK_JSTRIDE * sizeof(float);      // <= 64 * 1664 B = 104 KB of the CU's 160 KB
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_fk<SHAPED>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fk<SHAPED>, dim3((unsigned)((NF + FK_FRAMES - 1) / FK_FRAMES)), dim3(FK_THREADS), lds, s, x, mask, xyz, rotmat, B, T, P, J, C,
                       pose_rep, flags, sk, sh);
    return hipGetLastError();
}

hipError_t launch_fk(const float* x, const uint8_t* mask, float* xyz, float* rotmat, int B, int T, int P, int J, int pose_rep, int flags,
                     const FkSkel& sk, hipStream_t s) {
    return launch_fk_form<false>(x, mask, xyz, rotmat, B, T, P, J, pose_rep, flags, sk, FkShape{}, s);
}

hipError_t launch_fk_shaped(const float* x, const uint8_t* mask, float* xyz, float* rotmat, int B, int T, int P, int J, int pose_rep, int flags,
                            const FkSkel& sk, const FkShape& sh, hipStream_t s) {
    return launch_fk_form<true>(x, mask, xyz, rotmat, B, T, P, J, pose_rep, flags, sk, sh, s);
}

}  // namespace rgn
