// The wave body of the slab-staged attention kernels, defined once for the kernels that run it: k_attn_mfma and k_attn_x3 (rgn_attn.hip) and the
// attention phase of k_qkv_attn_long (rgn_qkv_attn_long.hip). The scheme: one workgroup per (sample, head), one wave per 32-query tile, everything
// computed TRANSPOSED so that no register shuffle sits between the two GEMMs -
//   S^T[key, query] = K . Q^T       a query's scores live in ONE lane pair (lane, lane ^ 32): register i of a lane in half kh is
//                                   key 32 kj + (i & 3) + 8 (i >> 2) + 4 kh of key tile kj (the C/D map of rgn_layout.h), query qrow = the lane's column
//   softmax over keys               in-register max / sum + one half-wave exchange (half_max / half_sum, rgn_device.h)
//   O^T[dh, query]  = V^T . P^T     B = P from the S^T accumulator registers (the C/D layout is the B layout up to a permutation of the key index,
//                                   which A follows), A = V^T from LDS
// and the result transposed through a per-wave fp32 patch in the dead slab, so that the global stores are row-contiguous.
// What is shared is what the kernels do to their OWN registers between the MFMA loops: the mask + maximum of an S^T tile, the exponential + sum, the P.V
// tile step on a 16-bit V^T slab (the plain form; k_attn_x3's split form and its mask loop are its own text, for its registers' sake), O^T -> patch, the patch read-back and the split plane store; and the slab geometry (AttnSlab). Operand staging
// (fp32 rows / attention-ready planes / slabs produced in place, early V loads, the V transpose), the Q.K^T loops, the fp32 kernel's 32x32x2 P.V loop and
// k_qkv_attn_long's running-max bookkeeping and flash merge stay with each kernel. Device code with internal linkage; AttnSlab is plain constexpr
// (the launchers size the dynamic LDS with it).
#pragma once
#include "rgn_internal.h"
#include "rgn_device.h"

namespace rgn {
namespace {

// ---- slab geometry of NT 32-token tiles at head dim DH (16, 32, 64 or 128). 16-bit slab: K [TQP][KLD] and V^T [DP][VLD] time-share one plane (two
// planes: hi and lo), rows padded so that the operand reads are conflict-free (KLD: ds_read_b128 of 8 dh; VLD: ds_read_b64 of 4 keys). fp32 slab
// (k_attn_mfma): K and V time-share [TQP][OLD]. Either way the slab ends as NT per-wave output patches [32 queries][OLD] of fp32.
template <int NT, int DH>
struct AttnSlab {
    static_assert(NT >= 1 && NT <= 5 && (DH == 16 || DH == 32 || DH == 64 || DH == 128), "instantiated: 1 .. 5 tiles x head dim 16 / 32 / 64 / 128");
    static constexpr int DP = DH < 32 ? 32 : DH;          // dh padded to a multiple of 32 for the PV tiles
    static constexpr int NS = DH / 16;                    // k16 steps of S^T
    static constexpr int ND = DP / 32;                    // 32-wide dh tiles of O^T
    static constexpr int TQP = 32 * NT;
    static constexpr int KLD = DH + 8;                    // K slab row stride (16-bit elements)
    static constexpr int VLD = TQP + 4;                   // V^T slab row stride (16-bit elements)
    static constexpr int PLANE = TQP * KLD > DP * VLD ? TQP * KLD : DP * VLD;   // elements per plane of the shared slab
    static constexpr int OLD = DP + 4;                    // fp32 patch (and fp32 slab) row stride
    static constexpr int PATCH = 32 * OLD;                // floats of one wave's patch
    static constexpr size_t LDS32 = (size_t)NT * PATCH * 4;                                        // fp32 slab = the patches
    static constexpr size_t LDS16 = (size_t)2 * PLANE * 2 > LDS32 ? (size_t)2 * PLANE * 2 : LDS32;   // two 16-bit planes, or the patches over them
};

// ---- mask + maximum of one S^T tile (key tile kj): keys beyond the query (CAUSAL) or beyond the sequence become -inf; returns max(mx, the lane's 16 scores)
template <bool CAUSAL>
__device__ __forceinline__ float attn_mask_max(f32x16& st, int kj, int kh, int qrow, int Tq, float mx) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int key = 32 * kj + mfma32_row(i, kh);
        const bool ok = (!CAUSAL || key <= qrow) && (key < Tq);
        st[i] = ok ? st[i] : -INFINITY;
        mx = fmaxf(mx, st[i]);
    }
    return mx;
}

// ---- scores -> unnormalised probabilities in place; returns sum + the lane's 16. Two forms, kept apart because their arithmetic differs and each
// kernel's bits are its own: attn_exp_sum is __expf(s - max) on scores of a PRE-SCALED q (k_attn_mfma, k_attn_x3); attn_exp2_sum is
// exp2(fma(s, qs2, nm)) with nm = -max qs2 on scores of an UNSCALED q, qs2 = log2(e) / sqrt(dh) (k_qkv_attn_long: the scale rides in the FMA)
__device__ __forceinline__ float attn_exp_sum(f32x16& st, float mx, float sum) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float e = __expf(st[i] - mx);
        st[i] = e;
        sum += e;
    }
    return sum;
}
__device__ __forceinline__ float attn_exp2_sum(f32x16& st, float qs2, float nm, float sum) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        st[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(st[i], qs2, nm));
        sum += st[i];
    }
    return sum;
}

// ---- O^T += V^T . P^T for key tile kj on the 16-bit V^T slab vt [DP][VLD]. P comes from the S^T registers in two runs of 8 keys (registers 8 step ..
// 8 step + 7 = keys kb .. kb + 3 and kb + 8 .. kb + 11, kb = 32 kj + 16 step + 4 kh), rounded to the operand format; V^T follows as two 8-byte halves at kb
// and kb + 8. (k_attn_x3 keeps the same step on (hi, lo) plane pairs, three MFMAs per product, in its own text: profiles/attn_refactor_resources.txt)
template <class OP, int VLD, int ND>
__device__ __forceinline__ void attn_pv_tile(f32x16 (&oa)[ND], const f32x16& st, const typename OP::t* vt, int kj, int l31, int kh) {
    typedef typename OP::v8 op8;
#pragma unroll
    for (int step = 0; step < 2; ++step) {
        op8 ph;
#pragma unroll
        for (int j = 0; j < 8; ++j) ph[j] = (typename OP::t)st[8 * step + j];
        const int kb = 32 * kj + 16 * step + 4 * kh;
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
            const int o = (32 * dt + l31) * VLD + kb;
            u32x4 vh;
            vh.lo = *reinterpret_cast<const u32x2*>(&vt[o]);
            vh.hi = *reinterpret_cast<const u32x2*>(&vt[o + 8]);
            oa[dt] = OP::mfma(__builtin_bit_cast(op8, vh), ph, oa[dt]);
        }
    }
}

// ---- O^T accumulators x inv -> this wave's fp32 patch [32 queries][LD]: the lane's query is row l31, register i of tile dt is dh 32 dt + C/D row
template <int LD, int ND>
__device__ __forceinline__ void attn_o_to_patch(float* patch, const f32x16 (&oa)[ND], float inv, int l31, int kh) {
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) patch[l31 * LD + 32 * dt + mfma32_row(i, kh)] = oa[dt][i] * inv;
}

// ---- patch read-back, row-contiguous: once the wave's patch writes have landed, f(q, c, v) for every query q = q0 + r < Tq of the tile and every
// group of 4 columns c .. c + 3 < DH, v = the four values
template <int DH, int LD, class F>
__device__ __forceinline__ void attn_patch_rows(const float* patch, int lane, int q0, int Tq, F&& f) {
    wait_lgkmcnt<0>();
    __builtin_amdgcn_wave_barrier();
    constexpr int C4 = DH / 4;
    for (int idx = lane; idx < 32 * C4; idx += 64) {
        const int r = idx / C4, c = (idx - r * C4) * 4;
        const int q = q0 + r;
        if (q < Tq) f(q, c, *reinterpret_cast<const f32x4*>(&patch[r * LD + c]));
    }
}
// ... and four consecutive columns of a row as split planes in the K32-blocked layout (they stay inside one 32-column block)
__device__ __forceinline__ void attn_store_split4(const Planes& op, size_t row, int col, f32x4 v) {
    const size_t o = plane_off(op.rows, row, col);
    bf16x4 h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        h[e] = (__bf16)v[e];
        l[e] = (__bf16)(v[e] - (float)h[e]);
    }
    *reinterpret_cast<bf16x4*>(op.hi + o) = h;
    if (op.lo) *reinterpret_cast<bf16x4*>(op.lo + o) = l;
}

}  // namespace
}  // namespace rgn
