// Self-attention as kernels of its own (the fused in_proj + attention kernels are rgn_qkv_attn.hip / rgn_qkv_attn_long.hip; k_layers has its own):
// causal (decoder layers, arch='online') or full (CAUSAL = false: encoder layers, arch='offline' - every wave visits every key tile, keys >= Tq
// stay masked). One workgroup per (sample, head) each.
//   k_attention   fp32 VALU, any head dim and sequence length that fits LDS: what is left when attn_tiles_supported says no
//   k_attn_mfma   fp32 operands on v_mfma_f32_32x32x2_f32 (precision f32), from the packed fp32 qkv rows
//   k_attn_x3     16-bit operands, split ("bf16x3": every product a.b of two fp32 quantities as ah.bh + ah.bl + al.bh, like the GEMMs) or plain, on
//                 v_mfma_f32_32x32x16_bf16, from the attention-ready planes (rgn_layout.h, layout 5) the in_proj GEMM epilogues emit
// The two MFMA kernels run the slab-staged scheme of rgn_attn.h: one wave per 32-query tile, everything transposed, K and V time-sharing one LDS slab,
// the result transposed through the dead slab. What each adds is its operand staging and its Q.K^T loop.
#include "rgn_internal.h"
#include "rgn_device.h"
#include "rgn_attn.h"

#include <hip/hip_runtime.h>
#include <math.h>

namespace rgn {

// =================================================================================================
// Causal self-attention, one workgroup per (sample, head). v1: fp32 VALU, K/V slab in LDS.
// Replaces nn.MultiheadAttention inside TransformerDecoderLayer._sa_block with the mask of
// generate_square_subsequent_mask (cmdm.py:168-171,220-227): softmax(q k^T / sqrt(dh) + causal) v.
// CAUSAL = false: TransformerEncoderLayer._sa_block without a mask (arch='offline', cmdm.py:237): every query sees all Tq keys.
// =================================================================================================
template <bool CAUSAL = true>
__global__ __launch_bounds__(256) void k_attention(const float* __restrict__ qkv, float* __restrict__ out, Planes op, Dims dm) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.x, hd = blockIdx.y;
    const int Tq = dm.Tq, dh = dm.dh, d = dm.d, ldk = dh + 1;
    float* Ks = smem;                       // [Tq][dh+1]
    float* Vs = Ks + Tq * ldk;              // [Tq][dh+1]
    float* qs = Vs + Tq * ldk;              // [4][dh]
    float* ps = qs + 4 * dh;                // [4][Tq]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row0 = (size_t)b * Tq;
    for (int idx = tid; idx < Tq * dh; idx += 256) {
        const int j = idx / dh, c = idx - j * dh;
        const float* base = qkv + (row0 + j) * (size_t)(3 * d) + hd * dh + c;
        Ks[j * ldk + c] = base[d];
        Vs[j * ldk + c] = base[2 * d];
    }
    __syncthreads();
    const float scale = 1.0f / sqrtf((float)dh);
    float* q = qs + wave * dh;
    float* p = ps + wave * Tq;
    for (int i0 = 0; i0 < Tq; i0 += 4) {   // uniform trip count: block barriers order the LDS hand-offs
        const int i = i0 + wave;
        const bool on = i < Tq;
        if (on)
            for (int c = lane; c < dh; c += 64) q[c] = qkv[(row0 + i) * (size_t)(3 * d) + hd * dh + c] * scale;
        __syncthreads();
        float inv = 0.f;
        const int jl = CAUSAL ? i : Tq - 1;   // last visible key
        if (on) {
            float mx = -INFINITY;
            for (int j = lane; j <= jl; j += 64) {
                float s = 0.f;
                const float* kr = Ks + j * ldk;
                for (int c = 0; c < dh; ++c) s = fmaf(q[c], kr[c], s);
                p[j] = s;
                mx = fmaxf(mx, s);
            }
            mx = wave_max_shfl(mx);
            float sum = 0.f;
            for (int j = lane; j <= jl; j += 64) {
                const float e = __expf(p[j] - mx);
                p[j] = e;
                sum += e;
            }
            inv = 1.0f / wave_sum_shfl(sum);
        }
        __syncthreads();
        if (on)
            for (int c = lane; c < dh; c += 64) {
                float o = 0.f;
                for (int j = 0; j <= jl; ++j) o = fmaf(p[j], Vs[j * ldk + c], o);
                if (out) out[(row0 + i) * (size_t)d + hd * dh + c] = o * inv;
                if (op.hi) plane_put(op, (int)(row0 + i), hd * dh + c, o * inv);
            }
        __syncthreads();
    }
}

// -------------------------------------------------------------------------------------------------
// MFMA attention on fp32 operands (v_mfma_f32_32x32x2_f32, exact fp32 products): A = K tile from LDS, B = Q held in registers (pre-scaled by
// 1/sqrt(dh)); P.V takes the S^T accumulator registers as they are, A = V from LDS, one key per MFMA.
// K and V time-share one LDS slab [32*NT][DH+4] (pad 4 floats: the 16 lanes of a ds_read_b128 group land on 16 different bank quads); a wave's output
// patch is the slab rows of its own queries. Causality: wave w only visits key tiles 0..w; the diagonal tile is masked.
// -------------------------------------------------------------------------------------------------
template <int NT, int DH, bool CAUSAL = true>
__global__ __launch_bounds__(64 * NT) void k_attn_mfma(const float* __restrict__ qkv, float* __restrict__ out, Planes op, Dims dm) {
    using S = AttnSlab<NT, DH>;
    constexpr int DP = S::DP, ND = S::ND;
    constexpr int LD = S::OLD;
    constexpr int NC = DH / 8;                    // 8-wide contraction chunks of QK^T
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* slab = smem;                           // [32*NT][LD]
    const int b = blockIdx.x, hd = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int Tq = dm.Tq, d = dm.d;
    const size_t row0 = (size_t)b * Tq;
    const float* qbase = qkv + row0 * (size_t)(3 * d) + hd * DH;

    auto load_slab = [&](int which) {             // which: 1 = K, 2 = V
        constexpr int C4 = DP / 4;
        for (int idx = tid; idx < 32 * NT * C4; idx += 64 * NT) {
            const int r = idx / C4, c = (idx - r * C4) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (r < Tq && c < DH) v = *reinterpret_cast<const f32x4*>(qbase + (size_t)r * (3 * d) + which * d + c);
            *reinterpret_cast<f32x4*>(&slab[r * LD + c]) = v;
        }
    };
    load_slab(1);
    // Q fragments: lane (query, half) holds Q[query][8c + 4*half + 0..3], scaled
    const float scale = 1.0f / sqrtf((float)DH);
    const int qrow = 32 * w + l31;
    f32x4 qf[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (qrow < Tq) v = *reinterpret_cast<const f32x4*>(qbase + (size_t)qrow * (3 * d) + 8 * c + 4 * half);
        qf[c] = v * scale;
    }
    __syncthreads();
    f32x16 st[NT];
#pragma unroll
    for (int kj = 0; kj < NT; ++kj) {
#pragma unroll
        for (int i = 0; i < 16; ++i) st[kj][i] = 0.f;
        if (!CAUSAL || kj <= w) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const f32x4 kf = *reinterpret_cast<const f32x4*>(&slab[(32 * kj + l31) * LD + 8 * c + 4 * half]);
#pragma unroll
                for (int j = 0; j < 4; ++j) st[kj] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[j], qf[c][j], st[kj], 0, 0, 0);
            }
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kj = 0; kj < NT; ++kj)
        if (!CAUSAL || kj <= w) mx = attn_mask_max<CAUSAL>(st[kj], kj, half, qrow, Tq, mx);
    mx = half_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int kj = 0; kj < NT; ++kj)
        if (!CAUSAL || kj <= w) sum = attn_exp_sum(st[kj], mx, sum);
    sum = half_sum(sum);
    const float inv = 1.0f / sum;
    __syncthreads();          // every wave is done with K
    load_slab(2);
    __syncthreads();
    f32x16 oa[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) oa[dt][i] = 0.f;
#pragma unroll
    for (int kj = 0; kj < NT; ++kj) {
        if (!CAUSAL || kj <= w) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = 32 * kj + mfma32_row(i, half);   // the key this lane's P register belongs to
                const float* vr = &slab[key * LD + l31];
#pragma unroll
                for (int dt = 0; dt < ND; ++dt)
                    oa[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[32 * dt], st[kj][i], oa[dt], 0, 0, 0);
            }
        }
    }
    __syncthreads();          // every wave is done with V: reuse the slab rows of this wave's queries
    float* patch = slab + w * S::PATCH;
    attn_o_to_patch<LD>(patch, oa, inv, l31, half);
    attn_patch_rows<DH, LD>(patch, lane, 32 * w, Tq, [&](int q, int c, f32x4 v) {
        if (out) *reinterpret_cast<f32x4*>(out + (row0 + q) * (size_t)d + hd * DH + c) = v;
        if (op.hi) attn_store_split4(op, row0 + q, hd * DH + c, v);
    });
}

// -------------------------------------------------------------------------------------------------
// MFMA attention on 16-bit operands from the attention-ready planes: A = K tile (LDS, rows padded to dh+8: conflict-free ds_read_b128), B = Q fragments
// loaded once from HBM into registers (pre-scaled by 1/sqrt(dh)); P.V on the V^T slab (attn_pv_tile): v is transposed on its way into LDS (two keys packed
// per 4-byte ds_write, lanes along keys: conflict-free). K and V^T time-share the LDS slab. The result is written as split planes in the K32-blocked
// layout the out_proj GEMM consumes.
// -------------------------------------------------------------------------------------------------
template <int NT, int DH, bool X3, bool CAUSAL = true>
__global__ __launch_bounds__(64 * NT) void k_attn_x3(AttnX3Args a) {
    using S = AttnSlab<NT, DH>;
    constexpr int DP = S::DP, NS = S::NS, ND = S::ND, TQP = S::TQP, KLD = S::KLD, VLD = S::VLD, PLANE = S::PLANE;
    extern __shared__ __attribute__((aligned(16))) char slab_x3[];
    __bf16* sh = reinterpret_cast<__bf16*>(slab_x3);  // [2 planes][PLANE]
    // XCD-affine mapping (block id -> XCD id%8): every XCD gets one contiguous range of samples, matching the row ranges
    // the in_proj / out_proj GEMM tiles occupy on that XCD
    const int vid = xcd_affine(blockIdx.x, gridDim.x);
    const int b = vid / a.H, hd = vid - b * a.H;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kh = lane >> 5, l31 = lane & 31;
    const int Tq = a.Tq;
    // this (sample, head)'s slab of the attention-ready planes: slab * Tqp * DH = attn_slab_base(H, Tqp, DH, b, hd), and below
    // (slab * Tqp + qrow) * DH + 8 kh = attn_slab_off(H, Tqp, DH, b, hd, qrow, 8 kh) of rgn_layout.h, spelled out (the register allocation moves
    // with the calls: profiles/attn_refactor_resources.txt)
    const size_t slab = (size_t)b * a.H + hd;
    const __bf16* gK[2] = {a.Khi + slab * a.Tqp * DH, a.Klo + (X3 ? slab * a.Tqp * DH : 0)};
    const __bf16* gV[2] = {a.Vthi + slab * a.Tqp * DH, a.Vtlo + (X3 ? slab * a.Tqp * DH : 0)};
    constexpr int NPL = X3 ? 2 : 1;

    // ---- K -> LDS (rows >= Tq read as zero)
    for (int p = 0; p < NPL; ++p)
        for (int idx = tid; idx < TQP * (DH / 8); idx += 64 * NT) {
            const int r = idx / (DH / 8), c = (idx - r * (DH / 8)) * 8;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (r < Tq) v = *reinterpret_cast<const u32x4*>(gK[p] + (size_t)r * DH + c);
            *reinterpret_cast<u32x4*>(&sh[p * PLANE + r * KLD + c]) = v;
        }
    // ---- Q fragments: lane (query, kh) holds q[query][16 s + 8 kh .. +7] for every k16 step s
    const int qrow = 32 * w + l31;
    bf16x8 qh[NS], ql[NS];
    {
        const __bf16* gq = a.Qhi + (slab * a.Tqp + qrow) * DH + 8 * kh;
        const __bf16* gl = a.Qlo + (X3 ? (slab * a.Tqp + qrow) * DH + 8 * kh : 0);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            u32x4 z = {0u, 0u, 0u, 0u};
            u32x4 vh = z, vl = z;
            if (qrow < Tq) {
                vh = *reinterpret_cast<const u32x4*>(gq + 16 * s);
                if (X3) vl = *reinterpret_cast<const u32x4*>(gl + 16 * s);
            }
            qh[s] = __builtin_bit_cast(bf16x8, vh);
            ql[s] = __builtin_bit_cast(bf16x8, vl);
        }
    }
    // ---- V rows -> registers now (two keys x 8 dh per item): their global round trip overlaps the K staging and the S^T
    //      phase instead of following the softmax; they go to LDS (transposed) once every wave is done with K
    //      (sequences of up to 64 tokens only: the latency-bound small launches; at 150 tokens the kernel is HBM-bound and
    //      the 32-64 extra live VGPRs cost more occupancy than the overlap returns: 27.3 -> 28.8 us at B=128)
    constexpr int V_IT = ((TQP / 2) * (DH / 8) + 64 * NT - 1) / (64 * NT);
    constexpr bool V_EARLY = NT <= 2;
    u32x4 vreg[NPL][V_IT][2];
    auto load_v = [&] {
#pragma unroll
    for (int p = 0; p < NPL; ++p)
#pragma unroll
        for (int it = 0; it < V_IT; ++it) {
            const int idx = tid + it * 64 * NT;
            const int kp = idx % (TQP / 2), c = (idx / (TQP / 2)) * 8, k0 = 2 * kp;
            const bool in = idx < (TQP / 2) * (DH / 8);
            u32x4 v0 = {0u, 0u, 0u, 0u}, v1 = {0u, 0u, 0u, 0u};
            if (in && k0 < Tq) v0 = *reinterpret_cast<const u32x4*>(gV[p] + (size_t)k0 * DH + c);
            if (in && k0 + 1 < Tq) v1 = *reinterpret_cast<const u32x4*>(gV[p] + (size_t)(k0 + 1) * DH + c);
            vreg[p][it][0] = v0;
            vreg[p][it][1] = v1;
        }
    };
    if constexpr (V_EARLY) load_v();
    __syncthreads();
    f32x16 st[NT];
#pragma unroll
    for (int kj = 0; kj < NT; ++kj) {
#pragma unroll
        for (int i = 0; i < 16; ++i) st[kj][i] = 0.f;
        if (!CAUSAL || kj <= w) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int o = (32 * kj + l31) * KLD + 16 * s + 8 * kh;
                const bf16x8 kfh = *reinterpret_cast<const bf16x8*>(&sh[o]);
                if (X3) {
                    const bf16x8 kfl = *reinterpret_cast<const bf16x8*>(&sh[PLANE + o]);
                    st[kj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfl, qh[s], st[kj], 0, 0, 0);
                    st[kj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfh, ql[s], st[kj], 0, 0, 0);
                }
                st[kj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfh, qh[s], st[kj], 0, 0, 0);
            }
        }
    }
    // ---- softmax over keys. The mask + maximum is attn_mask_max<CAUSAL>(st[kj], kj, kh, qrow, Tq, mx) of rgn_attn.h spelled out: through the call
    //      one extractelement lands elsewhere in the IR and the register allocation moves (profiles/attn_refactor_resources.txt)
    float mx = -INFINITY;
#pragma unroll
    for (int kj = 0; kj < NT; ++kj)
        if (!CAUSAL || kj <= w) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = 32 * kj + mfma32_row(i, kh);
                const bool ok = (!CAUSAL || key <= qrow) && (key < Tq);
                st[kj][i] = ok ? st[kj][i] : -INFINITY;
                mx = fmaxf(mx, st[kj][i]);
            }
        }
    mx = half_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int kj = 0; kj < NT; ++kj)
        if (!CAUSAL || kj <= w) sum = attn_exp_sum(st[kj], mx, sum);
    sum = half_sum(sum);
    const float inv = 1.0f / sum;
    __syncthreads();          // every wave is done with K
    // ---- V -> LDS transposed: Vt[dh][key] (row stride VLD); lanes run along key PAIRS so each ds_write_b32 packs
    //      (key, key+1) of one dh column and a wave's writes fall on consecutive banks. Keys >= Tq read as zero.
    if (DP > DH) {   // zero the dh padding rows (DH = 16 only)
        for (int idx = tid; idx < NPL * (DP - DH) * VLD / 2; idx += 64 * NT) {
            const int p = idx / ((DP - DH) * VLD / 2), o = idx - p * ((DP - DH) * VLD / 2);
            reinterpret_cast<unsigned int*>(&sh[p * PLANE + DH * VLD])[o] = 0u;
        }
    }
    if constexpr (!V_EARLY) load_v();
#pragma unroll
    for (int p = 0; p < NPL; ++p)
#pragma unroll
        for (int it = 0; it < V_IT; ++it) {
            const int idx = tid + it * 64 * NT;
            if (idx >= (TQP / 2) * (DH / 8)) continue;
            const int kp = idx % (TQP / 2), c = (idx / (TQP / 2)) * 8;
            const int k0 = 2 * kp;
            const u32x4 v0 = vreg[p][it][0], v1 = vreg[p][it][1];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned int e0 = (v0[j >> 1] >> (16 * (j & 1))) & 0xffffu;
                const unsigned int e1 = (v1[j >> 1] >> (16 * (j & 1))) & 0xffffu;
                *reinterpret_cast<unsigned int*>(&sh[p * PLANE + (c + j) * VLD + k0]) = e0 | (e1 << 16);
            }
        }
    __syncthreads();
    f32x16 oa[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) oa[dt][i] = 0.f;
    // (the P.V step of attn_pv_tile (rgn_attn.h) on (hi, lo) plane pairs, in this kernel's own text: through a shared call the V^T addresses are formed
    //  in another order and the instantiations at dh 16 / 32 change their register class: profiles/attn_refactor_resources.txt)
#pragma unroll
    for (int kj = 0; kj < NT; ++kj) {
        if (!CAUSAL || kj <= w) {
#pragma unroll
            for (int step = 0; step < 2; ++step) {
                bf16x8 ph, pl;     // B operand: this lane's 8 keys = registers 8*step .. 8*step+7
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float x = st[kj][8 * step + j];
                    ph[j] = (__bf16)x;
                    pl[j] = (__bf16)(x - (float)ph[j]);
                }
                const int kb = 32 * kj + 16 * step + 4 * kh;      // keys kb..kb+3 and kb+8..kb+11
#pragma unroll
                for (int dt = 0; dt < ND; ++dt) {
                    const int o = (32 * dt + l31) * VLD + kb;
                    u32x4 vh;
                    vh.lo = *reinterpret_cast<const u32x2*>(&sh[o]);
                    vh.hi = *reinterpret_cast<const u32x2*>(&sh[o + 8]);
                    const bf16x8 vfh = __builtin_bit_cast(bf16x8, vh);
                    if (X3) {
                        u32x4 vl;
                        vl.lo = *reinterpret_cast<const u32x2*>(&sh[PLANE + o]);
                        vl.hi = *reinterpret_cast<const u32x2*>(&sh[PLANE + o + 8]);
                        const bf16x8 vfl = __builtin_bit_cast(bf16x8, vl);
                        oa[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfl, ph, oa[dt], 0, 0, 0);
                        oa[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfh, pl, oa[dt], 0, 0, 0);
                    }
                    oa[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfh, ph, oa[dt], 0, 0, 0);
                }
            }
        }
    }
    __syncthreads();          // every wave is done with V^T: reuse the slab as this wave's private fp32 patch
    float* patch = reinterpret_cast<float*>(slab_x3) + w * S::PATCH;
    attn_o_to_patch<S::OLD>(patch, oa, inv, l31, kh);
    const size_t row0 = (size_t)b * Tq;
    attn_patch_rows<DH, S::OLD>(patch, lane, 32 * w, Tq, [&](int q, int c, f32x4 v) { attn_store_split4(a.out, row0 + q, hd * DH + c, v); });
}

// ---- launchers. (Tq, dh) -> (NT, DH): attn_tiles is the one place that names the instantiation set, NT = ceil(Tq / 32) in 1 .. 5 x DH in 16 / 32 / 64 /
// 128. It returns f(std::integral_constant<int, NT>{}, std::integral_constant<int, DH>{}), hipErrorInvalidValue outside the set; dispatch_bools
// (rgn_device.h) adds a kernel's bool forms. The predicate is the dispatch asked whether it has a case
template <class F>
static hipError_t attn_tiles(int Tq, int dh, F&& f) {
    auto tiles = [&](auto DH) {
        switch ((Tq + 31) / 32) {
            case 1: return f(std::integral_constant<int, 1>{}, DH);
            case 2: return f(std::integral_constant<int, 2>{}, DH);
            case 3: return f(std::integral_constant<int, 3>{}, DH);
            case 4: return f(std::integral_constant<int, 4>{}, DH);
            case 5: return f(std::integral_constant<int, 5>{}, DH);
        }
        return hipErrorInvalidValue;
    };
    switch (dh) {
        case 16: return tiles(std::integral_constant<int, 16>{});
        case 32: return tiles(std::integral_constant<int, 32>{});
        case 64: return tiles(std::integral_constant<int, 64>{});
        case 128: return tiles(std::integral_constant<int, 128>{});
    }
    return hipErrorInvalidValue;
}
bool attn_tiles_supported(int Tq, int dh) {
    return attn_tiles(Tq, dh, [](auto, auto) { return hipSuccess; }) == hipSuccess;
}

// a.x3 picks the arithmetic of a launch; configure (called once at finalize, never during graph capture) allows both forms' dynamic LDS
static hipError_t attn_x3_go(const AttnX3Args& a, hipStream_t s, bool causal, bool x3, bool configure_only) {
    return attn_tiles(a.Tq, a.dh, [&](auto NT, auto DH) {
        return dispatch_bools([&](auto X3, auto CAUSAL) {
            constexpr int nt = decltype(NT)::value, dh = decltype(DH)::value;
            constexpr size_t lds = AttnSlab<nt, dh>::LDS16;
            auto* k = k_attn_x3<nt, dh, decltype(X3)::value, decltype(CAUSAL)::value>;
            if (configure_only) return hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(k, dim3(a.Bm * a.H), dim3(64 * nt), lds, s, a);
            return hipGetLastError();
        }, x3, causal);
    });
}
hipError_t configure_attn_x3(int Tq, int dh) {
    AttnX3Args a{};
    a.Tq = Tq;
    a.dh = dh;
    for (bool causal : {true, false})
        for (bool x3 : {true, false}) {
            hipError_t e = attn_x3_go(a, nullptr, causal, x3, true);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}
hipError_t launch_attn_x3(const AttnX3Args& a, hipStream_t s, bool causal) { return attn_x3_go(a, s, causal, a.x3, false); }

static hipError_t attn_mfma_go(const float* qkv, float* out, Planes op, const Dims& dm, hipStream_t s, bool causal, bool configure_only) {
    return attn_tiles(dm.Tq, dm.dh, [&](auto NT, auto DH) {
        return dispatch_bools([&](auto CAUSAL) {
            constexpr int nt = decltype(NT)::value, dh = decltype(DH)::value;
            constexpr size_t lds = AttnSlab<nt, dh>::LDS32;
            auto* k = k_attn_mfma<nt, dh, decltype(CAUSAL)::value>;
            if (configure_only) return hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(k, dim3(dm.Bm, dm.H), dim3(64 * nt), lds, s, qkv, out, op, dm);
            return hipGetLastError();
        }, causal);
    });
}
static size_t attn_lds_bytes(int Tq, int dh) { return ((size_t)2 * Tq * (dh + 1) + 4 * dh + 4 * Tq) * sizeof(float); }
// Called once at finalize (never during graph capture): allow > 64 KiB of dynamic LDS (both the causal and the full form).
hipError_t configure_attention(int Tq, int dh) {
    if (attn_tiles_supported(Tq, dh)) {
        Dims dm{};
        dm.Tq = Tq;
        dm.dh = dh;
        hipError_t e = attn_mfma_go(nullptr, nullptr, Planes{nullptr, nullptr, 0}, dm, nullptr, true, true);
        return e != hipSuccess ? e : attn_mfma_go(nullptr, nullptr, Planes{nullptr, nullptr, 0}, dm, nullptr, false, true);
    }
    const size_t lds = attn_lds_bytes(Tq, dh);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_attention<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return e != hipSuccess ? e : hipFuncSetAttribute(reinterpret_cast<const void*>(k_attention<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}
hipError_t launch_attention(const float* qkv, float* out, Planes op, const Dims& dm, hipStream_t s, bool causal) {
    if (attn_tiles_supported(dm.Tq, dm.dh)) return attn_mfma_go(qkv, out, op, dm, s, causal, false);
    if (causal) hipLaunchKernelGGL(k_attention<true>, dim3(dm.Bm, dm.H), dim3(256), attn_lds_bytes(dm.Tq, dm.dh), s, qkv, out, op, dm);
    else hipLaunchKernelGGL(k_attention<false>, dim3(dm.Bm, dm.H), dim3(256), attn_lds_bytes(dm.Tq, dm.dh), s, qkv, out, op, dm);
    return hipGetLastError();
}

}  // namespace rgn
