// The decoder-layer tail of the plain 16-bit phase, defined once for the kernels that run it: k_mlp2 (rgn_mlp2.hip: a tile of 64 token rows, att and
// residual planes in, planes out) and k_layers (rgn_layers.hip: one sample's resident images). What is shared is the machinery - the accumulator <->
// image map, the weight ring and its GEMM pass, the single-exchange LayerNorm, the epilogue sweeps and the whole FFN stage (linear1, GELU, linear2);
// where the activations come from and go to (stages 1 and 3) stays with each kernel, composed from these pieces. Device code, internal linkage.
//
// A workgroup holds R = 32 MT token rows, wave w the output columns [CW w, CW w + CW), CW = 32 NT: MT x NT accumulator tiles of 32 x 32.
//   element (token 32 mt + l31, column CW wave + 32 nt + 8 i4 + 4 kh + e)  <->  register acc[nt][mt][4 i4 + e]         (l31 = lane & 31, kh = lane >> 5)
// An activation image is the swizzled LDS operand image of rgn_layout.h, [K / 32 k-blocks][R rows][64 B]; the weights are its fragment-ordered plane.
// The constants struct C of a kernel names MT, NT, NW (waves), R, RD (ring depth in granules), KB (bytes of a k-block) and RED / REDF (byte offset of
// the statistics exchange in LDS / floats of one of its two buffers, each [2 stats][NW waves][R tokens]).
#pragma once
#include "rgn_device.h"

namespace rgn {
namespace {

// What a lane knows about its place, made ONCE at the head of the kernel (tail_lane) and handed to every function below, which never forms these
// values from threadIdx again: the three LDS bases are opaque registers + immediates - left to itself the compiler forms every address with v_or
// into a register of its own and keeps them all alive across the kernel (k_layers: across the layer and step loops, spilled).
struct TailLane {
    char* smem;
    int lane16, wave, kh, swz;
    int img_base;    // this lane's 8-byte run of (nt, mt, i4) = 0 inside an image, before the swizzle
    int red_base;    // exchange writes: token l31
    int red_base2;   // post-barrier exchange reads: lane (l31, kh) reduces token 32 kh + l31
};
template <class C>
__device__ __forceinline__ TailLane tail_lane(char* smem, int lane, int wave) {
    const int l31 = lane & 31, kh = lane >> 5;
    int img_base = (C::NT * wave) * C::KB + l31 * 64 + 8 * kh;
    asm volatile("" : "+v"(img_base));
    int red_base = C::RED + 4 * l31;
    asm volatile("" : "+v"(red_base));
    int red_base2 = red_base + 128 * kh;
    asm volatile("" : "+v"(red_base2));
    return TailLane{smem, lane * 16, wave, kh, img_swz(l31), img_base, red_base, red_base2};
}

// ---- tile geometry
// B-operand fragment of token l31 (+ 32 mt: an immediate offset of 2 KiB) inside a k-block of the image at byte offset 0, per 16-wide k-half;
// an image past the first 64 KiB wants base registers of its own (16-bit ds_read offsets): the same offsets moved on by img bytes
__device__ __forceinline__ void tail_a_off(int (&a)[2], int lane) {
    const int l31 = lane & 31, kh = lane >> 5;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) a[ks] = img_frag(l31, ks, kh);
}
__device__ __forceinline__ void tail_a_off(int (&a)[2], const int (&a0)[2], int img) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) a[ks] = a0[ks] + img;
}
__device__ __forceinline__ int tail_col4(const TailLane& t, int nt, int i4) { return 32 * nt + 8 * i4 + 4 * t.kh; }   // inside the wave's column slice
// the 8-byte run of (nt, i4, mt) inside the image at byte offset img: one address register per i4, (nt, mt) an immediate offset of the access
template <class OP, class C>
__device__ __forceinline__ typename OP::v4* tail_img_run(const TailLane& t, int img, int nt, int i4, int mt) {
    return reinterpret_cast<typename OP::v4*>(t.smem + (img + t.img_base + img_slot(i4, t.swz)) + (nt * C::KB + mt * 2048));
}

// ---- weight ring: granule = half a k-step (16 k) of this wave's NT column blocks; W: fragment-ordered plane [K/32][nb_all][2][64][8]
//      (rgn_layout.h). Granule index hs = 2 kt + ks (frag_granule). Buffer loads: the resource (based at the wave's first column block cb0) is scalar and
//      every granule offset a compile-time constant, the lane contributes lane * 16
struct TailPass { __amdgpu_buffer_rsrc_t rs; int kstride, hs0; };   // kstride = nb_all * 2048 bytes per k-block
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tail_wrs(const __bf16* W, int cb0, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(W) + (size_t)cb0 * 1024, 0, bytes - cb0 * 2048, 0x00020000);
}
template <class OP, class C>
__device__ __forceinline__ void tail_load_g(typename OP::v8 (&wf)[C::RD][C::NT], const TailLane& t, const TailPass& ps, int hs_rel, int slot) {
    const int hs = ps.hs0 + hs_rel;
    // (the granule offset is materialised by a volatile s_mov right here: as plain literals the offsets of a layer are hoisted out of k_layers'
    // layer loop as loop invariants and live in spilled SGPRs. k_mlp2 has no such loop: with the s_mov it needs 57 SGPRs where plain literals took 106, its VGPRs the same)
    int soff;
    asm volatile("s_mov_b32 %0, %1" : "=s"(soff) : "i"(frag_granule(hs, ps.kstride)));
#pragma unroll
    for (int nt = 0; nt < C::NT; ++nt)
        wf[slot][nt] = __builtin_bit_cast(typename OP::v8, __builtin_amdgcn_raw_buffer_load_b128(ps.rs, t.lane16, soff + nt * 2048, 0));
}
// one GEMM pass over K = 16 NG: acc[nt][mt] += A_image(NG / 2 k-blocks at the byte offsets aoff) . W[the wave's column blocks, granules hs0 .. hs0 + NG - 1]^T.
// The ring never drains between passes: the tail of a pass requests the first RD - 1 granules of the NEXT pass (CH), so the epilogues run with the
// next pass's first fragments in flight. EX: vector-memory operations issued between the granules RD - 2 and RD - 1 of this pass that may stay
// in flight (the caller's count: its residual tile, per-column vectors, ...)
template <class OP, class C, int NG, bool CH, int EX>
__device__ __forceinline__ void tail_gemm(f32x16 (&acc)[C::NT][C::MT], typename OP::v8 (&wf)[C::RD][C::NT], const TailLane& t, const int (&aoff)[2],
                                          const TailPass& cur, const TailPass& nxt) {
    using op8 = typename OP::v8;
    constexpr int MT = C::MT, NT = C::NT, RD = C::RD, AH = RD - 1;
    __builtin_amdgcn_sched_barrier(0);
    op8 af[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) af[mt] = *reinterpret_cast<const op8*>(t.smem + aoff[0] + mt * 2048);
#pragma unroll
    for (int hs = 0; hs < NG; ++hs) {
        op8 afn[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            afn[mt] = af[mt];
            if (hs + 1 < NG) afn[mt] = *reinterpret_cast<const op8*>(t.smem + ((hs + 1) >> 1) * C::KB + aoff[(hs + 1) & 1] + mt * 2048);   // one granule ahead
        }
        if (hs + AH < NG) tail_load_g<OP, C>(wf, t, cur, hs + AH, (hs + AH) % RD);
        else if (CH) tail_load_g<OP, C>(wf, t, nxt, hs + AH - NG, (hs + AH) % RD);
        if (hs + AH < NG || CH) {
            if (hs < AH) wait_vmcnt<NT * AH + EX>();
            else wait_vmcnt<NT * AH>();   // this granule is in; the next RD - 1 stay in flight
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[nt][mt] = OP::mfma(wf[hs % RD][nt], af[mt], acc[nt][mt]);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[mt] = afn[mt];
    }
    __builtin_amdgcn_sched_barrier(0);
}

// ---- epilogue pieces
template <class C>
__device__ __forceinline__ void tail_init_bias(f32x16 (&acc)[C::NT][C::MT], const TailLane& t, const float* bias) {   // bias: the wave's column slice in LDS
#pragma unroll
    for (int nt = 0; nt < C::NT; ++nt)
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(bias + tail_col4(t, nt, i4));
#pragma unroll
            for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[nt][mt][4 * i4 + e] = b[e];
        }
}
// LayerNorm over the 512 columns of every token, in place: o = v (rstd gamma) + (shift - mean rstd gamma). One exchange of (sum, sum of
// squares) in fp32: halves by lane ^ 32, the NW column slices through LDS ([stat][wave][token], conflict-free both ways), mean folded into the
// final FMA. SLOT: two alternating buffers - a barrier separates each write from its reads. gam: the wave's column slice in LDS;
// shift(nt, i4, mt) -> f32x4: the additive vector of tile row block mt (per sample in k_mlp2, one sample in k_layers)
template <class C, int SLOT, class Shift>
__device__ __forceinline__ void tail_layernorm(f32x16 (&acc)[C::NT][C::MT], const TailLane& t, const float* gam, Shift shift) {
    constexpr int MT = C::MT, NT = C::NT, NW = C::NW, R = C::R;
    static_assert(MT == 2, "the two half_swaps hand over exactly two row tiles");
    const char* buf = t.smem + t.red_base + SLOT * C::REDF * 4;
    const char* buf2 = t.smem + t.red_base2 + SLOT * C::REDF * 4;
    const float invn = 1.0f / 512.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        f32x2 s2 = f32x2{0.f, 0.f}, q2 = f32x2{0.f, 0.f};
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 16; i += 2) {
                const f32x2 v = f32x2{acc[nt][mt][i], acc[nt][mt][i + 1]};
                s2 += v;
                q2 = __builtin_elementwise_fma(v, v, q2);
            }
        float s = s2[0] + s2[1], q = q2[0] + q2[1];
        half_swap(s, q);                                        // s = [s.lo | q.lo], q = [s.hi | q.hi]
        *reinterpret_cast<float*>(const_cast<char*>(buf) + (t.kh * (NW * R) + t.wave * R + 32 * mt) * 4) = s + q;   // kh = 0: the sum, kh = 1: the sum of squares
    }
    wait_lgkmcnt<0>();
    __builtin_amdgcn_s_barrier();
    f32x2 rs[MT], nm[MT];
    {   // the halves share the work - lane (l31, kh) reduces the NW partials of token 32 kh + l31, two swaps hand the results over
        float p[2][NW];
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int w = 0; w < NW; ++w) p[st][w] = *reinterpret_cast<const float*>(buf2 + (st * (NW * R) + w * R) * 4);
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int d = 1; d < NW; d *= 2)
#pragma unroll
                for (int w = 0; w < NW; w += 2 * d) p[st][w] += p[st][w + d];
        const float mean = p[0][0] * invn;
        const float var = __builtin_fmaxf(p[1][0] * invn - mean * mean, 0.f);
        float r0 = __builtin_amdgcn_rsqf(var + 1e-5f), n0 = -mean * r0;
        float r1 = r0, n1 = n0;
        asm volatile("" : "+v"(r1), "+v"(n1));               // (copies in registers of their own)
        half_swap(r0, r1);                                      // r0 = token l31's (tile 0), r1 = token 32 + l31's (tile 1), in every lane
        half_swap(n0, n1);
        rs[0] = f32x2{r0, r0}; rs[1] = f32x2{r1, r1};
        nm[0] = f32x2{n0, n0}; nm[1] = f32x2{n1, n1};
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        f32x4 ga[4], sh[4][MT];                                   // the LDS reads of a column block first, then the arithmetic
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4) {
            ga[i4] = *reinterpret_cast<const f32x4*>(gam + tail_col4(t, nt, i4));
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) sh[i4][mt] = shift(nt, i4, mt);
        }
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int e = 0; e < 4; e += 2) {
                    const f32x2 v = __builtin_elementwise_fma(f32x2{acc[nt][mt][4 * i4 + e], acc[nt][mt][4 * i4 + e + 1]}, rs[mt], nm[mt]);   // (v - mean) rstd
                    const f32x2 o = __builtin_elementwise_fma(v, f32x2{ga[i4][e], ga[i4][e + 1]}, f32x2{sh[i4][mt][e], sh[i4][mt][e + 1]});
                    acc[nt][mt][4 * i4 + e] = o[0];
                    acc[nt][mt][4 * i4 + e + 1] = o[1];
                }
    }
}
// the usual shift: one vector for every row, from the wave's column slice in LDS
__device__ __forceinline__ auto tail_rowvec(const TailLane& t, const float* v) {
    return [kh = t.kh, v](int nt, int i4, int) { return *reinterpret_cast<const f32x4*>(v + 32 * nt + 8 * i4 + 4 * kh); };
}

// acc -> the wave's own columns of the image at byte offset img, rounded to the operand format
template <class OP, class C>
__device__ __forceinline__ void tail_store_img(const f32x16 (&acc)[C::NT][C::MT], const TailLane& t, int img) {
#pragma unroll
    for (int nt = 0; nt < C::NT; ++nt)
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4)
#pragma unroll
            for (int mt = 0; mt < C::MT; ++mt) {
                typename OP::v4 h;
#pragma unroll
                for (int e = 0; e < 4; ++e) h[e] = (typename OP::t)acc[nt][mt][4 * i4 + e];
                *tail_img_run<OP, C>(t, img, nt, i4, mt) = h;
            }
}
// acc += the residual from the image at byte offset img (this wave's own columns): all the reads first, then the adds
template <class OP, class C>
__device__ __forceinline__ void tail_add_resid(f32x16 (&acc)[C::NT][C::MT], const TailLane& t, int img) {
    typename OP::v4 r[C::NT][C::MT][4];
#pragma unroll
    for (int nt = 0; nt < C::NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
            for (int i4 = 0; i4 < 4; ++i4) r[nt][mt][i4] = *tail_img_run<OP, C>(t, img, nt, i4, mt);
#pragma unroll
    for (int nt = 0; nt < C::NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
            for (int i4 = 0; i4 < 4; ++i4)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[nt][mt][4 * i4 + e] += (float)r[nt][mt][i4][e];
}
template <class C>
__device__ __forceinline__ void tail_gelu(f32x16 (&acc)[C::NT][C::MT]) {
#pragma unroll
    for (int nt = 0; nt < C::NT; ++nt)
#pragma unroll
        for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
            for (int i = 0; i < 16; i += 2) {
                const f32x2 gl = gelu2_p13(f32x2{acc[nt][mt][i], acc[nt][mt][i + 1]});
                acc[nt][mt][i] = gl[0];
                acc[nt][mt][i + 1] = gl[1];
            }
}

// ---- the FFN stage: acc2 = gelu( h' . W1^T + b1 ) . W2^T + b2, the hidden 1024 columns in two halves. h' is the complete image the offsets a_in
//      point into (a barrier behind its last store is the caller's); the GELU'd hidden halves go through the image at byte offset hid (a_hid: its
//      fragment offsets), which must be dead on entry. The four passes chain w1a -> w2a -> w1b -> w2b; the first RD - 1 granules of w1a are in
//      flight on entry (chained from the caller's last pass) and the ring is drained on exit. bf1: linear1's bias, the halves CW floats apart; bf2: linear2's
template <class OP, class C>
__device__ __forceinline__ void tail_ffn(f32x16 (&acc2)[C::NT][C::MT], typename OP::v8 (&wf)[C::RD][C::NT], const TailLane& t, const int (&a_in)[2],
                                         const int (&a_hid)[2], int hid, const TailPass& w1a, const TailPass& w1b, const TailPass& w2a, const TailPass& w2b,
                                         const float* bf1, const float* bf2) {
    f32x16 acc[C::NT][C::MT];
    tail_init_bias<C>(acc2, t, bf2);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        tail_init_bias<C>(acc, t, bf1 + 32 * C::NT * c);
        tail_gemm<OP, C, 32, true, 0>(acc, wf, t, a_in, c ? w1b : w1a, c ? w2b : w2a);   // hidden columns [512 c, 512 c + 512)
        tail_gelu<C>(acc);
        if (c == 1) __builtin_amdgcn_s_barrier();                 // every wave is done reading the first half's image
        tail_store_img<OP, C>(acc, t, hid);
        wait_lgkmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (c == 0) tail_gemm<OP, C, 32, true, 0>(acc2, wf, t, a_hid, w2a, w1b);         // linear2 over hidden k-blocks [16 c, 16 c + 16)
        else tail_gemm<OP, C, 32, false, 0>(acc2, wf, t, a_hid, w2b, w2b);
    }
}

}  // namespace
}  // namespace rgn
