// Z-buffer rasteriser: the frames the reference draws with pyrender on OSMesa (render/crendermotion.py:20-42, render/renderer.py:85-150), from the
// tensor rgn_rot2verts writes, [B, V, 3 P, T], to shaded RGB [B, T, H, W, 3] (and, on request, the depth and face-index buffers). The contract -
// camera, snapping, fill rule, depth key, normals, shading - is written once, in include/regennet_hip.h above rgn_render; tests/render_ref.py
// restates it in NumPy. Five launches on the caller's stream, nothing allocated, no global atomics:
//
//   k_rnd_centroid  one workgroup per motion: the mean of person 0's vertices in the first unmasked frame, summed in fp64 (the result, rounded to
//                   fp32, does not depend on the order of the sum in any case a test can construct); zeros when centring is off
//   k_rnd_project   one thread per (motion, person, vertex, frame), frames innermost as the input has them: centred position [frame][person][vertex]
//                   as float4 records and the snapped integer screen coordinates as int2 records - what a tile gathers from
//   k_rnd_normals   one thread per (frame, person, vertex): the cross products of the vertex's faces in ascending face order (CSR adjacency built
//                   at rgn_render_create: a gather, reproducible), normalised
//   k_rnd_bbox      one thread per (frame, person, face): the pixel box [x0, x1) x [y0, y1) whose centres the triangle can cover, empty for zero
//                   area, off-screen triangles and masked frames; a wave's 64 consecutive faces also leave the union of their boxes
//   k_rnd_raster    one workgroup per (frame, 64 x 64 pixel tile), the tile's 64-bit keys in 32 KB of LDS. A wave walks chunks of 64 faces: the
//                   chunk's union box against the tile (one scalar test skips 64 faces), then every lane its own face's box. A face that
//                   survives with at most 16 pixels of (its box ^ the tile) is rasterised by its own lane, 64 faces side by side; a larger one by
//                   the whole wave, one face after the other; the minimum is taken with LDS 64-bit atomics either way. After a
//                   barrier the same workgroup decodes each pixel's winner, recomputes its barycentrics, shades and stores: a wave covers one
//                   192-byte run of a tile row with three byte stores a lane. The image is written once and never read.
//
// Triangle -> tile assignment is the bounding-box rejection loop of the issue's two choices, made two-level by the chunk boxes; a binning pass
// (count, prefix, fill) was not built or measured. Bounds: no pixel index is derived from a coordinate without a clamp to the tile, every face
// index is checked at create time, every record index is 64-bit.
#include "../../include/regennet_hip.h"
#include "rgn_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

namespace {

constexpr int RND_MAX_V = 65536, RND_MAX_WH = 4096;
constexpr int RND_TILE = 64, RND_THREADS = 256, RND_WAVES = RND_THREADS / 64;
constexpr int RND_SNAP = 256, RND_CLAMP = 1 << 20;      // 1/256 pixel; |snapped coordinate| <= 2^20
constexpr unsigned long long RND_EMPTY = ~0ull;
constexpr int RND_SMALL = 16;                            // pixels of (box ^ tile) up to which a lane rasterises its face alone
constexpr long long RND_MAX_BLOCKS = (1ll << 24) - 1;   // (blocks x 256 threads stays below 2^32)

struct RndBox {                                         // pixel box [x0, x1) x [y0, y1), fields in [0, 4096]; empty: x0 = y0 = 4096, x1 = y1 = 0
    uint32_t lo, hi;                                    // lo = x0 | y0 << 16, hi = x1 | y1 << 16
};
struct RndShade {
    float col[RGN_RENDER_MAX_PERSONS][3];
    uint8_t bg[4];
};
struct RndWork {                                        // byte offsets into the workspace, each a multiple of 16
    uint64_t ctr, pos, nrm, scr, box, cbox, bytes;
};

__device__ __forceinline__ bool box_hits(RndBox b, int tx0, int ty0, int tx1, int ty1) {
    const int x0 = b.lo & 0xffff, y0 = b.lo >> 16, x1 = b.hi & 0xffff, y1 = b.hi >> 16;
    return x0 < tx1 && x1 > tx0 && y0 < ty1 && y1 > ty0;
}

// A triangle on the snapped integer grid, wound to positive area (two-sided: negative area swaps b and c). e0 + e1 + e2 = area.
struct RndTri {
    int ax, ay, bx, by, cx, cy;
    long long area;
    bool swapped;
};
__device__ __forceinline__ long long rnd_edge(int ax, int ay, int bx, int by, int px, int py) {   // of the edge a -> b at p; operands below 2^22
    return (long long)(bx - ax) * (py - ay) - (long long)(by - ay) * (px - ax);
}
__device__ __forceinline__ bool rnd_setup(int2 a, int2 b, int2 c, RndTri& t) {
    long long area = rnd_edge(a.x, a.y, b.x, b.y, c.x, c.y);
    t.swapped = area < 0;
    if (t.swapped) {
        const int2 s = b;
        b = c;
        c = s;
        area = -area;
    }
    t.ax = a.x, t.ay = a.y, t.bx = b.x, t.by = b.y, t.cx = c.x, t.cy = c.y, t.area = area;
    return area != 0;
}
// top-left rule: a pixel centre ON the edge a -> b belongs to the triangle iff the edge is a left edge (dy < 0) or a top edge (dy == 0, dx > 0)
__device__ __forceinline__ bool rnd_owns(int ax, int ay, int bx, int by) { return by - ay < 0 || (by == ay && bx - ax > 0); }
__device__ __forceinline__ void rnd_edges(const RndTri& t, int px, int py, long long& e0, long long& e1, long long& e2) {
    e0 = rnd_edge(t.bx, t.by, t.cx, t.cy, px, py);      // weight of a
    e1 = rnd_edge(t.cx, t.cy, t.ax, t.ay, px, py);      // weight of b
    e2 = rnd_edge(t.ax, t.ay, t.bx, t.by, px, py);      // weight of c
}
__device__ __forceinline__ float rnd_depth(long long e0, long long e1, long long e2, long long area, float za, float zb, float zc) {
    return ((float)e0 * za + (float)e1 * zb + (float)e2 * zc) / (float)area;
}
__device__ __forceinline__ int rnd_snap(float c) {
    float s = rintf(c * (float)RND_SNAP);
    s = fminf(fmaxf(s, -(float)RND_CLAMP), (float)RND_CLAMP);
    return (int)s;
}

// ---- per-motion centroid ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RND_THREADS) void k_rnd_centroid(const float* __restrict__ verts, const uint8_t* __restrict__ mask, float* __restrict__ ctr,
                                                              int T, int V, int P, int center) {
    __shared__ double red[3][RND_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    int t0 = -1;
    if (center)
        for (int t = 0; t < T; ++t)
            if (!mask || mask[(size_t)b * T + t]) {
                t0 = t;
                break;
            }
    double s[3] = {0., 0., 0.};
    if (t0 >= 0)
        for (int v = tid; v < V; v += RND_THREADS) {
            const float* src = verts + (((size_t)b * V + v) * 3 * P) * T + t0;
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] += (double)src[(size_t)c * T];
        }
#pragma unroll
    for (int c = 0; c < 3; ++c) red[c][tid] = s[c];
    __syncthreads();
    for (int w = RND_THREADS / 2; w > 0; w >>= 1) {
        if (tid < w)
#pragma unroll
            for (int c = 0; c < 3; ++c) red[c][tid] += red[c][tid + w];
        __syncthreads();
    }
    if (tid < 3) ctr[4 * b + tid] = t0 >= 0 ? (float)(red[tid][0] / (double)V) : 0.f;
}

// ---- projection ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RND_THREADS) void k_rnd_project(const float* __restrict__ verts, const uint8_t* __restrict__ mask, const float* __restrict__ ctr,
                                                             float4* __restrict__ pos, int2* __restrict__ scr, long long total, int T, int V, int P, float sx,
                                                             float sy, float tx, float ty, float hw, float hh) {
    const long long idx = (long long)blockIdx.x * RND_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int t = (int)(idx % T);
    long long r = idx / T;
    const int v = (int)(r % V);
    r /= V;
    const int p = (int)(r % P);
    const long long b = r / P;
    if (mask && !mask[b * T + t]) return;
    const float* src = verts + ((b * V + v) * 3 * P + 3 * p) * T + t;
    const float X = src[0] - ctr[4 * b], Y = src[T] - ctr[4 * b + 1], Z = src[2 * (size_t)T] - ctr[4 * b + 2];
    const float col = (1.f + sx * (X + tx)) * hw, row = (1.f + sy * (Y + ty)) * hh;
    const long long o = ((b * T + t) * P + p) * V + v;
    pos[o] = make_float4(X, Y, Z, 0.f);
    scr[o] = make_int2(rnd_snap(col), rnd_snap(row));
}

// ---- vertex normals --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RND_THREADS) void k_rnd_normals(const float4* __restrict__ pos, const uint8_t* __restrict__ mask, const int* __restrict__ faces,
                                                             const int* __restrict__ adj_ptr, const int* __restrict__ adj, float4* __restrict__ nrm,
                                                             long long total, int V, int P) {
    const long long idx = (long long)blockIdx.x * RND_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int v = (int)(idx % V);
    const long long q = idx / V, frame = q / P;         // q = frame * P + person
    if (mask && !mask[frame]) return;
    const float4* pb = pos + q * V;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int k = adj_ptr[v]; k < adj_ptr[v + 1]; ++k) {
        const int* fi = faces + 3 * (size_t)adj[k];
        const float4 a = pb[fi[0]], b = pb[fi[1]], c = pb[fi[2]];
        const float ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z, wx = c.x - a.x, wy = c.y - a.y, wz = c.z - a.z;
        sx += uy * wz - uz * wy;
        sy += uz * wx - ux * wz;
        sz += ux * wy - uy * wx;
    }
    const float len = sqrtf(sx * sx + sy * sy + sz * sz);
    nrm[idx] = len > 0.f ? make_float4(sx / len, sy / len, sz / len, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- face boxes ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RND_THREADS) void k_rnd_bbox(const int2* __restrict__ scr, const uint8_t* __restrict__ mask, const int* __restrict__ faces,
                                                          RndBox* __restrict__ box, RndBox* __restrict__ cbox, long long total, int V, int F, int Fc, int P,
                                                          int W, int H) {
    const long long idx = (long long)blockIdx.x * RND_THREADS + threadIdx.x;      // (total is a multiple of 64: a wave is inside or outside as a whole)
    if (idx >= total) return;
    const int Fpad = Fc * 64, f = (int)(idx % Fpad);
    const long long q = idx / Fpad, frame = q / P;
    int x0 = RND_MAX_WH, y0 = RND_MAX_WH, x1 = 0, y1 = 0;
    if (f < F && !(mask && !mask[frame])) {
        const int2* sb = scr + q * V;
        const int2 a = sb[faces[3 * (size_t)f]], b = sb[faces[3 * (size_t)f + 1]], c = sb[faces[3 * (size_t)f + 2]];
        RndTri t;
        if (rnd_setup(a, b, c, t)) {
            // pixel j's centre is at 256 j + 128: the centres inside [min, max] are ceil((min - 128) / 256) .. floor((max - 128) / 256)
            const int xa = (min(a.x, min(b.x, c.x)) - 128 + 255) >> 8, xb = ((max(a.x, max(b.x, c.x)) - 128) >> 8) + 1;
            const int ya = (min(a.y, min(b.y, c.y)) - 128 + 255) >> 8, yb = ((max(a.y, max(b.y, c.y)) - 128) >> 8) + 1;
            const int cx0 = max(xa, 0), cx1 = min(xb, W), cy0 = max(ya, 0), cy1 = min(yb, H);
            if (cx0 < cx1 && cy0 < cy1) x0 = cx0, x1 = cx1, y0 = cy0, y1 = cy1;
        }
    }
    box[idx] = RndBox{(uint32_t)x0 | (uint32_t)y0 << 16, (uint32_t)x1 | (uint32_t)y1 << 16};
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        x0 = min(x0, __shfl_xor(x0, d));
        y0 = min(y0, __shfl_xor(y0, d));
        x1 = max(x1, __shfl_xor(x1, d));
        y1 = max(y1, __shfl_xor(y1, d));
    }
    if ((threadIdx.x & 63) == 0) cbox[idx >> 6] = RndBox{(uint32_t)x0 | (uint32_t)y0 << 16, (uint32_t)x1 | (uint32_t)y1 << 16};
}

// ---- raster and shade ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long rnd_key(float z, uint32_t gface) {
    uint32_t u = __float_as_uint(z);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);     // order-preserving: unsigned comparison of u is the comparison of z
    return (unsigned long long)u << 32 | gface;
}

// Face f (< F: a padding face has an empty box) over the pixels [x0, x1) x [y0, y1) of the tile at (tx0, ty0), which lie inside the tile: pixels
// first, first + step, ... of the box in row order take part in the minimum.
__device__ __forceinline__ void rnd_raster_face(unsigned long long* zb, const int* __restrict__ faces, const int2* __restrict__ sb, const float4* __restrict__ pb,
                                                int f, uint32_t gface, int x0, int y0, int x1, int y1, int tx0, int ty0, int first, int step) {
    const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    RndTri t;
    rnd_setup(sb[i0], sb[i1], sb[i2], t);
    const float za = pb[i0].z, zb1 = pb[t.swapped ? i2 : i1].z, zc = pb[t.swapped ? i1 : i2].z;
    const bool o0 = rnd_owns(t.bx, t.by, t.cx, t.cy), o1 = rnd_owns(t.cx, t.cy, t.ax, t.ay), o2 = rnd_owns(t.ax, t.ay, t.bx, t.by);
    const int w = x1 - x0, n = w * (y1 - y0);
    for (int i = first; i < n; i += step) {
        const int yy = i / w, x = x0 + (i - yy * w), y = y0 + yy;
        long long e0, e1, e2;
        rnd_edges(t, x * RND_SNAP + RND_SNAP / 2, y * RND_SNAP + RND_SNAP / 2, e0, e1, e2);
        if ((e0 > 0 || (e0 == 0 && o0)) && (e1 > 0 || (e1 == 0 && o1)) && (e2 > 0 || (e2 == 0 && o2)))
            atomicMin(&zb[(y - ty0) * RND_TILE + (x - tx0)], rnd_key(rnd_depth(e0, e1, e2, t.area, za, zb1, zc), gface));
    }
}

__global__ __launch_bounds__(RND_THREADS) void k_rnd_raster(const float4* __restrict__ pos, const float4* __restrict__ nrm, const int2* __restrict__ scr,
                                                            const int* __restrict__ faces, const RndBox* __restrict__ box, const RndBox* __restrict__ cbox,
                                                            uint8_t* __restrict__ rgb, float* __restrict__ depth, int* __restrict__ face, int W, int H, int P,
                                                            int V, int F, int Fc, int tiles_x, const RndShade sh) {
    __shared__ unsigned long long zb[RND_TILE * RND_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long frame = blockIdx.x;
    const int tile = blockIdx.y, tx0 = (tile % tiles_x) * RND_TILE, ty0 = (tile / tiles_x) * RND_TILE;
    const int tx1 = min(tx0 + RND_TILE, W), ty1 = min(ty0 + RND_TILE, H);
    for (int i = tid; i < RND_TILE * RND_TILE; i += RND_THREADS) zb[i] = RND_EMPTY;
    __syncthreads();
    const long long vbase = frame * P * V, cbase = frame * P * Fc;
    for (int c = wave; c < P * Fc; c += RND_WAVES) {    // c, and every branch on it, is the same in all lanes of the wave
        if (!box_hits(cbox[cbase + c], tx0, ty0, tx1, ty1)) continue;
        const int p = c / Fc, f0 = (c - p * Fc) * 64;
        const RndBox mine = box[(cbase + c) * 64 + lane];
        const int2* sb = scr + vbase + (long long)p * V;
        const float4* pb = pos + vbase + (long long)p * V;
        // a face whose box leaves at most RND_SMALL pixels in the tile is rasterised by its own lane, 64 faces side by side with their loads in
        // flight together; a larger one by the whole wave, one face after the other
        const bool hit = box_hits(mine, tx0, ty0, tx1, ty1);
        const int mx0 = max((int)(mine.lo & 0xffff), tx0), my0 = max((int)(mine.lo >> 16), ty0);
        const int mx1 = min((int)(mine.hi & 0xffff), tx1), my1 = min((int)(mine.hi >> 16), ty1);
        const bool small = hit && (mx1 - mx0) * (my1 - my0) <= RND_SMALL;
        if (small) rnd_raster_face(zb, faces, sb, pb, f0 + lane, (uint32_t)(p * F + f0 + lane), mx0, my0, mx1, my1, tx0, ty0, 0, 1);
        unsigned long long m = __ballot(hit && !small);
        while (m) {
            const int k = __ffsll((long long)m) - 1;
            m &= m - 1;
            rnd_raster_face(zb, faces, sb, pb, f0 + k, (uint32_t)(p * F + f0 + k), __shfl(mx0, k), __shfl(my0, k), __shfl(mx1, k), __shfl(my1, k), tx0, ty0,
                            lane, 64);
        }
    }
    __syncthreads();
    // resolve: a wave takes one row of the tile per pass
    for (int i = tid; i < RND_TILE * RND_TILE; i += RND_THREADS) {
        const int x = tx0 + (i & (RND_TILE - 1)), y = ty0 + i / RND_TILE;
        if (x >= tx1 || y >= ty1) continue;
        const unsigned long long key = zb[i];
        const long long o = (frame * H + y) * W + x;
        uint8_t r = sh.bg[0], g = sh.bg[1], bl = sh.bg[2];
        float z = INFINITY;
        int gf = -1;
        if (key != RND_EMPTY) {
            gf = (int)(uint32_t)key;
            const uint32_t u = (uint32_t)(key >> 32);
            z = __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
            const int p = gf / F, f = gf - p * F;
            const long long vb = vbase + (long long)p * V;
            const int i0 = faces[3 * (size_t)f];
            int i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
            RndTri t;
            rnd_setup(scr[vb + i0], scr[vb + i1], scr[vb + i2], t);
            if (t.swapped) {
                const int s = i1;
                i1 = i2;
                i2 = s;
            }
            long long e0, e1, e2;
            rnd_edges(t, x * RND_SNAP + RND_SNAP / 2, y * RND_SNAP + RND_SNAP / 2, e0, e1, e2);
            const float fa = (float)t.area, b0 = (float)e0 / fa, b1 = (float)e1 / fa, b2 = (float)e2 / fa;
            const float4 pa = pos[vb + i0], pbb = pos[vb + i1], pc = pos[vb + i2], na = nrm[vb + i0], nb = nrm[vb + i1], nc = nrm[vb + i2];
            float nx = b0 * na.x + b1 * nb.x + b2 * nc.x, ny = b0 * na.y + b1 * nb.y + b2 * nc.y, nz = b0 * na.z + b1 * nb.z + b2 * nc.z;
            const float nl = sqrtf(nx * nx + ny * ny + nz * nz);
            if (nl > 0.f) nx /= nl, ny /= nl, nz /= nl;
            if (nz > 0.f) nx = -nx, ny = -ny, nz = -nz; // towards the camera, which looks along +Z
            const float X = b0 * pa.x + b1 * pbb.x + b2 * pc.x, Y = b0 * pa.y + b1 * pbb.y + b2 * pc.y;
            const float L[3][3] = {{0.f, 1.f, -1.f}, {0.f, -1.f, -1.f}, {1.f, -1.f, -2.f}};
            float I = 0.4f;
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                const float dx = L[l][0] - X, dy = L[l][1] - Y, dz = L[l][2] - z;
                const float dl = sqrtf(dx * dx + dy * dy + dz * dz);
                const float d = dl > 0.f ? (nx * dx + ny * dy + nz * dz) / dl : 0.f;
                I += 0.2f * fmaxf(0.f, d);
            }
            const float* base = sh.col[min(p, RGN_RENDER_MAX_PERSONS - 1)];
            r = (uint8_t)fminf(fmaxf(rintf(255.f * base[0] * I), 0.f), 255.f);
            g = (uint8_t)fminf(fmaxf(rintf(255.f * base[1] * I), 0.f), 255.f);
            bl = (uint8_t)fminf(fmaxf(rintf(255.f * base[2] * I), 0.f), 255.f);
        }
        rgb[3 * o] = r;
        rgb[3 * o + 1] = g;
        rgb[3 * o + 2] = bl;
        if (depth) depth[o] = z;
        if (face) face[o] = gf;
    }
}

inline uint64_t up16(uint64_t a) { return (a + 15) / 16 * 16; }

}  // namespace

// ---- the handle ------------------------------------------------------------------------------------------------------------------------------
struct rgn_render_ctx {
    int device = 0, V = 0, F = 0, Fc = 0;               // Fc: chunks of 64 faces
    int* blob = nullptr;                                // faces [F, 3] | adj_ptr [V + 1] | adj [3 F]
    int *faces = nullptr, *adj_ptr = nullptr, *adj = nullptr;
    std::string err;
    int fail(int code, const std::string& m) {
        err = m;
        return code;
    }
};

namespace {

thread_local std::string g_render_create_error;

#define RND_HIP(h, expr)                                                                                \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) return (h)->fail(RGN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// no C++ exception crosses the C boundary (see rgn_guard in rgn_abi.cpp)
template <class Fn>
int render_guard(rgn_render_ctx* h, const char* fn, Fn&& body) noexcept {
    try {
        return body();
    } catch (const std::exception& e) {
        try {
            std::string m = std::string(fn) + ": C++ exception at the boundary: " + e.what();
            if (h) h->err.swap(m);
            else g_render_create_error.swap(m);
        } catch (...) {
        }
        return RGN_ERR_INTERNAL;
    } catch (...) {
        return RGN_ERR_INTERNAL;
    }
}

// the shape checks rgn_render_workspace and rgn_render share; nullptr when the shape is served
const char* shape_error(const rgn_render_ctx* c, int B, int T, int P, int W, int H) {
    if (B < 1 || T < 1) return "B < 1 or T < 1";
    if (W < 1 || W > RND_MAX_WH || H < 1 || H > RND_MAX_WH) return "width or height outside [1, 4096]";
    if (P < 1) return "num_person < 1";
    if ((long long)P * c->F >= (1ll << 31)) return "num_person x F >= 2^31: a global face index no longer fits the depth key";
    const long long NF = (long long)B * T;
    if (NF > RND_MAX_BLOCKS) return "B x T above 2^24 - 1 frames: split the batch";
    const long long items = std::max<long long>(c->V, (long long)c->Fc * 64);
    if (P > RND_MAX_BLOCKS || NF * P > RND_MAX_BLOCKS || (NF * P * items + RND_THREADS - 1) / RND_THREADS > RND_MAX_BLOCKS)
        return "B x T x num_person x max(V, F) is more than one launch covers: split the batch";
    const long long tiles = (long long)((W + RND_TILE - 1) / RND_TILE) * ((H + RND_TILE - 1) / RND_TILE);
    if (NF * tiles > RND_MAX_BLOCKS) return "B x T x (tiles of 64 x 64 pixels) is more than one launch covers: split the batch";
    return nullptr;
}

RndWork carve(const rgn_render_ctx* c, long long B, long long T, long long P) {
    const uint64_t nv = (uint64_t)(B * T * P) * c->V, nc = (uint64_t)(B * T * P) * c->Fc;
    RndWork w;
    w.ctr = 0;
    w.pos = up16((uint64_t)B * 4 * sizeof(float));
    w.nrm = w.pos + nv * sizeof(float4);
    w.scr = w.nrm + nv * sizeof(float4);
    w.box = up16(w.scr + nv * sizeof(int2));
    w.cbox = up16(w.box + nc * 64 * sizeof(RndBox));
    w.bytes = up16(w.cbox + nc * sizeof(RndBox));
    return w;
}

inline unsigned blocks_of(long long total) { return (unsigned)((total + RND_THREADS - 1) / RND_THREADS); }

}  // namespace

extern "C" {

const char* rgn_render_last_error(rgn_render_handle r) { return r ? r->err.c_str() : g_render_create_error.c_str(); }

int rgn_render_create(int32_t device, int32_t V, int32_t F, const int32_t* faces, rgn_render_handle* out) {
    return render_guard(nullptr, "rgn_render_create", [&]() -> int {
        auto bad = [&](int code, const std::string& m) {
            g_render_create_error = "rgn_render_create: " + m;
            return code;
        };
        if (!out) return bad(RGN_ERR_INVALID_ARG, "null out");
        *out = nullptr;
        if (V < 1 || V > RND_MAX_V) return bad(RGN_ERR_INVALID_ARG, "V outside [1, 65536]");
        if (F < 1) return bad(RGN_ERR_INVALID_ARG, "F < 1");
        if ((long long)F > ((1ll << 31) - 1) / 3 - 64) return bad(RGN_ERR_INVALID_ARG, "F above 2^31 / 3: the face table's own indices no longer fit 32 bits");
        if (!faces) return bad(RGN_ERR_INVALID_ARG, "null faces");
        for (long long i = 0; i < 3ll * F; ++i)
            if (faces[i] < 0 || faces[i] >= V)
                return bad(RGN_ERR_INVALID_ARG, "faces[" + std::to_string(i / 3) + "][" + std::to_string(i % 3) + "] = " + std::to_string(faces[i]) + " outside [0, V)");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return bad(RGN_ERR_HIP, "no HIP device visible");
        if (device < 0 || device >= ndev) return bad(RGN_ERR_INVALID_ARG, "device ordinal out of range");
        if (hipSetDevice(device) != hipSuccess) return bad(RGN_ERR_HIP, "hipSetDevice failed");

        std::unique_ptr<rgn_render_ctx> c(new rgn_render_ctx());
        c->device = device;
        c->V = V;
        c->F = F;
        c->Fc = (F + 63) / 64;
        // vertex -> faces, CSR, faces ascending within a vertex; a face that names a vertex twice is listed twice for it (its cross product is 0)
        const size_t n_f = (size_t)3 * F, n_p = (size_t)V + 1;
        std::vector<int> host(n_f + n_p + n_f, 0);
        int *hf = host.data(), *hp = hf + n_f, *ha = hp + n_p;
        std::memcpy(hf, faces, n_f * sizeof(int));
        for (size_t i = 0; i < n_f; ++i) ++hp[faces[i] + 1];
        for (int v = 0; v < V; ++v) hp[v + 1] += hp[v];
        std::vector<int> fill(hp, hp + V);
        for (size_t i = 0; i < n_f; ++i) ha[fill[faces[i]]++] = (int)(i / 3);
        void* dev = nullptr;
        if (hipMalloc(&dev, host.size() * sizeof(int)) != hipSuccess) return bad(RGN_ERR_HIP, "hipMalloc of the face tables failed");
        if (hipMemcpy(dev, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(dev);
            return bad(RGN_ERR_HIP, "hipMemcpy of the face tables failed");
        }
        c->blob = reinterpret_cast<int*>(dev);
        c->faces = c->blob;
        c->adj_ptr = c->faces + n_f;
        c->adj = c->adj_ptr + n_p;
        *out = c.release();
        return RGN_OK;
    });
}

int rgn_render_destroy(rgn_render_handle r) {
    return render_guard(nullptr, "rgn_render_destroy", [&]() -> int {
        if (!r) return RGN_ERR_INVALID_ARG;
        (void)hipSetDevice(r->device);
        (void)hipDeviceSynchronize();
        if (r->blob) (void)hipFree(r->blob);
        delete r;
        return RGN_OK;
    });
}

int rgn_render_workspace(rgn_render_handle r, int32_t B, int32_t T, int32_t num_person, int32_t width, int32_t height, uint64_t* nbytes) {
    return render_guard(r, "rgn_render_workspace", [&]() -> int {
        if (!r) return RGN_ERR_INVALID_ARG;
        if (!nbytes) return r->fail(RGN_ERR_INVALID_ARG, "rgn_render_workspace: null nbytes");
        if (const char* why = shape_error(r, B, T, num_person, width, height)) return r->fail(RGN_ERR_INVALID_ARG, std::string("rgn_render_workspace: ") + why);
        *nbytes = carve(r, B, T, num_person).bytes;
        return RGN_OK;
    });
}

int rgn_render(rgn_render_handle h, const float* verts, const uint8_t* mask, int32_t B, int32_t T, int32_t num_person, const rgn_render_params* params,
               uint8_t* rgb, float* depth, int32_t* face, void* work, uint64_t work_bytes, void* stream) {
    return render_guard(h, "rgn_render", [&]() -> int {
        if (!h) return RGN_ERR_INVALID_ARG;
        if (!params) return h->fail(RGN_ERR_INVALID_ARG, "rgn_render: null params");
        if (!verts || !rgb || !work) return h->fail(RGN_ERR_INVALID_ARG, "rgn_render: null verts, rgb or work");
        const int W = params->width, H = params->height, P = num_person, V = h->V, F = h->F, Fc = h->Fc;
        if (const char* why = shape_error(h, B, T, P, W, H)) return h->fail(RGN_ERR_INVALID_ARG, std::string("rgn_render: ") + why);
        const RndWork w = carve(h, B, T, P);
        if (work_bytes < w.bytes)
            return h->fail(RGN_ERR_INVALID_ARG, "rgn_render: workspace of " + std::to_string(work_bytes) + " bytes, " + std::to_string(w.bytes) +
                                                    " needed (rgn_render_workspace)");
        if (reinterpret_cast<uintptr_t>(work) % 16) return h->fail(RGN_ERR_INVALID_ARG, "rgn_render: work is not 16-byte aligned");
        RndShade sh;
        std::memcpy(sh.col, params->colors, sizeof(sh.col));
        for (int c = 0; c < 3; ++c) {
            const float b = 255.f * params->background[c];
            sh.bg[c] = (uint8_t)(b >= 255.f ? 255.f : b > 0.f ? std::nearbyint(b) : 0.f);
        }
        sh.bg[3] = 0;
        RND_HIP(h, hipSetDevice(h->device));
        hipStream_t s = reinterpret_cast<hipStream_t>(stream);
        char* const wb = reinterpret_cast<char*>(work);
        float* ctr = reinterpret_cast<float*>(wb + w.ctr);
        float4 *pos = reinterpret_cast<float4*>(wb + w.pos), *nrm = reinterpret_cast<float4*>(wb + w.nrm);
        int2* scr = reinterpret_cast<int2*>(wb + w.scr);
        RndBox *box = reinterpret_cast<RndBox*>(wb + w.box), *cbox = reinterpret_cast<RndBox*>(wb + w.cbox);
        const long long NF = (long long)B * T, nv = NF * P * V, nb = NF * P * Fc * 64;
        hipLaunchKernelGGL(k_rnd_centroid, dim3(B), dim3(RND_THREADS), 0, s, verts, mask, ctr, T, V, P, params->center ? 1 : 0);
        RND_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(k_rnd_project, dim3(blocks_of(nv)), dim3(RND_THREADS), 0, s, verts, mask, ctr, pos, scr, nv, T, V, P, params->cam[0], params->cam[1],
                           params->cam[2], params->cam[3], 0.5f * (float)W, 0.5f * (float)H);
        RND_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(k_rnd_normals, dim3(blocks_of(nv)), dim3(RND_THREADS), 0, s, pos, mask, h->faces, h->adj_ptr, h->adj, nrm, nv, V, P);
        RND_HIP(h, hipGetLastError());
        hipLaunchKernelGGL(k_rnd_bbox, dim3(blocks_of(nb)), dim3(RND_THREADS), 0, s, scr, mask, h->faces, box, cbox, nb, V, F, Fc, P, W, H);
        RND_HIP(h, hipGetLastError());
        const int tiles_x = (W + RND_TILE - 1) / RND_TILE, tiles_y = (H + RND_TILE - 1) / RND_TILE;
        hipLaunchKernelGGL(k_rnd_raster, dim3((unsigned)NF, tiles_x * tiles_y), dim3(RND_THREADS), 0, s, pos, nrm, scr, h->faces, box, cbox, rgb, depth, face, W, H,
                           P, V, F, Fc, tiles_x, sh);
        RND_HIP(h, hipGetLastError());
        return RGN_OK;
    });
}

}  // extern "C"
