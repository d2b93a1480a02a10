// Stand-alone driver of tests/test_sg_stage_gpu.py: runs ONE launch of one fused ST-GCN kernel per case and hands the output rows back.
//
//   sg_stage_check <gcn | tconv | tconv_pre | tconv_s2 | x3_sg> <dir>
//
// <dir>/<kernel>.cases lists the cases, one per line (fields at each run_* below); every tensor is a raw little-endian fp32 file in natural layout
// (<dir>/<case>.<tensor>.f32). An activation PLANE file holds G = 4 V guard rows, the body rows and G guard rows, [G + rows + G][C]; the guard rows
// must be zero (the pad frames are the case's business: tests/sg_stage_cases.py writes them as zeros, as k_sg_zero leaves them). Every 16-bit operand
// is already representable - as a hi + lo pair of bf16, or as fp16 - and the program ends if a conversion would round. The program packs the
// planes with rgn_layout.h's plane_off, the temporal weights in the K order rgn_stgcn_finalize packs (channel block, tap, channel), launches the
// kernel ONCE through its launch_* function after configure_* and the *_supported predicate, and writes the body rows of the output planes as
// <dir>/<case>.out_hi.f32 / .out_lo.f32 (fp16 form and tail 0: out_hi only). Output planes are pre-filled with 0xFFFF (a NaN in both formats; the fp32
// output of tail 0 with 0xFFFFFFFF), guard rows and a margin of rows behind the plane included: an element the kernel must write and did not comes
// back as NaN, and an element outside the rows the launch covers that no longer holds the fill ends the program with its row and column.
// No timing, no loop, no retry. Any HIP error, a false *_supported predicate or a malformed case ends the program with the text and a non-zero status.
// Per case it prints the device's CU count and the case's tile count (the persistent walk: tile slot, slot + #CU, ...).
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I regennet_amd/csrc tests/sg_stage_check.hip regennet_amd/csrc/{rgn_sg_kernels,rgn_gemm_x3}.hip -o sg_stage_check
#include "rgn_internal.h"
#include "rgn_layout.h"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace rgn;

[[noreturn]] static void die(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "sg_stage_check: ");
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    exit(1);
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) die("HIP error: %s at %s:%d (%s)", hipGetErrorString(e_), __FILE__, __LINE__, #x); } while (0)

constexpr uint16_t FILL = 0xFFFF;
constexpr long MARGIN = 37;          // rows behind an output plane that must come back untouched (odd: the row stride is no multiple of anything)
static std::string g_dir;

static std::vector<float> read_f32(const std::string& stem, size_t n) {
    const std::string path = g_dir + "/" + stem + ".f32";
    std::ifstream f(path, std::ios::binary);
    if (!f) die("cannot open %s", path.c_str());
    std::vector<float> v(n);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * 4));
    if ((size_t)f.gcount() != n * 4 || f.peek() != EOF) die("%s does not hold %zu floats", path.c_str(), n);
    return v;
}
static void write_f32(const std::string& stem, const std::vector<float>& v) {
    const std::string path = g_dir + "/" + stem + ".f32";
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * 4));
    if (!f) die("cannot write %s", path.c_str());
}
template <class T>
static T* upload(const std::vector<T>& v) {
    void* p;
    CK(hipMalloc(&p, v.size() * sizeof(T)));
    CK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return (T*)p;
}
static uint16_t f16_bits(float v, const char* what) {
    const _Float16 h = (_Float16)v;
    if ((float)h != v) die("%s: %.9g is not representable in fp16", what, v);
    uint16_t b;
    memcpy(&b, &h, 2);
    return b;
}
static float f16_value(uint16_t b) {
    _Float16 h;
    memcpy(&h, &b, 2);
    return (float)h;
}
// v -> (hi, lo) with hi = bf16(v), lo = bf16(v - hi) and hi + lo == v
static void split_bits(float v, uint16_t& hi, uint16_t& lo, const char* what) {
    hi = f2bf(v);
    lo = f2bf(v - bf2f(hi));
    if (bf2f(hi) + bf2f(lo) != v) die("%s: %.9g is not a bf16 hi + lo pair", what, v);
}

// a 16-bit operand on the device: the split form's (hi, lo) planes, or one fp16 plane in hi
struct Dev16 { __bf16* hi = nullptr; __bf16* lo = nullptr; };
// natural [rows][K] -> K32-blocked plane(s) [K / 32][rows][32]
static Dev16 pack(const std::vector<float>& nat, long rows, int K, bool f16, const char* what) {
    if (nat.size() != (size_t)rows * K || K % 32) die("%s: %zu values for %ld x %d", what, nat.size(), rows, K);
    std::vector<uint16_t> hi((size_t)rows * K), lo(f16 ? 0 : (size_t)rows * K);
    for (long m = 0; m < rows; ++m)
        for (int k = 0; k < K; ++k) {
            const size_t o = plane_off((size_t)rows, (size_t)m, k);
            const float v = nat[(size_t)m * K + k];
            if (f16) hi[o] = f16_bits(v, what);
            else split_bits(v, hi[o], lo[o], what);
        }
    Dev16 d;
    d.hi = (__bf16*)upload(hi);
    if (!f16) d.lo = (__bf16*)upload(lo);
    return d;
}
// an activation plane file [G + rows + G][C]: the guard rows must be zero; the device pointers are those of body row 0
static Dev16 plane_in(const std::string& stem, long rows, long G, int C, bool f16, long* total) {
    const long R = rows + 2 * G;
    const std::vector<float> nat = read_f32(stem, (size_t)R * C);
    for (long m = 0; m < R; ++m)
        if (m < G || m >= G + rows)
            for (int c = 0; c < C; ++c)
                if (nat[(size_t)m * C + c] != 0.f) die("%s: guard row %ld is not zero", stem.c_str(), m - G);
    Dev16 d = pack(nat, R, C, f16, stem.c_str());
    d.hi += G * 32;
    if (d.lo) d.lo += G * 32;
    *total = R;
    return d;
}
// the temporal weights W2'[o][q][dt] (natural [N][C][9]) in finalize's K order: column ((q / 32) 9 + dt) 32 + q % 32
static Dev16 tconv_weights(const std::string& stem, int N, int C, bool f16) {
    const std::vector<float> nat = read_f32(stem, (size_t)N * C * 9);
    std::vector<float> W((size_t)N * 9 * C);
    for (int o = 0; o < N; ++o)
        for (int q = 0; q < C; ++q)
            for (int dt = 0; dt < 9; ++dt) W[(size_t)o * 9 * C + ((size_t)(q / 32) * 9 + dt) * 32 + q % 32] = nat[((size_t)o * C + q) * 9 + dt];
    return pack(W, N, 9 * C, f16, stem.c_str());
}
// output planes of `body` rows behind G guard rows, + G + MARGIN rows, all FILL
struct OutPlanes { Dev16 d; long body, G, R; int N; bool f16; };
static OutPlanes plane_out(long body, long G, int N, bool f16) {
    OutPlanes o{};
    o.body = body; o.G = G; o.R = G + body + G + MARGIN; o.N = N; o.f16 = f16;
    const std::vector<uint16_t> fill((size_t)o.R * N, FILL);
    o.d.hi = (__bf16*)upload(fill) + G * 32;
    if (!f16) o.d.lo = (__bf16*)upload(fill) + G * 32;
    return o;
}
// the body rows back as fp32 (hi and lo apart); a row outside `covered` (body row -> bool; nullptr: every body row) must still hold the fill
static void plane_back(const OutPlanes& o, const std::string& name, const std::vector<char>* covered) {
    for (int pl = 0; pl < (o.f16 ? 1 : 2); ++pl) {
        std::vector<uint16_t> raw((size_t)o.R * o.N);
        CK(hipMemcpy(raw.data(), (pl ? o.d.lo : o.d.hi) - o.G * 32, raw.size() * 2, hipMemcpyDeviceToHost));
        std::vector<float> nat((size_t)o.body * o.N);
        for (long m = 0; m < o.R; ++m) {
            const long b = m - o.G;
            const bool in = b >= 0 && b < o.body && (!covered || (*covered)[(size_t)b]);
            for (int n = 0; n < o.N; ++n) {
                const uint16_t v = raw[plane_off((size_t)o.R, (size_t)m, n)];
                if (!in && v != FILL) die("case %s: %s plane row %ld (body rows 0 .. %ld) column %d lies outside the rows the launch covers and was written", name.c_str(), pl ? "lo" : "hi", b, o.body - 1, n);
                if (b >= 0 && b < o.body) nat[(size_t)b * o.N + n] = o.f16 ? f16_value(v) : bf2f(v);
            }
        }
        write_f32(name + (pl ? ".out_lo" : ".out_hi"), nat);
    }
}

struct Case {
    std::string name;
    std::vector<long> v;
    long operator[](size_t i) const { if (i >= v.size()) die("case %s: field %zu missing", name.c_str(), i); return v[i]; }
};
static std::vector<Case> read_cases(const std::string& kernel) {
    const std::string path = g_dir + "/" + kernel + ".cases";
    std::ifstream f(path);
    if (!f) die("cannot open %s", path.c_str());
    std::vector<Case> out;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        Case c;
        if (!(ss >> c.name)) continue;
        long x;
        while (ss >> x) c.v.push_back(x);
        out.push_back(c);
    }
    if (out.empty()) die("%s lists no case", path.c_str());
    return out;
}
static void finish(const Case& c, long tiles) {
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    int dev = 0, cus = 0;
    CK(hipGetDevice(&dev));
    CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    printf("%s: ran, cus %d tiles %ld\n", c.name.c_str(), cus, tiles);
}
static long tiles_of(long M, int N, int BM, int BN) { return ((N + BN - 1) / BN) * ((M + BM - 1) / BM); }

// <name> f16 V M Cin N KP P cap per_block_barrier slot_k BN        files: x [G + M + G][Cin], W1 [N][KP Cin], b1 [P][N], slv [V][8], sla [V][8]
// BN: the tile width the case expects launch_sg_gcn to choose (restated below from its rule; the tile count printed rests on it)
static void run_gcn(const Case& c) {
    const bool f16 = c[0];
    const int V = c[1], Cin = c[3], N = c[4], KP = c[5], P = c[6], cap = c[7], pbb = c[8], BN = c[10];
    const long M = c[2], G = 4L * V;
    const unsigned slot_k = (unsigned)c[9];
    const int Kp = KP * Cin;
    if (!sg_gcn_supported(N, Kp, V, KP) || Cin % (f16 ? 64 : 32)) die("case %s: N = %d, Kp = %d, V = %d, KP = %d is not supported by k_sg_gcn", c.name.c_str(), N, Kp, V, KP);
    auto lds = [&](int bn) { return 2 * 2 * (256 + 2 * V) * 64 + 2 * 2 * bn * 64 + 2 * 4 * 8 * V; };   // (launch_sg_gcn's rule: the widest tile <= cap that fits 160 KiB)
    const int bn = N >= 256 && cap >= 256 && lds(256) <= 160 * 1024 ? 256 : N >= 128 && cap >= 128 && lds(128) <= 160 * 1024 ? 128 : 64;
    if (bn != BN) die("case %s: expects %d-wide tiles, the launch rule gives %d", c.name.c_str(), BN, bn);
    GemmX3Args g{};
    long R;
    const Dev16 x = plane_in(c.name + ".x", M, G, Cin, f16, &R);
    const Dev16 W = pack(read_f32(c.name + ".W1", (size_t)N * Kp), N, Kp, f16, "W1");
    g.Ahi = x.hi; g.Alo = x.lo; g.a_rows = (int)R;
    g.Whi = W.hi; g.Wlo = W.lo;
    g.M = (int)M; g.N = N; g.Kp = Kp;
    g.add = upload(read_f32(c.name + ".b1", (size_t)P * N)); g.ldadd = N; g.add_mod = P; g.act = 3;
    const OutPlanes o = plane_out(M, G, N, f16);
    g.Chi = o.d.hi; g.Clo = o.d.lo; g.c_rows = (int)o.R;
    g.f16 = f16;
    const std::vector<float> svf = read_f32(c.name + ".slv", (size_t)V * 8);
    std::vector<int> sv(svf.size());
    for (size_t i = 0; i < sv.size(); ++i) {
        sv[i] = (int)svf[i];
        if (sv[i] < 0 || sv[i] >= V || (float)sv[i] != svf[i]) die("case %s: slot source %g outside [0, %d)", c.name.c_str(), svf[i], V);
    }
    CK(configure_sg_gcn());
    CK(launch_sg_gcn(g, V, KP, slot_k, upload(sv), upload(read_f32(c.name + ".sla", (size_t)V * 8)), cap, pbb != 0, nullptr));
    finish(c, tiles_of(M, N, 256, BN));
    plane_back(o, c.name, nullptr);
}

// <name> f16 V M N tail small pre BM BN polyT region      files: g [G + M + G][N], W2 [N][N][9], b2 [N], tails 2, 3: R [G + M + G][N]
// pre: launch_sg_tconv_pre (small graph) instead of launch_sg_tconv; BM x BN: the tile shape the case expects (restated below from the launch rule);
// tail 3: polyT = frames per sequence of the rows, region = rows of one output region
static void run_tconv(const Case& c, bool pre) {
    const bool f16 = c[0], small = c[5];
    const int V = c[1], N = c[3], tail = c[4], BM = c[7], BN = c[8], polyT = c[9];
    const long M = c[2], G = 4L * V, region = c[10];
    if ((c[6] != 0) != pre) die("case %s: listed under the other temporal kernel", c.name.c_str());
    if (pre ? (f16 || !sg_tconv_pre_supported(N, 9 * N, V)) : !sg_tconv_supported(N, 9 * N, V)) die("case %s: N = %d, V = %d is not supported by this kernel", c.name.c_str(), N, V);
    if (tail < 0 || tail > 3 || (f16 && tail == 0)) die("case %s: tail %d", c.name.c_str(), tail);
    int bm, bn;
    if (pre) {
        bm = 256; bn = (N != 64 && tail != 3) ? 128 : 64;
    } else {   // (launch_sg_tconv's rule)
        const bool tall = !small && V % 8 == 0 && 8 * V <= 512;
        bm = (N == 64 || N == 128) && tall ? 512 : 256;
        bn = N == 64 ? 64 : (N == 128 ? 128 : (!small ? 256 : 128));
    }
    if (bm != BM || bn != BN) die("case %s: expects %d x %d tiles, the launch rule gives %d x %d", c.name.c_str(), BM, BN, bm, bn);
    GemmX3Args g{};
    long R;
    const Dev16 a = plane_in(c.name + ".g", M, G, N, f16, &R);
    const Dev16 W = tconv_weights(c.name + ".W2", N, N, f16);
    g.Ahi = a.hi; g.Alo = a.lo; g.a_rows = (int)R;
    g.Whi = W.hi; g.Wlo = W.lo;
    g.M = (int)M; g.N = N; g.Kp = 9 * N;
    g.a_taps = 9;
    for (int dt = 0; dt < 9; ++dt) g.a_tap[dt] = (long long)(dt - 4) * V * 64;
    g.f16 = f16;
    g.bias = upload(read_f32(c.name + ".b2", N));
    if (tail >= 2) {
        long Rr;
        const Dev16 r = plane_in(c.name + ".R", M, G, N, f16, &Rr);
        g.Rhi = r.hi; g.Rlo = r.lo; g.r_rows = (int)Rr;
    }
    CK(pre ? configure_sg_tconv_pre() : configure_sg_tconv());
    auto launch = [&]() { return pre ? launch_sg_tconv_pre(g, V, tail, nullptr) : launch_sg_tconv(g, V, tail, small, nullptr); };
    if (tail == 0) {
        const std::vector<uint32_t> fill((size_t)(M + MARGIN) * N, 0xFFFFFFFFu);
        uint32_t* C = upload(fill);
        g.C = reinterpret_cast<float*>(C); g.ldc = N;
        CK(launch());
        finish(c, tiles_of(M, N, BM, BN));
        std::vector<uint32_t> raw(fill.size());
        CK(hipMemcpy(raw.data(), C, raw.size() * 4, hipMemcpyDeviceToHost));
        for (size_t i = (size_t)M * N; i < raw.size(); ++i)
            if (raw[i] != 0xFFFFFFFFu) die("case %s: row %zu (launch covers %ld) column %zu of the fp32 output was written", c.name.c_str(), i / N, M, i % N);
        std::vector<float> nat((size_t)M * N);
        memcpy(nat.data(), raw.data(), nat.size() * 4);
        write_f32(c.name + ".out_hi", nat);
        return;
    }
    if (tail < 3) {
        const OutPlanes o = plane_out(M, G, N, f16);
        g.Chi = o.d.hi; g.Clo = o.d.lo; g.c_rows = (int)o.R;
        CK(launch());
        finish(c, tiles_of(M, N, BM, BN));
        plane_back(o, c.name, nullptr);
        return;
    }
    // polyphase: row (sequence, frame t < polyT of polyT + 4, vertex) -> region t & 1, frame t >> 1 of ceil(polyT / 2) + 4; nothing else is written
    const long Tp = polyT + 4, NM = M / (Tp * V), Tpo = (polyT + 1) / 2 + 4;
    if (NM * Tp * V != M || region != NM * Tpo * V) die("case %s: M = %ld, region = %ld do not fit %d frames of %d vertices", c.name.c_str(), M, region, polyT, V);
    const OutPlanes o = plane_out(2 * region, G, N, f16);
    g.Chi = o.d.hi; g.Clo = o.d.lo; g.c_rows = (int)o.R;
    g.poly_T = polyT; g.poly_V = V; g.poly_region = (int)region;
    std::vector<char> covered((size_t)(2 * region), 0);
    for (long nm = 0; nm < NM; ++nm)
        for (long t = 0; t < polyT; ++t)
            for (long v = 0; v < V; ++v) covered[(size_t)((t & 1) * region + (nm * Tpo + (t >> 1)) * V + v)] = 1;
    CK(launch());
    finish(c, tiles_of(M, N, BM, BN));
    plane_back(o, c.name, &covered);
}

// <name> f16 V M N Cin      files: g [G + 2 M + G][N] (region E | region O), x [G + 2 M + G][Cin], W2 [N][N][9], Wr [N][Cin], b [N] (= b2' + br')
// M: rows of one region = output rows; tiles are 256 x 128
static void run_tconv_s2(const Case& c) {
    const bool f16 = c[0];
    const int V = c[1], N = c[3], Cin = c[4];
    const long M = c[2], G = 4L * V;
    if (!sg_tconv_s2_supported(N, 9 * N, V) || Cin % (f16 ? 64 : 32)) die("case %s: N = %d, V = %d, Cin = %d is not supported by k_sg_tconv_s2", c.name.c_str(), N, V, Cin);
    GemmX3Args g{};
    long R, R2;
    const Dev16 a = plane_in(c.name + ".g", 2 * M, G, N, f16, &R);
    const Dev16 x = plane_in(c.name + ".x", 2 * M, G, Cin, f16, &R2);
    const Dev16 W = tconv_weights(c.name + ".W2", N, N, f16);
    const Dev16 Wr = pack(read_f32(c.name + ".Wr", (size_t)N * Cin), N, Cin, f16, "Wr");
    g.Ahi = a.hi; g.Alo = a.lo; g.a_rows = (int)R;
    g.Whi = W.hi; g.Wlo = W.lo;
    g.M = (int)M; g.N = N; g.Kp = 9 * N;
    g.a_taps = 9;
    for (int dt = 0; dt < 9; ++dt) g.a_tap[dt] = (dt & 1) == 0 ? (long long)((dt - 4) / 2) * V * 64 : ((long long)M + (long long)((dt - 5) / 2) * V) * 64;   // (as the forward sets them)
    g.f16 = f16;
    g.bias = upload(read_f32(c.name + ".b", N));
    g.A2hi = x.hi; g.A2lo = x.lo; g.a2_rows = (int)R2;
    g.W2hi = Wr.hi; g.W2lo = Wr.lo; g.k2 = Cin / 32;
    const OutPlanes o = plane_out(M, G, N, f16);
    g.Chi = o.d.hi; g.Clo = o.d.lo; g.c_rows = (int)o.R;
    CK(configure_sg_tconv());
    CK(launch_sg_tconv_s2(g, V, (long long)M, nullptr));
    finish(c, tiles_of(M, N, 256, 128));
    plane_back(o, c.name, nullptr);
}

// <name> kind V M N K      (launch_gemm_x3_sg: split bf16 only, 256-row tiles, 64 wide for N <= 64 and 128 wide otherwise, a workgroup per tile)
// kind 0: the row-shifted 9-tap GEMM, files g [G + M + G][N], W2 [N][N][9]; output: the fp32 convolution [M][N]
// kind 1: the same with the stride-2 tap table on polyphase planes, g [G + 2 M + G][N] (region E | region O), M = rows of one region
// kind 2: relu(z . W^T + b1[row % add_mod]) into split planes - the GEMM of the two-launch graph convolution; files z [G + M + G][K], W [N][K], b1 [V][N]
static void run_x3_sg(const Case& c) {
    const int kind = c[0], V = c[1], N = c[3], K = c[4];
    const long M = c[2], G = 4L * V;
    if (kind < 0 || kind > 2 || N % 32 || (kind == 2 && (K % 32 || V < 28))) die("case %s: kind %d, N = %d, K = %d, V = %d", c.name.c_str(), kind, N, K, V);
    GemmX3Args g{};
    long R;
    g.M = (int)M; g.N = N;
    CK(configure_gemm_x3_sg());
    const long tiles = tiles_of(M, N, 256, N <= 64 ? 64 : 128);
    if (kind == 2) {
        const Dev16 z = plane_in(c.name + ".z", M, G, K, false, &R);
        const Dev16 W = pack(read_f32(c.name + ".W", (size_t)N * K), N, K, false, "W");
        g.Ahi = z.hi; g.Alo = z.lo; g.a_rows = (int)R; g.Whi = W.hi; g.Wlo = W.lo; g.Kp = K;
        g.add = upload(read_f32(c.name + ".b1", (size_t)V * N)); g.ldadd = N; g.add_mod = V; g.act = 3;
        const OutPlanes o = plane_out(M, G, N, false);
        g.Chi = o.d.hi; g.Clo = o.d.lo; g.c_rows = (int)o.R;
        CK(launch_gemm_x3_sg(g, nullptr));
        finish(c, tiles);
        plane_back(o, c.name, nullptr);
        return;
    }
    const Dev16 a = plane_in(c.name + ".g", kind == 1 ? 2 * M : M, G, N, false, &R);
    const Dev16 W = tconv_weights(c.name + ".W2", N, N, false);
    g.Ahi = a.hi; g.Alo = a.lo; g.a_rows = (int)R; g.Whi = W.hi; g.Wlo = W.lo; g.Kp = 9 * N;
    g.a_taps = 9;
    for (int dt = 0; dt < 9; ++dt) {   // (as the forward sets them)
        if (kind == 0) g.a_tap[dt] = (long long)(dt - 4) * V * 64;
        else if ((dt & 1) == 0) g.a_tap[dt] = (long long)((dt - 4) / 2) * V * 64;
        else g.a_tap[dt] = ((long long)M + (long long)((dt - 5) / 2) * V) * 64;
    }
    const std::vector<uint32_t> fill((size_t)(M + MARGIN) * N, 0xFFFFFFFFu);
    uint32_t* C = upload(fill);
    g.C = reinterpret_cast<float*>(C); g.ldc = N;
    CK(launch_gemm_x3_sg(g, nullptr));
    finish(c, tiles);
    std::vector<uint32_t> raw(fill.size());
    CK(hipMemcpy(raw.data(), C, raw.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = (size_t)M * N; i < raw.size(); ++i)
        if (raw[i] != 0xFFFFFFFFu) die("case %s: row %zu (launch covers %ld) column %zu of the fp32 output was written", c.name.c_str(), i / N, M, i % N);
    std::vector<float> nat((size_t)M * N);
    memcpy(nat.data(), raw.data(), nat.size() * 4);
    write_f32(c.name + ".out_hi", nat);
}

int main(int argc, char** argv) {
    if (argc != 3) die("usage: sg_stage_check <gcn | tconv | tconv_pre | tconv_s2 | x3_sg> <dir>");
    const std::string kernel = argv[1];
    g_dir = argv[2];
    if (kernel != "gcn" && kernel != "tconv" && kernel != "tconv_pre" && kernel != "tconv_s2" && kernel != "x3_sg") die("unknown kernel %s", kernel.c_str());
    for (const Case& c : read_cases(kernel)) {
        if (kernel == "gcn") run_gcn(c);
        else if (kernel == "tconv") run_tconv(c, false);
        else if (kernel == "tconv_pre") run_tconv(c, true);
        else if (kernel == "tconv_s2") run_tconv_s2(c);
        else run_x3_sg(c);
    }
    return 0;
}
