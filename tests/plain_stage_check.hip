// Stand-alone driver of tests/test_plain_stage_gpu.py: runs ONE launch of one plain-phase kernel per case and hands the output back.
//
//   plain_stage_check <attn | long | mlp | rowgemm | layers> <dir>
//
// <dir>/<kernel>.cases lists the cases, one per line (fields below); every tensor is a raw little-endian fp32 file in natural layout
// (<dir>/<case>.<tensor>.f32, the layer's weights <dir>/w_<bf16 | fp16>.<tensor>.f32), every 16-bit operand already representable in the case's
// format (checked: converting must not round). The program packs them with the index functions of rgn_layout.h - K32-blocked planes, the
// fragment-ordered weight plane, the attention-ready slab - launches the kernel once through its launch_* function after configure_*, and writes
// <dir>/<case>.out.f32 in natural layout. Output planes have more rows than the launch covers and are pre-filled with 0xFFFF (a NaN in both
// formats): an element the kernel must write and did not comes back as NaN, one it must not write and did ends the program.
// No timing, no loop, no retry. Any HIP error, a false *_supported predicate or a malformed case ends the program with the text and a non-zero status.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I regennet_amd/csrc tests/plain_stage_check.hip \
//         regennet_amd/csrc/{rgn_qkv_attn,rgn_qkv_attn_long,rgn_mlp2,rgn_rowgemm,rgn_layers}.hip -o plain_stage_check
#include "rgn_internal.h"
#include "rgn_layout.h"

#include <hip/hip_runtime.h>

#include <cmath>
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
    fprintf(stderr, "plain_stage_check: ");
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    exit(1);
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) die("HIP error: %s at %s:%d (%s)", hipGetErrorString(e_), __FILE__, __LINE__, #x); } while (0)

constexpr int D = 512, FF = 1024, NH = 4, DH = 128;
constexpr uint16_t SENTINEL = 0xFFFF;
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

// fp32 -> the 16-bit element of the format; the value must be representable
static uint16_t to16(float v, bool f16, const char* what) {
    uint16_t b;
    float back;
    if (f16) {
        const _Float16 h = (_Float16)v;
        memcpy(&b, &h, 2);
        back = (float)h;
    } else {
        b = f2bf(v);
        back = bf2f(b);
    }
    if (back != v) die("%s: %.9g is not representable in %s", what, v, f16 ? "fp16" : "bf16");
    return b;
}
static float from16(uint16_t b, bool f16) {
    if (!f16) return bf2f(b);
    _Float16 h;
    memcpy(&h, &b, 2);
    return (float)h;
}

template <class T>
static T* upload(const std::vector<T>& v) {
    void* p;
    CK(hipMalloc(&p, v.size() * sizeof(T)));
    CK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return (T*)p;
}
// natural [M][K] -> K32-blocked plane [K / 32][rows][32], rows >= M (the surplus rows: sentinel)
static __bf16* plane_in(const std::vector<float>& nat, int M, int K, int rows, bool f16, const char* what) {
    std::vector<uint16_t> pl((size_t)rows * K, SENTINEL);
    for (int m = 0; m < M; ++m)
        for (int k = 0; k < K; ++k) pl[plane_off(rows, m, k)] = to16(nat[(size_t)m * K + k], f16, what);
    return (__bf16*)upload(pl);
}
static __bf16* plane_out(int rows, int N) { return (__bf16*)upload(std::vector<uint16_t>((size_t)rows * N, SENTINEL)); }
// plane -> natural [M][N]; the rows M .. rows - 1 must still hold the sentinel
static std::vector<float> plane_back(const __bf16* dev, int M, int N, int rows, bool f16, const char* what) {
    std::vector<uint16_t> pl((size_t)rows * N);
    CK(hipMemcpy(pl.data(), dev, pl.size() * 2, hipMemcpyDeviceToHost));
    std::vector<float> nat((size_t)M * N);
    for (int m = 0; m < rows; ++m)
        for (int n = 0; n < N; ++n) {
            const uint16_t b = pl[plane_off(rows, m, n)];
            if (m < M) nat[(size_t)m * N + n] = from16(b, f16);
            else if (b != SENTINEL) die("%s: row %d of %d (launch covers %d) column %d was written", what, m, rows, M, n);
        }
    return nat;
}
// natural nn.Linear weight [N][K] -> fragment-ordered plane [K / 32][N / 32][2][64][8]
static __bf16* frag_in(const std::vector<float>& nat, int N, int K, bool f16, const char* what) {
    std::vector<uint16_t> fr((size_t)N * K);
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k) fr[frag_off((size_t)N / 32, n, k)] = to16(nat[(size_t)n * K + k], f16, what);
    return (__bf16*)upload(fr);
}
static float* vec_in(const std::string& stem, size_t n) { return upload(read_f32(stem, n)); }

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
static std::string wstem(bool f16, const char* t) { return std::string(f16 ? "w_fp16." : "w_bf16.") + t; }
static LayerWts layer_wts(bool f16) {
    LayerWts w{};
    w.Wqkv = frag_in(read_f32(wstem(f16, "Wqkv"), (size_t)3 * D * D), 3 * D, D, f16, "Wqkv");
    w.Wo = frag_in(read_f32(wstem(f16, "Wo"), (size_t)D * D), D, D, f16, "Wo");
    w.W1 = frag_in(read_f32(wstem(f16, "W1"), (size_t)FF * D), FF, D, f16, "W1");
    w.W2 = frag_in(read_f32(wstem(f16, "W2"), (size_t)D * FF), D, FF, f16, "W2");
    w.bqkv = vec_in(wstem(f16, "bqkv"), 3 * D); w.bo = vec_in(wstem(f16, "bo"), D); w.bf1 = vec_in(wstem(f16, "bf1"), FF); w.bf2 = vec_in(wstem(f16, "bf2"), D);
    w.g1 = vec_in(wstem(f16, "g1"), D); w.b1 = vec_in(wstem(f16, "b1"), D); w.g2 = vec_in(wstem(f16, "g2"), D); w.b2 = vec_in(wstem(f16, "b2"), D);
    w.g3 = vec_in(wstem(f16, "g3"), D); w.b3 = vec_in(wstem(f16, "b3"), D);
    return w;
}
static int* step_in(int step) {
    int* p;
    CK(hipMalloc(&p, 4));
    CK(hipMemcpy(p, &step, 4, hipMemcpyHostToDevice));
    return p;
}
static void finish(const char* what) {
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    printf("%s: ran\n", what);
}
static float qscale() { return 1.0f / sqrtf((float)DH); }   // (rgn_plan.cpp)

// <name> f16 Bm Tq rows
static void run_attn(const Case& c, bool longk) {
    const bool f16 = c[0];
    const int Bm = c[1], Tq = c[2], rows = c[3], M = Bm * Tq;
    if (rows < M) die("case %s: %d plane rows for %d tokens", c.name.c_str(), rows, M);
    if (longk ? !qkv_attn_long_supported(Tq, DH, D) : !qkv_attn_supported(Tq, DH, D)) die("case %s: Tq = %d is not supported by this kernel", c.name.c_str(), Tq);
    QkvAttnArgs g{};
    g.Ahi = plane_in(read_f32(c.name + ".h", (size_t)M * D), M, D, rows, f16, "h");
    g.a_rows = rows;
    g.Wfr = frag_in(read_f32(wstem(f16, "Wqkv"), (size_t)3 * D * D), 3 * D, D, f16, "Wqkv");
    g.bias = vec_in(wstem(f16, "bqkv"), 3 * D);
    g.out.hi = plane_out(rows, D); g.out.lo = nullptr; g.out.rows = rows;
    g.Bm = Bm; g.Kp = D; g.d = D; g.H = NH; g.Tq = Tq; g.qscale = qscale(); g.f16 = f16;
    if (longk) {
        CK(configure_qkv_attn_long());
        CK(launch_qkv_attn_long(g, nullptr));
    } else {
        if (qkv_attn_form(g, false).form != QF_RS) die("case %s: the form rule does not pick the register-streamed kernel", c.name.c_str());
        CK(configure_qkv_attn());
        CK(launch_qkv_attn(g, false, nullptr));
    }
    finish(c.name.c_str());
    write_f32(c.name + ".out", plane_back(g.out.hi, M, D, rows, f16, c.name.c_str()));
}

// <name> f16 M Tq rows nper nsteps step
static void run_mlp(const Case& c) {
    const bool f16 = c[0];
    const int M = c[1], Tq = c[2], rows = c[3], nper = c[4], nsteps = c[5], step = c[6];
    // mlp_supported bounds the samples a FULL 64-row tile can touch (63 / Tq + 2 vector slots of 4, M2::NSAMP in rgn_mlp2.hip - not visible from here: if that
    // count changes, this condition must follow); a launch of one partial tile touches (M - 1) / Tq + 1. Only the 3 x 17-row case takes this way in
    const bool one_tile = M <= 64 && (M - 1) / Tq + 1 <= 4;
    if (!mlp_supported(D, FF, Tq) && !one_tile) die("case %s: Tq = %d is not supported by k_mlp2", c.name.c_str(), Tq);
    if (rows < M || (nper && nper < (M - 1) / Tq + 1) || (nsteps && step >= nsteps)) die("case %s: inconsistent sizes", c.name.c_str());
    MlpArgs g{};
    g.att = plane_in(read_f32(c.name + ".att", (size_t)M * D), M, D, rows, f16, "att");
    g.h = plane_in(read_f32(c.name + ".h", (size_t)M * D), M, D, rows, f16, "h");
    g.out = plane_out(rows, D);
    g.rows = rows; g.M = M; g.w = layer_wts(f16); g.Tq = Tq; g.f16 = f16;
    if (nper) { g.pervec = vec_in(c.name + ".pervec", (size_t)nper * D); g.ldper = D; }
    if (nsteps) { g.stepvec = vec_in(c.name + ".stepvec", (size_t)nsteps * D); g.ldstep = D; }
    g.d_step = step_in(step);
    CK(configure_mlp());
    CK(launch_mlp(g, nullptr));
    finish(c.name.c_str());
    write_f32(c.name + ".out", plane_back(g.out, M, D, rows, f16, c.name.c_str()));
}

// <name> epi (0: ln, 1: act 1, 2: act 2) M N K Tq rows two nper nsteps step      (bf16: the kernel has no fp16 form)
static void run_rowgemm(const Case& c) {
    const int epi = c[0], M = c[1], N = c[2], K = c[3], Tq = c[4], rows = c[5], two = c[6], nper = c[7], nsteps = c[8], step = c[9];
    const bool ln = epi == 0;
    if (!rowgemm_supported(N, K, ln)) die("case %s: N = %d, K = %d is not supported by k_rowgemm", c.name.c_str(), N, K);
    if (rows < M || (nper && nper < (M - 1) / Tq + 1) || (nsteps && step >= nsteps)) die("case %s: inconsistent sizes", c.name.c_str());
    RowGemmArgs g{};
    g.A = plane_in(read_f32(c.name + ".a", (size_t)M * K), M, K, rows, false, "a");
    g.a_rows = rows;
    g.W = frag_in(read_f32(c.name + ".W", (size_t)N * K), N, K, false, "W");
    g.bias = vec_in(c.name + ".bias", N);
    g.M = M; g.N = N; g.Kp = K; g.Tq = Tq;
    std::vector<float> out;
    CK(configure_rowgemm());
    if (ln) {
        g.Rhi = plane_in(read_f32(c.name + ".resid", (size_t)M * D), M, D, rows, false, "resid");
        g.r_rows = rows;
        g.Ohi = plane_out(rows, D); g.o_rows = rows;
        g.ga = vec_in(c.name + ".ga", D); g.ba = vec_in(c.name + ".ba", D);
        if (two) { g.gb = vec_in(c.name + ".gb", D); g.bb = vec_in(c.name + ".bb", D); }
        if (nper) { g.pervec = vec_in(c.name + ".pervec", (size_t)nper * D); g.ldper = D; }
        if (nsteps) { g.stepvec = vec_in(c.name + ".stepvec", (size_t)nsteps * D); g.ldstep = D; }
        g.d_step = step_in(step);
        CK(launch_rowgemm(g, true, nullptr));
        finish(c.name.c_str());
        out = plane_back(g.Ohi, M, D, rows, false, c.name.c_str());
    } else if (epi == 1) {
        g.act = 1;
        g.Chi = plane_out(rows, N); g.c_rows = rows;
        CK(launch_rowgemm(g, false, nullptr));
        finish(c.name.c_str());
        out = plane_back(g.Chi, M, N, rows, false, c.name.c_str());
    } else {
        // attention-ready slabs [Bm * H][Tqp][dh], Tqp = Tq rounded up to 32: natural output [M][q | k | v]
        if (N != 3 * D || M % Tq) die("case %s: act 2 wants N = 1536 and whole samples", c.name.c_str());
        const int Bm = M / Tq, Tqp = (Tq + 31) / 32 * 32;
        const size_t slab = (size_t)Bm * NH * Tqp * DH;
        __bf16* dst[3];
        for (auto& p : dst) p = (__bf16*)upload(std::vector<uint16_t>(slab, SENTINEL));
        g.act = 2; g.Qhi = dst[0]; g.Khi = dst[1]; g.Vhi = dst[2]; g.H = NH; g.dh = DH; g.Tqp = Tqp; g.qscale = qscale();
        CK(launch_rowgemm(g, false, nullptr));
        finish(c.name.c_str());
        out.assign((size_t)M * N, 0.f);
        std::vector<uint16_t> s(slab);
        for (int which = 0; which < 3; ++which) {
            CK(hipMemcpy(s.data(), dst[which], slab * 2, hipMemcpyDeviceToHost));
            for (int b = 0; b < Bm; ++b)
                for (int hd = 0; hd < NH; ++hd)
                    for (int t = 0; t < Tqp; ++t)
                        for (int e = 0; e < DH; ++e) {
                            const uint16_t v = s[attn_slab_off(NH, Tqp, DH, b, hd, t, e)];
                            if (t < Tq) out[(size_t)(b * Tq + t) * N + which * D + hd * DH + e] = bf2f(v);
                            else if (v != SENTINEL) die("case %s: padding row %d of slab %d was written", c.name.c_str(), t, which);
                        }
        }
    }
    write_f32(c.name + ".out", out);
}

// <name> f16 Bm Tq rows nper nsteps step        (L = 1, steps = 0: the stack of one evaluation, k_layers<false>)
static void run_layers(const Case& c) {
    const bool f16 = c[0];
    const int Bm = c[1], Tq = c[2], rows = c[3], nper = c[4], nsteps = c[5], step = c[6], M = Bm * Tq;
    if (!layers_supported(D, FF, NH, Tq, 1)) die("case %s: Tq = %d is not supported by k_layers", c.name.c_str(), Tq);
    if (rows < M || (nper && nper < Bm) || (nsteps && step >= nsteps)) die("case %s: inconsistent sizes", c.name.c_str());
    LayersArgs g{};
    g.h = plane_in(read_f32(c.name + ".h", (size_t)M * D), M, D, rows, f16, "h");
    g.out = plane_out(rows, D);
    g.rows = rows; g.Bm = Bm; g.Tq = Tq; g.L = 1; g.lw[0] = layer_wts(f16); g.qscale = qscale(); g.steps = 0; g.B = Bm; g.f16 = f16;
    if (nper) { g.pervec = vec_in(c.name + ".pervec", (size_t)nper * D); g.ldper = D; }
    if (nsteps) { g.stepvec = vec_in(c.name + ".stepvec", (size_t)nsteps * D); g.ldstep = D; }
    g.d_step = step_in(step);
    CK(configure_layers());
    CK(launch_layers(g, nullptr));
    finish(c.name.c_str());
    write_f32(c.name + ".out", plane_back(g.out, M, D, rows, f16, c.name.c_str()));
}

int main(int argc, char** argv) {
    if (argc != 3) die("usage: plain_stage_check <attn | long | mlp | rowgemm | layers> <dir>");
    const std::string kernel = argv[1];
    g_dir = argv[2];
    if (kernel != "attn" && kernel != "long" && kernel != "mlp" && kernel != "rowgemm" && kernel != "layers") die("unknown kernel %s", kernel.c_str());
    for (const Case& c : read_cases(kernel)) {
        if (kernel == "attn") run_attn(c, false);
        else if (kernel == "long") run_attn(c, true);
        else if (kernel == "mlp") run_mlp(c);
        else if (kernel == "rowgemm") run_rowgemm(c);
        else run_layers(c);
    }
    return 0;
}
