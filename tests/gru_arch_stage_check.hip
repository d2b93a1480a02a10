// Stand-alone driver of tests/test_gru_arch_stage_gpu.py: runs the GRU denoiser's layer stack alone, one scan per case, through launch_gru_stack, and
// hands the top layer's rows back.
//
//   gru_arch_stage_check <dir>
//
// <dir>/cases.txt lists the cases, one per line: name d L S N nseg order. Every tensor is a raw little-endian fp32 file in natural layout:
//   <dir>/<name>.w.f32    per layer  weight_ih [3d][d] | weight_hh [3d][d] | bias_ih [3d] | bias_hh [3d]   (nn.GRU's, gate order r, z, n)
//   <dir>/<name>.x.f32    [nseg][S][N][d]   the stack's input rows
//   <dir>/<name>.out.f32  [nseg][S][N][d]   written here: the top layer's state at every step
// The device buffers hold NP = N + 5 sequences per step, so every case has padding sequences whether or not N fills its last group of 16:
//   order 0  row (seg, s, n) at ((seg S + s) NP + n) d     steps outermost, the sequence stride is one row      (the 'batch' scan's order)
//   order 1  row (seg, s, n) at ((seg NP + n) S + s) d     sequences outermost, the step stride is one row      (the 'frames' scan's order)
// Input and output sit MARGIN rows inside their allocations. The scan runs twice: once with NaN in every padding sequence of x, in the whole state ring
// and (as the fill pattern 0xFFFFFFFF) in the whole output buffer, once with zeros in the padding sequences and the ring. The two results must agree
// bit for bit, every element of the output buffer and of the ring's margin outside the rows the scan covers must still hold its fill, and no covered
// element may: a step-0 cell that multiplied an unwritten state, a ring slot read before it was written or a padding sequence that reached a result
// all come back as NaN or as a difference. No timing, no loop, no retry. Any HIP error, a refused argument set or a malformed case ends the program
// with the text and a non-zero status.
#include "rgn_internal.h"

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
    fprintf(stderr, "gru_arch_stage_check: ");
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    exit(1);
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) die("HIP error: %s at %s:%d (%s)", hipGetErrorString(e_), __FILE__, __LINE__, #x); } while (0)

constexpr uint32_t FILL = 0xFFFFFFFFu;
constexpr long MARGIN = 37, EXTRA = 5;
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
static uint32_t bits(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
}

struct Case { std::string name; int d, L, S, N, nseg, order; };

// one scan; pad: what the padding sequences of x and the whole ring hold beforehand. Returns the covered output rows in natural layout.
static std::vector<float> run_scan(const Case& c, const float* d_w, const std::vector<float>& x, float pad) {
    const long d = c.d, NP = c.N + EXTRA, rows = (long)c.nseg * c.S * NP;
    const long step = c.order == 0 ? NP * d : d, seq = c.order == 0 ? d : (long)c.S * d, seg = (long)c.S * NP * d;
    auto at = [&](int sg, int s, int n) { return MARGIN * d + sg * seg + s * step + n * seq; };
    const size_t nbuf = (size_t)(rows + 2 * MARGIN) * d;
    std::vector<float> hx(nbuf, pad);
    for (int sg = 0; sg < c.nseg; ++sg)
        for (int s = 0; s < c.S; ++s)
            for (int n = 0; n < c.N; ++n) memcpy(&hx[at(sg, s, n)], &x[(((size_t)sg * c.S + s) * c.N + n) * d], (size_t)d * 4);
    const size_t nring = gru_stack_ring_floats(c.d, c.L, c.nseg, c.N), nring_buf = nring + (size_t)MARGIN * d;
    std::vector<float> hring(nring_buf, pad);
    for (size_t i = nring; i < nring_buf; ++i) memcpy(&hring[i], &FILL, 4);
    float *dx, *dout, *dring;
    CK(hipMalloc(&dx, nbuf * 4));
    CK(hipMalloc(&dout, nbuf * 4));
    CK(hipMalloc(&dring, nring_buf * 4));
    CK(hipMemcpy(dx, hx.data(), nbuf * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dout, 0xFF, nbuf * 4));
    CK(hipMemcpy(dring, hring.data(), nring_buf * 4, hipMemcpyHostToDevice));

    GruStackArgs g{};
    g.w = d_w; g.x = dx + MARGIN * d; g.out = dout + MARGIN * d; g.ring = c.L > 1 ? dring : nullptr;
    g.x_step = g.o_step = step; g.x_seq = g.o_seq = seq; g.x_seg = g.o_seg = seg;
    g.d = c.d; g.L = c.L; g.S = c.S; g.N = c.N; g.nseg = c.nseg;
    if (const char* why = gru_stack_args_error(g)) die("%s: arguments refused: %s", c.name.c_str(), why);
    CK(launch_gru_stack(g, nullptr));
    CK(hipDeviceSynchronize());

    std::vector<float> hout(nbuf);
    CK(hipMemcpy(hout.data(), dout, nbuf * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hring.data(), dring, nring_buf * 4, hipMemcpyDeviceToHost));
    std::vector<char> covered(nbuf / d, 0);
    std::vector<float> out((size_t)c.nseg * c.S * c.N * d);
    for (int sg = 0; sg < c.nseg; ++sg)
        for (int s = 0; s < c.S; ++s)
            for (int n = 0; n < c.N; ++n) {
                covered[at(sg, s, n) / d] = 1;
                memcpy(&out[(((size_t)sg * c.S + s) * c.N + n) * d], &hout[at(sg, s, n)], (size_t)d * 4);
            }
    for (size_t r = 0; r < covered.size(); ++r)
        for (long k = 0; k < d; ++k) {
            const bool fill = bits(hout[r * d + k]) == FILL;
            if (!covered[r] && !fill) die("%s: output row %zu (outside the scan) column %ld was written", c.name.c_str(), r, k);
            if (covered[r] && fill) die("%s: output row %zu column %ld still holds the fill", c.name.c_str(), r, k);
        }
    for (size_t i = nring; i < nring_buf; ++i)
        if (bits(hring[i]) != FILL) die("%s: the ring's margin was written at float %zu", c.name.c_str(), i - nring);
    CK(hipFree(dx));
    CK(hipFree(dout));
    CK(hipFree(dring));
    return out;
}

int main(int argc, char** argv) {
    if (argc != 2) die("usage: gru_arch_stage_check <dir>");
    g_dir = argv[1];
    std::ifstream f(g_dir + "/cases.txt");
    if (!f) die("cannot open %s/cases.txt", g_dir.c_str());
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream is(line);
        Case c;
        if (!(is >> c.name >> c.d >> c.L >> c.S >> c.N >> c.nseg >> c.order) || (c.order != 0 && c.order != 1)) die("malformed case: %s", line.c_str());
        if (const char* why = gru_stack_geometry_error(c.d, c.L)) die("%s: %s", c.name.c_str(), why);
        if (c.S < 1 || c.N < 1 || c.nseg < 1) die("%s: empty scan", c.name.c_str());
        const size_t d = c.d, per = 6 * d * d + 6 * d;
        const std::vector<float> w = read_f32(c.name + ".w", per * c.L);
        std::vector<float> packed;
        for (int l = 0; l < c.L; ++l) {
            const float* p = &w[per * l];
            const std::vector<float> pl = gru_stack_pack_layer(p, p + 3 * d * d, p + 6 * d * d, p + 6 * d * d + 3 * d, c.d);
            if (pl.size() != gru_stack_layer_floats(c.d)) die("%s: packed layer size", c.name.c_str());
            packed.insert(packed.end(), pl.begin(), pl.end());
        }
        float* d_w;
        CK(hipMalloc(&d_w, packed.size() * 4));
        CK(hipMemcpy(d_w, packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
        const std::vector<float> x = read_f32(c.name + ".x", (size_t)c.nseg * c.S * c.N * d);
        const std::vector<float> a = run_scan(c, d_w, x, NAN), b = run_scan(c, d_w, x, 0.f);
        for (size_t i = 0; i < a.size(); ++i)
            if (bits(a[i]) != bits(b[i])) die("%s: NaN in the padding changed output float %zu (%.9g vs %.9g)", c.name.c_str(), i, a[i], b[i]);
        CK(hipFree(d_w));
        write_f32(c.name + ".out", a);
        printf("%s: ran, launches %d\n", c.name.c_str(), gru_stack_launches(c.S, c.L));
    }
    return 0;
}
