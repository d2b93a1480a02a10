// Host-only check of the argument handling of rgn_poly_mmd, rgn_poly_mmd_workspace, rgn_knn_radius and rgn_manifold_hits, for a sanitizer build on a
// machine WITHOUT a GPU: every bad argument must come back as RGN_ERR_INVALID_ARG with its text in rgn_last_error(NULL), before the device is touched
// (`device` is -1 throughout - refused last, so a call with good arguments answers "device < 0" - and the "device" pointers are never dereferenced).
// Build rgn_abi.cpp with the host sanitizers and link the other objects of build/obj as they are:
//
//   S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c regennet_amd/csrc/rgn_abi.cpp -o build/abi_san.o
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c tools/metrics_args_check.cpp -o build/metrics_args_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined build/metrics_args_check.o build/abi_san.o $(ls build/obj/*.o | grep -v rgn_abi) -o build/metrics_args_check
//   build/metrics_args_check
//
// This build runs on the CPU only, never on a GPU machine.
#include "../include/regennet_hip.h"

#include <cmath>
#include <cstdio>
#include <cstring>

namespace {

struct Args {
    const float *x, *y, *a, *b, *radii;
    const int32_t *idx_x, *idx_y;
    double *mmds, *vars;
    void* work;
    float* radii_out;
    uint8_t* flags;
    int32_t* count;
    int32_t Nx = 130, Ny = 97, D = 256, S = 5, m = 70, degree = 3, N = 100, M = 90, k = 3;
    float gamma = 1.0f / 256, coef0 = 1.0f;
    long long work_bytes = -1;          // -1: what rgn_poly_mmd_workspace asks for
};

int failures = 0;

void report(const char* fn, const char* what, int rc, const char* text) {
    const char* err = rgn_last_error(nullptr);
    const size_t len = std::strlen(fn);
    const bool ok = rc == RGN_ERR_INVALID_ARG && err && std::strncmp(err, fn, len) == 0 && std::strncmp(err + len, ": ", 2) == 0 && std::strstr(err, text);
    std::printf("%-22s %-32s rc %d  %s%s\n", fn, what, rc, err ? err : "(null)", ok ? "" : "   <-- UNEXPECTED");
    failures += !ok;
}

void expect_mmd(const char* what, const Args& a, const char* text) {
    uint64_t need = 1ull << 40;
    if (a.work_bytes >= 0) need = (uint64_t)a.work_bytes;
    else (void)rgn_poly_mmd_workspace(a.S, a.m, &need);
    report("rgn_poly_mmd", what,
           rgn_poly_mmd(-1, a.x, a.Nx, a.y, a.Ny, a.D, a.idx_x, a.idx_y, a.S, a.m, a.degree, a.gamma, a.coef0, a.mmds, a.vars, a.work, need, nullptr), text);
}
void expect_knn(const char* what, const Args& a, const char* text) {
    report("rgn_knn_radius", what, rgn_knn_radius(-1, a.a, a.N, a.D, a.k, a.radii_out, nullptr), text);
}
void expect_hits(const char* what, const Args& a, const char* text) {
    report("rgn_manifold_hits", what, rgn_manifold_hits(-1, a.b, a.M, a.a, a.radii, a.N, a.D, a.flags, a.count, nullptr), text);
}

}  // namespace

int main() {
    alignas(16) static char dummy[64];              // stands for device memory: never read
    Args ok;
    ok.x = ok.y = ok.a = ok.b = ok.radii = reinterpret_cast<const float*>(dummy);
    ok.idx_x = ok.idx_y = reinterpret_cast<const int32_t*>(dummy);
    ok.mmds = ok.vars = reinterpret_cast<double*>(dummy);
    ok.work = dummy;
    ok.radii_out = reinterpret_cast<float*>(dummy);
    ok.flags = reinterpret_cast<uint8_t*>(dummy);
    ok.count = reinterpret_cast<int32_t*>(dummy);

    expect_mmd("all arguments good", ok, "device < 0");
    Args a = ok; a.x = nullptr; expect_mmd("null x", a, "null");
    a = ok; a.y = nullptr; expect_mmd("null y", a, "null");
    a = ok; a.idx_x = nullptr; expect_mmd("null idx_x", a, "null");
    a = ok; a.idx_y = nullptr; expect_mmd("null idx_y", a, "null");
    a = ok; a.mmds = nullptr; expect_mmd("null mmds", a, "null");
    a = ok; a.vars = nullptr; expect_mmd("null vars", a, "null");
    a = ok; a.work = nullptr; expect_mmd("null work", a, "null");
    a = ok; a.D = 254; expect_mmd("D = 254", a, "no multiple of 4");
    a = ok; a.D = 1028; expect_mmd("D = 1028", a, "[4, 1024]");
    a = ok; a.D = 0; expect_mmd("D = 0", a, "[4, 1024]");
    a = ok; a.D = 4; expect_mmd("D = 4 (allowed)", a, "device < 0");
    a = ok; a.D = 1024; expect_mmd("D = 1024 (allowed)", a, "device < 0");
    a = ok; a.S = 0; expect_mmd("S = 0", a, "S = 0");
    a = ok; a.S = 65536; expect_mmd("S = 65536", a, "[1, 65535]");
    a = ok; a.S = 65535; a.m = 3; expect_mmd("S = 65535, m = 3 (allowed)", a, "device < 0");
    a = ok; a.m = 2; expect_mmd("m = 2", a, "[3, 4096]");
    a = ok; a.m = 4097; expect_mmd("m = 4097", a, "[3, 4096]");
    a = ok; a.m = 4096; expect_mmd("m = 4096 (allowed)", a, "device < 0");
    a = ok; a.Nx = 1; expect_mmd("Nx = 1", a, "Nx < 2");
    a = ok; a.Ny = 0; expect_mmd("Ny = 0", a, "Ny < 2");
    a = ok; a.degree = 0; expect_mmd("degree = 0", a, "[1, 8]");
    a = ok; a.degree = 9; expect_mmd("degree = 9", a, "[1, 8]");
    a = ok; a.gamma = NAN; expect_mmd("gamma = NaN", a, "not finite");
    a = ok; a.coef0 = INFINITY; expect_mmd("coef0 = inf", a, "not finite");
    a = ok; a.x = reinterpret_cast<const float*>(dummy + 4); expect_mmd("x + 4 bytes", a, "not 16-byte aligned");
    a = ok; a.work = dummy + 8; expect_mmd("work + 8 bytes", a, "work is not 16-byte aligned");
    a = ok; a.work_bytes = 0; expect_mmd("work_bytes = 0", a, "needed (rgn_poly_mmd_workspace)");
    a = ok; a.work_bytes = 8ll * 5 * 10 * 128 - 1; expect_mmd("work_bytes one short", a, "needed (rgn_poly_mmd_workspace)");
    a = ok; a.work_bytes = 8ll * 5 * 10 * 128; expect_mmd("work_bytes exact (allowed)", a, "device < 0");

    uint64_t need = 0;
    report("rgn_poly_mmd_workspace", "null nbytes", rgn_poly_mmd_workspace(5, 70, nullptr), "null nbytes");
    report("rgn_poly_mmd_workspace", "m = 2", rgn_poly_mmd_workspace(5, 2, &need), "[3, 4096]");
    report("rgn_poly_mmd_workspace", "S = 0", rgn_poly_mmd_workspace(0, 70, &need), "S = 0");
    const int rc = rgn_poly_mmd_workspace(100, 1000, &need);
    std::printf("%-22s %-32s rc %d  %llu bytes%s\n", "rgn_poly_mmd_workspace", "S = 100, m = 1000", rc, (unsigned long long)need,
                rc == RGN_OK && need == 8ull * 100 * 24 * 1024 ? "" : "   <-- UNEXPECTED");
    failures += !(rc == RGN_OK && need == 8ull * 100 * 24 * 1024);

    expect_knn("all arguments good", ok, "device < 0");
    a = ok; a.a = nullptr; expect_knn("null a", a, "null");
    a = ok; a.radii_out = nullptr; expect_knn("null radii", a, "null");
    a = ok; a.D = 30; expect_knn("D = 30", a, "no multiple of 4");
    a = ok; a.D = 2048; expect_knn("D = 2048", a, "[4, 1024]");
    a = ok; a.N = 0; expect_knn("N = 0", a, "N = 0");
    a = ok; a.N = (1 << 24) + 1; expect_knn("N = 2^24 + 1", a, "[1, 2^24]");
    a = ok; a.N = 1 << 24; expect_knn("N = 2^24 (allowed)", a, "device < 0");
    a = ok; a.k = 0; expect_knn("k = 0", a, "[1, 15]");
    a = ok; a.k = 16; expect_knn("k = 16", a, "[1, 15]");
    a = ok; a.k = 15; expect_knn("k = 15 (allowed)", a, "device < 0");
    a = ok; a.k = 8; a.N = 8; expect_knn("k = N = 8", a, "is not below N = 8");
    a = ok; a.k = 8; a.N = 9; expect_knn("k = 8, N = 9 (allowed)", a, "device < 0");
    a = ok; a.a = reinterpret_cast<const float*>(dummy + 8); expect_knn("a + 8 bytes", a, "not 16-byte aligned");

    expect_hits("all arguments good", ok, "device < 0");
    a = ok; a.b = nullptr; expect_hits("null b", a, "null");
    a = ok; a.a = nullptr; expect_hits("null a", a, "null");
    a = ok; a.radii = nullptr; expect_hits("null radii", a, "null");
    a = ok; a.flags = nullptr; expect_hits("null flags", a, "null");
    a = ok; a.count = nullptr; expect_hits("null count", a, "null");
    a = ok; a.D = 7; expect_hits("D = 7", a, "no multiple of 4");
    a = ok; a.M = 0; expect_hits("M = 0", a, "M = 0");
    a = ok; a.N = -4; expect_hits("N = -4", a, "N = -4");
    a = ok; a.M = 1; a.N = 1; expect_hits("M = N = 1 (allowed)", a, "device < 0");
    a = ok; a.b = reinterpret_cast<const float*>(dummy + 4); expect_hits("b + 4 bytes", a, "not 16-byte aligned");
    std::printf("%d unexpected\n", failures);
    return failures ? 1 : 0;
}
