// Host-only check of the argument handling of rgn_q_sample_rows and rgn_vb_terms, for a sanitizer build on a machine WITHOUT a GPU: every bad
// argument must come back as RGN_ERR_INVALID_ARG with its text in rgn_last_error(NULL), before the handle or the device is touched (the handle is
// NULL throughout and the "device" pointers are never dereferenced). Build rgn_abi.cpp with the host sanitizers and link the other objects of
// build/obj as they are:
//
//   S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c regennet_amd/csrc/rgn_abi.cpp -o build/abi_san.o
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c tools/vb_args_check.cpp -o build/vb_args_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined build/vb_args_check.o build/abi_san.o $(ls build/obj/*.o | grep -v rgn_abi) -o build/vb_args_check
//   build/vb_args_check
#include "../include/regennet_hip.h"

#include <cstdio>
#include <cstring>

namespace {

struct Args {
    const float *x_start, *x_t, *output, *noise, *coef;
    const int32_t* t;
    float *out, *noise_out = nullptr;      // x_t_dev of rgn_q_sample_rows / terms_dev of rgn_vb_terms
    int32_t B = 2, N = 4, features = 3, T = 5, flags = RGN_VB_CLIP;
};

int failures = 0;

void report(const char* fn, const char* what, int rc, const char* text) {
    const char* err = rgn_last_error(nullptr);
    const size_t len = std::strlen(fn);
    const bool ok = rc == RGN_ERR_INVALID_ARG && err && std::strncmp(err, fn, len) == 0 && std::strncmp(err + len, ": ", 2) == 0 && std::strstr(err, text);
    std::printf("%-18s %-30s rc %d  %s%s\n", fn, what, rc, err ? err : "(null)", ok ? "" : "   <-- UNEXPECTED");
    failures += !ok;
}

void expect_q(const char* what, const Args& a, const char* text) {
    report("rgn_q_sample_rows", what,
           rgn_q_sample_rows(nullptr, a.x_start, a.noise, a.coef, a.t, a.B, a.N, a.features, a.T, 1234, 0, a.out, a.noise_out, nullptr), text);
}

void expect_vb(const char* what, const Args& a, const char* text) {
    report("rgn_vb_terms", what,
           rgn_vb_terms(nullptr, a.x_start, a.x_t, a.output, a.noise, a.t, a.coef, a.B, a.N, a.features, a.T, a.flags, a.out, nullptr), text);
}

}  // namespace

int main() {
    float dummy[4] = {0, 0, 0, 0};                  // stands for device memory: never read
    int32_t dt[4] = {0, 0, 0, 0};
    Args ok;
    ok.x_start = ok.x_t = ok.output = ok.noise = ok.coef = dummy;
    ok.t = dt;
    ok.out = dummy;

    for (int which = 0; which < 2; ++which) {
        auto expect = which ? expect_vb : expect_q;
        expect("all arguments good", ok, "null handle");
        Args a = ok; a.x_start = nullptr; expect("null x_start", a, "null");
        a = ok; a.coef = nullptr; expect("null coef", a, "null");
        a = ok; a.t = nullptr; expect("null t", a, "null");
        a = ok; a.out = nullptr; expect(which ? "null terms" : "null x_t", a, "null");
        a = ok; a.noise = nullptr; expect("null noise (allowed)", a, "null handle");
        a = ok; a.B = 0; expect("B = 0", a, "B < 1");
        a = ok; a.N = 0; expect("N = 0", a, "N < 1");
        a = ok; a.features = 0; expect("features = 0", a, "features < 1");
        a = ok; a.T = 0; expect("T = 0", a, "T < 1");
        a = ok; a.T = -3; expect("T = -3", a, "T < 1");
        a = ok; a.N = 5; expect("N = 5, B = 2", a, "no multiple of B = 2");
        a = ok; a.B = 1; a.N = 1; a.features = 1; a.T = 1; expect("one row of one element", a, "null handle");
        a = ok; a.features = 1 << 20; a.T = 4096; expect("a row of 2^32 elements", a, "more than 2^31 - 1");
        a = ok; a.features = 0x7fffffff; a.T = 1; expect("a row of 2^31 - 1 elements", a, "null handle");
    }
    Args a = ok; a.N = 65536; expect_q("N = 65536 (allowed)", a, "null handle");
    a = ok; a.B = 1; a.N = 0x7fffffff; a.features = 3; a.T = 100; expect_q("2^32 - 2 workgroups", a, "more than 2^31 - 1 workgroups");
    a = ok; a.B = 1; a.N = 0x7fffffff; a.features = 16; a.T = 16; expect_q("2^31 - 1 workgroups", a, "null handle");
    a = ok; a.noise = nullptr; a.T = 4097; expect_q("drawn noise, T = 4097", a, "T <= 4096");
    a = ok; a.noise = nullptr; a.T = 4096; expect_q("drawn noise, T = 4096", a, "null handle");
    a = ok; a.T = 4097; expect_q("given noise, T = 4097", a, "null handle");
    a = ok; a.noise = nullptr; a.features = (1 << 19) + 1; a.T = 2; expect_q("drawn noise, features 2^19+1", a, "features <= 2^19");
    a = ok; a.noise = nullptr; a.features = 1 << 19; a.T = 2; expect_q("drawn noise, features 2^19", a, "null handle");
    a = ok; a.noise_out = dummy; expect_q("noise_out given", a, "null handle");
    a = ok; a.x_t = nullptr; expect_vb("null x_t", a, "null");
    a = ok; a.output = nullptr; expect_vb("null output", a, "null");
    a = ok; a.flags = 2; expect_vb("unknown flag", a, "unknown flag");
    a = ok; a.flags = 0; expect_vb("no flag", a, "null handle");
    std::printf("%d unexpected\n", failures);
    return failures ? 1 : 0;
}
