// Host-only check of rgn_hml_to_joints' argument handling (csrc/rgn_hml_check.h through rgn_abi.cpp), for a sanitizer build on a machine WITHOUT a
// GPU: every bad argument must come back as RGN_ERR_INVALID_ARG with its text in rgn_last_error(NULL), before the handle or the device is touched
// (the handle is NULL throughout and the "device" pointers are never dereferenced). Build rgn_abi.cpp with the host sanitizers and link the other
// objects of build/obj as they are:
//
//   S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c regennet_amd/csrc/rgn_abi.cpp -o build/abi_san.o
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c tools/hml_args_check.cpp -o build/hml_args_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined build/hml_args_check.o build/abi_san.o $(ls build/obj/*.o | grep -v rgn_abi) -o build/hml_args_check
//   build/hml_args_check
#include "../include/regennet_hip.h"
#include "../regennet_amd/csrc/rgn_hml_check.h"

#include <cstdio>
#include <cstring>

namespace {

struct Args {
    const float *x, *mean, *stdv;
    float* xyz;
    int32_t B = 2, T = 5, D = 263, J = 22;
};

int failures = 0;

void expect(const char* what, const Args& a, const char* text) {
    const int rc = rgn_hml_to_joints(nullptr, a.x, a.mean, a.stdv, a.B, a.T, a.D, a.J, a.xyz, nullptr);
    const char* err = rgn_last_error(nullptr);
    const bool ok = rc == RGN_ERR_INVALID_ARG && err && std::strncmp(err, "rgn_hml_to_joints: ", 19) == 0 && std::strstr(err, text);
    // ... and the rule itself says the same as the entry point (a NULL handle is the entry point's own complaint)
    const std::string why = rgn::hml_check_args(a.x, a.mean, a.stdv, a.B, a.T, a.D, a.J, a.xyz);
    const bool same = why.empty() ? std::strcmp(text, "null handle") == 0 : (err && std::strstr(err, why.c_str()) != nullptr);
    std::printf("%-34s rc %d  %s%s\n", what, rc, err ? err : "(null)", ok && same ? "" : "   <-- UNEXPECTED");
    failures += !(ok && same);
}

}  // namespace

int main() {
    float dummy[4] = {0, 0, 0, 0};                  // stands for device memory: never read
    Args ok;
    ok.x = ok.mean = ok.stdv = dummy;
    ok.xyz = dummy;

    expect("all arguments good", ok, "null handle");
    Args a = ok; a.mean = a.stdv = nullptr; expect("no statistics (allowed)", a, "null handle");
    a = ok; a.x = nullptr; expect("null x", a, "null x or xyz");
    a = ok; a.xyz = nullptr; expect("null xyz", a, "null x or xyz");
    a = ok; a.mean = nullptr; expect("std without mean", a, "go together");
    a = ok; a.stdv = nullptr; expect("mean without std", a, "go together");
    a = ok; a.B = 0; expect("B = 0", a, "B < 1");
    a = ok; a.B = -7; expect("B = -7", a, "B < 1");
    a = ok; a.B = 0x7fffffff; expect("B = 2^31 - 1 (allowed)", a, "null handle");
    a = ok; a.T = 0; expect("T = 0", a, "T = 0 outside [1, 4096]");
    a = ok; a.T = -1; expect("T = -1", a, "outside [1, 4096]");
    a = ok; a.T = 4097; expect("T = 4097", a, "T = 4097 outside [1, 4096]");
    a = ok; a.T = 4096; expect("T = 4096 (allowed)", a, "null handle");
    a = ok; a.T = 1; expect("T = 1 (allowed)", a, "null handle");
    a = ok; a.J = 1; a.D = 11; expect("J = 1", a, "J = 1 outside [2, 64]");
    a = ok; a.J = 65; a.D = 779; expect("J = 65", a, "J = 65 outside [2, 64]");
    a = ok; a.J = 2; a.D = 23; expect("J = 2 (allowed)", a, "null handle");
    a = ok; a.J = 64; a.D = 767; expect("J = 64 (allowed)", a, "null handle");
    a = ok; a.J = 21; a.D = 251; expect("KIT: J = 21, D = 251 (allowed)", a, "null handle");
    a = ok; a.D = 251; expect("22 joints on 251 rows", a, "D = 251 rows, 12 J - 1 = 263 expected");
    a = ok; a.J = 21; expect("21 joints on 263 rows", a, "D = 263 rows, 12 J - 1 = 251 expected");
    a = ok; a.D = 0; expect("D = 0", a, "D = 0 rows");
    a = ok; a.J = 0x7fffffff; expect("J = 2^31 - 1", a, "outside [2, 64]");
    std::printf("%d unexpected\n", failures);
    return failures ? 1 : 0;
}
