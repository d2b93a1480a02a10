// Host-only check of rgn_loss_terms' argument handling, for a sanitizer build on a machine WITHOUT a GPU: every bad argument must come back as
// RGN_ERR_INVALID_ARG with its text in rgn_last_error(NULL), before the handle or the device is touched (the handle is NULL throughout and the
// "device" pointers are never dereferenced). Build rgn_abi.cpp with the host sanitizers and link the other objects of build/obj as they are:
//
//   S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c regennet_amd/csrc/rgn_abi.cpp -o build/abi_san.o
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c tools/loss_args_check.cpp -o build/loss_args_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined build/loss_args_check.o build/abi_san.o $(ls build/obj/*.o | grep -v rgn_abi) -o build/loss_args_check
//   build/loss_args_check
#include "../include/regennet_hip.h"

#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Args {
    const float *target, *output, *cmotion;
    const uint8_t* mask;
    float* terms;
    const float* rest;
    const int32_t* parents;
    const int32_t* foot;
    int32_t B = 1, T = 2, R = 4, J = 3, row = 3, flags = RGN_LOSS_FC;
};

int failures = 0;

void expect(const char* what, const Args& a, const char* text) {
    const int rc = rgn_loss_terms(nullptr, a.target, a.output, a.cmotion, a.mask, a.B, a.T, a.R, a.J, a.rest, a.parents, a.foot, a.row, 0.01f, a.flags,
                                  a.terms, nullptr);
    const char* err = rgn_last_error(nullptr);
    const bool ok = rc == RGN_ERR_INVALID_ARG && err && std::strncmp(err, "rgn_loss_terms: ", 16) == 0 && std::strstr(err, text);
    std::printf("%-28s rc %d  %s%s\n", what, rc, err ? err : "(null)", ok ? "" : "   <-- UNEXPECTED");
    failures += !ok;
}

}  // namespace

int main() {
    float dummy[4] = {0, 0, 0, 0};                  // stands for device memory: never read
    uint8_t dmask[4] = {1, 1, 1, 1};
    std::vector<float> rest(3 * 65, 0.f);
    std::vector<int32_t> chain(65);
    for (int i = 0; i < 65; ++i) chain[i] = i - 1;
    const int32_t foot[4] = {0, 1, 2, 1};
    Args ok;
    ok.target = ok.output = ok.cmotion = dummy;
    ok.mask = dmask;
    ok.terms = dummy;
    ok.rest = rest.data();
    ok.parents = chain.data();
    ok.foot = foot;

    expect("all arguments good", ok, "null handle");
    Args a = ok; a.target = nullptr; expect("null target", a, "null");
    a = ok; a.output = nullptr; expect("null output", a, "null");
    a = ok; a.cmotion = nullptr; expect("null cmotion", a, "null");
    a = ok; a.mask = nullptr; expect("null mask", a, "null");
    a = ok; a.terms = nullptr; expect("null terms", a, "null");
    a = ok; a.rest = nullptr; expect("null rest_joints", a, "null");
    a = ok; a.parents = nullptr; expect("null parents", a, "null");
    a = ok; a.foot = nullptr; expect("null foot_joints", a, "null");
    a = ok; a.B = 0; expect("B = 0", a, "B < 1");
    a = ok; a.T = 0; expect("T = 0", a, "T < 1");
    a = ok; a.J = 0; a.R = 1; expect("J = 0", a, "J outside [1, 64]");
    a = ok; a.J = 65; a.R = 66; expect("J = 65", a, "J outside [1, 64]");
    a = ok; a.J = 64; a.R = 65; a.row = 64; expect("J = 64 (the limit)", a, "null handle");
    const int32_t p_root[3] = {0, 0, 1}, p_self[3] = {-1, 1, 1}, p_fwd[3] = {-1, 0, 2}, p_neg[3] = {-1, 0, -1};
    a = ok; a.parents = p_root; expect("parents[0] = 0", a, "parents[0] != -1");
    a = ok; a.parents = p_self; expect("parents[1] = 1", a, "parents[1]");
    a = ok; a.parents = p_fwd; expect("parents[2] = 2", a, "parents[2]");
    a = ok; a.parents = p_neg; expect("parents[2] = -1", a, "parents[2]");
    a = ok; a.R = 3; expect("R = J", a, "J + 1 = 4");
    a = ok; a.R = 5; expect("R = J + 2", a, "J + 1 = 4");
    const int32_t f_hi[4] = {0, 1, 3, 1}, f_lo[4] = {-1, 1, 2, 1};
    a = ok; a.foot = f_hi; expect("foot joint = J", a, "foot_joints[2] = 3");
    a = ok; a.foot = f_lo; expect("foot joint = -1", a, "foot_joints[0] = -1");
    a = ok; a.row = 4; expect("transl_row = R", a, "transl_row 4");
    a = ok; a.row = -1; expect("transl_row = -1", a, "transl_row -1");
    a = ok; a.flags = 2; expect("unknown flag", a, "unknown flag");
    std::printf("%d unexpected\n", failures);
    return failures ? 1 : 0;
}
