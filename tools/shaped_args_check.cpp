// Host-only check of the argument handling of rgn_rot2xyz_shaped and rgn_rot2verts_shaped, for a sanitizer build on a machine WITHOUT a GPU: every
// bad argument must come back as RGN_ERR_INVALID_ARG with its text in rgn_last_error(NULL) / rgn_body_last_error(NULL), before the handle or the
// device is touched (the handle is NULL throughout and the "device" pointers are never dereferenced). What needs a body handle - nb larger than the
// body's, a short workspace - is in tests/test_rot2xyz_shaped_gpu.py. Build rgn_abi.cpp and rgn_lbs.hip with the host sanitizers and link the
// other objects of build/obj as they are:
//
//   S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c regennet_amd/csrc/rgn_abi.cpp -o build/abi_san.o
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c regennet_amd/csrc/rgn_lbs.hip -o build/lbs_san.o
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c tools/shaped_args_check.cpp -o build/shaped_args_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined build/shaped_args_check.o build/abi_san.o build/lbs_san.o \
//         $(ls build/obj/*.o | grep -v -e rgn_abi -e rgn_lbs) -o build/shaped_args_check
//   build/shaped_args_check
#include "../include/regennet_hip.h"

#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Args {
    const float* x;
    float* out;
    const float* rest;
    const int32_t* parents;
    const float* sj;
    const float* betas;
    const float* glob_rot = nullptr;
    int32_t B = 1, T = 2, J = 3, nb = 10, rep = RGN_POSE_ROT6D, P = 1, flags = RGN_R2X_TRANSLATION | RGN_R2X_GLOB;
    int64_t sb = 10, sp = 0, st = 0;
};

int failures = 0;

void report(const char* fn, const char* what, int rc, const char* err, const char* text) {
    const size_t n = std::strlen(fn);
    const bool ok = rc == RGN_ERR_INVALID_ARG && err && std::strncmp(err, fn, n) == 0 && std::strncmp(err + n, ": ", 2) == 0 && std::strstr(err, text);
    std::printf("%-22s %-26s rc %d  %s%s\n", fn, what, rc, err ? err : "(null)", ok ? "" : "   <-- UNEXPECTED");
    failures += !ok;
}

// joints: J is an argument; vertices: J belongs to the (absent) body handle, so the J and parent-table refusals are the joints call's alone
void expect(const char* what, const Args& a, const char* text, bool joints_only = false) {
    int rc = rgn_rot2xyz_shaped(nullptr, a.x, nullptr, a.B, a.T, a.J, a.rest, a.parents, a.sj, a.nb, a.betas, a.sb, a.sp, a.st, a.rep, a.P, a.flags, a.glob_rot,
                                a.out, nullptr, nullptr);
    report("rgn_rot2xyz_shaped", what, rc, rgn_last_error(nullptr), text);
    if (joints_only) return;
    rc = rgn_rot2verts_shaped(nullptr, a.x, nullptr, a.B, a.T, a.rest, a.parents, a.sj, a.nb, a.betas, a.sb, a.sp, a.st, a.rep, a.P, a.flags, a.glob_rot, a.out,
                              nullptr, nullptr, 0, nullptr);
    report("rgn_rot2verts_shaped", what, rc, rgn_body_last_error(nullptr), text);
}

}  // namespace

int main() {
    float dummy[4] = {0, 0, 0, 0};                  // stands for device memory: never read
    std::vector<float> rest(3 * 65, 0.f);
    std::vector<int32_t> chain(65);
    for (int i = 0; i < 65; ++i) chain[i] = i - 1;
    const float glob_rot[3] = {0.1f, 0.2f, 0.3f};
    Args ok;
    ok.x = ok.sj = ok.betas = dummy;
    ok.out = dummy;
    ok.rest = rest.data();
    ok.parents = chain.data();

    expect("all arguments good", ok, "null handle");
    Args a = ok; a.x = nullptr; expect("null x", a, "null x");
    a = ok; a.out = nullptr; expect("null output", a, "null x");
    a = ok; a.rest = nullptr; expect("null rest_joints", a, "null x");
    a = ok; a.parents = nullptr; expect("null parents", a, "null x");
    a = ok; a.sj = nullptr; expect("null shape_joints_dev", a, "null shape_joints_dev or betas_dev");
    a = ok; a.betas = nullptr; expect("null betas_dev", a, "null shape_joints_dev or betas_dev");
    a = ok; a.nb = 0; expect("nb = 0", a, "nb outside [1, 16]");
    a = ok; a.nb = 17; expect("nb = 17", a, "nb outside [1, 16]");
    a = ok; a.nb = 16; a.sb = 16; expect("nb = 16 (the limit)", a, "null handle");
    a = ok; a.sb = -1; expect("stride_b = -1", a, "negative beta stride");
    a = ok; a.sp = -10; expect("stride_p = -10", a, "negative beta stride");
    a = ok; a.st = -1; expect("stride_t = -1", a, "negative beta stride");
    a = ok; a.sb = 0; expect("every stride 0", a, "null handle");
    a = ok; a.B = 0; expect("B = 0", a, "B < 1");
    a = ok; a.T = 0; expect("T = 0", a, "T < 1");
    a = ok; a.P = 0; expect("num_person = 0", a, "num_person < 1");
    a = ok; a.rep = 4; expect("pose_rep = 4", a, "unknown pose_rep");
    a = ok; a.flags = 8; expect("unknown flag", a, "unknown flag");
    a = ok; a.flags = RGN_R2X_TRANSLATION; expect("no GLOB, no glob_rot", a, "glob_rot is required");
    a = ok; a.flags = RGN_R2X_TRANSLATION; a.glob_rot = glob_rot; expect("no GLOB with glob_rot", a, "null handle");
    a = ok; a.J = 0; expect("J = 0", a, "J outside [1, 64]", true);
    a = ok; a.J = 65; expect("J = 65", a, "J outside [1, 64]", true);
    a = ok; a.J = 64; expect("J = 64 (the limit)", a, "null handle", true);
    const int32_t p_root[3] = {0, 0, 1}, p_self[3] = {-1, 1, 1}, p_neg[3] = {-1, 0, -1};
    a = ok; a.parents = p_root; expect("parents[0] = 0", a, "parents[0] != -1", true);
    a = ok; a.parents = p_self; expect("parents[1] = 1", a, "parents[1]", true);
    a = ok; a.parents = p_neg; expect("parents[2] = -1", a, "parents[2]", true);
    std::printf("%d unexpected\n", failures);
    return failures ? 1 : 0;
}
