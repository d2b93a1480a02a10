// Host-only check of the argument handling of the GRU classifier's entry points (rgn_gru_create, rgn_gru_forward and the NULL-handle answers of the
// rest) and of the LDS plan every accepted geometry gets, for a sanitizer build on a machine WITHOUT a GPU: every bad argument must come back with its
// status and its text in rgn_gru_last_error(NULL) before the handle or the device is touched (the "device" pointers are never dereferenced), and an
// accepted geometry must get as far as the device (RGN_ERR_HIP, "no HIP device") or, with a GPU, a handle. Build rgn_gru.hip with the host sanitizers
// and link the other objects of build/obj as they are:
//
//   S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off $S -c regennet_amd/csrc/rgn_gru.hip -o build/gru_san.o
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c tools/gru_args_check.cpp -o build/gru_args_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined build/gru_args_check.o build/gru_san.o $(ls build/obj/*.o | grep -v rgn_gru) -o build/gru_args_check
//   build/gru_args_check
#include "../include/regennet_hip.h"
#include "../regennet_amd/csrc/rgn_gru_check.h"

#include <cstdio>
#include <cstring>

namespace {

int failures = 0;

void report(const char* fn, const char* what, int rc, int want_rc, const char* text) {
    const char* err = rgn_gru_last_error(nullptr);
    const size_t len = std::strlen(fn);
    const bool ok = rc == want_rc && err && std::strncmp(err, fn, len) == 0 && std::strncmp(err + len, ": ", 2) == 0 && std::strstr(err, text);
    std::printf("%-16s %-34s rc %d  %s%s\n", fn, what, rc, err ? err : "(null)", ok ? "" : "   <-- UNEXPECTED");
    failures += !ok;
}

rgn_gru_config good() { return rgn_gru_config{72, 128, 2, 30, 12, 0}; }

void expect_create(const char* what, const rgn_gru_config& c, int want_rc, const char* text) {
    rgn_gru_handle h = nullptr;
    int rc = rgn_gru_create(&c, &h);
    if (rc == RGN_OK) {                       // a machine with a GPU: an accepted geometry is a handle
        rgn_gru_destroy(h);
        if (want_rc == RGN_ERR_HIP) {
            std::printf("%-16s %-34s rc 0 (a device is present)\n", "rgn_gru_create", what);
            return;
        }
    }
    report("rgn_gru_create", what, rc, want_rc, text);
}

struct Fwd {
    int32_t N = 3, T = 5;
    const float *x, *h0;
    const int64_t* lengths;
    float *features, *logits;
};
void expect_forward(const char* what, const Fwd& a, const char* text) {
    report("rgn_gru_forward", what, rgn_gru_forward(nullptr, a.N, a.T, a.x, a.lengths, a.h0, a.features, a.logits, nullptr), RGN_ERR_INVALID_ARG, text);
}

}  // namespace

int main() {
    rgn_gru_handle h = nullptr;
    report("rgn_gru_create", "null config", rgn_gru_create(nullptr, &h), RGN_ERR_INVALID_ARG, "null");
    rgn_gru_config c = good();
    report("rgn_gru_create", "null out", rgn_gru_create(&c, nullptr), RGN_ERR_INVALID_ARG, "null");
    expect_create("the reference geometry", c, RGN_ERR_HIP, "no HIP device");
    const int bad_h[] = {0, -32, 16, 100, 257, 288};
    for (int v : bad_h) { c = good(); c.hidden_size = v; expect_create("hidden_size outside", c, RGN_ERR_UNSUPPORTED, "hidden_size"); }
    const int bad_l[] = {0, -1, 5};
    for (int v : bad_l) { c = good(); c.num_layers = v; expect_create("num_layers outside", c, RGN_ERR_UNSUPPORTED, "num_layers"); }
    const int bad_i[] = {0, -7, 1025};
    for (int v : bad_i) { c = good(); c.input_size = v; expect_create("input_size outside", c, RGN_ERR_UNSUPPORTED, "input_size"); }
    const int bad_f[] = {0, 65};
    for (int v : bad_f) { c = good(); c.lin1_size = v; expect_create("lin1_size outside", c, RGN_ERR_UNSUPPORTED, "lin1_size"); }
    const int bad_c[] = {0, 1025};
    for (int v : bad_c) { c = good(); c.output_size = v; expect_create("output_size outside", c, RGN_ERR_UNSUPPORTED, "output_size"); }
    c = good(); c.device = -1; expect_create("device -1", c, RGN_ERR_HIP, "no HIP device");

    // every accepted geometry: reaches the device, and its LDS image fits a workgroup with at least one staged frame
    int plans = 0;
    for (int H = 32; H <= 256; H += 32)
        for (int L = 1; L <= 4; ++L)
            for (int I : {1, 9, 16, 54, 72, 96, 1000, 1024}) {
                const rgn::GruLds p = rgn::gru_lds_plan(I, H, L);
                const bool ok = p.tc >= 1 && p.tc <= 8 && p.bytes <= rgn::GRU_LDS_LIMIT && p.x_ld % 4 == 0 && p.h_ld % 4 == 0 && p.x_off % 4 == 0 &&
                                p.x_ld >= I + 4 && p.feat_off == L * rgn::GRU_TILE * p.h_ld;
                if (!ok) std::printf("gru_lds_plan(%d, %d, %d): tc %d bytes %d   <-- UNEXPECTED\n", I, H, L, p.tc, p.bytes);
                failures += !ok;
                ++plans;
                if (I == 1024 || I == 1) {
                    c = rgn_gru_config{I, H, L, I == 1 ? 1 : 64, I == 1 ? 1 : 1024, 0};
                    expect_create("an accepted geometry", c, RGN_ERR_HIP, "no HIP device");
                }
            }
    std::printf("%d LDS plans checked\n", plans);

    float dummy[4] = {0, 0, 0, 0};              // stands for device memory: never read
    int64_t dl[4] = {1, 1, 1, 1};
    Fwd ok;
    ok.x = ok.h0 = dummy; ok.lengths = dl; ok.features = ok.logits = dummy;
    expect_forward("all arguments good", ok, "null handle");
    Fwd a = ok; a.x = nullptr; expect_forward("null x", a, "null x");
    a = ok; a.lengths = nullptr; expect_forward("null lengths", a, "null x / lengths");
    a = ok; a.h0 = nullptr; expect_forward("null h0", a, "h0");
    a = ok; a.features = nullptr; expect_forward("features null (allowed)", a, "null handle");
    a = ok; a.logits = nullptr; expect_forward("logits null (allowed)", a, "null handle");
    a = ok; a.features = a.logits = nullptr; expect_forward("both outputs null", a, "both null");
    a = ok; a.N = 0; expect_forward("N = 0", a, "N < 1");
    a = ok; a.N = -4; expect_forward("N = -4", a, "N < 1");
    a = ok; a.N = 0x7fffffff; expect_forward("N = 2^31 - 1 (allowed)", a, "null handle");
    a = ok; a.T = 0; expect_forward("T = 0", a, "T outside");
    a = ok; a.T = 4097; expect_forward("T = 4097", a, "T outside");
    a = ok; a.T = 4096; expect_forward("T = 4096 (allowed)", a, "null handle");

    int32_t flag = 0;
    const int64_t shape[2] = {384, 72};
    const bool nulls = rgn_gru_destroy(nullptr) == RGN_ERR_INVALID_ARG && rgn_gru_finalize(nullptr) == RGN_ERR_INVALID_ARG &&
                       rgn_gru_load_weight(nullptr, "recurrent.weight_ih_l0", dummy, shape, 2) == RGN_ERR_INVALID_ARG &&
                       rgn_gru_length_status(nullptr, &flag) == RGN_ERR_INVALID_ARG;
    std::printf("null handles %s\n", nulls ? "refused" : "NOT refused   <-- UNEXPECTED");
    failures += !nulls;
    std::printf("%d unexpected\n", failures);
    return failures ? 1 : 0;
}
