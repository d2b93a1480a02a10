// Host-only check of the argument handling of the text-to-motion evaluator's entry points (rgn_t2m_*) and of the workspace plan, for a sanitizer build
// on a machine WITHOUT a GPU: every bad argument must come back with its status and its text in rgn_t2m_last_error(NULL) before the handle or the
// device is touched (the "device" pointers are never dereferenced), and an accepted geometry must get as far as the device (RGN_ERR_HIP, "no HIP
// device") or, with a GPU, a handle. Build rgn_t2m.hip with the host sanitizers and link the other objects of build/obj as they are:
//
//   S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off $S -c regennet_amd/csrc/rgn_t2m.hip -o build/t2m_san.o
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c tools/t2m_args_check.cpp -o build/t2m_args_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined build/t2m_args_check.o build/t2m_san.o $(ls build/obj/*.o | grep -v rgn_t2m) -o build/t2m_args_check
//   build/t2m_args_check
#include "../include/regennet_hip.h"
#include "../regennet_amd/csrc/rgn_t2m_check.h"

#include <cstdio>
#include <cstring>

namespace {

int failures = 0;

void report(const char* fn, const char* what, int rc, int want_rc, const char* text) {
    const char* err = rgn_t2m_last_error(nullptr);
    const size_t len = std::strlen(fn);
    const bool ok = rc == want_rc && err && std::strncmp(err, fn, len) == 0 && std::strncmp(err + len, ": ", 2) == 0 && std::strstr(err, text);
    std::printf("%-26s %-34s rc %d  %s%s\n", fn, what, rc, err ? err : "(null)", ok ? "" : "   <-- UNEXPECTED");
    failures += !ok;
}

rgn_t2m_config good() { return rgn_t2m_config{0, 263, 512, 512, 1024, 300, 15, 512, 512, 4}; }

void expect_create(const char* what, const rgn_t2m_config& c, int want_rc, const char* text) {
    rgn_t2m_handle h = nullptr;
    int rc = rgn_t2m_create(&c, &h);
    if (rc == RGN_OK) {                       // a machine with a GPU: an accepted geometry is a handle
        rgn_t2m_destroy(h);
        if (want_rc == RGN_ERR_HIP) {
            std::printf("%-26s %-34s rc 0 (a device is present)\n", "rgn_t2m_create", what);
            return;
        }
    }
    report("rgn_t2m_create", what, rc, want_rc, text);
}

float dummy[4] = {0, 0, 0, 0};                // stands for device memory: never read
int64_t dl[4] = {1, 1, 1, 1};
int32_t di[4] = {0, 0, 0, 0};

void expect_motion(const char* what, int N, int T, const float* m, const int64_t* l, float* out, void* work, const char* text) {
    report("rgn_t2m_motion_embeddings", what, rgn_t2m_motion_embeddings(nullptr, N, T, m, l, out, work, 1 << 20, nullptr), RGN_ERR_INVALID_ARG, text);
}
void expect_text(const char* what, int N, int Lw, const float* w, const float* p, const int64_t* l, float* out, void* work, const char* text) {
    report("rgn_t2m_text_embeddings", what, rgn_t2m_text_embeddings(nullptr, N, Lw, w, p, l, out, work, 1 << 20, nullptr), RGN_ERR_INVALID_ARG, text);
}
void expect_match(const char* what, const float* t, const float* m, int N, int D, int group, float* diag, int32_t* rank, int want, const char* text) {
    const int rc = rgn_t2m_match(0, t, m, N, D, group, diag, rank, nullptr);
    if (rc == RGN_OK && want == RGN_ERR_HIP) return;      // (never reached without real device memory; kept for symmetry)
    report("rgn_t2m_match", what, rc, want, text);
}

}  // namespace

int main() {
    rgn_t2m_handle h = nullptr;
    report("rgn_t2m_create", "null config", rgn_t2m_create(nullptr, &h), RGN_ERR_INVALID_ARG, "null");
    rgn_t2m_config c = good();
    report("rgn_t2m_create", "null out", rgn_t2m_create(&c, nullptr), RGN_ERR_INVALID_ARG, "null");
    expect_create("the reference geometry", c, RGN_ERR_HIP, "no HIP device");
    c.dim_pose = 251; expect_create("the KIT geometry", c, RGN_ERR_HIP, "no HIP device");
    for (int v : {0, 4, 1025}) { c = good(); c.dim_pose = v; expect_create("dim_pose outside", c, RGN_ERR_UNSUPPORTED, "dim_pose"); }
    for (int v : {0, -64, 32, 100, 1088}) {
        c = good(); c.movement_hidden = v; expect_create("movement_hidden outside", c, RGN_ERR_UNSUPPORTED, "movement_hidden");
        c = good(); c.movement_latent = v; expect_create("movement_latent outside", c, RGN_ERR_UNSUPPORTED, "movement_latent");
        c = good(); c.motion_hidden = v; expect_create("motion_hidden outside", c, RGN_ERR_UNSUPPORTED, "motion_hidden");
        c = good(); c.text_hidden = v; expect_create("text_hidden outside", c, RGN_ERR_UNSUPPORTED, "text_hidden");
    }
    for (int v : {0, 3, 301, 1028}) { c = good(); c.dim_word = v; expect_create("dim_word outside", c, RGN_ERR_UNSUPPORTED, "dim_word"); }
    for (int v : {0, 1025}) { c = good(); c.dim_pos_ohot = v; expect_create("dim_pos_ohot outside", c, RGN_ERR_UNSUPPORTED, "dim_pos_ohot"); }
    for (int v : {0, 2, 510, 1028}) { c = good(); c.coemb = v; expect_create("coemb outside", c, RGN_ERR_UNSUPPORTED, "coemb"); }
    for (int v : {0, 2, 8}) { c = good(); c.unit_length = v; expect_create("unit_length not 4", c, RGN_ERR_UNSUPPORTED, "unit_length"); }
    c = good(); c.device = -1; expect_create("device -1", c, RGN_ERR_HIP, "no HIP device");
    for (int H = 64; H <= 1024; H += 64) {
        c = rgn_t2m_config{0, H == 64 ? 5 : 1024, H, 1088 - H, H, H == 64 ? 4 : 1024, H == 64 ? 1 : 1024, 1088 - H, H == 64 ? 4 : 1024, 4};
        expect_create("an accepted geometry", c, RGN_ERR_HIP, "no HIP device");
    }

    // the workspace plan: aligned, disjoint, monotone in N, T and Lw
    const rgn::T2mGeom g{263, 512, 512, 1024, 300, 15, 512, 512};
    int plans = 0;
    size_t prev = 0;
    for (int N : {1, 2, 17, 32, 1024, 1 << 19})
        for (int T : {4, 7, 64, 196, 4096})
            for (int Lw : {1, 22, 256}) {
                const rgn::T2mPlan m = rgn::t2m_motion_plan(g, N, T), t = rgn::t2m_text_plan(g, N, Lw);
                const size_t tot = rgn::t2m_workspace_bytes(g, N, T, Lw);
                bool ok = tot >= m.total && tot >= t.total && m.lens < m.a && m.a < m.b && m.b < m.c && m.c < m.emb && m.emb < m.gi && m.gi < m.hcat &&
                          m.hcat < m.y1 && m.y1 < m.y2 && m.y2 < m.total && t.lens < t.a && t.a < t.emb && t.emb < t.gi && t.gi < t.hcat && t.y2 < t.total;
                for (size_t o : {m.a, m.b, m.c, m.emb, m.gi, m.hcat, m.y1, m.y2, m.total, t.a, t.emb, t.gi, t.hcat, t.y1, t.y2, t.total}) ok = ok && o % 16 == 0;
                ok = ok && tot >= rgn::t2m_workspace_bytes(g, N > 1 ? N - 1 : 1, T, Lw) && tot >= rgn::t2m_workspace_bytes(g, N, T > 4 ? T - 1 : 4, Lw) &&
                     tot >= rgn::t2m_workspace_bytes(g, N, T, Lw > 1 ? Lw - 1 : 1);
                if (!ok) std::printf("workspace plan (%d, %d, %d): %zu   <-- UNEXPECTED\n", N, T, Lw, tot);
                failures += !ok;
                prev = tot;
                ++plans;
            }
    // ... and over consecutive values: never shrinking along N, T or Lw, strictly growing along N
    int steps = 0;
    for (int T : {4, 196})
        for (int Lw : {1, 22}) {
            size_t last = 0;
            for (int N = 1; N <= 300; ++N, ++steps) {
                const size_t b = rgn::t2m_workspace_bytes(g, N, T, Lw);
                if (b <= last) { std::printf("workspace shrinks at N %d T %d Lw %d   <-- UNEXPECTED\n", N, T, Lw); ++failures; }
                last = b;
            }
        }
    for (int N : {1, 33}) {
        size_t last = 0;
        for (int T = 4; T <= 4096; ++T, ++steps) {
            const size_t b = rgn::t2m_workspace_bytes(g, N, T, 1);
            if (b < last) { std::printf("workspace shrinks at N %d T %d   <-- UNEXPECTED\n", N, T); ++failures; }
            last = b;
        }
        last = 0;
        for (int Lw = 1; Lw <= 256; ++Lw, ++steps) {
            const size_t b = rgn::t2m_workspace_bytes(g, N, 4, Lw);
            if (b < last) { std::printf("workspace shrinks at N %d Lw %d   <-- UNEXPECTED\n", N, Lw); ++failures; }
            last = b;
        }
    }
    std::printf("%d workspace plans checked (largest %zu bytes), %d consecutive steps swept\n", plans, prev, steps);
    const bool t12 = rgn::t2m_t1(196) == 98 && rgn::t2m_t2(196) == 49 && rgn::t2m_t1(7) == 3 && rgn::t2m_t2(7) == 1 && rgn::t2m_t2(4) == 1;
    std::printf("frame counts %s\n", t12 ? "as the convolutions give them" : "WRONG   <-- UNEXPECTED");
    failures += !t12;

    void* work = dummy;
    expect_motion("all arguments good", 3, 196, dummy, dl, dummy, work, "null handle");
    expect_motion("null motions", 3, 196, nullptr, dl, dummy, work, "null motions");
    expect_motion("null m_lens", 3, 196, dummy, nullptr, dummy, work, "m_lens");
    expect_motion("null output", 3, 196, dummy, dl, nullptr, work, "output");
    expect_motion("null workspace", 3, 196, dummy, dl, dummy, nullptr, "null workspace");
    expect_motion("N = 0", 0, 196, dummy, dl, dummy, work, "N < 1");
    expect_motion("N = -2", -2, 196, dummy, dl, dummy, work, "N < 1");
    expect_motion("N = 2^19 + 1", (1 << 19) + 1, 196, dummy, dl, dummy, work, "N above");
    expect_motion("T = 3", 3, 3, dummy, dl, dummy, work, "T outside");
    expect_motion("T = 4097", 3, 4097, dummy, dl, dummy, work, "T outside");
    expect_motion("T = 4 (allowed)", 3, 4, dummy, dl, dummy, work, "null handle");
    expect_motion("T = 4096 (allowed)", 3, 4096, dummy, dl, dummy, work, "null handle");
    report("rgn_t2m_movements", "null x", rgn_t2m_movements(nullptr, 3, 196, 263, nullptr, nullptr, dummy, work, 1, nullptr), RGN_ERR_INVALID_ARG, "null motions");
    report("rgn_t2m_movements", "m_lens null (allowed)", rgn_t2m_movements(nullptr, 3, 196, 263, dummy, nullptr, dummy, work, 1, nullptr), RGN_ERR_INVALID_ARG,
           "null handle");
    report("rgn_t2m_encode_movements", "T2 = 0", rgn_t2m_encode_movements(nullptr, 3, 0, dummy, dl, dummy, work, 1, nullptr), RGN_ERR_INVALID_ARG, "T2 outside");
    report("rgn_t2m_encode_movements", "T2 = 1025", rgn_t2m_encode_movements(nullptr, 3, 1025, dummy, dl, dummy, work, 1, nullptr), RGN_ERR_INVALID_ARG,
           "T2 outside");
    report("rgn_t2m_encode_movements", "null lens", rgn_t2m_encode_movements(nullptr, 3, 49, dummy, nullptr, dummy, work, 1, nullptr), RGN_ERR_INVALID_ARG,
           "m_lens");
    report("rgn_t2m_encode_movements", "all arguments good", rgn_t2m_encode_movements(nullptr, 3, 49, dummy, dl, dummy, work, 1, nullptr), RGN_ERR_INVALID_ARG,
           "null handle");

    expect_text("all arguments good", 3, 22, dummy, dummy, dl, dummy, work, "null handle");
    expect_text("null word_embs", 3, 22, nullptr, dummy, dl, dummy, work, "null word_embs");
    expect_text("null pos_ohot", 3, 22, dummy, nullptr, dl, dummy, work, "pos_ohot");
    expect_text("null cap_lens", 3, 22, dummy, dummy, nullptr, dummy, work, "cap_lens");
    expect_text("null output", 3, 22, dummy, dummy, dl, nullptr, work, "output");
    expect_text("null workspace", 3, 22, dummy, dummy, dl, dummy, nullptr, "null workspace");
    expect_text("N = 0", 0, 22, dummy, dummy, dl, dummy, work, "N < 1");
    expect_text("Lw = 0", 3, 0, dummy, dummy, dl, dummy, work, "Lw outside");
    expect_text("Lw = 257", 3, 257, dummy, dummy, dl, dummy, work, "Lw outside");
    expect_text("Lw = 256 (allowed)", 3, 256, dummy, dummy, dl, dummy, work, "null handle");

    expect_match("null text", nullptr, dummy, 4, 4, 4, dummy, di, RGN_ERR_INVALID_ARG, "null text");
    expect_match("null motion", dummy, nullptr, 4, 4, 4, dummy, di, RGN_ERR_INVALID_ARG, "motion");
    expect_match("null diag", dummy, dummy, 4, 4, 4, nullptr, di, RGN_ERR_INVALID_ARG, "diag");
    expect_match("null rank", dummy, dummy, 4, 4, 4, dummy, nullptr, RGN_ERR_INVALID_ARG, "rank");
    expect_match("N = 0", dummy, dummy, 0, 4, 4, dummy, di, RGN_ERR_INVALID_ARG, "N < 1");
    for (int D : {0, 2, 6, 1028}) expect_match("D outside", dummy, dummy, 4, D, 4, dummy, di, RGN_ERR_INVALID_ARG, "D must be");
    for (int G : {0, -1, 33}) expect_match("group outside", dummy, dummy, 4, 4, G, dummy, di, RGN_ERR_INVALID_ARG, "group outside");

    size_t bytes = 0;
    int32_t flag = 0;
    const int64_t shape[3] = {512, 259, 4};
    const bool nulls = rgn_t2m_destroy(nullptr) == RGN_ERR_INVALID_ARG && rgn_t2m_finalize(nullptr) == RGN_ERR_INVALID_ARG &&
                       rgn_t2m_load_weight(nullptr, "movement_encoder.main.0.weight", dummy, shape, 3) == RGN_ERR_INVALID_ARG &&
                       rgn_t2m_length_status(nullptr, &flag) == RGN_ERR_INVALID_ARG && rgn_t2m_workspace(nullptr, 1, 4, 1, &bytes) == RGN_ERR_INVALID_ARG;
    std::printf("null handles %s\n", nulls ? "refused" : "NOT refused   <-- UNEXPECTED");
    failures += !nulls;
    std::printf("%d unexpected\n", failures);
    return failures ? 1 : 0;
}
