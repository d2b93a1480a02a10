// Host-only check of rgn_body_set_joint_regressors' compaction and of the argument handling of the rgn_rot2joints entry points, for a sanitizer
// build on a machine WITHOUT a GPU.
//
// Part 1 (always): the compaction is host code with no device call (regennet_amd/csrc/rgn_lbs_compact.h); it is run here on small bodies and its
// result checked element by element against the definitions - S, the restricted planes, the permuted joint weights. This part needs no other
// object of the library:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer tools/joints_args_check.cpp -o build/joints_args_check
//   build/joints_args_check
//
// Part 2 (-DWITH_LIBRARY, linked like tools/shaped_args_check.cpp: rgn_lbs.hip built with the host sanitizers, the other objects as they are):
// every bad argument of rgn_body_set_joint_regressors / rgn_rot2joints / rgn_rot2joints_shaped that needs no body handle must come back as
// RGN_ERR_INVALID_ARG with its text in rgn_body_last_error(NULL), before the handle or the device is touched (the handle is NULL throughout and the
// "device" pointers are never dereferenced). What needs a body handle is in tests/test_rot2joints_gpu.py.
//
//   S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -c regennet_amd/csrc/rgn_lbs.hip -o build/lbs_san.o
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $S -DWITH_LIBRARY -c tools/joints_args_check.cpp -o build/joints_args_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined build/joints_args_check.o build/lbs_san.o \
//         $(ls build/obj/*.o | grep -v rgn_lbs) -o build/joints_args_check
#include "../regennet_amd/csrc/rgn_lbs_compact.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#ifdef WITH_LIBRARY
#include "../include/regennet_hip.h"
#endif

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

struct Body {
    rgn::LbsDims d;
    std::vector<float> vt, sd, pd, w;
};

Body make_body(int V, int J, int nb, bool pose, std::mt19937& rng) {
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    Body b;
    const int K = 9 * (J - 1);
    b.d = rgn::LbsDims{V, J, (J + 1) / 2 * 2, nb, (nb + 7) / 8 * 8, K, (K + 7) / 8 * 8, pose && J > 1};
    b.vt.resize((size_t)3 * V);
    b.sd.resize((size_t)3 * V * nb);
    b.pd.resize(b.d.pose ? (size_t)K * 3 * V : 0);
    b.w.resize((size_t)V * J);
    for (auto* a : {&b.vt, &b.sd, &b.pd, &b.w})
        for (float& x : *a) x = u(rng);
    return b;
}

// the compaction against its definition, for one body and one set of picks / regressor
void check_compaction(const Body& b, const std::vector<int32_t>& picks, int Jr, const std::vector<float>& reg, const char* label) {
    const rgn::LbsDims& d = b.d;
    rgn::LbsCompact c;
    const std::string why = rgn::lbs_compact(d, b.vt.data(), b.sd.data(), b.pd.data(), b.w.data(), (int)picks.size(), picks.data(), Jr, reg.data(), c);
    if (!why.empty()) {
        std::printf("FAILED: %s: %s\n", label, why.c_str());
        ++failures;
        return;
    }
    std::vector<int32_t> S;
    for (int v = 0; v < d.V; ++v) {
        bool used = std::find(picks.begin(), picks.end(), v) != picks.end();
        for (int r = 0; r < Jr; ++r) used = used || reg[(size_t)r * d.V + v] != 0.f;
        if (used) S.push_back(v);
    }
    const int Sp = S.empty() ? 32 : ((int)S.size() + 31) / 32 * 32;
    bool ok = c.S == S && c.nS == (int)S.size() && c.Sp == Sp && c.Np == (int)picks.size() && c.Jr == Jr;
    ok = ok && c.blob.size() == c.o_wj + (size_t)(Sp / 32) * 16 * 64;
    const float* bl = c.blob.data();
    for (int s = 0; ok && s < Sp; ++s) {
        const bool in = s < (int)S.size();
        const size_t v = in ? S[s] : 0;
        for (int cc = 0; cc < 3; ++cc) {
            ok = ok && bl[c.o_vtp + (size_t)cc * Sp + s] == (in ? b.vt[3 * v + cc] : 0.f);
            if (in) ok = ok && bl[c.o_vt + 3 * s + cc] == b.vt[3 * v + cc];
            for (int k = 0; k < d.nbp; ++k)
                ok = ok && bl[c.o_sdp + ((size_t)k * 3 + cc) * Sp + s] == (in && k < d.nb ? b.sd[(3 * v + cc) * d.nb + k] : 0.f);
            for (int k = 0; in && k < d.nb; ++k) ok = ok && bl[c.o_sd + ((size_t)3 * s + cc) * d.nb + k] == b.sd[(3 * v + cc) * d.nb + k];
            for (int k = 0; d.pose && k < d.Kp; ++k)
                ok = ok && bl[c.o_pd + ((size_t)k * 3 + cc) * Sp + s] == (in && k < d.K ? b.pd[(size_t)k * 3 * d.V + 3 * v + cc] : 0.f);
        }
        for (int j = 0; j < d.Jp; ++j) ok = ok && bl[c.o_wt + (size_t)j * Sp + s] == (in && j < d.J ? b.w[v * d.J + j] : 0.f);
    }
    ok = ok && c.o_pd == c.o_sdp + (size_t)d.nbp * 3 * Sp;            // the shape planes end where the posedirs planes begin
    // the joint weights: un-permute, compare with W[row][S[s]]; every picked row holds a single 1
    for (int t = 0; ok && t < Sp / 32; ++t)
        for (int q = 0; q < 16; ++q)
            for (int l = 0; l < 64; ++l) {
                const int row = l & 31, s = 32 * t + 8 * (q >> 2) + 4 * (l >> 5) + (q & 3);
                float want = 0.f;
                if (s < (int)S.size() && row < (int)picks.size()) want = S[s] == picks[row] ? 1.f : 0.f;
                else if (s < (int)S.size() && row < (int)picks.size() + Jr) want = reg[(size_t)(row - picks.size()) * d.V + S[s]];
                ok = ok && bl[c.o_wj + ((size_t)t * 16 + q) * 64 + l] == want;
            }
    std::printf("%-46s V %5d  J %2d  nb %2d  |S| %5zu  Sp %5d  %s\n", label, d.V, d.J, d.nb, S.size(), Sp, ok ? "ok" : "MISMATCH");
    failures += !ok;
}

void refuse(const Body& b, int Np, const int32_t* picks, int Jr, const float* reg, const char* text) {
    rgn::LbsCompact c;
    const std::string why = rgn::lbs_compact(b.d, b.vt.data(), b.sd.data(), b.pd.data(), b.w.data(), Np, picks, Jr, reg, c);
    const bool ok = why.find(text) != std::string::npos;
    std::printf("refused: %-60s %s\n", why.c_str(), ok ? "" : "   <-- UNEXPECTED");
    failures += !ok;
}

#ifdef WITH_LIBRARY
void report(const char* fn, const char* what, int rc, const char* text) {
    const char* err = rgn_body_last_error(nullptr);
    const size_t n = std::strlen(fn);
    const bool ok = rc == RGN_ERR_INVALID_ARG && err && std::strncmp(err, fn, n) == 0 && std::strncmp(err + n, ": ", 2) == 0 && std::strstr(err, text);
    std::printf("%-30s %-28s rc %d  %s%s\n", fn, what, rc, err ? err : "(null)", ok ? "" : "   <-- UNEXPECTED");
    failures += !ok;
}

struct Args {
    const float* x;
    float* out;
    const float* rest;
    const int32_t* parents;
    const float *sj, *betas;
    const float* glob_rot = nullptr;
    const int32_t* map;
    int32_t B = 1, T = 2, nb = 10, rep = RGN_POSE_ROT6D, P = 1, flags = RGN_R2X_TRANSLATION | RGN_R2X_GLOB, n_map = 3, root = 1;
    int64_t sb = 10, sp = 0, st = 0;
};

void both(const char* what, const Args& a, const char* text, bool shaped_only = false) {
    if (!shaped_only) {
        const int rc = rgn_rot2joints(nullptr, a.x, nullptr, a.B, a.T, a.rest, a.parents, a.rep, a.P, a.flags, a.glob_rot, nullptr, a.n_map, a.map, a.root, a.out,
                                      nullptr, nullptr, 0, nullptr);
        report("rgn_rot2joints", what, rc, text);
    }
    const int rc = rgn_rot2joints_shaped(nullptr, a.x, nullptr, a.B, a.T, a.rest, a.parents, a.sj, a.nb, a.betas, a.sb, a.sp, a.st, a.rep, a.P, a.flags, a.glob_rot,
                                         a.n_map, a.map, a.root, a.out, nullptr, nullptr, 0, nullptr);
    report("rgn_rot2joints_shaped", what, rc, text);
}
#endif

}  // namespace

int main() {
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    // ---- part 1: the compaction ----
    struct Case {
        int V, J, nb, Np, Jr, support;             // support 0: a dense regressor
        bool pose;
        const char* label;
    };
    const Case cases[] = {{1, 1, 0, 1, 0, 0, false, "one vertex, one joint, a pick"},        {33, 2, 3, 7, 0, 0, true, "picks alone"},
                          {70, 24, 10, 21, 9, 6, true, "the reference's counts"},            {130, 55, 10, 0, 5, 6, true, "a regressor alone"},
                          {1000, 24, 16, 16, 16, 0, true, "dense: S is every vertex"},       {64, 3, 1, 2, 1, 1, false, "no posedirs"},
                          {6890, 24, 10, 21, 9, 6, true, "a body model's size"}};
    for (const Case& k : cases) {
        const Body b = make_body(k.V, k.J, k.nb, k.pose, rng);
        std::vector<int32_t> picks(k.Np);
        for (auto& p : picks) p = (int32_t)(rng() % k.V);           // (repeats allowed)
        std::vector<float> reg((size_t)k.Jr * k.V, 0.f);
        for (int r = 0; r < k.Jr; ++r)
            for (int i = 0; i < (k.support ? k.support : k.V); ++i) reg[(size_t)r * k.V + (k.support ? rng() % k.V : i)] = 0.1f + std::fabs(u(rng)) * (i % 2 ? -1.f : 1.f);
        check_compaction(b, picks, k.Jr, reg, k.label);
    }
    {   // a regressor of zeros and no picks: S is empty, one tile of pad vertices
        const Body b = make_body(40, 2, 2, true, rng);
        check_compaction(b, {}, 3, std::vector<float>((size_t)3 * 40, 0.f), "an all-zero regressor");
        const int32_t ids[3] = {0, 39, 40}, neg[1] = {-1};
        std::vector<float> reg((size_t)2 * 40, 0.5f), bad = reg;
        bad[45] = std::numeric_limits<float>::infinity();
        refuse(b, 3, ids, 0, nullptr, "vertex_joints[2] outside [0, V)");
        refuse(b, 1, neg, 0, nullptr, "vertex_joints[0] outside [0, V)");
        refuse(b, 0, nullptr, 2, bad.data(), "regressor[1][5] is not finite");
        bad[45] = std::numeric_limits<float>::quiet_NaN();
        refuse(b, 0, nullptr, 2, bad.data(), "regressor[1][5] is not finite");
        refuse(b, 0, nullptr, 0, nullptr, "both 0");
        refuse(b, -1, ids, 1, reg.data(), "Np or Jr < 0");
        refuse(b, 2, ids, 31, reg.data(), "Np + Jr = 33 > 32");
        refuse(b, 2, nullptr, 1, reg.data(), "Np > 0 without vertex_joints");
        refuse(b, 2, ids, 1, nullptr, "Jr > 0 without a regressor");
    }
#ifdef WITH_LIBRARY
    // ---- part 2: the entry points' checks, NULL handle ----
    float dummy[4] = {0, 0, 0, 0};                  // stands for device memory: never read
    std::vector<float> rest(3 * 3, 0.f);
    const int32_t chain[3] = {-1, 0, 1}, map[3] = {0, 1, 1}, neg_map[3] = {0, -2, 1};
    std::vector<int32_t> long_map(65, 0);
    const float glob_rot[3] = {0.1f, 0.2f, 0.3f};
    Args ok;
    ok.x = ok.sj = ok.betas = dummy;
    ok.out = dummy;
    ok.rest = rest.data();
    ok.parents = chain;
    ok.map = map;
    both("all arguments good", ok, "null handle");
    Args a = ok; a.x = nullptr; both("null x", a, "null x");
    a = ok; a.out = nullptr; both("null joints", a, "null x");
    a = ok; a.rest = nullptr; both("null rest_joints", a, "null x");
    a = ok; a.parents = nullptr; both("null parents", a, "null x");
    a = ok; a.sj = nullptr; both("null shape_joints_dev", a, "null shape_joints_dev or betas_dev", true);
    a = ok; a.betas = nullptr; both("null betas_dev", a, "null shape_joints_dev or betas_dev", true);
    a = ok; a.nb = 0; both("nb = 0", a, "nb outside [1, 16]", true);
    a = ok; a.nb = 17; both("nb = 17", a, "nb outside [1, 16]", true);
    a = ok; a.st = -1; both("stride_t = -1", a, "negative beta stride", true);
    a = ok; a.B = 0; both("B = 0", a, "B < 1");
    a = ok; a.T = 0; both("T = 0", a, "T < 1");
    a = ok; a.P = 0; both("num_person = 0", a, "num_person < 1");
    a = ok; a.rep = 4; both("pose_rep = 4", a, "unknown pose_rep");
    a = ok; a.flags = 8; both("unknown flag", a, "unknown flag");
    a = ok; a.flags = RGN_R2X_TRANSLATION; both("no GLOB, no glob_rot", a, "glob_rot is required");
    a = ok; a.flags = RGN_R2X_TRANSLATION; a.glob_rot = glob_rot; both("no GLOB with glob_rot", a, "null handle");
    a = ok; a.n_map = 0; both("n_map = 0", a, "n_map outside [1, 64]");
    a = ok; a.n_map = 65; a.map = long_map.data(); both("n_map = 65", a, "n_map outside [1, 64]");
    a = ok; a.n_map = 64; a.map = long_map.data(); both("n_map = 64 (the limit)", a, "null handle");
    a = ok; a.map = nullptr; both("null map", a, "null map");
    a = ok; a.root = 3; both("root = n_map", a, "root outside [0, n_map)");
    a = ok; a.root = -1; both("root = -1", a, "root outside [0, n_map)");
    a = ok; a.map = neg_map; both("map[1] = -2", a, "map[1] < 0");
    const int32_t ids[4] = {0, 1, 2, 3};
    report("rgn_body_set_joint_regressors", "good counts", rgn_body_set_joint_regressors(nullptr, 4, ids, 2, dummy), "null handle");
    report("rgn_body_set_joint_regressors", "Np + Jr = 33", rgn_body_set_joint_regressors(nullptr, 30, ids, 3, dummy), "Np + Jr = 33 > 32");
    report("rgn_body_set_joint_regressors", "Np = Jr = 0", rgn_body_set_joint_regressors(nullptr, 0, nullptr, 0, nullptr), "both 0");
    report("rgn_body_set_joint_regressors", "null vertex_joints", rgn_body_set_joint_regressors(nullptr, 4, nullptr, 2, dummy), "without vertex_joints");
    report("rgn_body_set_joint_regressors", "null regressor", rgn_body_set_joint_regressors(nullptr, 4, ids, 2, nullptr), "without a regressor");
#endif
    std::printf("%d unexpected\n", failures);
    return failures ? 1 : 0;
}
