// The ST-GCN recogniser's BLOCK PLAN and small-graph geometry as pure host functions (no device, no HIP): what rgn_stgcn_set_blocks accepts and what
// rgn_stgcn_finalize derives from the vertex count. Shared by rgn_stgcn.hip and tools/sg_plan_check.cpp (a stand-alone program built with
// -fsanitize=address,undefined).
//
// A plan is the (out_channels, stride) list of the st_gcn blocks; everything else follows from st_gcn.__init__ (eval/a2m/recognition/models/stgcn.py:183-219,
// eval/unconstrained/models/stgcn.py:157-201): block 0 has no residual branch, a later block has the convolved shortcut exactly when its channel count or its
// stride changes and the identity otherwise.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace rgn {

struct SgBlockDef { int ci, co, stride; bool res_conv, res_id; };   // ci == 0: the first block's input (in_channels / persons)

constexpr int SG_MIN_BLOCKS = 2, SG_MAX_BLOCKS = 10;

// the ten blocks of eval/a2m/recognition/models/stgcn.py:51-62
inline std::vector<SgBlockDef> sg_default_plan() {
    return {{0, 64, 1, false, false},   {64, 64, 1, false, true},   {64, 64, 1, false, true},   {64, 64, 1, false, true},   {64, 128, 2, true, false},
            {128, 128, 1, false, true}, {128, 128, 1, false, true}, {128, 256, 2, true, false}, {256, 256, 1, false, true}, {256, 256, 1, false, true}};
}

// Accepted: 2 to 10 blocks; channels from {64, 128, 256}, never decreasing, the last block 256 (the features are [N, 256]); stride 1 or 2, stride 2 only
// on a block whose channel count changes (block 0's input is not a channel count of the plan: its stride is 1). Returns true and fills `plan`, or false
// with the offending entry named in `err`.
inline bool sg_plan_check(int32_t n_blocks, const int32_t* out_channels, const int32_t* strides, std::vector<SgBlockDef>* plan, std::string* err) {
    auto fail = [&](const std::string& m) {
        if (err) *err = m;
        return false;
    };
    if (!out_channels || !strides) return fail("null out_channels / strides");
    if (n_blocks < SG_MIN_BLOCKS || n_blocks > SG_MAX_BLOCKS)
        return fail("n_blocks = " + std::to_string(n_blocks) + " outside [" + std::to_string(SG_MIN_BLOCKS) + ", " + std::to_string(SG_MAX_BLOCKS) + "]");
    std::vector<SgBlockDef> p((size_t)n_blocks);
    for (int i = 0; i < n_blocks; ++i) {
        const int co = out_channels[i], st = strides[i], ci = i ? out_channels[i - 1] : 0;
        const std::string at = "[" + std::to_string(i) + "]";
        if (co != 64 && co != 128 && co != 256) return fail("out_channels" + at + " = " + std::to_string(co) + " is not 64, 128 or 256");
        if (i && co < ci) return fail("out_channels" + at + " = " + std::to_string(co) + " decreases from " + std::to_string(ci));
        if (st != 1 && st != 2) return fail("strides" + at + " = " + std::to_string(st) + " is not 1 or 2");
        if (st == 2 && (i == 0 || co == ci)) return fail("strides" + at + " = 2 on a block whose channel count does not change");
        const bool changes = i > 0 && (co != ci || st != 1);
        p[(size_t)i] = SgBlockDef{ci, co, st, changes, i > 0 && !changes};
    }
    if (out_channels[n_blocks - 1] != 256) return fail("out_channels[" + std::to_string(n_blocks - 1) + "] = " + std::to_string(out_channels[n_blocks - 1]) + ": the last block must have 256 channels");
    if (plan) plan->swap(p);
    return true;
}

// Small graphs (V < 28) run on a padded vertex count Vp = max(16, 4 ceil(V / 4)) in {16, 20, 24, 28}; larger graphs run as they are.
inline int sg_padded_nodes(int V) { return V >= 28 ? V : (V <= 16 ? 16 : (V + 3) / 4 * 4); }
// The period of the per-vertex bias table (add_mod of the plane kernels: a 32-row MFMA tile may wrap it at most once, so it is >= 28): the table of Vp
// rows replicated to P = Vp ceil(28 / Vp) rows - 32, 40, 48 or 28; V >= 28: V itself
inline int sg_bias_period(int V) {
    const int Vp = sg_padded_nodes(V);
    return V >= 28 ? V : Vp * ((28 + Vp - 1) / Vp);
}
// block index of a state_dict key "st_gcn_networks.<i>." / "edge_importance.<i>", or -1
inline int sg_key_block(const std::string& key) {
    for (const char* pre : {"st_gcn_networks.", "edge_importance."}) {
        const std::string p(pre);
        if (key.compare(0, p.size(), p) == 0) {
            size_t j = p.size();
            long v = 0;
            bool any = false;
            while (j < key.size() && key[j] >= '0' && key[j] <= '9' && v < 100000) {
                v = v * 10 + (key[j] - '0');
                ++j;
                any = true;
            }
            if (any && (j == key.size() || key[j] == '.')) return (int)v;
        }
    }
    return -1;
}

}  // namespace rgn
