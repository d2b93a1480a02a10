// The geometry and argument rules of the GRU action classifier (rgn_gru_create / rgn_gru_forward) as pure host code: what the kernels of rgn_gru.hip
// accept, decided before the device is touched. Shared by rgn_gru.hip and tools/gru_args_check.cpp (a stand-alone program built with the host
// sanitizers), so the rules have one definition.
#pragma once
#include <cstdint>
#include <string>

namespace rgn {

constexpr int GRU_TILE = 16;          // sequences per workgroup: the column count of the 16x16x4 fp32 MFMA
constexpr int GRU_WAVES = 8;          // waves per workgroup; a wave owns tiles of 16 hidden units
constexpr int GRU_KC = 16;            // k granule of the packed weights: one 16-byte load per lane feeds four MFMAs
constexpr int GRU_MAX_LAYERS = 4;
constexpr int GRU_MAX_T = 4096;
constexpr int GRU_LDS_LIMIT = 160 * 1024;

inline int gru_pad_k(int k) { return (k + GRU_KC - 1) / GRU_KC * GRU_KC; }

// nullptr when the geometry is served; otherwise the reason
inline const char* gru_geometry_error(int input_size, int hidden_size, int num_layers, int lin1_size, int output_size) {
    if (hidden_size < 32 || hidden_size > 256 || hidden_size % 32) return "hidden_size must be a multiple of 32 in [32, 256]";
    if (num_layers < 1 || num_layers > GRU_MAX_LAYERS) return "num_layers must be in [1, 4]";
    if (input_size < 1 || input_size > 1024) return "input_size must be in [1, 1024]";
    if (lin1_size < 1 || lin1_size > 64) return "lin1_size must be in [1, 64]";
    if (output_size < 1 || output_size > 1024) return "output_size must be in [1, 1024]";
    return nullptr;
}

// LDS image of one workgroup, in floats: the state of every layer, the head's features, the tile's lengths, then `tc` staged frames of the input
struct GruLds {
    int h_ld, x_ld, h_off, feat_off, len_off, x_off, tc, bytes;
};
inline GruLds gru_lds_plan(int input_size, int hidden_size, int num_layers) {
    GruLds p{};
    p.h_ld = hidden_size + 4;                  // + 4: the 16 rows a quad-of-k read touches start 4 banks apart
    p.x_ld = gru_pad_k(input_size) + 4;
    p.h_off = 0;
    p.feat_off = p.h_off + num_layers * GRU_TILE * p.h_ld;
    p.len_off = p.feat_off + GRU_TILE * 64;
    p.x_off = p.len_off + GRU_TILE;
    const int frame = GRU_TILE * p.x_ld;
    const int room = GRU_LDS_LIMIT / 4 - p.x_off;
    int tc = room / frame;
    p.tc = tc > 8 ? 8 : tc;                    // >= 1 for every accepted geometry (static_assert below states the worst case)
    p.bytes = (p.x_off + p.tc * frame) * 4;
    return p;
}
static_assert((GRU_MAX_LAYERS * GRU_TILE * 260 + GRU_TILE * 64 + GRU_TILE + GRU_TILE * 1028) * 4 <= GRU_LDS_LIMIT, "the largest geometry must fit one frame");

// nullptr when a forward call's arguments are served
inline const char* gru_forward_error(int64_t N, int64_t T, const void* x, const void* lengths, const void* h0, const void* features, const void* logits) {
    if (!x || !lengths || !h0) return "null x / lengths / h0";
    if (!features && !logits) return "features and logits both null";
    if (N < 1) return "N < 1";
    if (T < 1 || T > GRU_MAX_T) return "T outside [1, 4096]";
    return nullptr;
}

}  // namespace rgn
