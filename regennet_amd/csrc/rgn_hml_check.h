// The argument rules of rgn_hml_to_joints (rgn_hml.hip), host only and free of HIP: rgn_abi.cpp applies them before the handle or the device is
// touched, and tools/hml_args_check.cpp exercises them under the host sanitizers on a machine without a GPU.
//
// The HumanML3D / KIT feature vector of J joints (data_loaders/humanml/scripts/motion_process.py:355-361) has D = 12 J - 1 rows:
//   0                        rotation velocity of the root about Y
//   1, 2                     root velocity in the root's frame (x, z)
//   3                        root height
//   4 .. 3 (J-1) + 3         local joint positions, (x, y, z) per joint 1 .. J-1
//   then 6 (J-1) rotations, 3 J velocities and 4 foot contacts, which recover_from_ric never reads.
#pragma once
#include <cstdint>
#include <string>

namespace rgn {

constexpr int HML_MAX_FRAMES = 4096;     // rgn_create's own frame limit
constexpr int HML_MIN_JOINTS = 2;
constexpr int HML_MAX_JOINTS = 64;

// rows of the feature vector / the last row recover_from_ric reads
constexpr int hml_rows(int J) { return 12 * J - 1; }
constexpr int hml_last_read_row(int J) { return 3 * (J - 1) + 3; }

// The complaint's text (without the entry point's name), or empty when the call may go on to the handle.
inline std::string hml_check_args(const void* x, const void* mean, const void* stdv, int32_t B, int32_t T, int32_t D, int32_t J, const void* xyz) {
    if (!x || !xyz) return "null x or xyz";
    if ((mean == nullptr) != (stdv == nullptr)) return "mean and std go together: both given or both null";
    if (B < 1) return "B < 1";
    if (T < 1 || T > HML_MAX_FRAMES) return "T = " + std::to_string(T) + " outside [1, " + std::to_string(HML_MAX_FRAMES) + "]";
    if (J < HML_MIN_JOINTS || J > HML_MAX_JOINTS) return "J = " + std::to_string(J) + " outside [" + std::to_string(HML_MIN_JOINTS) + ", " + std::to_string(HML_MAX_JOINTS) + "]";
    if (D != hml_rows(J))
        return "D = " + std::to_string(D) + " rows, 12 J - 1 = " + std::to_string(hml_rows(J)) + " expected for J = " + std::to_string(J) + " joints (263: 22, 251: 21)";
    return std::string();
}

}  // namespace rgn
