// The launch decisions of CreateNewMapPoints' device code (matcher.hip), one source for the
// launchers, k_tri_match and the host-only orbmi_debug_tri_plan the tests read them through.
#pragma once
#include <algorithm>

#if defined(__HIP__) || defined(__HIPCC__)
#define ORBMI_PLAN_HD __host__ __device__
#else
#define ORBMI_PLAN_HD
#endif

namespace orbmi {

// k_tri_match's path of a KF2 node with nf features: 0 tri_node_regs<2> (at most 128 candidates
// in registers), 1 tri_node_regs<4> (at most 256), 2 tri_node_mem
constexpr int kTriRegs2Max = 128, kTriRegs4Max = 256;
ORBMI_PLAN_HD constexpr int tri_node_path(int nf) { return nf <= kTriRegs2Max ? 0 : nf <= kTriRegs4Max ? 1 : 2; }

// slices per KF1 node: enough waves for the chip (~4096 over all pairs) while a slice keeps ~16
// KF1 features to amortise loading the node's KF2 candidates
inline int tri_splits(int kf1_n, int fv1_nnodes, int npairs) {
    const int nodes = std::max(fv1_nnodes, 1);
    const int by_chip = 4096 / std::max(nodes * npairs, 1);
    const int by_size = std::max(kf1_n / nodes / 16, 1);
    return std::max(1, std::min(std::min(by_chip, by_size), 64));
}

// lanes per KF1 keypoint of k_triangulate_par (the smallest instance holding npairs), 0 = the
// sequential k_triangulate
constexpr int tri_group_width(int npairs) {
    return npairs <= 4 ? 4 : npairs <= 8 ? 8 : npairs <= 16 ? 16 : npairs <= 32 ? 32 : npairs <= 64 ? 64 : 0;
}

}  // namespace orbmi
