// xq_mirror.h -- the left-right mirror image of a Xiangqi position (file x <-> 8 - x, a symmetry of the rules), device side.
//
// Shared by the trainer's mirror augmentation (xq_train.hip: flagged rows of k_gather_planes / k_policy_value_loss) and the
// search's random leaf mirror (xq_search_tree.h: d_mirror, leaf_coin; cz_search_set_leaf_mirror).  The host's view of the label map is
// cz_label_mirror (czero.h).
#pragma once
#include "xq_rules.h"

namespace xq {

XQ_D int mirror_sq(int s)      // (x, y) -> (8 - x, y)
{
    const int y = s / 9;
    return s + 8 - 2 * (s - y * 9);
}

// The board of the mirrored position, in place: every lane reads its one or two source squares, then writes.
XQ_D void mirror_board(int8_t* b)
{
    const int lane = lane_id();
    const int8_t p0 = b[mirror_sq(lane)];
    const int8_t p1 = lane < 26 ? b[mirror_sq(lane + 64)] : (int8_t)0;
    wave_sync();
    b[lane] = p0;
    if (lane < 26) b[lane + 64] = p1;
    wave_sync();
}

// M(label): from what the device already holds (lab_ft -> mirror both squares -> label_of) instead of a third table; the
// label set is closed under the mirror (cz_label_mirror, tests/test_mirror_cpu.py), and a row has a few dozen labels at
// most, so the two dependent table reads are not worth 4 KB more constant data.  label < NLABELS.
// (The search reads M inside a latency chain and keeps the one-read table: MirrorTab below.)
XQ_D int mirror_label(int label)
{
    const int ft = label_ft(label);
    return label_of(mirror_sq(ft >> 8), mirror_sq(ft & 0xFF));
}

// M as one table, built at compile time from the same two tables: m[label] = mirror_label(label).
struct MirrorTab {
    uint16_t m[NLABELS + 2];
};
constexpr MirrorTab make_mirror_tab()
{
    MirrorTab t{};
    for (int l = 0; l < NLABELS; ++l) {
        const int f = h_tab.lab_ft[l] >> 8, d = h_tab.lab_ft[l] & 0xFF;
        t.m[l] = h_tab.label_of[(f + 8 - 2 * (f % 9)) * NSQ + (d + 8 - 2 * (d % 9))];
    }
    t.m[NLABELS] = 0; t.m[NLABELS + 1] = 0;
    return t;
}

}  // namespace xq
