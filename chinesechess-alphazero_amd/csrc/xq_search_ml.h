// xq_search_ml.h -- part of xq_search.hip's translation unit; do not compile it into a second one (xq_search_tree.h says why).
//
// The moves-left utility (include/czero.h, cz_search_set_moves_left): the option's state (MovesLeftState), an edge's M record
// (MRec), the leaf's prediction in quanta (ml_quanta), the integer wave sum (wave_add_i64), the backup of m (backup_m) and the
// utility of one edge (ml_edge_d, ml_utility).  Everything here is reached from the ML instantiations alone (k_sim_ml, k_reserve_ml,
// k_node_moves_left, k_ml_quanta): the kernels launched while the option is off do not hold a line of it.
#pragma once
#include "xq_search_tree.h"
#include "../../include/czero.h"

namespace {

constexpr int ML_QUANTA = 16;                   // quanta per ply
constexpr int ML_K_MAX = 16 * 1023;             // cap of a leaf's prediction
static_assert(ML_QUANTA == CZ_MOVES_LEFT_QUANTA && ML_K_MAX == CZ_MOVES_LEFT_K_MAX, "czero.h: moves-left utility");

// Like the stop rules' state it reaches the kernels that use it as an argument of its own: SearchParams / SearchBuffers go to
// every search kernel and stay as they are.
struct MovesLeftState {
    double slope;           // 0 = off
    double cap;
    const float* x;         // caller-owned [G*K] raw moves-left rows, indexed as `value` is
};

// one edge's moves-left statistics; edge j of a node = granule stat + nm + j, directly behind the node's EdgeStat block
struct __attribute__((aligned(16))) MRec {
    long long ksum;         // sum over the completed backups through the edge of m, in quanta
    int32_t mn;             // how many
    int32_t spare;
};
static_assert(sizeof(MRec) == 16, "one granule per edge");

// k = min(rint(512 * softplus(x)), 16 * 1023), float32, softplus in its stable form; a product that is not finite or
// negative gives 0, +infinity the cap
XQ_D int ml_quanta(float x)
{
    const float sp = fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x)));
    const float t = 512.0f * sp;
    if (!(t >= 0.0f)) return 0;                                  // NaN (and a negative product: cannot happen)
    if (t >= (float)ML_K_MAX) return ML_K_MAX;                   // (+infinity too)
    return (int)rintf(t);
}

// sum of a 64-bit integer over the 64 lanes on wave_add_f64's ladder (a lane without a source adds 0); exact, so the order
// does not matter.  All 64 lanes call it.
#define XQ_DPP_STEP_ADD_I64(v, ctrl, rmask, bound)                                                                   \
    do {                                                                                                             \
        const int lo_ = __builtin_amdgcn_update_dpp(0, (int)v, ctrl, rmask, 0xF, bound);                            \
        const int hi_ = __builtin_amdgcn_update_dpp(0, (int)(v >> 32), ctrl, rmask, 0xF, bound);                    \
        v += (long long)(((unsigned long long)(unsigned int)hi_ << 32) | (unsigned int)lo_);                         \
    } while (0)
XQ_D long long wave_add_i64(long long v)
{
    XQ_DPP_STEP_ADD_I64(v, 0x111, 0xF, true);
    XQ_DPP_STEP_ADD_I64(v, 0x112, 0xF, true);
    XQ_DPP_STEP_ADD_I64(v, 0x114, 0xF, true);
    XQ_DPP_STEP_ADD_I64(v, 0x118, 0xF, true);
    XQ_DPP_STEP_ADD_I64(v, 0x142, 0xA, false);
    XQ_DPP_STEP_ADD_I64(v, 0x143, 0xC, false);
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)v, 63);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(v >> 32), 63);
    return (long long)(((unsigned long long)hi << 32) | lo);
}
#undef XQ_DPP_STEP_ADD_I64

// the M records of a node's statistics block `sb` (nm edges)
XQ_D MRec* m_block(EdgeStat* sb, int nm) { return reinterpret_cast<MRec*>(sb + nm); }
XQ_D const MRec* m_block(const EdgeStat* sb, int nm) { return reinterpret_cast<const MRec*>(sb + nm); }

// the leaf's k in word 3 of the node header (free while the Gumbel search is off: store_net_value), written by lane 0 beside
// the attach's store_meta
XQ_D void store_ml_k(char* base, int k) { *reinterpret_cast<int32_t*>(base + NODE_OFF_HDR + 12) = k; }

// The backup of m for the path in L.path_* (depth entries), k the quanta of the simulation's end: walking up, m = k + 16 per
// level, the edge's ksum += m and mn += 1.  Lane i = level i, as backup(); call it BEFORE backup(), whose fence orders these
// stores too.  The move count of the level's node (its M records start nm granules behind its statistics) was written when
// the node was made, launches ago.
XQ_D void backup_m(const GameView& gv, const SearchLDS& L, int depth, int k)
{
    for (int i = lane_id(); i < depth; i += 64) {
        char* nb = rec_ptr(gv, (uint32_t)L.path_node[i]);
        const int nm = (int)(*reinterpret_cast<const uint32_t*>(nb + NODE_OFF_HDR + 4) & 0xFF);
        MRec* m = reinterpret_cast<MRec*>(rec_ptr(gv, (uint32_t)L.path_edge[i] + (uint32_t)nm));
        const MRec cur = *m;                                     // one 16-byte load
        m->ksum = cur.ksum + (long long)(k + ML_QUANTA * (depth - i));
        m->mn = cur.mn + 1;
    }
}

// The utility of one edge in two steps (include/czero.h has the rule; float64, this operation order).  ml_edge_d: the clamped
// slope * (Mj - Mp) of the edge's record r under the parent's mean Mp in plies, 0 for an edge without a backup -- formed
// before the scoring loop, so that the records and Mp do not live through it.  ml_utility: u_m from d and the edge's q as the
// selection reads it.
XQ_D double ml_edge_d(const MovesLeftState& M, long long ksum, int mn, double Mp)
{
    if (mn <= 0) return 0.0;
    const double Mj = ((double)ksum / 16.0) / (double)mn;
    const double d = M.slope * (Mj - Mp);
    return d > M.cap ? M.cap : (d < -M.cap ? -M.cap : d);
}
XQ_D double ml_utility(double d, double q)
{
    const double aq = fabs(q);
    const double a = aq < 1.0 ? aq : 1.0;
    const double f = 1.6521 * a + (-0.6521) * (a * a);
    return q > 0.0 ? -(d * f) : (q < 0.0 ? d * f : 0.0);
}

}  // namespace
