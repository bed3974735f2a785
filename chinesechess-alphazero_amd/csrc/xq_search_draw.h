// xq_search_draw.h -- part of xq_search.hip's translation unit; do not compile it into a second one (xq_search_tree.h says why).
//
// The draw average (include/czero.h, cz_search_set_draw): the option's state (DrawState), an edge's D record (DRec), a leaf's
// draw probability in quanta (draw_quanta), the backup of d (backup_d) and the selection's term (draw_sigma, draw_term).  The
// D records lie where the moves-left utility's M records lie (m_block, xq_search_ml.h), which is why the two options exclude
// each other.  Everything here is reached from the DRAW instantiations alone (k_sim_draw, k_node_draws, k_draw_quanta): the
// kernels launched while the option is off do not hold a line of it.
#pragma once
#include "xq_search_tree.h"
#include "xq_search_ml.h"
#include "../../include/czero.h"

namespace {

constexpr int DRAW_QUANTA = 1 << 20;            // quanta per unit of probability
static_assert(DRAW_QUANTA == CZ_DRAW_QUANTA, "czero.h: draw average");

// Like the moves-left utility's state it reaches the kernels that use it as an argument of its own.
struct DrawState {
    double score;           // what a draw is worth to the side to move at the root, in [-1, 1]
    int on;                 // 0 = off
    const float* wdl;       // caller-owned [G*K][3] win / draw / loss rows, indexed as `value` is
};

// one edge's draw statistics; edge j of a node = granule stat + nm + j, directly behind the node's EdgeStat block (MRec's place)
struct __attribute__((aligned(16))) DRec {
    long long dsum;         // sum over the completed backups through the edge of dq, in quanta
    int32_t dn;             // how many
    int32_t spare;
};
static_assert(sizeof(DRec) == sizeof(MRec), "one granule per edge, the M record's");

// dq = rint(d * 2^20), the product exact in float32; NaN or d < 0 gives 0, d >= 1 gives 2^20
XQ_D int draw_quanta(float d)
{
    if (!(d >= 0.0f)) return 0;                                  // NaN, a negative d (and -0.0 goes on: 0)
    if (d >= 1.0f) return DRAW_QUANTA;                           // (+infinity too)
    return (int)rintf(d * (float)DRAW_QUANTA);
}

XQ_D DRec* d_block(EdgeStat* sb, int nm) { return reinterpret_cast<DRec*>(sb + nm); }
XQ_D const DRec* d_block(const EdgeStat* sb, int nm) { return reinterpret_cast<const DRec*>(sb + nm); }

// The backup of d for the path in L.path_* (depth entries), dq the quanta of the simulation's end: on every edge of the path
// dsum += dq and dn += 1 -- no sign, no change per level.  Lane i = level i, as backup_m(); call it BEFORE backup(), whose
// fence orders these stores too.
XQ_D void backup_d(const GameView& gv, const SearchLDS& L, int depth, int dq)
{
    for (int i = lane_id(); i < depth; i += 64) {
        char* nb = rec_ptr(gv, (uint32_t)L.path_node[i]);
        const int nm = (int)(*reinterpret_cast<const uint32_t*>(nb + NODE_OFF_HDR + 4) & 0xFF);
        DRec* r = reinterpret_cast<DRec*>(rec_ptr(gv, (uint32_t)L.path_edge[i] + (uint32_t)nm));
        const DRec cur = *r;                                     // one 16-byte load
        r->dsum = cur.dsum + (long long)dq;
        r->dn = cur.dn + 1;
    }
}

// The selection's term in two steps (include/czero.h has the rule; float64, this operation order).  draw_sigma: what a draw is
// worth to the mover of a node `depth` edges below the ply's root.  draw_term: sigma * dbar of one edge's record, 0 for an edge
// without a backup -- formed before the scoring loop, so that the records do not live through it.
XQ_D double draw_sigma(const DrawState& D, int depth) { return (depth & 1) ? -D.score : D.score; }
XQ_D double draw_term(double sigma, long long dsum, int dn)
{
    const double dbar = dn > 0 ? ((double)dsum / 1048576.0) / (double)dn : 0.0;
    return sigma * dbar;
}

}  // namespace
