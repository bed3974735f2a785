// xq_search_var.h -- part of xq_search.hip's translation unit; do not compile it into a second one (xq_search_tree.h says why).
//
// The lower-confidence-bound move choice (include/czero.h, cz_search_set_lcb): the option's state (LcbState), an edge's V record
// (VRec), the backup of the squared value (backup_v), a node's edges as the rule reads them (LcbEdges and its loader) and the
// rule itself (lcb_pick).  The V records lie where the moves-left utility's M records and the draw average's D records lie
// (m_block, xq_search_ml.h), which is why the three options exclude each other.  Everything here is reached from the VAR / LCB
// instantiations alone (k_sim_var, k_advance_lcb, k_choose_lcb, k_pv_lcb, k_node_values, k_root_lcb, k_lcb_rows): the kernels
// launched while the option is off do not hold a line of it.
#pragma once
#include "xq_search_tree.h"
#include "xq_search_ml.h"
#include "../../include/czero.h"

namespace {

// Like the moves-left utility's state it reaches the kernels that use it as an argument of its own.
struct LcbState {
    double z;               // how many standard errors below the mean the bound lies, finite and >= 0
    double ratio;           // an edge takes part with n >= ratio * (the greatest n), in [0, 1]
    int on;                 // 0 = off
};

// one edge's second moment; edge j of a node = granule stat + nm + j, directly behind the node's EdgeStat block (MRec's place)
struct __attribute__((aligned(16))) VRec {
    double s2;              // sum over the completed backups through the edge of x * x, x what backup() adds to W beyond the virtual loss
    int32_t vn;             // how many
    int32_t spare;
};
static_assert(sizeof(VRec) == sizeof(MRec), "one granule per edge, the M record's");

XQ_D VRec* v_block(EdgeStat* sb, int nm) { return reinterpret_cast<VRec*>(sb + nm); }
XQ_D const VRec* v_block(const EdgeStat* sb, int nm) { return reinterpret_cast<const VRec*>(sb + nm); }

// The backup of x * x for the path in L.path_* (depth entries), v the value backup() is about to take up: on every edge of the
// path s2 = s2 + x * x and vn += 1, x = backup()'s vi of the level -- the product rounded, then the sum, nothing fused.  Lane i =
// level i, as backup_m(); call it BEFORE backup(), whose fence orders these stores too.
XQ_D void backup_v(const GameView& gv, const SearchLDS& L, int depth, double v)
{
    for (int i = lane_id(); i < depth; i += 64) {
        char* nb = rec_ptr(gv, (uint32_t)L.path_node[i]);
        const int nm = (int)(*reinterpret_cast<const uint32_t*>(nb + NODE_OFF_HDR + 4) & 0xFF);
        VRec* r = reinterpret_cast<VRec*>(rec_ptr(gv, (uint32_t)L.path_edge[i] + (uint32_t)nm));
        const double vi = ((depth - i) & 1) ? -v : v;
        const VRec cur = *r;                                     // one 16-byte load
        r->s2 = __dadd_rn(cur.s2, __dmul_rn(vi, vi));
        r->vn = cur.vn + 1;
    }
}

// A node's edges as one wavefront hands them to lcb_pick, edge j = lane + 64 h: the label (at a root with VISIT_BANNED), n / w of
// the EdgeStat, s2 / vn of the V record.  What an edge at or beyond nm would hold is zero.
struct LcbEdges {
    int nm;
    uint16_t lab[2];
    int n[2];
    double w[2];
    double s2[2];
    int vn[2];
};

// ... of the game's current root in the tree, with the bans of g_no_act; no root: nm = 0.  All 64 lanes call it.  Only while
// the option is on: a tree grown without it has no V records.
XQ_D LcbEdges load_lcb_root(const SearchBuffers& B, const GameView& gv)
{
    LcbEdges E{};
    const int lane = lane_id();
    const int g = gv.g;
    const int root = uni(B.g_root[g]);
    if (root <= 0) return E;                                    // (id 0 is "none": an object never given a root)
    char* base = rec_ptr(gv, (uint32_t)root);
    const NodeHdr hdr = load_hdr(base);
    const int nm = (int)(hdr.meta & 0xFF);
    const uint16_t* pm = node_mv(base, nm);
    E.nm = nm > MAXMOVES ? MAXMOVES : nm;
    const EdgeStat* sb = hdr.stat ? edge_ptr(gv, hdr.stat) : nullptr;
    const int n_no_act = uni((int)B.g_n_no_act[g]);
    const uint16_t* no_act = B.g_no_act + (size_t)g * MAX_NO_ACT;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        if (j >= E.nm) continue;
        const uint16_t mv = pm[j];
        bool banned = false;
        for (int k = 0; k < n_no_act; ++k) banned = banned || (no_act[k] == mv);
        E.lab[h] = (uint16_t)(mv | (banned ? VISIT_BANNED : 0));
        if (sb) {
            const EdgeStat es = sb[j];
            const VRec vr = v_block(sb, nm)[j];
            E.n[h] = es.n; E.w[h] = es.w; E.s2[h] = vr.s2; E.vn[h] = vr.vn;
        }
    }
    return E;
}

// Among the edges cand[] names: the greatest n, then the lowest label, then the lowest index; -1 without a candidate.  The two
// extremes run on the DPP ladder (integers below 2^31 are exact doubles), the lanes that hold them vote by ballot.  Wave-uniform.
XQ_D int lcb_most_visited(const bool cand[2], const int n[2], const uint16_t lab[2])
{
    double mn = -1.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) if (cand[h] && (double)n[h] > mn) mn = (double)n[h];
    mn = wave_max_f64(mn);
    double ml = -65536.0;                                       // the negated label: the greatest is the lowest label
    bool top[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        top[h] = cand[h] && (double)n[h] == mn;
        if (top[h] && -(double)(lab[h] & 0x7FFF) > ml) ml = -(double)(lab[h] & 0x7FFF);
    }
    ml = wave_max_f64(ml);
    return lowest_bit(__ballot(top[0] && -(double)(lab[0] & 0x7FFF) == ml), __ballot(top[1] && -(double)(lab[1] & 0x7FFF) == ml));
}

// The rule of include/czero.h ("lower confidence bound"), float64 in its order with every operation rounded on its own.  lcb[]
// receives this lane's two bounds, NaN for an edge that is not eligible or past the edges.  Returns the edge the rule picks, the
// most visited non-banned edge where none is eligible, -1 where there is no non-banned edge.  All 64 lanes; wave-uniform.
XQ_D int lcb_pick(const LcbEdges& E, double z, double ratio, double lcb[2])
{
    const int lane = lane_id();
    bool open[2];                                               // an edge that is not banned
    double n_max = -1.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        open[h] = lane + 64 * h < E.nm && !(E.lab[h] & VISIT_BANNED);
        if (open[h] && (double)E.n[h] > n_max) n_max = (double)E.n[h];
    }
    n_max = wave_max_f64(n_max);
    const double floor_n = __dmul_rn(ratio, n_max);
    bool elig[2];
    double best = -__builtin_inf();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        lcb[h] = __builtin_nan("");
        elig[h] = open[h] && E.vn[h] >= 2 && E.n[h] > 0 && (double)E.n[h] >= floor_n;
        if (elig[h]) {
            const double vn = (double)E.vn[h];
            const double q = __ddiv_rn(E.w[h], (double)E.n[h]);
            double var = __dsub_rn(__ddiv_rn(E.s2[h], vn), __dmul_rn(q, q));
            if (var < 0.0) var = 0.0;
            var = __dmul_rn(var, __ddiv_rn(vn, (double)(E.vn[h] - 1)));
            const double b = __dsub_rn(q, __dmul_rn(z, __dsqrt_rn(__ddiv_rn(var, vn))));
            lcb[h] = b;
            elig[h] = b == b;                                   // (a bound that is NaN takes no part)
            if (elig[h] && b > best) best = b;
        }
    }
    best = wave_max_f64(best);
    bool top[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) top[h] = elig[h] && lcb[h] == best;
    if (__ballot(top[0] || top[1])) return lcb_most_visited(top, E.n, E.lab);
    return lcb_most_visited(open, E.n, E.lab);
}

}  // namespace
