// xq_search_solver.h -- part of xq_search.hip's translation unit; do not compile it into a second one.  Why: the same text as a
// unit of its own gave all eight k_sim* kernels 0.4-1.7 % more or fewer instructions (k_sim<false,false> 18 740 against
// 18 608, equal registers and scratch, nothing called out of line; cause not found).  The benchmark measures those kernels, so
// text only moves between these headers, and the proof of a move is the unit's device assembly, kernel by kernel
// (EXPERIMENTS.md, "the search unit's text in headers").
//
// The MCTS solver (include/czero.h, cz_search_set_solver): what the bit fields say (child_id, child_mark, meta_proof, meta_dist,
// child_dist), solve_least, solve_root_edge, solve_root_decided, select_solve, solve_walk.
#pragma once
#include "xq_search_tree.h"
#include "xq_search_select.h"

namespace {

// ---- MCTS solver (include/czero.h, cz_search_set_solver): what the words say ------------------------------------------
// An edge's child link without its mark: what every reader that follows the link uses.  The codes (< 0) stay as they are.
XQ_D int child_id(int c) { return c < 0 ? c : (c & CHILD_ID_MASK); }
// The edge mark: the Proof of the child.  A terminal child is marked by its code: (True, +1) is WIN(1), (True, -1) LOSS(0).
XQ_D int child_mark(int c)
{
    if (c >= 0) return (c >> CHILD_MARK_SHIFT) & 3;
    return c == CHILD_TERM_WIN ? PROOF_WIN : (c == CHILD_TERM_LOSS ? PROOF_LOSS : PROOF_OPEN);
}
XQ_D int meta_proof(uint32_t meta) { return (int)(meta >> NODE_PROOF_SHIFT) & 3; }
XQ_D int meta_dist(uint32_t meta) { return (int)(meta >> NODE_DIST_SHIFT) & 0xFF; }
// d of a MARKED child, fetched from the child's header (a first proof is final, so the header still says what the mark was
// made from).  Any lane may ask: the header is lane 0's word, and every store of a proof is followed by a fence (solve_walk).
XQ_D int child_dist(const GameView& gv, int c)
{
    if (c < 0) return c == CHILD_TERM_WIN ? 1 : 0;
    return meta_dist(*reinterpret_cast<const uint32_t*>(rec_ptr(gv, (uint32_t)(c & CHILD_ID_MASK)) + NODE_OFF_HDR + 4));
}

// ---- MCTS solver: selection, marking and deriving (include/czero.h, cz_search_set_solver) -------------------------------
// Rule 1's edge among the lanes' winning edges (win[h]: edge lane + 64 h is winning and may be taken; ch[h] its child
// word): the least d, the first in edge order on a tie; -1 without one.  The distances come from the child headers, which
// is why this runs only once a winning edge exists.  Wave-uniform.
XQ_D int solve_least(const GameView& gv, const bool win[2], const int ch[2])
{
    if ((__ballot(win[0]) | __ballot(win[1])) == 0ull) return -1;
    const int lane = lane_id();
    double key = -1.0e300;                                     // max of -(d * 128 + j) = the least (d, j)
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (win[h]) {
            const double k = -(double)(child_dist(gv, ch[h]) * MAXMOVES + lane + 64 * h);
            key = k > key ? k : key;
        }
    return (int)(-wave_max_f64(key)) & (MAXMOVES - 1);
}

// Rule 1 at a root: the non-banned winning edge of least d of the node at `base` (nm moves, statistics sb or nullptr), -1
// without one.  The move choice (choose_action) and the decided-root test ask it.  All 64 lanes call it.
XQ_D int solve_root_edge(const GameView& gv, char* base, const EdgeStat* sb, int nm, int n_no_act, const uint16_t* no_act)
{
    const int lane = lane_id();
    const uint16_t* pm = node_mv(base, nm);
    bool win[2] = {false, false};
    int ch[2] = {CHILD_UNKNOWN, CHILD_UNKNOWN};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        if (j >= nm || !sb) continue;
        ch[h] = sb[j].child;
        bool banned = false;
        for (int k = 0; k < n_no_act; ++k) banned = banned || (no_act[k] == pm[j]);
        win[h] = !banned && child_mark(ch[h]) == PROOF_LOSS;
    }
    return solve_least(gv, win, ch);
}

// Is the game's root decided -- LOSS, or WIN with a non-banned winning edge?  Then no further simulation starts this ply.
// *edge (optional): rule 1's edge at such a WIN root, else -1.  All 64 lanes call it; wave-uniform.
XQ_D bool solve_root_decided(const SearchBuffers& B, const GameView& gv, int* edge)
{
    if (edge) *edge = -1;
    const int root = uni(B.g_root[gv.g]);
    if (root <= 0) return false;                                // (-1: not in the tree; 0, "none": an object never given a root)
    char* base = rec_ptr(gv, (uint32_t)root);
    const NodeHdr hdr = load_hdr(base);
    const int st = meta_proof(hdr.meta);
    if (st == PROOF_LOSS) return true;
    if (st != PROOF_WIN) return false;
    const int nm = (int)(hdr.meta & 0xFF);
    const int j = solve_root_edge(gv, base, hdr.stat ? edge_ptr(gv, hdr.stat) : nullptr, nm, uni((int)B.g_n_no_act[gv.g]),
                                  B.g_no_act + (size_t)gv.g * MAX_NO_ACT);
    if (edge) *edge = j;
    return j >= 0;
}

// select_edge with the solver on, at the root and at OPEN nodes (the SOLVE instantiations of k_sim call it instead):
//   1. among the non-banned edges a winning one is taken at once, the least d, the first in edge order on a tie;
//   2. otherwise select_edge's rule -- the same expressions in the same order, the q > 1 - 1e-7 shortcut included -- over
//      the non-banned edges that are not losing;
//   3. every non-banned edge losing: over all non-banned edges.
// Edge j is loaded by the lane that owns it (j & 63), both halves held at once: the marks come with the 16-byte load.
template <bool SCHED = false>
XQ_D int select_solve(const SearchParams& P, const GameView& gv, char* base, const EdgeStat* sb, int sum_n, int nm,
                      const RootCtx& rc)
{
    const int lane = lane_id();
    const double xx = __dsqrt_rn((double)(sum_n + 1));
    double c = P.c_puct;
    float c32 = P.c_puct_f32;
    if constexpr (SCHED) { c = cpuct_of(P, sum_n); c32 = (float)c; }     // (the SCHED instantiations of k_sim_solve: select_edge)
    const float* pp = node_p(base);
    const uint16_t* pm = node_mv(base, nm);
    bool nb[2] = {false, false}, live[2] = {false, false}, win[2] = {false, false}, sure[2] = {false, false};
    int ch[2] = {CHILD_UNKNOWN, CHILD_UNKNOWN}, mk[2] = {PROOF_OPEN, PROOF_OPEN};
    double sc[2] = {-1.0e300, -1.0e300};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        if (j >= nm) continue;
        EdgeStat es{0.0, 0, CHILD_UNKNOWN};
        if (sb) es = sb[j];
        const float p = pp[j];
        const uint16_t mv = pm[j];
        const int n = es.n;
        const double w = es.w;
        const double q = n ? w / (double)n : 0.0;
        bool valid = true;
        double u;
        if (rc.is_root) {
            if (rc.n_no_act) valid = !root_banned(rc, mv);
            u = root_u(c, root_prior(P, rc, p, j), xx, n);
        } else {
            const float a = c32 * p;
            u = (double)a * xx / (double)(1 + n);
        }
        if (!valid) continue;
        nb[h] = true;
        ch[h] = es.child;
        mk[h] = child_mark(es.child);
        win[h] = mk[h] == PROOF_LOSS;
        const double score = q + u;
        live[h] = score >= -99999999.0;                         // (a rejected score leaves the edge out, as it does there)
        sc[h] = score;
        sure[h] = live[h] && q > (1.0 - 1e-7);
    }
    const int won = solve_least(gv, win, ch);                   // rule 1
    if (won >= 0) return won;
    // rules 2 and 3: the losing edges stay out unless every non-banned edge is one
    const bool all_losing = (__ballot(nb[0] && mk[0] != PROOF_WIN) | __ballot(nb[1] && mk[1] != PROOF_WIN)) == 0ull;
    double best_s = -1.0e300;
    int best_j = -1;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        live[h] = live[h] && (all_losing || mk[h] != PROOF_WIN);
        sure[h] = sure[h] && live[h];
        if (live[h] && sc[h] >= best_s) { best_s = sc[h]; best_j = lane + 64 * h; }   // h = 1 has the larger index: wins ties
    }
    const int first_win = lowest_bit(__ballot(sure[0]), __ballot(sure[1]));     // player.py:309-311
    if (first_win >= 0) return first_win;
    const double m = wave_max_f64(best_s);                      // player.py:312-314: the LAST maximum, select_edge's vote
    const bool top = best_j >= 0 && best_s == m;
    const uint64_t t1 = __ballot(top && best_j >= 64), t0 = __ballot(top);
    return t1 ? 64 + (63 - __clzll((long long)t1)) : (t0 ? 63 - __clzll((long long)t0) : -1);
}

// The second step of a backup, after the level-parallel one and only for a value of +-2: the simulation whose path (depth
// entries) is in L.path_* ended on a terminal child or on a proven node.  Its last edge is marked with that position's
// status, the node above derived if it is OPEN, and while a node becomes proven the walk goes on one level up; it stops at
// the first node that stays OPEN (or was proven before).  Sequential over the levels; each level is one scan of the
// node's edges over both halves, every edge read and written by its owner lane (j & 63), the header by lane 0.  The
// distances of the marked children come from their headers, any lane asking: hence the fence after every proof stored.
XQ_D void solve_walk(const GameView& gv, const SearchLDS& L, int depth)
{
    if (depth <= 0) return;
    const int lane = lane_id();
    int st;
    {
        const int c = uni(edge_ptr(gv, (uint32_t)L.path_edge[depth - 1])->child);
        st = child_mark(c);                                     // a terminal child: its code
        if (c >= 0) st = meta_proof(load_hdr(rec_ptr(gv, (uint32_t)child_id(c))).meta);
    }
    for (int i = depth - 1; i >= 0 && st != PROOF_OPEN; --i) {
        const int e = L.path_edge[i];
        char* base = rec_ptr(gv, (uint32_t)L.path_node[i]);
        const NodeHdr hdr = load_hdr(base);
        const int nm = (int)(hdr.meta & 0xFF);
        const int je = (int)((uint32_t)e - hdr.stat);
        EdgeStat* sb = edge_ptr(gv, hdr.stat);
        if (lane == (je & 63)) {                                // marking
            const int c = sb[je].child;
            if (c >= 0) sb[je].child = (c & CHILD_ID_MASK) | (st << CHILD_MARK_SHIFT);
        }
        if (meta_proof(hdr.meta) != PROOF_OPEN) break;          // a first proof is final
        bool win[2] = {false, false}, lose[2] = {false, false};
        double near = -1.0e300, far = -1.0;                     // max of -d over the winning edges, max of d over the losing
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = lane + 64 * h;
            if (j >= nm) continue;
            const int c = sb[j].child;
            const int mk = child_mark(c);
            if (mk == PROOF_OPEN) continue;
            const double d = (double)child_dist(gv, c);
            win[h] = mk == PROOF_LOSS;
            lose[h] = mk == PROOF_WIN;
            if (win[h]) near = -d > near ? -d : near;
            else far = d > far ? d : far;
        }
        int d;
        if (__ballot(win[0]) | __ballot(win[1])) {
            st = PROOF_WIN;
            d = 1 + (int)(-wave_max_f64(near));
        } else if (nm > 0 && __popcll(__ballot(lose[0])) + __popcll(__ballot(lose[1])) == nm) {
            st = PROOF_LOSS;
            d = 1 + (int)wave_max_f64(far);
        } else break;
        d = d < PROOF_DIST_MAX ? d : PROOF_DIST_MAX;
        if (lane == 0)
            store_meta(base, hdr.meta | ((uint32_t)st << NODE_PROOF_SHIFT) | ((uint32_t)d << NODE_DIST_SHIFT));
        count(gv, CT_PROOFS);
        wave_sync_global();
    }
    wave_sync_global();
}

}  // namespace
