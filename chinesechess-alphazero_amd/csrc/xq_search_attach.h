// xq_search_attach.h -- part of xq_search.hip's translation unit; do not compile it into a second one.  Why: the same text as a
// unit of its own gave all eight k_sim* kernels 0.4-1.7 % more or fewer instructions (k_sim<false,false> 18 740 against
// 18 608, equal registers and scratch, nothing called out of line; cause not found).  The benchmark measures those kernels, so
// text only moves between these headers, and the proof of a move is the unit's device assembly, kernel by kernel
// (EXPERIMENTS.md, "the search unit's text in headers").
//
// Prior spreading, the attach of an evaluated leaf: logits_to_weights, prior_norm, attach_policy, the one-leaf-ahead prefetch
// (LeafPre, leaf_pre_a / leaf_pre_b), attach_and_backup.
#pragma once
#include "xq_search_tree.h"

namespace {

// ---- prior spreading: select_action_q_and_u, player.py:272-284 ----------------------------------
// Network rows as raw logits (cz_search_policy_logits): the reference spreads the softmax output over the legal moves,
// p_j / sum_legal p (player.py:272-283), in which the softmax's own denominator cancels -- so only the legal moves' logits
// matter: p_j := exp(l_j - max over the node's moves).  (The engine's own queue then skips the normalising pass over all
// 2086 columns: 546 MB of traffic per round for the 4 % of the entries that are read.)
// inv_t: the policy temperature (cz_search_set_policy_temperature) as float32(1 / T), the softmax of l / T over the legal moves:
// the difference to the maximum is scaled, one float32 product rounded on its own.  T = 1 is 1.0f, an exact product.
XQ_D void logits_to_weights(float& q0, float& q1, int nm, float inv_t)
{
    const int lane = lane_id();
    const bool h0 = lane < nm, h1 = lane + 64 < nm;
    float m = h0 ? q0 : -3.0e38f;
    if (h1 && q1 > m) m = q1;
    m = wave_max_f32(m);
    q0 = h0 ? __expf((q0 - m) * inv_t) : 0.0f;
    q1 = h1 ? __expf((q1 - m) * inv_t) : 0.0f;
}

// The priors of a node from its row's entries, lane j holding move j in p0 and move j + 64 in p1 (0 past the node's nm
// moves): prior j = (p0 or p1 after the call) / the returned sum.  Raw logits first become weights relative to the largest
// legal one; the sum is the float32 accumulation in move order (select_action_q_and_u, player.py:272-284), the terms read
// straight from the lanes' registers (a loop over an LDS copy paid an LDS round trip per term).  The one place the priors
// are formed: the attach of an evaluated leaf and the evaluation cache's fill (k_cache_fill) both call it, so a cached
// entry holds the attach's bits by construction.
XQ_D float prior_norm(float& p0, float& p1, int nm, bool logits, float inv_t)
{
    if (logits) logits_to_weights(p0, p1, nm, inv_t);      // (raw logits: weights relative to the largest legal one)
    float all_p = 0.0f;
    if (nm > 0) {
        all_p = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p0), 0));          // int 0 + float32
        const int n0 = nm < 64 ? nm : 64;
        for (int j = 1; j < n0; ++j) all_p = all_p + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p0), j));
        for (int j = 64; j < nm; ++j) all_p = all_p + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p1), j - 64));
    }
    if (all_p == 0.0f) all_p = 1.0f;
    return all_p;
}

// keep_v: the leaf's network value v goes into the node header as well (k_sim's keep_v: constant false outside the GUM
// instantiations, so their text does not hold the store)
XQ_D void attach_policy(const GameView& gv, SearchLDS& L, int node, const float* __restrict__ prow, bool logits,
                        float inv_t, bool keep_v, float v)
{
    const int lane = lane_id();
    char* base = rec_ptr(gv, (uint32_t)node);
    const NodeHdr hdr = load_hdr(base);
    const uint32_t meta = hdr.meta;
    const int nm = (int)(meta & 0xFF);
    float* pp = node_p(base);
    const uint16_t* pm = node_mv(base, nm);
    // a mirrored leaf's row is in the mirrored frame: the entry of move a is column M(a); p[] and the moves stay as they are
    const bool mir = (meta & NODE_MIRRORED) != 0u;
    float q0 = 0.0f, q1 = 0.0f;
    if (lane < nm) q0 = prow[row_col(pm[lane], mir)];
    if (lane + 64 < nm) q1 = prow[row_col(pm[lane + 64], mir)];
    const float all_p = prior_norm(q0, q1, nm, logits, inv_t);
    if (lane < nm) pp[lane] = q0 / all_p;
    if (lane + 64 < nm) pp[lane + 64] = q1 / all_p;
    // p[j] is written and later read (select_edge) by the same lane, the header by lane 0: no global fence
    if (lane == 0) store_meta(base, meta & ~(uint32_t)(NODE_WAITING | NODE_MIRRORED));
    if (keep_v && lane == 0) store_net_value(base, v);
    wave_sync();
}

// attach_policy + load_path + backup of one evaluated leaf with their independent loads issued together: the move labels
// with the path's edge ids, then the priors of those labels with the statistics of those edges -- two dependent memory
// round trips per leaf instead of five (the BACKUP launch is nothing but such chains, eight leaves one after the other).
// Same arithmetic, same lanes writing the same words as the three functions it replaces.  depth <= 64.
// (round 5) The part of a leaf's chain that does not depend on the tree -- its move labels, its path's edge ids, the network
// row's entries for those labels -- is fetched one leaf AHEAD (LeafPre: leaf_pre_a, then leaf_pre_b once the labels are
// back), under the previous leaf's edge update and fence; what stays in a leaf's serial chain is the edge statistics' load,
// the arithmetic and the store fence: two memory round trips per leaf instead of three.
struct LeafPre {
    uint16_t m0, m1;
    int e;
    float p0, p1;
};
XQ_D void leaf_pre_a(const GameView& gv, LeafPre& lp, int node, uint32_t meta, int depth, const int32_t* __restrict__ hp_edge)
{
    const int lane = lane_id();
    char* base = rec_ptr(gv, (uint32_t)node);
    const int nm = (int)(meta & 0xFF);
    const uint16_t* pm = node_mv(base, nm);
    lp.m0 = 0; lp.m1 = 0; lp.e = 0;
    if (lane < nm) lp.m0 = pm[lane];
    if (lane + 64 < nm) lp.m1 = pm[lane + 64];
    if (lane < depth) lp.e = hp_edge[lane];
}
XQ_D void leaf_pre_b(LeafPre& lp, uint32_t meta, const float* __restrict__ prow)
{
    const int lane = lane_id();
    const int nm = (int)(meta & 0xFF);
    lp.p0 = 0.0f; lp.p1 = 0.0f;
    const bool mir = (meta & NODE_MIRRORED) != 0u;             // (the row of a mirrored leaf: column M(label), one table read)
    if (lane < nm) lp.p0 = prow[row_col(lp.m0, mir)];
    if (lane + 64 < nm) lp.p1 = prow[row_col(lp.m1, mir)];
}

// `lp`: this leaf's prefetched labels / edge ids / row entries.  `next`: issued between this leaf's edge-statistics load and
// its arithmetic -- the caller's prefetch of the following leaf.
// keep_v: as attach_policy's; v is float(v) of the slot's float32, so the cast back is exact.
template <typename Next>
XQ_D void attach_and_backup(const SearchParams& P, const GameView& gv, SearchLDS& L, int node, uint32_t meta, int depth,
                            const LeafPre& lp, double v, bool logits, float inv_t, bool keep_v, Next&& next)
{
    const int lane = lane_id();
    char* base = rec_ptr(gv, (uint32_t)node);
    const int nm = (int)(meta & 0xFF);
    float* pp = node_p(base);
    float p0 = lp.p0, p1 = lp.p1;
    EdgeStat cur{0.0, 0, 0};
    EdgeStat* ep = nullptr;
    if (lane < depth) { ep = edge_ptr(gv, (uint32_t)lp.e); cur = *ep; }
    next();
    const float all_p = prior_norm(p0, p1, nm, logits, inv_t);   // prior spreading (select_action_q_and_u, player.py:272-284)
    if (lane < nm) pp[lane] = p0 / all_p;
    if (lane + 64 < nm) pp[lane + 64] = p1 / all_p;
    if (lane == 0) store_meta(base, meta & ~(uint32_t)(NODE_WAITING | NODE_MIRRORED));
    if (keep_v && lane == 0) store_net_value(base, (float)v);
    // update_tree (player.py:357-366): lane i = level i
    if (lane < depth) {
        const double vi = ((depth - lane) & 1) ? -v : v;
        ep->n = cur.n + (1 - P.vl);
        ep->w = cur.w + (vi + (double)P.vl);
    }
    count(gv, CT_SIMS);
    count(gv, CT_SUM_DEPTH, (unsigned long long)depth);
    count_max(gv, CT_MAX_DEPTH, (unsigned long long)depth);
    wave_sync_global();
}

}  // namespace
