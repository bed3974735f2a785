// xq_search_records.h -- part of xq_search.hip's translation unit; do not compile it into a second one.  Why: the same text as a
// unit of its own gave all eight k_sim* kernels 0.4-1.7 % more or fewer instructions (k_sim<false,false> 18 740 against
// 18 608, equal registers and scratch, nothing called out of line; cause not found).  The benchmark measures those kernels, so
// text only moves between these headers, and the proof of a move is the unit's device assembly, kernel by kernel
// (EXPERIMENTS.md, "the search unit's text in headers").
//
// What a finished search records about its root: RootEdges and its two loaders, root_net_value, gumbel_choose, gumbel_targets,
// prune_targets, root_value, root_surprise, root_maxq, emit_visits.
#pragma once
#include "xq_search_tree.h"
#include "xq_search_select.h"

namespace {

// A root's edges as one wavefront holds them, edge j = lane + 64 h: the label with VISIT_BANNED, the raw statistics n / w,
// the float32 prior WITHOUT noise.  What an edge at or beyond nm, or an array the source lacks, would hold is zero.
struct RootEdges {
    int nm, sum_n;
    uint16_t lab[2];
    int n[2];
    double w[2];
    float p[2];
};

// ... of the game's current root in the tree, with the bans of g_no_act; no root: nm = 0.  All 64 lanes call it.
XQ_D RootEdges load_root_edges(const SearchBuffers& B, const GameView& gv)
{
    RootEdges E{};
    const int lane = lane_id();
    const int g = gv.g;
    const int root = uni(B.g_root[g]);
    if (root < 0) return E;
    char* base = rec_ptr(gv, (uint32_t)root);
    const NodeHdr hdr = load_hdr(base);
    const uint16_t* pm = node_mv(base, (int)(hdr.meta & 0xFF));
    E.nm = (int)(hdr.meta & 0xFF) > MAXMOVES ? MAXMOVES : (int)(hdr.meta & 0xFF);
    E.sum_n = hdr.sum_n;
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
        if (sb) { const EdgeStat es = sb[j]; E.n[h] = es.n; E.w[h] = es.w; }
        E.p[h] = node_p(base)[j];
    }
    return E;
}

// the stored network value of the game's current root (store_net_value); no root: 0
XQ_D float root_net_value(const SearchBuffers& B, const GameView& gv)
{
    const int root = uni(B.g_root[gv.g]);
    if (root < 0) return 0.0f;
    return __uint_as_float(load_hdr(rec_ptr(gv, (uint32_t)root)).val);
}

// ... of row r of caller-supplied arrays [rows][128]; a NULL array stays zero
XQ_D RootEdges load_row_edges(const uint16_t* __restrict__ labels, const int32_t* __restrict__ n,
                              const double* __restrict__ w, const float* __restrict__ p,
                              const uint8_t* __restrict__ n_edges, int r)
{
    RootEdges E{};
    E.nm = n_edges[r] > MAXMOVES ? MAXMOVES : n_edges[r];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const size_t i = (size_t)r * MAXMOVES + lane_id() + 64 * h;
        if (lane_id() + 64 * h >= E.nm) continue;
        E.lab[h] = labels[i];
        if (n) E.n[h] = n[i];
        if (w) E.w[h] = w[i];
        if (p) E.p[h] = p[i];
    }
    return E;
}

// The move a Gumbel ply plays (include/czero.h): among the non-banned edges with the greatest started count the greatest
// g_j + log p_j + sigma(q01_j), with w and n as they are after the last backup; the later edge on a tie.  All 64 lanes.
XQ_D int gumbel_choose(const SearchParams& P, const SearchBuffers& B, const GameView& gv)
{
    const int lane = lane_id();
    const RootEdges E = load_root_edges(B, gv);
    const int32_t* started = B.g_started + (size_t)gv.g * MAXMOVES;
    const double* gum = B.g_gumbel + (size_t)gv.g * MAXMOVES;
    int st[2] = {-1, -1};
    int max_n = 0, max_st = -1;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        if (j >= E.nm || (E.lab[h] & VISIT_BANNED)) continue;
        st[h] = started[j];
        max_st = st[h] > max_st ? st[h] : max_st;
        max_n = E.n[h] > max_n ? E.n[h] : max_n;
    }
    max_st = (int)wave_max_f64((double)max_st);
    max_n = (int)wave_max_f64((double)max_n);
    double best_s = -__builtin_inf();
    int best_j = -1;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        if (st[h] < 0 || st[h] != max_st) continue;
        const double sc = gumbel_score(gum[j], E.p[h],
                                       gumbel_sigma(P.gumbel_visit, P.gumbel_scale, max_n, gumbel_q01(E.n[h], E.w[h])));
        if (sc >= best_s) { best_s = sc; best_j = j; }
    }
    const int pick = gumbel_argmax(best_s, best_j);
    if (pick < 0) return 0;                                     // every edge banned: what calc_policy's empty vector gives
    const int lab = pick < 64 ? __builtin_amdgcn_readlane((int)E.lab[0], pick) : __builtin_amdgcn_readlane((int)E.lab[1], pick - 64);
    return lab & 0x7FFF;
}

// The Gumbel policy target (include/czero.h, cz_search_set_gumbel): one wavefront, edge j = lane + 64 h.  lab[h] carries
// VISIT_BANNED, n / w are the raw statistics, p the float32 prior WITHOUT noise.  m[] receives floor(65536 pi'_j + 1/2),
// pi' = softmax(log p + sigma(completed q)); banned edges 0.  Float64, each sum the lane's two terms first and then the
// DPP ladder.  Returns S, the raw total of the non-banned edges.  All 64 lanes call it.
// FULL (cz_search_set_gumbel_full): an unvisited edge is completed with v_mix of the root -- gumbel_vmix over the non-banned
// edges with the root's stored network value v -- instead of the visited edges' mean vbar: the paper's target.  Nothing
// visited: every edge is completed with vhat and the target is the prior.  The <false> instantiation is the text it was.
template <bool FULL>
XQ_D int gumbel_targets(int nm, const uint16_t lab[2], int m[2], const int n[2], const double w[2], const float p[2],
                        double c_visit, double c_scale, float v = 0.0f)
{
    const int lane = lane_id();
    bool live[2];
    int s = 0, max_n = 0;
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        live[h] = lane + 64 * h < nm && !(lab[h] & VISIT_BANNED);
        m[h] = 0;
        if (!live[h]) continue;
        s += n[h];
        max_n = n[h] > max_n ? n[h] : max_n;
        if (n[h] > 0) {
            num = __dadd_rn(num, __dmul_rn((double)p[h], gumbel_q01(n[h], w[h])));
            den = __dadd_rn(den, (double)p[h]);
        }
    }
    const int S = __builtin_amdgcn_readlane(wave_incl_scan(s), 63);
    max_n = (int)wave_max_f64((double)max_n);
    num = wave_add_f64(num);
    den = wave_add_f64(den);
    const double vbar = FULL ? gumbel_vmix(v, S, den, num)
                             : (den > 0.0 ? num / den : 0.5);   // (nothing visited, or only edges of prior 0: one half)
    double sg[2] = {0.0, 0.0}, mx = -__builtin_inf();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (!live[h]) continue;
        sg[h] = gumbel_sigma(c_visit, c_scale, max_n, n[h] > 0 ? gumbel_q01(n[h], w[h]) : vbar);
        mx = sg[h] > mx ? sg[h] : mx;
    }
    mx = wave_max_f64(mx);
    double e[2] = {0.0, 0.0};
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (live[h]) e[h] = __dmul_rn((double)p[h], exp(sg[h] - mx));
    const double tot = wave_add_f64(__dadd_rn(e[0], e[1]));
    if (!(tot > 0.0)) return S;                                 // no live edge, or every prior 0: all zero
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (live[h]) m[h] = (int)floor(__dadd_rn(__dmul_rn(65536.0, e[h] / tot), 0.5));
    return S;
}

// Policy target pruning (include/czero.h, cz_search_set_forced_playouts): one wavefront, edge j = lane + 64 h.  lab[h]
// carries VISIT_BANNED, n / w are the raw statistics, p the float32 prior WITHOUT noise; the pruned counts replace n[].
// All arithmetic in float64, in the order czero.h writes it.  Returns S, the raw total of the non-banned edges.
// c_puct, cf, cb: the exploration constant is cpuct_at(c_puct, cf, cb, S), the schedule's value at the raw total (cf = 0:
// c_puct itself).
XQ_D int prune_targets(int nm, const uint16_t lab[2], int n[2], const double w[2], const float p[2], double c_puct, double cf,
                       double cb, double k)
{
    const int lane = lane_id();
    long long s = 0;
    int bn = -1, bl = 0x10000;              // this lane's candidate for c*: greatest n, then lowest label
    double bw = 0.0;
    float bp = 0.0f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const bool live = lane + 64 * h < nm && !(lab[h] & VISIT_BANNED);
        if (!live) continue;
        s += n[h];
        const int l = lab[h] & 0x7FFF;
        if (n[h] > bn || (n[h] == bn && l < bl)) { bn = n[h]; bl = l; bw = w[h]; bp = p[h]; }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        s += __shfl_xor(s, d, 64);
        const int on = __shfl_xor(bn, d, 64), ol = __shfl_xor(bl, d, 64);
        const double ow = __shfl_xor(bw, d, 64);
        const float op = __shfl_xor(bp, d, 64);
        if (on > bn || (on == bn && ol < bl)) { bn = on; bl = ol; bw = ow; bp = op; }
    }
    const int S = (int)s;
    if (S <= 0) return 0;                   // nothing searched (or everything banned): the counts stay
    const double Sd = (double)S;
    const double sq = __dsqrt_rn(Sd);
    c_puct = cpuct_at(c_puct, cf, cb, S);
    const double e_star = bw / (double)bn + ((c_puct * (double)bp) * sq) / (double)(1 + bn);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const bool live = lane + 64 * h < nm && !(lab[h] & VISIT_BANNED);
        if (!live || n[h] <= 0 || (int)(lab[h] & 0x7FFF) == bl) continue;
        const double nj = (double)n[h], pj = (double)p[h];
        const double f = floor(__dsqrt_rn((k * pj) * Sd));
        const double d = e_star - w[h] / nj;
        double need = nj;
        if (d > 0.0) {
            need = ceil(((c_puct * pj) * sq) / d - 1.0);
            need = need < 0.0 ? 0.0 : (need > nj ? nj : need);
        }
        const double keep = nj - f;
        int m = (int)(need > keep ? need : keep);
        if (m < n[h] && m <= 1) m = 0;
        n[h] = m;
    }
    return S;
}

// Root search value (include/czero.h, cz_search_record_values): one wavefront, edge j = lane + 64 h.  lab[h] carries
// VISIT_BANNED, m is the count the visit entry records (pruned or raw), n / w the raw statistics.  Float64 throughout:
// q_root = (sum m_j * (w_j / n_j)) / (sum m_j) over the non-banned edges with n_j > 0; NaN when that leaves nothing.  The
// lane's two terms first, then the DPP ladder of wave_add_f64: a fixed order, no LDS permute.  All 64 lanes call it.
XQ_D double root_value(int nm, const uint16_t lab[2], const int m[2], const int n[2], const double w[2])
{
    const int lane = lane_id();
    double num = 0.0, den = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const bool live = lane + 64 * h < nm && !(lab[h] & VISIT_BANNED) && n[h] > 0;
        if (!live) continue;
        const double mj = (double)m[h];
        num = __dadd_rn(num, __dmul_rn(mj, w[h] / (double)n[h]));
        den = __dadd_rn(den, mj);                   // integers below 2^53: exact in any order
    }
    num = wave_add_f64(num);
    den = wave_add_f64(den);
    return den > 0.0 ? num / den : __builtin_nan("");
}

// Policy surprise (include/czero.h, cz_search_record_surprise): one wavefront, edge j = lane + 64 h.  lab[h] carries
// VISIT_BANNED, m is the count the visit entry records (pruned or raw), p the float32 prior WITHOUT noise.  Float64
// throughout, every operation rounded once: s = sum t_j log(t_j / r_j) over the non-banned edges with m_j > 0, t_j =
// m_j / M, r_j = max(p_j / P, 1e-30), clamped at 0 from below; NaN when M = 0 or P is not positive.  Each sum takes the
// lane's two terms first, then the DPP ladder of wave_add_f64: a fixed order, no LDS permute.  All 64 lanes call it.
XQ_D double root_surprise(int nm, const uint16_t lab[2], const int m[2], const float p[2])
{
    const int lane = lane_id();
    double M = 0.0, Ps = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const bool live = lane + 64 * h < nm && !(lab[h] & VISIT_BANNED);
        if (!live) continue;
        M = __dadd_rn(M, (double)m[h]);             // integers below 2^53: exact in any order
        Ps = __dadd_rn(Ps, (double)p[h]);
    }
    M = wave_add_f64(M);
    Ps = wave_add_f64(Ps);
    if (!(M > 0.0) || !(Ps > 0.0)) return __builtin_nan("");   // wave-uniform: both are wave sums
    double s = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const bool live = lane + 64 * h < nm && !(lab[h] & VISIT_BANNED) && m[h] > 0;
        if (!live) continue;
        const double t = (double)m[h] / M;
        double r = (double)p[h] / Ps;
        r = r > SURPRISE_R_FLOOR ? r : SURPRISE_R_FLOOR;    // (a NaN prior takes the floor as well)
        s = __dadd_rn(s, __dmul_rn(t, log(t / r)));
    }
    s = wave_add_f64(s);
    return s > 0.0 ? s : 0.0;
}

// The number a ply's resignation test compares (include/czero.h, cz_search_record_maxq): one wavefront, edge j = lane +
// 64 h.  lab[h] carries VISIT_BANNED, n / w are the raw statistics.  choose_action's arithmetic: the maximum over the
// non-banned edges of n ? w / n : 0.0 in float64, starting from -100 (so: no such edge gives -100).  A maximum is exact,
// the lane order is free.  All 64 lanes call it.
XQ_D double root_maxq(int nm, const uint16_t lab[2], const int n[2], const double w[2])
{
    const int lane = lane_id();
    double maxq = -100.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const bool live = lane + 64 * h < nm && !(lab[h] & VISIT_BANNED);
        if (!live) continue;
        const double q = n[h] ? w[h] / (double)n[h] : 0.0;
        maxq = q > maxq ? q : maxq;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_xor(maxq, d, 64);
        maxq = o > maxq ? o : maxq;
    }
    return unid(maxq);
}

// Root visit record (cz_search_record_visits): the root's edges as choose_action saw them -- edge order, exact
// counts, banned edges flagged (calc_policy zeroes them, player.py:375-406) -- for the ply that just chose its move.
// prune (forced playouts on, a full ply): the counts are the pruned policy targets, the entry says so (VISIT_PRUNED,
// raw_total); the tree keeps the raw counts and choose_action has already used them.
// FULL: a Gumbel ply's target is the full search's (gumbel_targets<true> with the root's stored value).
// early: a stop rule ended the ply (VISIT_EARLY; only k_advance_stop ever passes true).
template <bool FULL>
XQ_D void emit_visits(const SearchParams& P, const SearchBuffers& B, const GameView& gv, const VisitRing& V, int turns,
                      bool resigned, bool fast, bool prune, bool gumbel, bool early = false)
{
    const int lane = lane_id();
    const int g = gv.g;
    if (uni(B.g_root[g]) < 0) return;
    unsigned int pos = 0;
    int drop = 0;
    if (lane == 0) {
        pos = atomicAdd(&V.ctl[0], 1u);
        drop = pos - V.ctl[1] >= V.cap ? 1 : 0;             // full: never overwrite what the host has not drained
        if (drop) {
            atomicAdd(V.dropped, 1ull);
            V.g_lost[g] = 1;
        }
    }
    pos = uniu(pos);
    if (uni(drop)) return;
    uint8_t* e = V.ring + (size_t)(pos % V.cap) * VISIT_STRIDE;
    uint16_t* lab = reinterpret_cast<uint16_t*>(e + sizeof(VisitEntryHdr));
    int32_t* cnt = reinterpret_cast<int32_t*>(e + sizeof(VisitEntryHdr) + 2 * VISIT_MAX_EDGES);
    const RootEdges E = load_root_edges(B, gv);
    const int nm = E.nm;
    int m[2] = {E.n[0], E.n[1]};            // the counts the entry records: raw, or pruned
    // (a Gumbel ply: the counts are the policy target pi' scaled to 65536 -- the halving counts are no target)
    const int raw_total = gumbel ? gumbel_targets<FULL>(nm, E.lab, m, E.n, E.w, E.p, P.gumbel_visit, P.gumbel_scale,
                                                        FULL ? root_net_value(B, gv) : 0.0f)
                                 : (prune ? prune_targets(nm, E.lab, m, E.w, E.p, P.c_puct, P.cpuct_factor, P.cpuct_base, P.forced_k) : 0);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        if (j < nm) { lab[j] = E.lab[h]; cnt[j] = m[h]; }
    }
    const bool pruned = !gumbel && raw_total > 0;      // S == 0: nothing to prune, the entry is the one written without pruning
    // the value and the surprise record (cz_search_record_values, _surprise): the entry's slot in a ring of their own
    if (V.q) {
        const double q = root_value(nm, E.lab, m, E.n, E.w);
        if (lane == 0) V.q[pos % V.cap] = q;
    }
    if (V.s) {
        const double sv = root_surprise(nm, E.lab, m, E.p);
        if (lane == 0) V.s[pos % V.cap] = sv;
    }
    // the max-q record (cz_search_record_maxq): what choose_action compared with the threshold, likewise; while it is on
    // the entry also says whether its game plays on without resignation
    bool no_resign = false;
    if (V.mq) {
        const double mq = root_maxq(nm, E.lab, E.n, E.w);
        if (lane == 0) V.mq[pos % V.cap] = mq;
        no_resign = uni((int)B.g_enable_resign[g]) == 0;
    }
    if (lane == 0) {
        VisitEntryHdr* h = reinterpret_cast<VisitEntryHdr*>(e);
        h->game_id = B.g_game_id[g];
        h->ply = (uint16_t)turns;
        h->n_edges = (uint8_t)nm;
        h->flags = (uint8_t)((resigned ? VISIT_RESIGN : 0u) | (fast ? VISIT_FAST : 0u) | (pruned ? VISIT_PRUNED : 0u) |
                               (gumbel ? VISIT_GUMBEL : 0u) | (early ? VISIT_EARLY : 0u) |
                               (no_resign ? VISIT_NO_RESIGN : 0u));
        h->sum_n = E.sum_n;
        h->raw_total = (uint32_t)raw_total;
    }
}

}  // namespace
