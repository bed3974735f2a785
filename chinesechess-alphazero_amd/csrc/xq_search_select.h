// xq_search_select.h -- part of xq_search.hip's translation unit; do not compile it into a second one.  Why: the same text as a
// unit of its own gave all eight k_sim* kernels 0.4-1.7 % more or fewer instructions (k_sim<false,false> 18 740 against
// 18 608, equal registers and scratch, nothing called out of line; cause not found).  The benchmark measures those kernels, so
// text only moves between these headers, and the proof of a move is the unit's device assembly, kernel by kernel
// (EXPERIMENTS.md, "the search unit's text in headers").
//
// Selection: the root's side of PUCT (RootCtx, root_banned, root_prior, root_u), the Gumbel helpers (gumbel_seq .. gumbel_argmax,
// gumbel_vmix), gumbel_interior, Picked, select_gumbel, select_edge.
#pragma once
#include "xq_search_tree.h"
#include "xq_search_ml.h"
#include "xq_search_draw.h"

namespace {

// ---- select_action_q_and_u, player.py:286-320 --------------------------------------------------------
struct RootCtx {
    bool is_root;
    int n_no_act;
    const uint16_t* no_act;
    const double* noise;        // this game's Dirichlet rows [K][MAXMOVES] written by k_noise (NULL when eps == 0)
    int sim;
    bool force;                 // forced playouts at this root (cz_search_set_forced_playouts; never on a fast ply)
};

// The root's side of the selection, one text for select_edge's scoring loop and its forcing pass: the two must agree bit
// for bit.  Ban test (player.py:298-300), the prior this simulation uses (:304), the exploration term (:306).
XQ_D bool root_banned(const RootCtx& rc, uint16_t mv)
{
    bool banned = false;
    for (int k = 0; k < rc.n_no_act; ++k) banned = banned || (rc.no_act[k] == mv);
    return banned;
}
XQ_D double root_prior(const SearchParams& P, const RootCtx& rc, float p, int j)
{
    const float a = (rc.noise ? P.one_minus_eps_f32 : 1.0f) * p;   // (no rows: eps = 0, also on a fast ply of the playout cap)
    double p_ = (double)a;
    if (rc.noise) p_ = p_ + P.noise_eps * rc.noise[(size_t)rc.sim * MAXMOVES + j];   // player.py:304
    return p_;
}
// c: the node's exploration constant, cpuct_of(P, sum_n)
XQ_D double root_u(double c, double p_, double xx, int n) { return c * p_ * xx / (double)(1 + n); }

// ---- the schedule of c_puct (include/czero.h, cz_search_set_cpuct_schedule) ---------------------------------------------
// c(sum_n) = c_puct + F * log((1 + sum_n + B) / B): float64, every operation rounded on its own, in the order written.  The
// one statement of it: select_edge, select_solve, the callers of prune_targets and cz_debug_cpuct read it.  F = 0 (off) is
// c_puct itself, bit for bit, and its float32 is c_puct_f32.  All 64 lanes call it with the same sum_n; the result is handed
// back in scalar registers, where c_puct itself lives.
// In k_sim the call stands in the SCHED instantiations alone (select_edge, select_solve), launched while F > 0: inlined behind
// a wave-uniform branch, the logarithm -- the library's, and a 12-term series of our own alike -- raised the scratch of
// every k_sim instantiation although the branch was never taken (k_sim<false, false> 44 -> 96 .. 136 bytes; EXPERIMENTS.md,
// "c_puct schedule").
XQ_D double cpuct_at(double c_puct, double factor, double base, int sum_n)
{
    if (!(factor > 0.0)) return c_puct;
    return unid(c_puct + factor * log(((1.0 + (double)uni(sum_n)) + base) / base));
}
XQ_D double cpuct_of(const SearchParams& P, int sum_n) { return cpuct_at(P.c_puct, P.cpuct_factor, P.cpuct_base, sum_n); }

// ---- Gumbel root search with sequential halving (include/czero.h, cz_search_set_gumbel) -------------------------------
// seq(m, n)[t]: how many selections the edge taken by the t-th root selection of the ply must already have.  A phase of
// the halving with k survivors appends e = max(1, n / (L k)) runs of k equal values, so entry t is found by walking the
// phases; nothing is stored.  Scalar, wave-uniform.
XQ_D int gumbel_seq(int m, int n, int t)
{
    if (m <= 1) return t;
    int L = 0;
    while ((1 << L) < m) ++L;
    int k = m, pos = 0, base = 0;
    for (;;) {
        int e = n / (L * k);
        if (e < 1) e = 1;
        if (t < pos + e * k) return base + (t - pos) / k;
        pos += e * k;
        base += e;
        k = k / 2 > 2 ? k / 2 : 2;
    }
}
XQ_D double gumbel_q01(int n, double w)
{
    if (n <= 0) return 0.0;
    const double q = (w / (double)n + 1.0) / 2.0;
    return q < 0.0 ? 0.0 : (q > 1.0 ? 1.0 : q);
}
XQ_D double gumbel_sigma(double c_visit, double c_scale, int max_n, double x) { return ((c_visit + (double)max_n) * c_scale) * x; }
// g_j + log p_j + sigma(q01_j); p = 0 scores -infinity
XQ_D double gumbel_score(double g, float p, double sig)
{
    const double lp = p > 0.0f ? log((double)p) : -__builtin_inf();
    return (g + lp) + sig;
}
// arg max of (score, index) over the lanes' candidates (best_j < 0: none), the later edge on a tie: select_edge's vote
XQ_D int gumbel_argmax(double best_s, int best_j)
{
    const double m = wave_max_f64(best_s);
    const bool top = best_j >= 0 && best_s == m;
    const uint64_t t1 = __ballot(top && best_j >= 64), t0 = __ballot(top);
    return t1 ? 64 + (63 - __clzll((long long)t1)) : (t0 ? 63 - __clzll((long long)t0) : -1);
}

// ---- full Gumbel search (include/czero.h, cz_search_set_gumbel_full) ----------------------------------------------------
// v_mix of a node: its own network value v mixed with the visited edges' prior-weighted mean q, N = sum of the edge counts,
// A = sum of the visited edges' priors, Bq = sum of p_j q01_j over them.  (A NaN value reads as 0: never NaN.)
XQ_D double gumbel_vmix(float v, int N, double A, double Bq)
{
    const double x = ((double)v + 1.0) / 2.0;
    const double vhat = x > 0.0 ? (x > 1.0 ? 1.0 : x) : 0.0;
    if (!(A > 0.0)) return vhat;
    return (vhat + (double)N * (Bq / A)) / (double)(1 + N);
}
// The selection below the root: one wavefront, edge j = lane + 64 h of the node's nm edges; n / w as selection reads them
// (virtual losses included), p the float32 prior, v the node's stored network value.  pi' = softmax(log p + sigma(completed
// q)), an unvisited edge completed with v_mix; score_j = pi'_j - n_j / (1 + N), returned in score[] (0 past nm); the result
// is the edge of the greatest score, the later one on a tie, -1 without an edge.  Float64, each sum the lane's two terms
// first and then the DPP ladder, the maximum and the vote as select_edge's.  All 64 lanes call it.
XQ_D int gumbel_interior(int nm, const int n[2], const double w[2], const float p[2], float v, double c_visit,
                         double c_scale, double score[2])
{
    const int lane = lane_id();
    bool live[2];
    int s = 0, max_n = 0;
    double A = 0.0, Bq = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        live[h] = lane + 64 * h < nm;
        score[h] = 0.0;
        if (!live[h]) continue;
        s += n[h];
        max_n = n[h] > max_n ? n[h] : max_n;
        if (n[h] > 0) {
            Bq = __dadd_rn(Bq, __dmul_rn((double)p[h], gumbel_q01(n[h], w[h])));
            A = __dadd_rn(A, (double)p[h]);
        }
    }
    const int N = __builtin_amdgcn_readlane(wave_incl_scan(s), 63);
    max_n = (int)wave_max_f64((double)max_n);
    Bq = wave_add_f64(Bq);
    A = wave_add_f64(A);
    const double vmix = gumbel_vmix(v, N, A, Bq);
    double sg[2] = {0.0, 0.0}, mx = -__builtin_inf();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (!live[h]) continue;
        sg[h] = gumbel_sigma(c_visit, c_scale, max_n, n[h] > 0 ? gumbel_q01(n[h], w[h]) : vmix);
        mx = sg[h] > mx ? sg[h] : mx;
    }
    mx = wave_max_f64(mx);
    double e[2] = {0.0, 0.0};
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (live[h]) e[h] = __dmul_rn((double)p[h], exp(sg[h] - mx));
    const double tot = wave_add_f64(__dadd_rn(e[0], e[1]));
    const double d = (double)(1 + N);
    double best_s = -__builtin_inf();
    int best_j = -1;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (!live[h]) continue;
        const double pi = tot > 0.0 ? e[h] / tot : 0.0;             // (every prior 0: the least n wins)
        score[h] = pi - (double)n[h] / d;
        if (score[h] >= best_s) { best_s = score[h]; best_j = lane + 64 * h; }   // h = 1 has the larger index: wins ties
    }
    return gumbel_argmax(best_s, best_j);
}

struct Picked {
    int j;              // edge index inside the node, -1 = none
    bool have;          // n / w / child / mv below are valid (winner among the first 64 edges)
    int n, child, mv;
    double w;
};

// The root's whole selection on a Gumbel ply: this is the t-th root selection of the ply, t = sum started; among the
// non-banned edges with started_j == seq(m, n)[t] the greatest g_j + log p_j + sigma(q01_j), the later edge on a tie.  No
// proven-win shortcut, no noise.  The winner's started count goes up by one, written by the lane that reads it (j & 63).
XQ_D int select_gumbel(int gumbel_m, double c_visit, double c_scale, int32_t* started, const double* gum, int budget,
                       char* base, const EdgeStat* sb, int nm, int n_no_act, const uint16_t* no_act)
{
    const int lane = lane_id();
    const float* pp = node_p(base);
    const uint16_t* pm = node_mv(base, nm);
    int st[2] = {0, 0}, n[2] = {0, 0};
    double w[2] = {0.0, 0.0};
    bool live[2] = {false, false};
    int max_n = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        if (j >= nm) continue;
        bool banned = false;
        for (int k = 0; k < n_no_act; ++k) banned = banned || (no_act[k] == pm[j]);
        live[h] = !banned;
        if (!live[h]) continue;
        st[h] = started[j];
        if (sb) { const EdgeStat es = sb[j]; n[h] = es.n; w[h] = es.w; }
        max_n = n[h] > max_n ? n[h] : max_n;
    }
    const int t = __builtin_amdgcn_readlane(wave_incl_scan(st[0] + st[1]), 63);
    max_n = (int)wave_max_f64((double)max_n);
    const int n_live = __popcll(__ballot(live[0])) + __popcll(__ballot(live[1]));
    const int v = gumbel_seq(gumbel_m < n_live ? gumbel_m : n_live, budget, t);
    double best_s = -__builtin_inf();
    int best_j = -1;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        if (!live[h] || st[h] != v) continue;
        const double sc = gumbel_score(gum[j], pp[j],
                                       gumbel_sigma(c_visit, c_scale, max_n, gumbel_q01(n[h], w[h])));
        if (sc >= best_s) { best_s = sc; best_j = j; }         // h = 1 has the larger index: wins ties
    }
    const int pick = gumbel_argmax(best_s, best_j);
    if (pick >= 0 && lane == (pick & 63)) started[pick] = st[pick >> 6] + 1;
    return pick;
}

// base: the node's record; sb: its stat block (nullptr: allocated in this visit, every edge is {0, 0, unknown}).
// GUM: the k_sim instantiation that is launched while the Gumbel root search is on -- the others do not hold its code,
// so their registers and their text are what they were without it.  net_value: the header's fourth word (GUM: the float32
// network value; ML: the leaf's k).
// ML: the k_sim instantiation that is launched while the moves-left utility is on (cz_search_set_moves_left); likewise.  Every
// lane loads its edges' M records, two integer wave sums give the parent's mean, and the score is (q + u) + u_m.
// DRAW: the k_sim instantiation that is launched while the draw average is on (cz_search_set_draw); likewise.  Every lane
// loads its edges' D records, and the score is (q + u) + sigma * dbar; sigma: draw_sigma of the node's depth.
// SCHED: the k_sim instantiation that is launched while the schedule of c_puct is on (cz_search_set_cpuct_schedule); likewise.
// The others read the constants P.c_puct and P.c_puct_f32 as they always did.
template <bool GUM, bool ML = false, bool DRAW = false, bool SCHED = false>
XQ_D Picked select_edge(const SearchParams& P, const SearchBuffers& B, int g, char* base, const EdgeStat* sb, int sum_n,
                        int nm, const RootCtx& rc, uint32_t net_value, const MovesLeftState& M = MovesLeftState{},
                        double sigma = 0.0)
{
    if (GUM && rc.is_root && P.gumbel_m > 0) {                  // wave-uniform
        Picked r;                                               // (have = false: the caller reloads the edge, this is not the hot path)
        r.j = select_gumbel(P.gumbel_m, P.gumbel_visit, P.gumbel_scale, B.g_started + (size_t)g * MAXMOVES,
                            B.g_gumbel + (size_t)g * MAXMOVES, uni(B.g_budget[g]), base, sb, nm, rc.n_no_act, rc.no_act);
        r.have = false;
        r.n = 0; r.child = CHILD_UNKNOWN; r.mv = 0; r.w = 0.0;
        return r;
    }
    if (GUM && !rc.is_root && P.gumbel_full && P.gumbel_m > 0) {    // wave-uniform
        // the full search below the root: the whole selection, the proven-win shortcut included, is gumbel_interior's.
        // Every edge takes part (only roots have bans); edge j is loaded by the lane that owns it, as below.
        const int lane = lane_id();
        const float* pp = node_p(base);
        int n[2] = {0, 0};
        double w[2] = {0.0, 0.0}, score[2];
        float p[2] = {0.0f, 0.0f};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = lane + 64 * h;
            if (j >= nm) continue;
            if (sb) { const EdgeStat es = sb[j]; n[h] = es.n; w[h] = es.w; }
            p[h] = pp[j];
        }
        Picked r;
        r.j = gumbel_interior(nm, n, w, p, __uint_as_float(net_value), P.gumbel_visit, P.gumbel_scale, score);
        r.have = false;
        r.n = 0; r.child = CHILD_UNKNOWN; r.mv = 0; r.w = 0.0;
        return r;
    }
    const int lane = lane_id();
    const double xx = __dsqrt_rn((double)(sum_n + 1));
    double c = P.c_puct;                                    // the node's exploration constant and its float32
    float c32 = P.c_puct_f32;
    if constexpr (SCHED) { c = cpuct_of(P, sum_n); c32 = (float)c; }
    const float* pp = node_p(base);
    const uint16_t* pm = node_mv(base, nm);
    int n0 = 0, child0 = CHILD_UNKNOWN, mv0 = 0;           // this lane's edge of the first half
    double w0 = 0.0;
    double best_s = -1.0e300;
    int best_j = -1;
    bool win0 = false, win1 = false;
    const int halves = nm > 64 ? 2 : 1;                     // almost every position has <= 64 moves
    double d0 = 0.0, d1 = 0.0;                              // (ML) this lane's clamped slope * (Mj - Mp) of the two halves
    if constexpr (ML) {
        MRec mr0{0, 0, 0}, mr1{0, 0, 0};
        if (sb) {                                           // (a fresh statistics block: every record is {0, 0})
            const MRec* mb = m_block(sb, nm);
            if (lane < nm) mr0 = mb[lane];                  // one 16-byte load
            if (lane + 64 < nm) mr1 = mb[lane + 64];
        }
        const long long K = (long long)(int)net_value + wave_add_i64(mr0.ksum + mr1.ksum);
        const int N = 1 + __builtin_amdgcn_readlane(wave_incl_scan(mr0.mn + mr1.mn), 63);
        const double Mp = ((double)K / 16.0) / (double)N;   // the node's own mean, in plies
        d0 = ml_edge_d(M, mr0.ksum, mr0.mn, Mp);
        d1 = ml_edge_d(M, mr1.ksum, mr1.mn, Mp);
    }
    if constexpr (DRAW) {                                   // d0, d1: this lane's sigma * dbar of the two halves
        DRec dr0{0, 0, 0}, dr1{0, 0, 0};
        if (sb) {                                           // (a fresh statistics block: every record is {0, 0})
            const DRec* db = d_block(sb, nm);
            if (lane < nm) dr0 = db[lane];                  // one 16-byte load
            if (lane + 64 < nm) dr1 = db[lane + 64];
        }
        d0 = draw_term(sigma, dr0.dsum, dr0.dn);
        d1 = draw_term(sigma, dr1.dsum, dr1.dn);
    }
#pragma nounroll
    for (int h = 0; h < halves; ++h) {
        const int j = lane + 64 * h;
        bool valid = j < nm;
        double score = -1.0e300;
        bool win = false;
        if (valid) {
            EdgeStat es{0.0, 0, CHILD_UNKNOWN};
            if (sb) es = sb[j];                              // N, W and the child link in one 16-byte load
            const float p = pp[j];
            const uint16_t mv = pm[j];
            const int n = es.n;
            const double w = es.w;
            if (h == 0) { n0 = n; w0 = w; child0 = es.child; mv0 = mv; }
            const double q = n ? w / (double)n : 0.0;
            double u;
            if (rc.is_root) {
                if (rc.n_no_act) valid = !root_banned(rc, mv);
                u = root_u(c, root_prior(P, rc, p, j), xx, n);
            } else {
                const float a = c32 * p;
                u = (double)a * xx / (double)(1 + n);
            }
            if (valid) {
                score = q + u;
                if constexpr (ML) score = score + ml_utility(h == 0 ? d0 : d1, q);
                if constexpr (DRAW) score = score + (h == 0 ? d0 : d1);
                win = q > (1.0 - 1e-7);
                if (!(score >= -99999999.0)) valid = false;
            }
        }
        if (h == 0) win0 = valid && win; else win1 = valid && win;
        if (valid && score >= best_s) { best_s = score; best_j = j; }   // h = 1 has the larger index: wins ties
    }
    if (rc.is_root && rc.force) {
        // forced playouts, a pass of its own so that the loop above stays what it was: a tried root child with
        // n < sqrt(k * p_ * sum_n) scores +infinity.  Compared squared: integers times integers against a product, no
        // square root and nothing a contraction could fuse.  Not for a banned edge or one whose score was rejected.
#pragma nounroll
        for (int h = 0; h < halves; ++h) {
            const int j = lane + 64 * h;
            if (j >= nm || !sb) continue;                       // (a fresh statistics block: nothing tried yet)
            const EdgeStat es = sb[j];
            const int n = es.n;
            if (n <= 0 || root_banned(rc, pm[j])) continue;
            const double p_ = root_prior(P, rc, pp[j], j);
            if (!((double)n * (double)n < P.forced_k * p_ * (double)sum_n)) continue;
            if (!(es.w / (double)n + root_u(c, p_, xx, n) >= -99999999.0)) continue;
            best_s = __builtin_inf();
            best_j = j;                                         // h = 1 has the larger index: wins ties
        }
    }
    // proven-win shortcut: first edge in order with q > 1 - 1e-7 (player.py:309-311)
    const int first_win = lowest_bit(__ballot(win0), __ballot(win1));
    int pick;
    if (first_win >= 0) pick = first_win;
    else {
        // arg max of (score, index): `>=` keeps the LAST maximal move (player.py:312-314).  The maximum itself by a
        // butterfly on the score alone (never NaN: see `valid`), then the lanes that hold it vote: the largest index wins,
        // and an index of the second half (lane + 64) beats any of the first.
        const double m = wave_max_f64(best_s);                       // DPP ladder (xq_rules.h), no LDS permutes
        const bool top = best_j >= 0 && best_s == m;
        const uint64_t t1 = __ballot(top && best_j >= 64), t0 = __ballot(top);
        pick = t1 ? 64 + (63 - __clzll((long long)t1)) : (t0 ? 63 - __clzll((long long)t0) : -1);
    }
    Picked r;
    r.j = pick;
    r.have = pick >= 0 && pick < 64;
    r.n = 0; r.child = CHILD_UNKNOWN; r.mv = 0; r.w = 0.0;
    if (r.have) {                                              // pick is wave-uniform: register reads, no LDS permute
        r.n = __builtin_amdgcn_readlane(n0, pick);
        r.child = __builtin_amdgcn_readlane(child0, pick);
        r.mv = __builtin_amdgcn_readlane(mv0, pick);
        const long long wb = __double_as_longlong(w0);
        const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)wb, pick);
        const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)((unsigned long long)wb >> 32), pick);
        r.w = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    }
    return r;
}

}  // namespace
