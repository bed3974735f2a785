// xq_search_aux.h -- part of xq_search.hip's translation unit; do not compile it into a second one.  Why: the same text as a
// unit of its own gave all eight k_sim* kernels 0.4-1.7 % more or fewer instructions (k_sim<false,false> 18 740 against
// 18 608, equal registers and scratch, nothing called out of line; cause not found).  The benchmark measures those kernels, so
// text only moves between these headers, and the proof of a move is the unit's device assembly, kernel by kernel
// (EXPERIMENTS.md, "the search unit's text in headers").
//
// Every kernel outside the round (k_start_selfplay .. k_debug_sqrt: roots, resets, the readers of the tree and of caller-supplied
// rows, the move choice, the test hooks) and walk_path.
#pragma once
#include "xq_search_tree.h"
#include "xq_search_ml.h"
#include "xq_search_draw.h"
#include "xq_search_var.h"
#include "xq_search_select.h"
#include "xq_search_solver.h"
#include "xq_search_ply.h"
#include "xq_search_records.h"
#include "xq_noise.h"

namespace {

// ---- auxiliary kernels ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_start_selfplay(SearchParams P, SearchBuffers B, uint32_t first_game_id)
{
    __shared__ SearchLDS L;
    const int g = blockIdx.x;
    if (g >= P.G) return;
    const GameView gv = make_view(B, P, g, B.counters + (size_t)g * CT_COUNT, L.chtab);   // counts go straight to the global block
    const int lane = lane_id();
    for (int i = lane; i < P.K; i += 64) gv.s_state[i] = SIM_IDLE;
    for (int i = lane; i < CT_COUNT; i += 64) gv.ctr[i] = 0;
    wave_sync_global();
    new_game(P, B, gv, L, first_game_id + (uint32_t)g);
}

// k_start_selfplay with a script on: slot g starts on script first_game_id + g, or idle where there is none
__global__ __launch_bounds__(64) void k_start_script(SearchParams P, SearchBuffers B, ScriptState X, uint32_t first_game_id)
{
    __shared__ SearchLDS L;
    const int g = blockIdx.x;
    if (g >= P.G) return;
    const GameView gv = make_view(B, P, g, B.counters + (size_t)g * CT_COUNT, L.chtab);   // counts go straight to the global block
    const int lane = lane_id();
    for (int i = lane; i < P.K; i += 64) gv.s_state[i] = SIM_IDLE;
    for (int i = lane; i < CT_COUNT; i += 64) gv.ctr[i] = 0;
    wave_sync_global();
    new_script_game(P, B, gv, L, X, first_game_id + (uint32_t)g);
}

__global__ __launch_bounds__(64) void k_set_roots(SearchParams P, SearchBuffers B, const int8_t* __restrict__ boards,
                                                 const int32_t* __restrict__ turns, const uint16_t* __restrict__ no_act,
                                                 const uint8_t* __restrict__ n_no_act, const uint8_t* __restrict__ inc,
                                                 const uint8_t* __restrict__ enable_resign,
                                                 const uint8_t* __restrict__ select_mask,
                                                 const int8_t* __restrict__ prev_boards,
                                                 const uint8_t* __restrict__ hist_kind)
{
    __shared__ SearchLDS L;
    const int g = blockIdx.x;
    if (g >= P.G) return;
    if (select_mask && !select_mask[g]) return;
    const GameView gv = make_view(B, P, g, B.counters + (size_t)g * CT_COUNT, L.chtab);   // counts go straight to the global block
    const int lane = lane_id();
    load_board(boards + (size_t)g * NSQ, L.r.bd[0]);
    int8_t* gb = B.g_board + (size_t)g * BOARD_LDS;
    gb[lane] = L.r.bd[0][lane];
    if (lane < 32) gb[lane + 64] = L.r.bd[0][lane + 64];
    const int nna = n_no_act ? (int)n_no_act[g] : 0;
    if (lane < MAX_NO_ACT) B.g_no_act[(size_t)g * MAX_NO_ACT + lane] = (no_act && lane < nna) ? no_act[(size_t)g * MAX_NO_ACT + lane] : (uint16_t)NOMOVE;
    for (int i = lane; i < P.K; i += 64) gv.s_state[i] = SIM_IDLE;
    {
        const int hk = hist_kind ? (int)hist_kind[g] : 0;
        int8_t* pb = B.g_prev_board + (size_t)g * BOARD_LDS;
        if (hk == 1 && prev_boards) {
            for (int i = lane; i < NSQ; i += 64) pb[i] = prev_boards[(size_t)g * NSQ + i];
        }
        if (lane == 0) B.g_hist_kind[g] = (uint8_t)((hk == 1 && !prev_boards) ? 2 : hk);
    }
    if (lane == 0) {
        B.g_turns[g] = turns ? turns[g] : 0;
        B.g_n_no_act[g] = (uint8_t)(nna < MAX_NO_ACT ? nna : MAX_NO_ACT);
        B.g_increase_temp[g] = inc ? inc[g] : 0;
        B.g_enable_resign[g] = enable_resign ? enable_resign[g] : 0;
    }
    wave_sync_global();
    // a terminal root has nothing to search (the reference's simulations would all return at once)
    const DoneResult d = wave_done(L.r.bd[0], L.r.bd[1], L.r.ml[0], L.r.ml[1], L.r.plist, false);
    begin_search(P, B, gv, L);
    if (d.over && lane == 0) { B.g_tasks_left[g] = 0; }
}

__global__ __launch_bounds__(64) void k_reset_trees(SearchParams P, SearchBuffers B)
{
    __shared__ uint32_t chtab[MAX_CHUNKS];
    const int g = blockIdx.x;
    if (g >= P.G) return;
    const GameView gv = make_view(B, P, g, B.counters + (size_t)g * CT_COUNT, chtab);   // counts go straight to the global block
    clear_tree(P, B, gv, chtab);
    const int lane = lane_id();
    for (int i = lane; i < P.K; i += 64) gv.s_state[i] = SIM_IDLE;
    if (lane == 0) { B.g_phase[g] = PH_IDLE; B.g_active[g] = 0; B.g_tasks_left[g] = 0; }
}

// chunks returned by earlier launches become takeable (entry points outside the round call this first)
__global__ void k_pool_commit(SearchBuffers B) { pool_commit(B); }

__global__ void k_pending(SearchParams P, SearchBuffers B)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < P.G && B.g_phase[g] == PH_SEARCH) atomicAdd(B.pending, 1);
}

// queue rows that hold a new leaf (a position the network has to evaluate) after a round, compacted; rows[] order is
// arbitrary.  counts[0] = searches still running, counts[1] = rows written.
__global__ void k_leaf_rows(SearchParams P, SearchBuffers B, int32_t* __restrict__ rows, int32_t* __restrict__ counts)
{
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= P.G * P.K) return;
    const int g = slot / P.K;
    if (B.g_phase[g] != PH_SEARCH) return;
    if (slot == g * P.K) atomicAdd(&counts[0], 1);
    if (B.s_state[slot] == SIM_LEAF) rows[atomicAdd(&counts[1], 1)] = slot;
}

// the node reached from the game's root along path[g][0 .. path_len) (move labels, NOMOVE ends the path early; NULL: the
// root), -1 when it is not linked in the tree.  All 64 lanes call it.
XQ_D int walk_path(const SearchBuffers& B, const GameView& gv, const uint16_t* __restrict__ path, int path_len)
{
    const int lane = lane_id();
    const int g = gv.g;
    int root = B.g_root[g];
    for (int d = 0; path && d < path_len && root >= 0; ++d) {
        const uint16_t mv = path[(size_t)g * path_len + d];
        if (mv == NOMOVE) break;
        char* base = rec_ptr(gv, (uint32_t)root);
        const NodeHdr hdr = load_hdr(base);
        const int pn = (int)(hdr.meta & 0xFF);
        const uint16_t* pm = node_mv(base, pn);
        int child = -1;
        if (hdr.stat) {
            const EdgeStat* sb = edge_ptr(gv, hdr.stat);
            for (int j = lane; j < pn; j += 64)
                if (pm[j] == mv) child = child_id(sb[j].child);
        }
        const unsigned long long hit = __ballot(child >= 0);
        root = hit ? __shfl(child, __ffsll((long long)hit) - 1) : -1;
    }
    return root;
}

// statistics of the root, or of the node reached from the root along path[g][0 .. path_len) (move labels, NOMOVE ends
// the path early); a node that is not linked in the tree reports count 0
__global__ __launch_bounds__(64) void k_root_stats(SearchParams P, SearchBuffers B, const uint16_t* __restrict__ path,
                                                  int path_len, uint16_t* __restrict__ moves,
                                                  int32_t* __restrict__ n, double* __restrict__ w,
                                                  float* __restrict__ p, int32_t* __restrict__ sum_n,
                                                  uint8_t* __restrict__ counts)
{
    __shared__ uint32_t chtab[MAX_CHUNKS];
    const int g = blockIdx.x;
    if (g >= P.G) return;
    const GameView gv = make_view(B, P, g, B.counters + (size_t)g * CT_COUNT, chtab);   // counts go straight to the global block
    const int lane = lane_id();
    const int root = walk_path(B, gv, path, path_len);
    int nm = 0, root_sum_n = 0;
    char* base = nullptr;
    const EdgeStat* sb = nullptr;
    if (root >= 0) {
        base = rec_ptr(gv, (uint32_t)root);
        const NodeHdr hdr = load_hdr(base);
        nm = (int)(hdr.meta & 0xFF);
        root_sum_n = hdr.sum_n;
        if (hdr.stat) sb = edge_ptr(gv, hdr.stat);
    }
    for (int j = lane; j < MAXMOVES; j += 64) {
        const bool ok = j < nm;
        EdgeStat es{0.0, 0, CHILD_UNKNOWN};
        if (ok && sb) es = sb[j];
        if (moves) moves[(size_t)g * MAXMOVES + j] = ok ? node_mv(base, nm)[j] : (uint16_t)NOMOVE;
        if (n) n[(size_t)g * MAXMOVES + j] = es.n;
        if (w) w[(size_t)g * MAXMOVES + j] = es.w;
        if (p) p[(size_t)g * MAXMOVES + j] = ok ? node_p(base)[j] : 0.0f;
    }
    if (lane == 0) {
        if (sum_n) sum_n[g] = root_sum_n;
        if (counts) counts[g] = (uint8_t)nm;
    }
}

// Moves-left utility: the M records of the root, or of the node reached from it along path[g][0 .. path_len) as in
// k_root_stats: per edge ksum and mn (0 past the node's edges and without a statistics block), per game the node's own k.
// Launched only while the option is on: a tree grown without it has no M records.
__global__ __launch_bounds__(64) void k_node_moves_left(SearchParams P, SearchBuffers B, const uint16_t* __restrict__ path,
                                                       int path_len, long long* __restrict__ ksum, int32_t* __restrict__ mn,
                                                       int32_t* __restrict__ k_net, uint8_t* __restrict__ counts)
{
    __shared__ uint32_t chtab[MAX_CHUNKS];
    const int g = blockIdx.x;
    if (g >= P.G) return;
    const GameView gv = make_view(B, P, g, B.counters + (size_t)g * CT_COUNT, chtab);
    const int lane = lane_id();
    int node = walk_path(B, gv, path, path_len);
    if (node == 0) node = -1;                                   // (id 0 is "none": an object never given a root)
    int nm = 0, k = 0;
    const MRec* mb = nullptr;
    if (node >= 0) {
        const NodeHdr hdr = load_hdr(rec_ptr(gv, (uint32_t)node));
        nm = (int)(hdr.meta & 0xFF);
        k = (int)hdr.val;
        if (hdr.stat) mb = m_block(edge_ptr(gv, hdr.stat), nm);
    }
    for (int j = lane; j < MAXMOVES; j += 64) {
        MRec r{0, 0, 0};
        if (j < nm && mb) r = mb[j];
        if (ksum) ksum[(size_t)g * MAXMOVES + j] = r.ksum;
        if (mn) mn[(size_t)g * MAXMOVES + j] = r.mn;
    }
    if (lane == 0) {
        if (k_net) k_net[g] = k;
        if (counts) counts[g] = (uint8_t)nm;
    }
}

// k[i] = ml_quanta(x[i]): the attach's conversion, row by row (cz_moves_left_quanta)
__global__ void k_ml_quanta(const float* __restrict__ x, int32_t* __restrict__ k, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) k[i] = ml_quanta(x[i]);
}

// Draw average: the D records of the root, or of the node reached from it along path[g][0 .. path_len) as in k_root_stats:
// per edge dsum and dn (0 past the node's edges and without a statistics block), per game the node's own dq.  Launched only
// while the option is on: a tree grown without it has no D records.
__global__ __launch_bounds__(64) void k_node_draws(SearchParams P, SearchBuffers B, const uint16_t* __restrict__ path,
                                                  int path_len, long long* __restrict__ dsum, int32_t* __restrict__ dn,
                                                  int32_t* __restrict__ dq_net, uint8_t* __restrict__ counts)
{
    __shared__ uint32_t chtab[MAX_CHUNKS];
    const int g = blockIdx.x;
    if (g >= P.G) return;
    const GameView gv = make_view(B, P, g, B.counters + (size_t)g * CT_COUNT, chtab);
    const int lane = lane_id();
    int node = walk_path(B, gv, path, path_len);
    if (node == 0) node = -1;                                   // (id 0 is "none": an object never given a root)
    int nm = 0, dq = 0;
    const DRec* db = nullptr;
    if (node >= 0) {
        const NodeHdr hdr = load_hdr(rec_ptr(gv, (uint32_t)node));
        nm = (int)(hdr.meta & 0xFF);
        dq = (int)hdr.val;
        if (hdr.stat) db = d_block(edge_ptr(gv, hdr.stat), nm);
    }
    for (int j = lane; j < MAXMOVES; j += 64) {
        DRec r{0, 0, 0};
        if (j < nm && db) r = db[j];
        if (dsum) dsum[(size_t)g * MAXMOVES + j] = r.dsum;
        if (dn) dn[(size_t)g * MAXMOVES + j] = r.dn;
    }
    if (lane == 0) {
        if (dq_net) dq_net[g] = dq;
        if (counts) counts[g] = (uint8_t)nm;
    }
}

// dq[i] = draw_quanta(d[i * stride]): the attach's conversion of a strided column (cz_draw_quanta)
__global__ void k_draw_quanta(const float* __restrict__ d, int stride, int32_t* __restrict__ dq, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dq[i] = draw_quanta(d[(size_t)i * stride]);
}

// MCTS solver: the proof state of the root, or of the node reached from it along path[g][0 .. path_len) as in k_root_stats:
// status [G] (Proof; -1 where the position is not linked in the tree) and dist [G]; per edge the mark (Proof of the child:
// terminal children by their code) and the marked child's distance, 0 past the node's edges and for an unmarked edge.
__global__ __launch_bounds__(64) void k_node_proof(SearchParams P, SearchBuffers B, const uint16_t* __restrict__ path,
                                                  int path_len, int8_t* __restrict__ status, uint8_t* __restrict__ dist,
                                                  uint8_t* __restrict__ mark, uint8_t* __restrict__ mark_dist)
{
    __shared__ uint32_t chtab[MAX_CHUNKS];
    const int g = blockIdx.x;
    if (g >= P.G) return;
    const GameView gv = make_view(B, P, g, B.counters + (size_t)g * CT_COUNT, chtab);
    const int lane = lane_id();
    int node = walk_path(B, gv, path, path_len);
    if (node == 0) node = -1;                                   // (id 0 is "none": an object never given a root)
    int nm = 0;
    uint32_t meta = 0u;
    const EdgeStat* sb = nullptr;
    if (node >= 0) {
        const NodeHdr hdr = load_hdr(rec_ptr(gv, (uint32_t)node));
        meta = hdr.meta;
        nm = (int)(meta & 0xFF);
        if (hdr.stat) sb = edge_ptr(gv, hdr.stat);
    }
    for (int j = lane; j < MAXMOVES; j += 64) {
        int mk = PROOF_OPEN, d = 0;
        if (j < nm && sb) {
            const int c = sb[j].child;
            mk = child_mark(c);
            if (mk != PROOF_OPEN) d = child_dist(gv, c);
        }
        if (mark) mark[(size_t)g * MAXMOVES + j] = (uint8_t)mk;
        if (mark_dist) mark_dist[(size_t)g * MAXMOVES + j] = (uint8_t)d;
    }
    if (lane == 0) {
        if (status) status[g] = node >= 0 ? (int8_t)meta_proof(meta) : (int8_t)-1;
        if (dist) dist[g] = (uint8_t)meta_dist(meta);
    }
}

// MCTS solver: out [G] = 1 where the game's current root is decided (solve_root_decided), with the bans of the ply
__global__ __launch_bounds__(64) void k_root_decided(SearchParams P, SearchBuffers B, uint8_t* __restrict__ out)
{
    __shared__ uint32_t chtab[MAX_CHUNKS];
    const int g = blockIdx.x;
    if (g >= P.G) return;
    const GameView gv = make_view(B, P, g, B.counters + (size_t)g * CT_COUNT, chtab);
    const bool dec = solve_root_decided(B, gv, nullptr);
    if (lane_id() == 0) out[g] = dec ? (uint8_t)1 : (uint8_t)0;
}

// What emit_visits would record for every current root, with the bans of the current set_roots (cz_search_root_targets,
// _root_value, _root_surprise, _root_maxq): the pruned counts n [G][128] and their raw total, the search value q, the policy
// surprise s, the resignation test's max q (NaN: the root is not in the tree).  A NULL output is not computed.  One
// wavefront per game.
// gumbel (or the option on): the counts are the Gumbel policy targets, as a VISIT_GUMBEL entry holds them; FULL: the full
// search's (launched while cz_search_set_gumbel_full is on).
template <bool FULL>
__global__ __launch_bounds__(64) void k_root_records(SearchParams P, SearchBuffers B, int32_t* __restrict__ n,
                                                    int32_t* __restrict__ raw_total, double* __restrict__ q,
                                                    double* __restrict__ s, int gumbel, double* __restrict__ mq)
{
    __shared__ uint32_t chtab[MAX_CHUNKS];
    const int g = blockIdx.x;
    if (g >= P.G) return;
    const GameView gv = make_view(B, P, g, B.counters + (size_t)g * CT_COUNT, chtab);
    const int lane = lane_id();
    const RootEdges E = load_root_edges(B, gv);
    int m[2] = {E.n[0], E.n[1]};
    const int S = (gumbel || P.gumbel_m > 0) ? gumbel_targets<FULL>(E.nm, E.lab, m, E.n, E.w, E.p, P.gumbel_visit, P.gumbel_scale,
                                                                    FULL ? root_net_value(B, gv) : 0.0f)
                                             : prune_targets(E.nm, E.lab, m, E.w, E.p, P.c_puct, P.cpuct_factor, P.cpuct_base, P.forced_k);
    if (n) {
#pragma unroll
        for (int h = 0; h < 2; ++h) n[(size_t)g * MAXMOVES + lane + 64 * h] = lane + 64 * h < E.nm ? m[h] : 0;
    }
    if (raw_total && lane == 0) raw_total[g] = S;
    if (q) {
        const double v = root_value(E.nm, E.lab, m, E.n, E.w);
        if (lane == 0) q[g] = v;
    }
    if (s) {
        const double v = root_surprise(E.nm, E.lab, m, E.p);
        if (lane == 0) s[g] = v;
    }
    if (mq) {
        // (no root: -1 after a search began on a position the tree does not hold, 0 -- the id that names no record --
        //  in an object that has not been given roots yet)
        const double v = uni(B.g_root[g]) <= 0 ? __builtin_nan("") : root_maxq(E.nm, E.lab, E.n, E.w);
        if (lane == 0) mq[g] = v;
    }
}

// cz_policy_target_prune, cz_root_value, cz_root_surprise, cz_root_maxq: the same arithmetic on caller-supplied rows [rows][128], one
// wavefront per row.  out_n (with out_raw_total): the counts n are pruned; otherwise m holds the recorded counts.  A
// NULL input reads as zeros, a NULL output is not computed.
__global__ __launch_bounds__(64) void k_row_records(const uint16_t* __restrict__ labels, const int32_t* __restrict__ m_in,
                                                   const int32_t* __restrict__ n, const double* __restrict__ w,
                                                   const float* __restrict__ p, const uint8_t* __restrict__ n_edges,
                                                   int rows, double c_puct, double k, int32_t* __restrict__ out_n,
                                                   int32_t* __restrict__ out_raw_total, double* __restrict__ out_q,
                                                   double* __restrict__ out_s, double* __restrict__ out_mq)
{
    const int r = blockIdx.x;
    if (r >= rows) return;
    const int lane = lane_id();
    const RootEdges E = load_row_edges(labels, n, w, p, n_edges, r);
    int m[2] = {E.n[0], E.n[1]};
    if (out_mq) {                           // cz_root_maxq: the raw statistics alone, no recorded counts
        const double v = root_maxq(E.nm, E.lab, E.n, E.w);
        if (lane == 0) out_mq[r] = v;
        return;
    }
    if (out_n) {
        const int S = prune_targets(E.nm, E.lab, m, E.w, E.p, c_puct, 0.0, 1.0, k);
#pragma unroll
        for (int h = 0; h < 2; ++h) out_n[(size_t)r * MAXMOVES + lane + 64 * h] = lane + 64 * h < E.nm ? m[h] : 0;
        if (lane == 0) out_raw_total[r] = S;
    } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) m[h] = lane + 64 * h < E.nm ? m_in[(size_t)r * MAXMOVES + lane + 64 * h] : 0;
    }
    if (out_q) {
        const double v = root_value(E.nm, E.lab, m, E.n, E.w);
        if (lane == 0) out_q[r] = v;
    }
    if (out_s) {
        const double v = root_surprise(E.nm, E.lab, m, E.p);
        if (lane == 0) out_s[r] = v;
    }
}

// cz_gumbel_policy_target: gumbel_targets on caller-supplied rows [rows][128], one wavefront per row
// FULL (cz_gumbel_policy_target_v): the full search's target, v [rows] the rows' network values
template <bool FULL>
__global__ __launch_bounds__(64) void k_gumbel_rows(const uint16_t* __restrict__ labels, const int32_t* __restrict__ n,
                                                   const double* __restrict__ w, const float* __restrict__ p,
                                                   const uint8_t* __restrict__ n_edges, int rows, double c_visit,
                                                   double c_scale, int32_t* __restrict__ out_m,
                                                   int32_t* __restrict__ out_raw_total, const float* __restrict__ v)
{
    const int r = blockIdx.x;
    if (r >= rows) return;
    const int lane = lane_id();
    const RootEdges E = load_row_edges(labels, n, w, p, n_edges, r);
    int m[2];
    const int S = gumbel_targets<FULL>(E.nm, E.lab, m, E.n, E.w, E.p, c_visit, c_scale, FULL ? v[r] : 0.0f);
#pragma unroll
    for (int h = 0; h < 2; ++h) out_m[(size_t)r * MAXMOVES + lane + 64 * h] = m[h];
    if (lane == 0) out_raw_total[r] = S;
}

// cz_search_node_net_value: the stored network value (store_net_value) of the node k_root_stats reports for the same path;
// NaN when the position is not linked in the tree or still waits for its evaluation.  One wavefront per game.
__global__ __launch_bounds__(64) void k_node_net_value(SearchParams P, SearchBuffers B, const uint16_t* __restrict__ path,
                                                      int path_len, float* __restrict__ v)
{
    __shared__ uint32_t chtab[MAX_CHUNKS];
    const int g = blockIdx.x;
    if (g >= P.G) return;
    const GameView gv = make_view(B, P, g, B.counters + (size_t)g * CT_COUNT, chtab);
    const int node = walk_path(B, gv, path, path_len);
    float out = __builtin_nanf("");
    if (node >= 0) {
        const NodeHdr hdr = load_hdr(rec_ptr(gv, (uint32_t)node));
        if (!(hdr.meta & NODE_WAITING)) out = __uint_as_float(hdr.val);
    }
    if (lane_id() == 0) v[g] = out;
}

// cz_gumbel_interior_pick: gumbel_interior, the full search's selection below the root, on caller-supplied rows
// [rows][128], one wavefront per row; out_score [rows][128] (0 past n_edges), out_pick -1 for a row without edges
__global__ __launch_bounds__(64) void k_gumbel_interior_rows(const int32_t* __restrict__ n, const double* __restrict__ w,
                                                            const float* __restrict__ p,
                                                            const uint8_t* __restrict__ n_edges,
                                                            const float* __restrict__ v, int rows, double c_visit,
                                                            double c_scale, int32_t* __restrict__ out_pick,
                                                            double* __restrict__ out_score)
{
    const int r = blockIdx.x;
    if (r >= rows) return;
    const int lane = lane_id();
    const int nm = n_edges[r] > MAXMOVES ? MAXMOVES : n_edges[r];
    int nn[2] = {0, 0};
    double ww[2] = {0.0, 0.0}, score[2];
    float pp[2] = {0.0f, 0.0f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const size_t i = (size_t)r * MAXMOVES + lane + 64 * h;
        if (lane + 64 * h >= nm) continue;
        nn[h] = n[i]; ww[h] = w[i]; pp[h] = p[i];
    }
    const int pick = gumbel_interior(nm, nn, ww, pp, v[r], c_visit, c_scale, score);
#pragma unroll
    for (int h = 0; h < 2; ++h) out_score[(size_t)r * MAXMOVES + lane + 64 * h] = score[h];
    if (lane == 0) out_pick[r] = pick;
}

// cz_debug_cpuct: cpuct_at, the schedule of c_puct, on a list of sums, one wavefront per sum as the selection calls it; out_c32
// the float32 the selection below the root multiplies the prior with
__global__ __launch_bounds__(64) void k_cpuct_rows(const int32_t* __restrict__ sum_n, int rows, double c_puct, double factor,
                                                  double base, double* __restrict__ out_c, float* __restrict__ out_c32)
{
    const int r = blockIdx.x;
    if (r >= rows) return;
    const double c = cpuct_at(c_puct, factor, base, sum_n[r]);
    if (lane_id() == 0) {
        out_c[r] = c;
        out_c32[r] = (float)c;
    }
}

// Principal variation (print_depth_info, player.py:408-433): from the root follow the most-visited edge -- `>=` keeps
// the LAST maximum, banned moves are skipped at the root only -- until a node that was never selected from (the
// reference creates a node's edges at its first selection: an empty `a` ends the line), a terminal / unlinked child or
// max_len moves.  moves [G][max_len] (NOMOVE padded), visits [G][max_len].
__global__ __launch_bounds__(64) void k_pv(SearchParams P, SearchBuffers B, int max_len, uint16_t* __restrict__ moves,
                                          int32_t* __restrict__ visits)
{
    __shared__ uint32_t chtab[MAX_CHUNKS];
    const int g = blockIdx.x;
    if (g >= P.G) return;
    const GameView gv = make_view(B, P, g, B.counters + (size_t)g * CT_COUNT, chtab);
    const int lane = lane_id();
    const int n_no_act = B.g_n_no_act[g];
    const uint16_t* no_act = B.g_no_act + (size_t)g * MAX_NO_ACT;
    int node = B.g_root[g];
    int d = 0;
    for (; d < max_len && node >= 0; ++d) {
        char* base = rec_ptr(gv, (uint32_t)node);
        const NodeHdr hdr = load_hdr(base);
        const int nm = (int)(hdr.meta & 0xFF);
        if (hdr.stat == 0u || nm == 0) break;
        const uint16_t* pm = node_mv(base, nm);
        const EdgeStat* sb = edge_ptr(gv, hdr.stat);
        int best_n = 0, best_j = -1;                          // per lane: last j with n >= running maximum
        for (int j = lane; j < nm; j += 64) {
            const int n = sb[j].n;
            bool banned = false;
            if (d == 0) for (int k = 0; k < n_no_act; ++k) banned = banned || (no_act[k] == pm[j]);
            if (!banned && n >= best_n) { best_n = n; best_j = j; }
        }
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {                   // arg max of (n, j)
            const int on = __shfl_xor(best_n, s, 64), oj = __shfl_xor(best_j, s, 64);
            if (oj >= 0 && (best_j < 0 || on > best_n || (on == best_n && oj > best_j))) { best_n = on; best_j = oj; }
        }
        best_n = uni(best_n); best_j = uni(best_j);
        if (best_j < 0 || best_n <= 0) break;
        if (lane == 0) {
            moves[(size_t)g * max_len + d] = pm[best_j];
            visits[(size_t)g * max_len + d] = best_n;
        }
        node = child_id(uni(sb[best_j].child));
    }
    for (int i = d + lane; i < max_len; i += 64) {
        moves[(size_t)g * max_len + i] = (uint16_t)NOMOVE;
        visits[(size_t)g * max_len + i] = 0;
    }
}

// k_pv with the lower-confidence-bound move choice on (cz_search_set_lcb): the line's first move is lcb_pick's on the root's
// fields as they stand, so that a finished search's line starts with the move choose_action plays; below the root the line is
// k_pv's.  A kernel of its own with k_pv's walk written out again: k_pv keeps its text (the same walk as a function of both gave
// k_pv another instruction stream).
__global__ __launch_bounds__(64) void k_pv_lcb(SearchParams P, SearchBuffers B, int max_len, uint16_t* __restrict__ moves,
                                              int32_t* __restrict__ visits, LcbState Z)
{
    __shared__ uint32_t chtab[MAX_CHUNKS];
    const int g = blockIdx.x;
    if (g >= P.G) return;
    const GameView gv = make_view(B, P, g, B.counters + (size_t)g * CT_COUNT, chtab);
    const int lane = lane_id();
    int node = B.g_root[g];
    int d = 0;
    for (; d < max_len && node >= 0; ++d) {
        char* base = rec_ptr(gv, (uint32_t)node);
        const NodeHdr hdr = load_hdr(base);
        const int nm = (int)(hdr.meta & 0xFF);
        if (hdr.stat == 0u || nm == 0) break;
        const uint16_t* pm = node_mv(base, nm);
        const EdgeStat* sb = edge_ptr(gv, hdr.stat);
        int best_n = 0, best_j = -1;
        if (d == 0) {                                         // the root: the rule, with the ply's bans
            const LcbEdges E = load_lcb_root(B, gv);
            double bound[2];
            best_j = lcb_pick(E, Z.z, Z.ratio, bound);
            if (best_j >= 0) best_n = best_j < 64 ? __builtin_amdgcn_readlane(E.n[0], best_j & 63)
                                                  : __builtin_amdgcn_readlane(E.n[1], best_j & 63);
        } else {                                              // below it: last j with n >= running maximum, as k_pv
            for (int j = lane; j < nm; j += 64) {
                const int n = sb[j].n;
                if (n >= best_n) { best_n = n; best_j = j; }
            }
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {               // arg max of (n, j)
                const int on = __shfl_xor(best_n, s, 64), oj = __shfl_xor(best_j, s, 64);
                if (oj >= 0 && (best_j < 0 || on > best_n || (on == best_n && oj > best_j))) { best_n = on; best_j = oj; }
            }
            best_n = uni(best_n); best_j = uni(best_j);
        }
        if (best_j < 0 || best_n <= 0) break;
        if (lane == 0) {
            moves[(size_t)g * max_len + d] = pm[best_j];
            visits[(size_t)g * max_len + d] = best_n;
        }
        node = child_id(uni(sb[best_j].child));
    }
    for (int i = d + lane; i < max_len; i += 64) {
        moves[(size_t)g * max_len + i] = (uint16_t)NOMOVE;
        visits[(size_t)g * max_len + i] = 0;
    }
}

template <bool SOLVE>
__global__ __launch_bounds__(64) void k_choose(SearchParams P, SearchBuffers B, const double* __restrict__ u,
                                              int32_t* __restrict__ action)
{
    __shared__ SearchLDS L;
    const int g = blockIdx.x;
    if (g >= P.G) return;
    const GameView gv = make_view(B, P, g, B.counters + (size_t)g * CT_COUNT, L.chtab);   // counts go straight to the global block
    const int a = choose_action<SOLVE>(P, B, gv, L, u ? u[g] : 0.5, B.g_enable_resign[g] != 0);
    if (lane_id() == 0) action[g] = a;
}

// k_choose with the lower-confidence-bound move choice on (cz_search_set_lcb refuses the solver)
__global__ __launch_bounds__(64) void k_choose_lcb(SearchParams P, SearchBuffers B, const double* __restrict__ u,
                                                  int32_t* __restrict__ action, LcbState Z)
{
    __shared__ SearchLDS L;
    const int g = blockIdx.x;
    if (g >= P.G) return;
    const GameView gv = make_view(B, P, g, B.counters + (size_t)g * CT_COUNT, L.chtab);   // counts go straight to the global block
    const int a = choose_action<false, true>(P, B, gv, L, u ? u[g] : 0.5, B.g_enable_resign[g] != 0, Z);
    if (lane_id() == 0) action[g] = a;
}

// Lower-confidence-bound move choice: the V records of the root, or of the node reached from it along path[g][0 .. path_len) as
// in k_root_stats: per edge s2 and vn (0 past the node's edges and without a statistics block).  Launched only while the option is
// on: a tree grown without it has no V records.
__global__ __launch_bounds__(64) void k_node_values(SearchParams P, SearchBuffers B, const uint16_t* __restrict__ path,
                                                   int path_len, double* __restrict__ s2, int32_t* __restrict__ vn,
                                                   uint8_t* __restrict__ counts)
{
    __shared__ uint32_t chtab[MAX_CHUNKS];
    const int g = blockIdx.x;
    if (g >= P.G) return;
    const GameView gv = make_view(B, P, g, B.counters + (size_t)g * CT_COUNT, chtab);
    const int lane = lane_id();
    int node = walk_path(B, gv, path, path_len);
    if (node == 0) node = -1;                                   // (id 0 is "none": an object never given a root)
    int nm = 0;
    const VRec* vb = nullptr;
    if (node >= 0) {
        const NodeHdr hdr = load_hdr(rec_ptr(gv, (uint32_t)node));
        nm = (int)(hdr.meta & 0xFF);
        if (hdr.stat) vb = v_block(edge_ptr(gv, hdr.stat), nm);
    }
    for (int j = lane; j < MAXMOVES; j += 64) {
        VRec r{0.0, 0, 0};
        if (j < nm && vb) r = vb[j];
        if (s2) s2[(size_t)g * MAXMOVES + j] = r.s2;
        if (vn) vn[(size_t)g * MAXMOVES + j] = r.vn;
    }
    if (lane == 0 && counts) counts[g] = (uint8_t)nm;
}

// cz_search_root_lcb: lcb_pick on every current root, with the bans of the current set_roots: lcb [G][128] (NaN for an edge that
// is not eligible or past the edges), pick [G] (-1: the root is not in the tree, or every edge is banned).
__global__ __launch_bounds__(64) void k_root_lcb(SearchParams P, SearchBuffers B, LcbState Z, double* __restrict__ lcb,
                                                int32_t* __restrict__ pick)
{
    __shared__ uint32_t chtab[MAX_CHUNKS];
    const int g = blockIdx.x;
    if (g >= P.G) return;
    const GameView gv = make_view(B, P, g, B.counters + (size_t)g * CT_COUNT, chtab);
    const int lane = lane_id();
    const LcbEdges E = load_lcb_root(B, gv);
    double bound[2];
    const int j = lcb_pick(E, Z.z, Z.ratio, bound);
    if (lcb) {
#pragma unroll
        for (int h = 0; h < 2; ++h) lcb[(size_t)g * MAXMOVES + lane + 64 * h] = bound[h];
    }
    if (pick && lane == 0) pick[g] = j;
}

// cz_lcb_pick: the same arithmetic on caller-supplied rows [rows][128], one wavefront per row
__global__ __launch_bounds__(64) void k_lcb_rows(const uint16_t* __restrict__ labels, const int32_t* __restrict__ n,
                                                const double* __restrict__ w, const double* __restrict__ s2,
                                                const int32_t* __restrict__ vn, const uint8_t* __restrict__ n_edges, int rows,
                                                double z, double ratio, double* __restrict__ out_lcb,
                                                int32_t* __restrict__ out_pick)
{
    const int r = blockIdx.x;
    if (r >= rows) return;
    const int lane = lane_id();
    LcbEdges E{};
    E.nm = n_edges[r] > MAXMOVES ? MAXMOVES : n_edges[r];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const size_t i = (size_t)r * MAXMOVES + lane + 64 * h;
        if (lane + 64 * h >= E.nm) continue;
        E.lab[h] = labels[i]; E.n[h] = n[i]; E.w[h] = w[i]; E.s2[h] = s2[i]; E.vn[h] = vn[i];
    }
    double bound[2];
    const int j = lcb_pick(E, z, ratio, bound);
    if (out_lcb) {
#pragma unroll
        for (int h = 0; h < 2; ++h) out_lcb[(size_t)r * MAXMOVES + lane + 64 * h] = bound[h];
    }
    if (out_pick && lane == 0) out_pick[r] = j;
}

// cz_search_stop: no further simulations are STARTED; the ones in flight are backed up by the next round
__global__ void k_stop(SearchParams P, SearchBuffers B)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < P.G && B.g_phase[g] == PH_SEARCH) B.g_tasks_left[g] = 0;
}

// test hook: `n` draws of the root noise exactly as k_noise produces them (same generator, same stream addressing: one
// counter sequence per (epoch, sim, move) triple)
__global__ void k_debug_noise(uint64_t seed, uint32_t game_key, float alpha, int nm, double* __restrict__ out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t epoch = (uint32_t)(i / (8 * 128)), sim = (uint32_t)(i / 128) % 8u, j = (uint32_t)i % 128u;
    NoiseRng rng = NoiseRng::make(seed, game_key, epoch, sim, j);
    out[i] = dirichlet0(alpha, nm, rng);
}

__global__ void k_debug_sqrt(const int32_t* __restrict__ x, double* __restrict__ y, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = __dsqrt_rn((double)(x[i] + 1));
}

}  // namespace
