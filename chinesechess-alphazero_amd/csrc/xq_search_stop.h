// xq_search_stop.h -- part of xq_search.hip's translation unit; do not compile it into a second one.  Why: the same text as a
// unit of its own gave all eight k_sim* kernels 0.4-1.7 % more or fewer instructions (k_sim<false,false> 18 740 against
// 18 608, equal registers and scratch, nothing called out of line; cause not found).  The benchmark measures those kernels, so
// text only moves between these headers, and the proof of a move is the unit's device assembly, kernel by kernel
// (EXPERIMENTS.md, "the search unit's text in headers").
//
// Early stop of a settled ply (include/czero.h, cz_search_set_kld_gain and cz_search_set_smart_pruning): stop_reset,
// ply_settled.  Only the STOP instantiations (k_sim_stop, k_advance_stop) and k_stop_reset read a StopState.
#pragma once
#include "xq_search_tree.h"
#include "xq_search_ply.h"
#include "xq_search_records.h"

namespace {

constexpr int STOP_NONE = 0, STOP_KLD = 1, STOP_LEAD = 2;

// A ply's search begins (begin_search in self-play, cz_search_set_roots in external mode): the snapshot is empty, nothing is
// measured, no rule has ended the ply.  prev_n needs no reset: it is read only while prev_sum >= 0.
XQ_D void stop_reset(const StopState& S, int g)
{
    if (lane_id() == 0) {
        S.prev_sum[g] = -1;
        S.start_tasks[g] = -1;
        S.last_gain[g] = __builtin_nan("");
        S.checks[g] = 0;
        S.cut[g] = (uint8_t)STOP_NONE;
    }
}

// Has the ply of game g settled?  Called by sim_body<..., STOP> where a new lock-step batch would start: nothing is in
// flight, the deferred values are flushed, tasks = g_tasks_left > 0.  Returns the rule that ends the ply (STOP_KLD,
// STOP_LEAD) or STOP_NONE; the caller zeroes g_tasks_left and counts.  All 64 lanes call it, the result is wave-uniform; one
// lane holds edges lane and lane + 64 (load_root_edges).
// Out of line: it runs once per batch, and inlined it adds its float64 registers to those of the simulation (scratch of
// k_sim_stop<false> 376 bytes against 44 of k_sim<false, false>).  Its arguments are the words it reads, not the kernel's
// argument structures: a reference to those would put them on the stack.
__device__ __noinline__ int ply_settled_core(char* pool, const uint32_t* chtab, int g, int tasks, int32_t* g_root,
                                             uint8_t* g_n_no_act, uint16_t* g_no_act, int32_t* g_turns,
                                             uint8_t* g_increase_temp, double tau_decay_rate, int evaluate, StopState S)
{
    GameView gv{};
    gv.pool = pool;
    gv.chtab = chtab;
    gv.g = g;
    SearchBuffers B{};
    B.g_root = g_root;
    B.g_n_no_act = g_n_no_act;
    B.g_no_act = g_no_act;
    B.g_turns = g_turns;
    B.g_increase_temp = g_increase_temp;
    SearchParams P{};
    P.tau_decay_rate = tau_decay_rate;
    P.evaluate = evaluate;
    const int lane = lane_id();
    const int root = uni(B.g_root[g]);
    bool loaded = false;
    RootEdges E{};
    if (S.gain > 0.0) {
        int start = uni(S.start_tasks[g]);
        if (start < 0) {                                            // the ply's first test point: nothing has finished yet
            start = tasks;
            if (lane == 0) S.start_tasks[g] = tasks;
        }
        const int M = uni(S.prev_sum[g]);
        // the integer check.  Every visit of a root edge is a selection through the root, each of which adds 1 to the root's
        // sum_n (1 when the root was made), so N <= sum_n - 1: while sum_n - 1 < M + I no checkpoint is due
        bool due;
        if (M < 0) due = start - tasks >= S.interval;
        else due = root > 0 && uni(*reinterpret_cast<const int32_t*>(rec_ptr(gv, (uint32_t)root) + NODE_OFF_HDR)) - 1 >= M + S.interval;
        if (due) {
            E = load_root_edges(B, gv);
            loaded = true;
            const int N = __builtin_amdgcn_readlane(wave_incl_scan(E.n[0] + E.n[1]), 63);
            if (M < 0 || N >= M + S.interval) {                     // a checkpoint
                int32_t* prev = S.prev_n + (size_t)g * MAXMOVES;
                bool stop = false;
                if (M >= 0) {
                    const double Md = (double)M, Nd = (double)N;
                    double d = 0.0;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int j = lane + 64 * h;
                        const int m = j < E.nm ? prev[j] : 0;
                        if (m <= 0) continue;
                        const double t = (double)m / Md;
                        d = __dadd_rn(d, __dmul_rn(t, log(t / ((double)E.n[h] / Nd))));     // n_j >= m_j > 0
                    }
                    const double gain = wave_add_f64(d) / (double)(N - M);
                    if (lane == 0) S.last_gain[g] = gain;
                    stop = gain < S.gain;
                }
                if (lane == 0) S.checks[g] += 1;
                if (stop) return STOP_KLD;
                prev[lane] = E.n[0];                                // (edges at or beyond nm hold 0)
                prev[lane + 64] = E.n[1];
                if (lane == 0) S.prev_sum[g] = N;
            }
        }
    }
    if (S.lead && ply_tau(P, uni(B.g_turns[g]), uni((int)B.g_increase_temp[g])) == 0.0) {
        if (!loaded) E = load_root_edges(B, gv);
        // a, b: the largest and the second-largest count over the non-banned edges (0 where there is no such edge)
        int v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) v[h] = (lane + 64 * h < E.nm && !(E.lab[h] & VISIT_BANNED)) ? E.n[h] : 0;
        const int a = (int)wave_max_f64((double)(v[0] > v[1] ? v[0] : v[1]));
        const uint64_t h0 = __ballot(v[0] == a), h1 = __ballot(v[1] == a);
        if (h0) { if (lane == __ffsll((long long)h0) - 1) v[0] = 0; }              // one holder of a leaves the field
        else if (lane == __ffsll((long long)h1) - 1) v[1] = 0;
        const int b = (int)wave_max_f64((double)(v[0] > v[1] ? v[0] : v[1]));
        if (a - b > tasks) return STOP_LEAD;
    }
    return STOP_NONE;
}

XQ_D int ply_settled(const SearchParams& P, const SearchBuffers& B, const GameView& gv, const StopState& S, int tasks)
{
    return uni(ply_settled_core(gv.pool, gv.chtab, gv.g, tasks, B.g_root, B.g_n_no_act, B.g_no_act, B.g_turns,
                                B.g_increase_temp, P.tau_decay_rate, P.evaluate, S));
}

}  // namespace
