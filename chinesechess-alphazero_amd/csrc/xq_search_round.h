// xq_search_round.h -- part of xq_search.hip's translation unit; do not compile it into a second one.  Why: the same text as a
// unit of its own gave all eight k_sim* kernels 0.4-1.7 % more or fewer instructions (k_sim<false,false> 18 740 against
// 18 608, equal registers and scratch, nothing called out of line; cause not found).  The benchmark measures those kernels, so
// text only moves between these headers, and the proof of a move is the unit's device assembly, kernel by kernel
// (EXPERIMENTS.md, "the search unit's text in headers").
//
// The round's kernels: sim_body and its instantiations k_sim, k_sim_cached, k_sim_solve, k_sim_stop, k_sim_ml, k_sim_draw, k_sim_var;
// k_reserve_ml, k_cache_fill, k_advance, k_advance_lcb, k_advance_stop, k_advance_script, k_stop_reset, k_noise.
#pragma once
#include "xq_search_tree.h"
#include "xq_search_attach.h"
#include "xq_search_select.h"
#include "xq_search_ml.h"
#include "xq_search_draw.h"
#include "xq_search_var.h"
#include "xq_search_solver.h"
#include "xq_search_sim.h"
#include "xq_search_ply.h"
#include "xq_search_selfplay.h"
#include "xq_search_stop.h"
#include "xq_noise.h"
#include "xq_evalcache.h"

namespace {

// ---- the round kernels --------------------------------------------------------------------------------------
// One lock-step round = k_sim(BACKUP) -> k_advance -> k_sim(SELECT)   (+ k_noise before k_sim(SELECT) when the
// root noise is on).  Splitting the round keeps the hot simulation kernel free of the cold, register-hungry code
// (move sampling with pow(), game rules, chunk reservation, Gamma sampling).
constexpr int SIM_BACKUP = 1, SIM_SELECT = 2;

// HIST: 28 input planes (use_history); kept out of the common 14-plane instantiation.  GUM: the Gumbel root search
// (cz_search_set_gumbel) is on; likewise.
// CACHE: the evaluation cache (cz_search_set_eval_cache) is on; likewise, so that the kernels launched while it is off
// are the text they were.  The body of both kernels: k_sim below (CACHE false, C never read) and k_sim_cached.
// SOLVE: the MCTS solver (cz_search_set_solver) is on; likewise.  The body of k_sim_solve too.
// STOP: a stop rule (cz_search_set_kld_gain, cz_search_set_smart_pruning) is on; likewise.  The body of k_sim_stop too; S is
// read by that instantiation alone.
// ML: the moves-left utility (cz_search_set_moves_left) is on; likewise.  The body of k_sim_ml too; M is read by that
// instantiation alone.  Its attach turns the leaf's moves-left row into k (ml_quanta), keeps k in the node header and takes m up
// the path (backup_m); it runs leaf by leaf without the one-leaf-ahead prefetch.
// DRAW: the draw average (cz_search_set_draw) is on; likewise.  The body of k_sim_draw too; D is read by that instantiation
// alone.  Its attach turns the draw column of the leaf's win / draw / loss row into dq (draw_quanta), keeps dq in the node header
// and takes it up the path (backup_d), d then v; leaf by leaf without the prefetch, as ML's.
// VAR: the lower-confidence-bound move choice (cz_search_set_lcb) is on; likewise.  The body of k_sim_var too.  Its attach takes
// the leaf's squared value up the path (backup_v) before the value; leaf by leaf without the prefetch, as ML's.  The selection is
// the plain one and no state of the option is read here: z and the ratio matter to the move choice alone.
// SCHED: the schedule of c_puct (cz_search_set_cpuct_schedule) is on; likewise.  Every kernel below has the instantiation: the
// schedule is a plain parameter that runs beside each of the options above, and only the selection differs.
template <bool HIST, bool GUM, bool CACHE, bool SOLVE = false, bool STOP = false, bool ML = false, bool DRAW = false,
          bool VAR = false, bool SCHED = false>
XQ_D void sim_body(SearchLDS& L, const SearchParams& P, const SearchBuffers& B, const float* __restrict__ policy,
                   const float* __restrict__ value, void* planes, int mask, int compact,
                   int32_t* __restrict__ q_rows, int32_t* __restrict__ q_count, const EvalCache& C,
                   const StopState& S = StopState{}, const MovesLeftState& M = MovesLeftState{},
                   const DrawState& D = DrawState{})
{
    const int g = blockIdx.x;
    // first kernel of a round: chunks returned during the previous round become takeable (see pool_commit)
    if (g == 0 && (mask & SIM_BACKUP) && lane_id() == 0) {
        pool_commit(B);
        if (q_count) *q_count = 0;          // compact queue of this round: filled by the k_sim(SELECT) launch below
        // the round's fill (k_cache_fill, the launch before this one) is over: the next round claims with the next stamp
        if constexpr (CACHE) *C.stamp = *C.stamp + 1u;
    }
    if (g >= P.G) return;
    if (uni((int)B.g_phase[g]) != PH_SEARCH) return;
    const GameView gv = make_view(B, P, g, L.ctr, L.chtab);
    counters_begin(gv);
#ifdef CZ_SIM_PROFILE
    const long long prof_k0 = clock64();
#endif
    const RoundIO io{planes, P.planes_dtype, P.in_planes, B.leaf_masks, B.leaf_planes_off != 0, B.leaf_flags};
    int active = uni(B.g_active[g]);
    Arena ar{uniu(B.g_heap_top[g]), uni(B.g_nchunks[g]), uni(B.g_node_count[g])};
    // (no root noise on a fast ply of the playout cap: k_noise drew no rows for it)
    // and no forced playouts either: a fast ply has no noise to examine
    // (nor on a Gumbel ply, whose root rule replaces both)
    const bool noisy = P.noise_eps != 0.0 && !(GUM && P.gumbel_m > 0) && !ply_is_fast(P, uniu(B.g_game_id[g]), uni(B.g_turns[g]));
    const bool force = P.forced_k > 0.0 && !ply_is_fast(P, uniu(B.g_game_id[g]), uni(B.g_turns[g]));
    const RootCtx rc{false, uni((int)B.g_n_no_act[g]), B.g_no_act + (size_t)g * MAX_NO_ACT,
                     noisy ? B.noise + (size_t)g * P.K * MAXMOVES : nullptr, 0, force};
    // while the Gumbel root search is on every attach keeps the leaf's network value in the node header (store_net_value)
    const bool keep_v = GUM && P.gumbel_m > 0;
    int resume_i = P.K;
    // the slot table as it is when the launch starts, slot i on lane i: one load per array instead of one dependent
    // round trip per slot and field (a simulation only ever changes its own slot, and each slot is visited once per list)
    const bool snap = (mask & SIM_BACKUP) && active > 0 && P.K <= 64;
    int sn_state = SIM_IDLE, sn_node = 0, sn_depth = 0;
    if (snap && lane_id() < P.K) {
        sn_state = gv.s_state[lane_id()];
        sn_node = gv.s_node[lane_id()];
        sn_depth = gv.s_depth[lane_id()];
    }
    if (snap) {
        // 1. attach + backup evaluated leaves, in simulation order (update_tree, player.py:340-373)
        const int lane = lane_id();
        int my_row = g * P.K + lane;
        uint32_t my_meta = 0u;
        float my_v = 0.0f;
        if (sn_state == SIM_LEAF) {
            if (compact) {                                            // the previous round built a compact queue: the row
                const int row = B.s_qrow[(size_t)g * P.K + lane];     // it gave this leaf
                if (row >= 0) my_row = row;
            }
            my_meta = *reinterpret_cast<const uint32_t*>(rec_ptr(gv, (uint32_t)sn_node) + NODE_OFF_HDR + 4);
            my_v = value[my_row];
        }
        int my_k = 0;                                                 // (ML) the leaf's moves-left prediction in quanta
        if constexpr (ML) {
            if (sn_state == SIM_LEAF) my_k = ml_quanta(M.x[my_row]);
        }
        if constexpr (DRAW) {                                         // (DRAW) my_k: the leaf's draw probability in quanta
            if (sn_state == SIM_LEAF) my_k = draw_quanta(D.wdl[3 * (size_t)my_row + 1]);
        }
        // the leaves the cache answered (SIM_CACHED) join the walk below at their place in simulation order: their value
        // waits in s_cval, no policy row is read and nothing is prefetched for them
        uint64_t cached = 0ull;
        if constexpr (CACHE) {
            if (sn_state == SIM_CACHED) my_v = C.s_cval[(size_t)g * P.K + lane];
            cached = __ballot(sn_state == SIM_CACHED);
        }
        PROF_BEGIN();
        // the evaluated leaves of this game, in simulation order, as a bit set; leaf_at(i) = its wave-uniform fields
        const uint64_t leaves = (__ballot(sn_state == SIM_LEAF) | cached) & (P.K < 64 ? (1ull << P.K) - 1ull : ~0ull);
        auto pre_a = [&](LeafPre& lp, int i) {
            const int depth = __builtin_amdgcn_readlane(sn_depth, i);
            if (depth <= 64 && !((cached >> i) & 1ull))
                leaf_pre_a(gv, lp, __builtin_amdgcn_readlane(sn_node, i), (uint32_t)__builtin_amdgcn_readlane((int)my_meta, i),
                           depth, gv.path_edge + (size_t)i * P.max_depth);
        };
        auto pre_b = [&](LeafPre& lp, int i) {
            if (__builtin_amdgcn_readlane(sn_depth, i) <= 64 && !((cached >> i) & 1ull))
                leaf_pre_b(lp, (uint32_t)__builtin_amdgcn_readlane((int)my_meta, i),
                           policy + (size_t)__builtin_amdgcn_readlane(my_row, i) * NLABELS);
        };
        LeafPre lp{0, 0, 0, 0.0f, 0.0f};
        uint64_t rest = leaves;
        if (!ML && !DRAW && !VAR && rest) {
            const int i0 = __ffsll((long long)rest) - 1;
            pre_a(lp, i0);
            pre_b(lp, i0);
        }
        while (rest) {
            const int i = __ffsll((long long)rest) - 1;
            rest &= rest - 1;
            const int i_next = rest ? __ffsll((long long)rest) - 1 : -1;
            const int node = __builtin_amdgcn_readlane(sn_node, i);
            const int depth = __builtin_amdgcn_readlane(sn_depth, i);
            const size_t slot = (size_t)__builtin_amdgcn_readlane(my_row, i);
            const double v = (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_v), i));   // float(v) of a float32
            LeafPre nx{0, 0, 0, 0.0f, 0.0f};
            if constexpr (ML) {
                const int k = __builtin_amdgcn_readlane(my_k, i);
                attach_policy(gv, L, node, policy + slot * NLABELS, P.policy_logits != 0, P.inv_temp, false, 0.0f);
                if (lane_id() == 0) store_ml_k(rec_ptr(gv, (uint32_t)node), k);
                load_path(P, gv, L, i, depth);
                backup_m(gv, L, depth, k);
                backup(P, gv, L, depth, v);
            } else if constexpr (DRAW) {
                const int dq = __builtin_amdgcn_readlane(my_k, i);
                attach_policy(gv, L, node, policy + slot * NLABELS, P.policy_logits != 0, P.inv_temp, false, 0.0f);
                if (lane_id() == 0) store_ml_k(rec_ptr(gv, (uint32_t)node), dq);      // (word 3, as the moves-left k)
                load_path(P, gv, L, i, depth);
                backup_d(gv, L, depth, dq);
                backup(P, gv, L, depth, v);
            } else if constexpr (VAR) {
                attach_policy(gv, L, node, policy + slot * NLABELS, P.policy_logits != 0, P.inv_temp, false, 0.0f);
                load_path(P, gv, L, i, depth);
                backup_v(gv, L, depth, v);
                backup(P, gv, L, depth, v);
            } else if (CACHE && ((cached >> i) & 1ull)) {
                cached_attach(gv, node, keep_v, (float)v);
                load_path(P, gv, L, i, depth);
                backup(P, gv, L, depth, v);
                if (i_next >= 0) { pre_a(nx, i_next); pre_b(nx, i_next); }
            } else if (depth <= 64) {
                attach_and_backup(P, gv, L, node, (uint32_t)__builtin_amdgcn_readlane((int)my_meta, i), depth, lp, v,
                                  P.policy_logits != 0, P.inv_temp, keep_v, [&]() {
                                      if (i_next >= 0) { pre_a(nx, i_next); pre_b(nx, i_next); }
                                  });
            } else {
                attach_policy(gv, L, node, policy + slot * NLABELS, P.policy_logits != 0, P.inv_temp, keep_v, (float)v);
                load_path(P, gv, L, i, depth);
                backup(P, gv, L, depth, v);
                if (i_next >= 0) { pre_a(nx, i_next); pre_b(nx, i_next); }
            }
            lp = nx;
            sim_finish(gv, i, &active);
        }
        PROF(CT_CYC_ATTACH);
        resume_i = 0;                                                 // 2. then resume the parked simulations
    } else if ((mask & SIM_BACKUP) && active > 0) {                   // (more than 64 slots per game: slot by slot)
        for (int i = 0; i < P.K; ++i) {
            const int st = uni((int)gv.s_state[i]);
            if (st != SIM_LEAF && !(CACHE && st == SIM_CACHED)) continue;
            const int node = uni(gv.s_node[i]);
            const int depth = uni(gv.s_depth[i]);
            size_t slot = (size_t)g * P.K + i;
            if constexpr (CACHE) {
                if (st == SIM_CACHED) {                               // answered by the cache: the value waits in s_cval
                    const float cv = __int_as_float(uni(__float_as_int(C.s_cval[slot])));
                    cached_attach(gv, node, keep_v, cv);
                    load_path(P, gv, L, i, depth);
                    backup(P, gv, L, depth, (double)cv);
                    sim_finish(gv, i, &active);
                    continue;
                }
            }
            if (compact) {
                const int row = uni(B.s_qrow[slot]);
                if (row >= 0) slot = (size_t)row;
            }
            attach_policy(gv, L, node, policy + slot * NLABELS, P.policy_logits != 0, P.inv_temp, keep_v, value[slot]);
            load_path(P, gv, L, i, depth);
            if constexpr (ML) {
                const int k = uni(ml_quanta(M.x[slot]));
                if (lane_id() == 0) store_ml_k(rec_ptr(gv, (uint32_t)node), k);
                backup_m(gv, L, depth, k);
            }
            if constexpr (DRAW) {
                const int dq = uni(draw_quanta(D.wdl[3 * slot + 1]));
                if (lane_id() == 0) store_ml_k(rec_ptr(gv, (uint32_t)node), dq);
                backup_d(gv, L, depth, dq);
            }
            if constexpr (VAR) backup_v(gv, L, depth, (double)value[slot]);
            backup(P, gv, L, depth, (double)value[slot]);             // float(v) of a float32
            sim_finish(gv, i, &active);
        }
        resume_i = 0;
    }
    int new_i = 0, new_n = 0, batches = 0;
    Deferred df{0ull, 0};
    for (int guard = 0; guard < (1 << 20); ++guard) {
        int sim, node, depth;
        bool fresh;
        if (resume_i < P.K) {                                         // parked simulations, in index order
            const int i = resume_i++;
            if (snap) {
                if (__builtin_amdgcn_readlane(sn_state, i) != SIM_PARKED) continue;
                node = __builtin_amdgcn_readlane(sn_node, i); depth = __builtin_amdgcn_readlane(sn_depth, i);
            } else {
                if (uni((int)gv.s_state[i]) != SIM_PARKED) continue;
                node = uni(gv.s_node[i]); depth = uni(gv.s_depth[i]);
            }
            sim = i; fresh = false;
            load_path(P, gv, L, i, depth);
        } else if (new_i < new_n) {                                   // the simulations of a fresh batch
            sim = new_i++; node = uni(B.g_root[g]); depth = 0; fresh = true;
        } else if (df.lo != 0 || df.hi != 0) {
            // the descents of this phase (resumed simulations / a fresh batch) are over: the terminal and repetition
            // values they produced are applied now, in index order
            flush_deferred<SOLVE, ML, DRAW, VAR>(P, gv, L, df, &active);
            continue;
        } else if ((mask & SIM_SELECT) && active == 0) {              // 3. next lock-step batch (player.py:169-178)
            const int tasks = uni(B.g_tasks_left[g]);
            if (tasks <= 0) break;                                    // search complete: k_advance takes over
            if constexpr (SOLVE) {
                // a decided root starts no further simulation this ply: tested before each batch, the first of a ply
                // included (a root proven in an earlier ply's search costs nothing); nothing is in flight here
                if (solve_root_decided(B, gv, nullptr)) {
                    if (lane_id() == 0) B.g_tasks_left[g] = 0;
                    count(gv, CT_DECIDED_PLIES);
                    break;
                }
            }
            if constexpr (STOP) {
                // a settled ply starts no further simulation either: the same test point, the rules of xq_search_stop.h
                const int why = ply_settled(P, B, gv, S, tasks);
                if (why != STOP_NONE) {
                    if (lane_id() == 0) { B.g_tasks_left[g] = 0; S.cut[g] = (uint8_t)why; }
                    count_direct(gv, why == STOP_KLD ? CT_KLD_PLIES : CT_LEAD_PLIES);
                    count_direct(gv, why == STOP_KLD ? CT_KLD_SIMS_CUT : CT_LEAD_SIMS_CUT, (unsigned long long)tasks);
                    break;
                }
            }
            // A batch whose simulations all end on terminal / repeated positions needs no evaluation and the next one
            // could start at once -- in a won endgame that chains hundreds of batches inside one launch and the whole
            // round waits for this wave.  The order of simulations does not depend on where the chain is cut.
            if (++batches > P.max_batches) break;
            new_n = tasks < P.K ? tasks : P.K;
            new_i = 0;
            active = new_n;
            if (lane_id() == 0) B.g_tasks_left[g] = tasks - new_n;
            continue;
        } else break;
        run_sim<HIST, GUM, CACHE, SOLVE, ML, DRAW, VAR, SCHED>(P, B, gv, L, io, rc, uni(B.g_root[g]), sim, node, depth, &active,
                                                               ar, fresh, df, C, (mask & SIM_SELECT) != 0, M, D);
    }
    if (lane_id() == 0) { B.g_active[g] = active; B.g_node_count[g] = ar.ncount; B.g_heap_top[g] = ar.top; }
    if ((mask & SIM_SELECT) && q_rows) {
        // Compact evaluation queue: this game's slots that hold a new leaf (also those a resumed simulation made in
        // the BACKUP launch) are appended to q_rows -- one atomic per game, the order of the games is arbitrary -- and
        // each remembers its row for the next round's attach (s_qrow).
        wave_sync_global();                                   // lane 0 wrote the slot states
        const int lane = lane_id();
        for (int base = 0; base < P.K; base += 64) {
            const int i = base + lane;
            const bool leaf = i < P.K && gv.s_state[i] == SIM_LEAF;
            const uint64_t m = __ballot(leaf);
            if (m == 0) continue;
            int at = 0;
            if (lane == 0) at = atomicAdd(q_count, __popcll(m));
            at = uni(at);
            if (leaf) {
                const int row = at + __popcll(m & ((1ull << lane) - 1ull));
                q_rows[row] = g * P.K + i;
                B.s_qrow[(size_t)g * P.K + i] = row;
            }
        }
    }
#ifdef CZ_SIM_PROFILE
    count(gv, (mask & SIM_SELECT) ? CT_CYC_KERNEL_SELECT : CT_CYC_KERNEL_BACKUP, (unsigned long long)(clock64() - prof_k0));
#endif
    counters_flush(gv);
}

template <bool HIST, bool GUM, bool SCHED = false>
__global__ __launch_bounds__(64, 4) void k_sim(SearchParams P, SearchBuffers B, const float* __restrict__ policy,
                                           const float* __restrict__ value, void* planes, int mask, int compact,
                                           int32_t* __restrict__ q_rows, int32_t* __restrict__ q_count)
{
    __shared__ SearchLDS L;
    sim_body<HIST, GUM, false, false, false, false, false, false, SCHED>(L, P, B, policy, value, planes, mask, compact, q_rows, q_count, EvalCache{});
}

// k_sim with the evaluation cache on (14 input planes only: cz_search_set_eval_cache refuses the history input)
template <bool GUM, bool SCHED = false>
__global__ __launch_bounds__(64, 4) void k_sim_cached(SearchParams P, SearchBuffers B, const float* __restrict__ policy,
                                                  const float* __restrict__ value, void* planes, int mask, int compact,
                                                  int32_t* __restrict__ q_rows, int32_t* __restrict__ q_count, EvalCache C)
{
    __shared__ SearchLDS L;
    sim_body<false, GUM, true, false, false, false, false, false, SCHED>(L, P, B, policy, value, planes, mask, compact, q_rows, q_count, C);
}

// k_sim with the MCTS solver on (cz_search_set_solver refuses the Gumbel search, forced playouts and the evaluation cache)
template <bool HIST, bool SCHED = false>
__global__ __launch_bounds__(64, 4) void k_sim_solve(SearchParams P, SearchBuffers B, const float* __restrict__ policy,
                                                 const float* __restrict__ value, void* planes, int mask, int compact,
                                                 int32_t* __restrict__ q_rows, int32_t* __restrict__ q_count)
{
    __shared__ SearchLDS L;
    sim_body<HIST, false, false, true, false, false, false, false, SCHED>(L, P, B, policy, value, planes, mask, compact, q_rows, q_count, EvalCache{});
}

// k_sim with a stop rule on (cz_search_set_kld_gain and cz_search_set_smart_pruning refuse the Gumbel search, the solver and the
// evaluation cache)
template <bool HIST, bool SCHED = false>
__global__ __launch_bounds__(64, 4) void k_sim_stop(SearchParams P, SearchBuffers B, const float* __restrict__ policy,
                                                const float* __restrict__ value, void* planes, int mask, int compact,
                                                int32_t* __restrict__ q_rows, int32_t* __restrict__ q_count, StopState S)
{
    __shared__ SearchLDS L;
    sim_body<HIST, false, false, false, true, false, false, false, SCHED>(L, P, B, policy, value, planes, mask, compact, q_rows, q_count, EvalCache{}, S);
}

// k_sim with the moves-left utility on (cz_search_set_moves_left refuses the Gumbel search, the solver, the stop rules, the
// evaluation cache and a script)
template <bool HIST, bool SCHED = false>
__global__ __launch_bounds__(64, 4) void k_sim_ml(SearchParams P, SearchBuffers B, const float* __restrict__ policy,
                                              const float* __restrict__ value, void* planes, int mask, int compact,
                                              int32_t* __restrict__ q_rows, int32_t* __restrict__ q_count, MovesLeftState M)
{
    __shared__ SearchLDS L;
    sim_body<HIST, false, false, false, false, true, false, false, SCHED>(L, P, B, policy, value, planes, mask, compact, q_rows, q_count, EvalCache{},
                                                     StopState{}, M);
}

// k_sim with the draw average on (cz_search_set_draw refuses the Gumbel search, the solver, the stop rules, the evaluation
// cache, a script and the moves-left utility)
template <bool HIST, bool SCHED = false>
__global__ __launch_bounds__(64, 4) void k_sim_draw(SearchParams P, SearchBuffers B, const float* __restrict__ policy,
                                                const float* __restrict__ value, void* planes, int mask, int compact,
                                                int32_t* __restrict__ q_rows, int32_t* __restrict__ q_count, DrawState D)
{
    __shared__ SearchLDS L;
    sim_body<HIST, false, false, false, false, false, true, false, SCHED>(L, P, B, policy, value, planes, mask, compact, q_rows, q_count,
                                                            EvalCache{}, StopState{}, MovesLeftState{}, D);
}

// k_sim with the lower-confidence-bound move choice on (cz_search_set_lcb refuses the Gumbel search, the solver, the stop rules,
// the evaluation cache, a script, the moves-left utility and the draw average)
template <bool HIST, bool SCHED = false>
__global__ __launch_bounds__(64, 4) void k_sim_var(SearchParams P, SearchBuffers B, const float* __restrict__ policy,
                                               const float* __restrict__ value, void* planes, int mask, int compact,
                                               int32_t* __restrict__ q_rows, int32_t* __restrict__ q_count)
{
    __shared__ SearchLDS L;
    sim_body<HIST, false, false, false, false, false, false, true, SCHED>(L, P, B, policy, value, planes, mask, compact, q_rows,
                                                                   q_count, EvalCache{});
}

// The moves-left utility's share of the per-ply reservation (the draw average's and the V records' too: its D records take the M records' place,
// and cz_search_round launches this kernel for either): a statistics block is twice the size while the option is on, so
// between k_advance (whose begin_search reserved the plain blocks) and k_sim(SELECT) every searching game tops its chunks up to
// what its outstanding simulations can use.  A game that cannot be served here has just begun its ply (a ply under way was
// served when it began and uses no more than that): its tree is dropped as begin_search would, the chunks it keeps hold one
// full search of the larger blocks (keep_chunks_for).
__global__ __launch_bounds__(64) void k_reserve_ml(SearchParams P, SearchBuffers B)
{
    __shared__ SearchLDS L;
    const int g = blockIdx.x;
    if (g >= P.G) return;
    if (uni((int)B.g_phase[g]) != PH_SEARCH) return;
    const int tasks = uni(B.g_tasks_left[g]) + uni(B.g_active[g]);
    if (tasks <= 0) return;
    const GameView gv = make_view(B, P, g, L.ctr, L.chtab);
    counters_begin(gv);
    if (!reserve_ply<true>(P, B, gv, L.chtab, tasks) && uni(B.g_active[g]) == 0) {
        clear_tree(P, B, gv, L.chtab);
        count(gv, CT_TREE_RESETS);
        const int sims = ply_is_fast(P, uniu(B.g_game_id[g]), uni(B.g_turns[g])) ? P.fast_sims : P.sims;
        if (lane_id() == 0) B.g_tasks_left[g] = sims;
        (void)reserve_ply<true>(P, B, gv, L.chtab, sims);
    }
    counters_flush(gv);
}

// The evaluation cache's only writer: the first launch of a round (before k_sim(BACKUP), which attaches the same rows),
// one wave per queue slot.  A slot that holds an evaluated leaf (SIM_LEAF) of a searching game forms the leaf's priors from
// its policy row with the attach's own functions (leaf_pre_b, prior_norm: the same bits by construction) and writes key,
// mirror bit, value, move count and priors into the position's entry, over whatever was there.  Two waves may want one entry
// in the same launch: one compare-and-swap on the entry's claim word with the round's stamp decides, the loser drops its
// store and counts nothing -- at most one writer per entry and round, nothing to reset, no wave waits for another.
__global__ __launch_bounds__(64) void k_cache_fill(SearchParams P, SearchBuffers B, EvalCache C,
                                                  const float* __restrict__ policy, const float* __restrict__ value,
                                                  int compact)
{
    const int slot = blockIdx.x;
    if (slot >= P.G * P.K) return;
    // stamp 0: the first round after the table was made or emptied -- its rows were evaluated before that (by the network
    // the caller replaced, cz_search_eval_cache_clear) and stay out; 0 is also the claim word of an entry never claimed
    const uint32_t stamp = uniu(*C.stamp);
    if (stamp == 0u) return;
    const int g = slot / P.K;
    if (uni((int)B.g_phase[g]) != PH_SEARCH) return;                  // (k_sim attaches nothing for such a game either)
    if (uni((int)B.s_state[slot]) != SIM_LEAF) return;
    const int lane = lane_id();
    int row = slot;
    if (compact) {
        const int r = uni(B.s_qrow[slot]);
        if (r >= 0) row = r;
    }
    const uint32_t node = uniu((uint32_t)B.s_node[slot]);
    const uint32_t chunk = uniu(B.g_chunk_tab[(size_t)g * P.max_chunks + (node >> CHUNK_SHIFT)]);
    char* base = rec_addr(B.pool, chunk, node);
    const uint32_t meta = load_hdr(base).meta;
    if (!(meta & NODE_WAITING)) return;
    const int nm = (int)(meta & 0xFF);
    const bool mir = (meta & NODE_MIRRORED) != 0u;
    const uint32_t* nk = reinterpret_cast<const uint32_t*>(base);
    const uint32_t kw = lane < KEY_WORDS ? nk[lane] : 0u;
    const uint64_t h = uni64(hash_of_key(nk));
    EvalCacheEntry* e = C.tab + ec_slot(h, mir, C.log2);
    int won = 0;
    if (lane == 0) {
        const uint32_t old = __hip_atomic_load(&e->claim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old != stamp) won = atomicCAS(&e->claim, old, stamp) == old ? 1 : 0;
    }
    if (!uni(won)) return;
    const uint16_t* pm = node_mv(base, nm);
    LeafPre lp{0, 0, 0, 0.0f, 0.0f};
    if (lane < nm) lp.m0 = pm[lane];
    if (lane + 64 < nm) lp.m1 = pm[lane + 64];
    leaf_pre_b(lp, meta, policy + (size_t)row * NLABELS);
    float p0 = lp.p0, p1 = lp.p1;
    const float all_p = prior_norm(p0, p1, nm, P.policy_logits != 0, P.inv_temp);
    if (lane < KEY_WORDS) e->key[lane] = kw;
    if (lane < nm) e->p[lane] = p0 / all_p;
    if (lane + 64 < nm) e->p[lane + 64] = p1 / all_p;
    if (lane == 0) {
        e->value = value[row];
        e->meta = ec_meta(nm, mir);
        C.s_stores[slot] += 1ull;                                     // (this slot's wave is the word's only writer)
    }
}

// End of a search: external mode marks the game READY; self-play mode plays the move, applies the game rules
// and sets up the next search (or the next game).
// FULL: the full Gumbel search is on (cz_search_set_gumbel_full): the visit entries hold its target.  An instantiation of
// its own, so that the kernel launched while it is off is the text it was.
// SOLVE: the MCTS solver is on (cz_search_set_solver): choose_action's; likewise.
// (k_advance_lcb below is this kernel with choose_action's LCB.)
template <bool FULL, bool SOLVE = false>
__global__ __launch_bounds__(64) void k_advance(SearchParams P, SearchBuffers B, VisitRing V)
{
    __shared__ SearchLDS L;
    const int g = blockIdx.x;
    if (g >= P.G) return;
    if (uni((int)B.g_phase[g]) != PH_SEARCH || uni(B.g_active[g]) != 0 || uni(B.g_tasks_left[g]) != 0) return;
    const GameView gv = make_view(B, P, g, L.ctr, L.chtab);
    counters_begin(gv);
    if (P.mode == MODE_SELFPLAY) {
        for (int it = 0; it < 8; ++it) {          // a search with nothing to do (fully reused root) ends at once
            advance_game<FULL, SOLVE>(P, B, gv, L, V);
            if (uni((int)B.g_phase[g]) != PH_SEARCH || uni(B.g_tasks_left[g]) != 0) break;
        }
    } else if (lane_id() == 0) {
        B.g_phase[g] = PH_READY;
    }
    counters_flush(gv);
}

// k_advance with the lower-confidence-bound move choice on (cz_search_set_lcb): a tau = 0 ply plays lcb_pick's move.  A kernel
// of its own, so that the ones launched while the option is off keep their names and their text.
__global__ __launch_bounds__(64) void k_advance_lcb(SearchParams P, SearchBuffers B, VisitRing V, LcbState Z)
{
    __shared__ SearchLDS L;
    const int g = blockIdx.x;
    if (g >= P.G) return;
    if (uni((int)B.g_phase[g]) != PH_SEARCH || uni(B.g_active[g]) != 0 || uni(B.g_tasks_left[g]) != 0) return;
    const GameView gv = make_view(B, P, g, L.ctr, L.chtab);
    counters_begin(gv);
    if (P.mode == MODE_SELFPLAY) {
        for (int it = 0; it < 8; ++it) {          // a search with nothing to do (fully reused root) ends at once
            advance_game<false, false, false, false, true>(P, B, gv, L, V, StopState{}, ScriptState{}, Z);
            if (uni((int)B.g_phase[g]) != PH_SEARCH || uni(B.g_tasks_left[g]) != 0) break;
        }
    } else if (lane_id() == 0) {
        B.g_phase[g] = PH_READY;
    }
    counters_flush(gv);
}

// k_advance with a stop rule on: the visit entry of a ply that a rule ended carries VISIT_EARLY, and every search that
// advance_game begins starts with an empty snapshot (stop_reset).  External mode's searches begin in cz_search_set_roots, which
// launches k_stop_reset.
__global__ __launch_bounds__(64) void k_advance_stop(SearchParams P, SearchBuffers B, VisitRing V, StopState S)
{
    __shared__ SearchLDS L;
    const int g = blockIdx.x;
    if (g >= P.G) return;
    if (uni((int)B.g_phase[g]) != PH_SEARCH || uni(B.g_active[g]) != 0 || uni(B.g_tasks_left[g]) != 0) return;
    const GameView gv = make_view(B, P, g, L.ctr, L.chtab);
    counters_begin(gv);
    if (P.mode == MODE_SELFPLAY) {
        for (int it = 0; it < 8; ++it) {          // a search with nothing to do (fully reused root) ends at once
            advance_game<false, false, true>(P, B, gv, L, V, S);
            stop_reset(S, g);
            if (uni((int)B.g_phase[g]) != PH_SEARCH || uni(B.g_tasks_left[g]) != 0) break;
        }
    } else if (lane_id() == 0) {
        B.g_phase[g] = PH_READY;
    }
    counters_flush(gv);
}

// k_advance with a script on (cz_search_set_script); launched in self-play mode only, external mode keeps k_advance.  A slot
// that has walked its last script is PH_IDLE and is left alone by every kernel of the round.
__global__ __launch_bounds__(64) void k_advance_script(SearchParams P, SearchBuffers B, VisitRing V, ScriptState X)
{
    __shared__ SearchLDS L;
    const int g = blockIdx.x;
    if (g >= P.G) return;
    if (uni((int)B.g_phase[g]) != PH_SEARCH || uni(B.g_active[g]) != 0 || uni(B.g_tasks_left[g]) != 0) return;
    const GameView gv = make_view(B, P, g, L.ctr, L.chtab);
    counters_begin(gv);
    for (int it = 0; it < 8; ++it) {              // a search with nothing to do (fully reused root) ends at once
        advance_game<false, false, false, true>(P, B, gv, L, V, StopState{}, X);
        if (uni((int)B.g_phase[g]) != PH_SEARCH || uni(B.g_tasks_left[g]) != 0) break;
    }
    counters_flush(gv);
}

// the searches of the games `select_mask` names (NULL: all) begin: cz_search_set_roots, cz_search_start_selfplay
__global__ void k_stop_reset(StopState S, int G, const uint8_t* __restrict__ select_mask)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G || (select_mask && !select_mask[g])) return;
    S.prev_sum[g] = -1;
    S.start_tasks[g] = -1;
    S.last_gain[g] = __builtin_nan("");
    S.checks[g] = 0;
    S.cut[g] = (uint8_t)STOP_NONE;
}

// Dirichlet(alpha 1_n)[0] for every (simulation slot, root edge) of the batch that the next k_sim(SELECT) launch starts:
// X / (X + Y), X ~ Gamma(alpha), Y ~ Gamma(alpha (n - 1)) (xq_noise.h).  The reference redraws it per move per root visit
// (player.py:304); a simulation selects at the root at most once, so one row per slot per batch is enough.
// ONE launch per round, before k_sim(SELECT), and only games that start a batch there draw anything.  The rare game
// whose root is not in the tree yet (first search of a game, a search after a reset) needs rows too: its simulation 0
// expands the root, the others park on it and select at the root when the NEXT round's k_sim(BACKUP) resumes them --
// with the rows drawn here, for the move count this kernel works out itself from the root position (round 2 ran a
// second k_noise launch before every k_sim(BACKUP) for that case: 19 us per round for 4096 waves that found nothing).
// (Drawing the rows inside k_sim, by the game's own wave when a batch starts, was measured and is SLOWER: the 6 x 64
// draws of a batch are dependent instruction chains for one wave; here they spread over 4 waves per game.)
__global__ __launch_bounds__(256) void k_noise(SearchParams P, SearchBuffers B)
{
    __shared__ int s_nm;
    const int g = blockIdx.x;
    if (g >= P.G || B.g_phase[g] != PH_SEARCH) return;
    if (ply_is_fast(P, B.g_game_id[g], B.g_turns[g])) return;   // playout cap: no root noise on a fast ply, the epoch stays
    if (P.gumbel_m > 0) return;                                 // nor on a Gumbel ply
    // a new batch starts only when nothing is in flight (k_sim(BACKUP) may just have finished the old one)
    if (B.g_active[g] != 0) return;
    const int tasks = B.g_tasks_left[g];
    const int last = tasks < P.K ? tasks : P.K;                 // slots [0, last)
    if (last <= 0) return;
    const int root = B.g_root[g];
    const int tid = threadIdx.x;
    int nm;
    if (root >= 0) {
        const char* rbase = rec_addr(B.pool, B.g_chunk_tab[(size_t)g * P.max_chunks + ((uint32_t)root >> CHUNK_SHIFT)],
                                     (uint32_t)root);
        nm = (int)(*reinterpret_cast<const uint32_t*>(rbase + NODE_OFF_HDR + 4) & 0xFF);
    } else {
        // the root position is in g_board: count its moves from wave_movegen's three ballot sets (gen_piece's counting
        // form, one or two squares per lane), without the lists.  Wave 0 only; the other waves wait at the barrier.
        if (tid < 64) {
            const int8_t* gb = B.g_board + (size_t)g * BOARD_LDS;
            const int p0 = gb[tid];
            const int p1 = tid < 26 ? gb[tid + 64] : 0;
            const Set90 occ{__ballot(p0 != 0), __ballot(p1 != 0)};
            const Set90 own{__ballot(p0 > 0), __ballot(p1 > 0)};
            const Set90 oking{__ballot(p0 == -KING), __ballot(p1 == -KING)};
            int c = 0;
            if (p0 > 0) c += gen_piece<false>(p0, tid, occ, own, oking, nullptr, nullptr, 0);
            if (p1 > 0) c += gen_piece<false>(p1, tid + 64, occ, own, oking, nullptr, nullptr, 0);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
            if (tid == 0) s_nm = c < MAXMOVES ? c : MAXMOVES;      // (expand_node caps the list the same way)
        }
        __syncthreads();
        nm = s_nm;
    }
    const uint32_t epoch = B.g_noise_epoch[g];
    double* rows = B.noise + (size_t)g * P.K * MAXMOVES;
    const float alpha = (float)P.dirichlet_alpha;
    const uint32_t key = B.g_game_id[g] + (uint32_t)g * 2654435761u;
    // one (simulation slot, root move) pair per thread and step: 8 x 44 pairs are two steps of the 256 threads
    for (int item = tid; item < last * nm; item += (int)blockDim.x) {
        const int sim = item / nm, j = item - sim * nm;
        NoiseRng rng = NoiseRng::make(P.seed, key, epoch, (uint32_t)sim, (uint32_t)j);
        rows[(size_t)sim * MAXMOVES + j] = dirichlet0(alpha, nm, rng);
    }
    __syncthreads();
    if (tid == 0) B.g_noise_epoch[g] = epoch + 1;
}

}  // namespace
