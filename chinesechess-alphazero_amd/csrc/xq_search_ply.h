// xq_search_ply.h -- part of xq_search.hip's translation unit; do not compile it into a second one.  Why: the same text as a
// unit of its own gave all eight k_sim* kernels 0.4-1.7 % more or fewer instructions (k_sim<false,false> 18 740 against
// 18 608, equal registers and scratch, nothing called out of line; cause not found).  The benchmark measures those kernels, so
// text only moves between these headers, and the proof of a move is the unit's device assembly, kernel by kernel
// (EXPERIMENTS.md, "the search unit's text in headers").
//
// Between the searches of a game: the chunk pool (pool_commit, pool_take), clear_tree, reserve_ply, ply_is_fast, begin_search,
// choose_action, the start positions (set_init_board, the book), open_game, new_game, new_script_game, script_move, emit_record.
#pragma once
#include "xq_search_tree.h"
#include "xq_search_solver.h"
#include "xq_search_var.h"
#include "xq_search_records.h"

namespace {

// ---- the chunk pool ---------------------------------------------------------------------------------------------
// Free chunks sit in a ring: entries [head, tail) are free.  Games take chunks (begin_search) and give them back
// (clear_tree) inside the same kernels, so takers only go up to `tail_vis`, the tail as of an earlier kernel boundary
// (committed by pool_commit): a ring entry is never read in the launch that wrote it.
XQ_D void pool_commit(const SearchBuffers& B)
{
    *B.pool_tail_vis = __hip_atomic_load(B.pool_tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one chunk for this game, or -1 when the pool is empty (wave-uniform result)
XQ_D int pool_take(const SearchParams& P, const SearchBuffers& B)
{
    int id = -1;
    if (lane_id() == 0) {
        unsigned int old = __hip_atomic_load(B.pool_head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned int vis = *B.pool_tail_vis;
        while ((int)(vis - old) > 0) {
            const unsigned int seen = atomicCAS(B.pool_head, old, old + 1u);
            if (seen == old) { id = (int)B.pool_ring[old % (unsigned int)P.n_chunks]; break; }
            old = seen;
        }
    }
    return uni(id);
}

// Drop the game's tree (new game, reset): empty hash table, bump pointer back to the start, every chunk beyond the
// first `keep_chunks` back to the pool.
XQ_D void clear_tree(const SearchParams& P, const SearchBuffers& B, const GameView& gv, uint32_t* chtab)
{
    const int lane = lane_id();
    const int g = gv.g;
    {
        uint4* h4 = reinterpret_cast<uint4*>(gv.hash);                // hash_cap is a power of two >= 64
        for (int i = lane; i < P.hash_cap / 2; i += 64) h4[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    const int nch = uni(B.g_nchunks[g]);
    for (int i = P.keep_chunks + lane; i < nch; i += 64) {
        const unsigned int slot = atomicAdd(B.pool_tail, 1u);
        B.pool_ring[slot % (unsigned int)P.n_chunks] = chtab[i];
    }
    if (lane == 0) {
        B.g_nchunks[g] = nch < P.keep_chunks ? nch : P.keep_chunks;
        B.g_heap_top[g] = 1u;                                         // id 0 = "none"
        B.g_node_count[g] = 0;
        B.g_root[g] = -1;
    }
    wave_sync_global();
}

// Make sure the game owns room for `tasks` more simulations (each may add one node record and one statistics block of
// RESERVE_MOVES moves): takes chunks from the pool.  false = the pool, the game's chunk table or its hash table is
// exhausted.  ML: the moves-left utility is on, a statistics block carries one M record per edge (k_reserve_ml).
template <bool ML = false>
XQ_D bool reserve_ply(const SearchParams& P, const SearchBuffers& B, const GameView& gv, uint32_t* chtab, int tasks)
{
    const int g = gv.g;
    const uint32_t top = uniu(B.g_heap_top[g]);
    int nch = uni(B.g_nchunks[g]);
    const int ncount = uni(B.g_node_count[g]);
    if ((long long)ncount + tasks + 1 > (long long)P.hash_cap * 7 / 8) return false;      // open addressing: keep it sparse
    constexpr int PER_TASK = NODE_HDR_GRANULES + (6 * RESERVE_MOVES + 15) / 16 + (ML ? 2 : 1) * RESERVE_MOVES;
    constexpr int USABLE = CHUNK_GRANULES - (ML ? 2 : 1) * MAXMOVES;  // a record that does not fit moves to the next chunk
    const long long need = (long long)(tasks + 1) * PER_TASK;
    long long have = (long long)(nch - (int)(top >> CHUNK_SHIFT)) * USABLE - (long long)(top & (uint32_t)(CHUNK_GRANULES - 1));
    bool ok = true;
    while (have < need) {
        if (nch >= P.max_chunks) { ok = false; break; }
        const int id = pool_take(P, B);
        if (id < 0) { ok = false; break; }
        if (lane_id() == 0) {
            B.g_chunk_tab[(size_t)g * P.max_chunks + nch] = (uint32_t)id;
            chtab[nch] = (uint32_t)id;
        }
        nch += 1;
        have += USABLE;
        count(gv, CT_CHUNKS_TAKEN);
    }
    if (lane_id() == 0) B.g_nchunks[g] = nch;
    wave_sync();
    return ok;
}

// Playout cap randomization (cz_search_set_playout_cap): is ply `turns` of self-play game `game_id` a FAST search?  A pure
// function of (seed, game_id, turns), like book_index: begin_search, k_noise, k_sim, emit_visits and emit_record all ask
// it, no per-game state is kept.  Stream 2 of the game's generator (stream 0: the per-game lotteries, stream 1: the move
// choice); rates 0 and 1 decide without a draw.  External mode never has fast plies.
XQ_D bool ply_is_fast(const SearchParams& P, uint32_t game_id, int turns)
{
    if (P.fast_sims <= 0 || P.mode != MODE_SELFPLAY || P.full_rate >= 1.0) return false;
    if (!(P.full_rate > 0.0)) return true;
    return !(philox_uniform(P.seed, game_id, 2, (uint64_t)turns) < P.full_rate);
}

// Start the search of the position in g_board (CChessPlayer.action, player.py:145-164): find the
// root in the tree, apply the reuse rule, reserve the ply's memory.  In self-play the ply's budget is fast_sims on a
// fast ply of the playout cap (a reused root that already has more visits searches nothing: tasks = 0).
XQ_D void begin_search(const SearchParams& P, const SearchBuffers& B, const GameView& gv, SearchLDS& L)
{
    const int lane = lane_id();
    const int g = gv.g;
    const int8_t* gb = B.g_board + (size_t)g * BOARD_LDS;
    L.r.bd[1][lane] = gb[lane];
    if (lane < 32) L.r.bd[1][lane + 64] = (lane < 26) ? gb[lane + 64] : (int8_t)0;
    wave_sync_global();
    const uint64_t h = pack_key(L.r.bd[1], L.key);
    int slot;
    int root = hash_lookup(gv, P, L.key, h, &slot);
    int done_n = root >= 0 ? uni(*reinterpret_cast<const int32_t*>(rec_ptr(gv, (uint32_t)root) + NODE_OFF_HDR)) : 0;   // :153-155
    const int n_no_act = uni((int)B.g_n_no_act[g]), inc = uni((int)B.g_increase_temp[g]);
    const int sims = ply_is_fast(P, uniu(B.g_game_id[g]), uni(B.g_turns[g])) ? P.fast_sims : P.sims;
    if (n_no_act > 0 || inc || done_n == sims) done_n = 0;                        // :156-158
    int tasks = sims - done_n;
    if (tasks < 0) tasks = 0;
    // Memory policy: the reference keeps a game's tree for the whole game (self_play.py:84,98-100) and so does the
    // engine as long as the pool has chunks.  Only when the coming ply cannot be reserved is the game's tree dropped
    // (counted: tree_resets; the chunks it keeps hold one full search).
    if (tasks > 0 && !reserve_ply(P, B, gv, L.chtab, tasks)) {
        clear_tree(P, B, gv, L.chtab);
        count(gv, CT_TREE_RESETS);
        root = -1;
        tasks = sims;
        done_n = 0;
        (void)reserve_ply(P, B, gv, L.chtab, tasks);     // within keep_chunks by construction; else overflow_sims counts
    }
    count(gv, CT_ROOT_REUSED_SIMS, (unsigned long long)done_n);
    if (P.gumbel_m > 0) {
        // Gumbel root search: the ply's draws g_j = -log(-log u_j), u_j = stream 4 of the generator keyed like the root
        // noise, draw (turns << 32 | j); fixed for the whole ply.  started = 0, the budget is what this ply searches.
        const uint32_t key = uniu(B.g_game_id[g]) + (uint32_t)g * 2654435761u;
        const uint64_t hi = (uint64_t)uniu((uint32_t)B.g_turns[g]) << 32;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = lane + 64 * h;
            double u = philox_uniform(P.seed, key, 4, hi | (uint64_t)j);
            if (u == 0.0) u = 1.1102230246251565e-16;          // 2^-53
            B.g_gumbel[(size_t)g * MAXMOVES + j] = -log(-log(u));
            B.g_started[(size_t)g * MAXMOVES + j] = 0;
        }
        if (lane == 0) B.g_budget[g] = tasks;
    }
    if (lane == 0) {
        B.g_root[g] = root;
        B.g_tasks_left[g] = tasks;
        B.g_active[g] = 0;
        B.g_phase[g] = PH_SEARCH;
    }
    wave_sync_global();
}

// The temperature of the move choice at ply `turns` (player.py:453-461); inc: the ply's increase_temp.  Stated once:
// choose_action applies it, and the unreachable-lead stop (xq_search_stop.h) asks whether it will be 0.
XQ_D double ply_tau(const SearchParams& P, int turns, int inc)
{
    double tau = 0.0;
    if (turns < 30 && P.tau_decay_rate != 0.0) tau = pow(P.tau_decay_rate, (double)(turns + 1));
    if (tau < 0.1 || (turns >= 4 && P.evaluate)) tau = 0.0;
    if (inc && !P.evaluate) tau = 0.5;
    return tau;
}

// ---- calc_policy + apply_temperature + choice (player.py:375-406, 453-470, :195) ---------------------
// returns the chosen label, or -1 when the player resigns.  u is the uniform draw of np.random.choice.
// SOLVE (the MCTS solver is on, an instantiation of its own): at a WIN root with a non-banned winning edge the move is
// that edge (rule 1 of select_solve), whatever tau is; resignation is tested first.
// LCB (the lower-confidence-bound move choice is on, cz_search_set_lcb; an instantiation of its own): at tau = 0 the move is
// lcb_pick's on the root's fields; the resignation test and the sampling at tau > 0 are what they were.
template <bool SOLVE = false, bool LCB = false>
XQ_D int choose_action(const SearchParams& P, const SearchBuffers& B, const GameView& gv, SearchLDS& L, double u,
                       bool enable_resign, const LcbState& Z = LcbState{})
{
    const int lane = lane_id();
    const int g = gv.g;
    const int root = uni(B.g_root[g]);
    if (root < 0) return -2;
    char* base = rec_ptr(gv, (uint32_t)root);
    const NodeHdr hdr = load_hdr(base);
    const int nm = (int)(hdr.meta & 0xFF);
    if (nm == 0) return -1;             // no move at all (the reference player dead-locks here): give the game up
    const uint16_t* pm = node_mv(base, nm);
    const EdgeStat* sb = hdr.stat ? edge_ptr(gv, hdr.stat) : nullptr;   // none: the root was never selected from
    const int n_no_act = uni((int)B.g_n_no_act[g]);
    const uint16_t* no_act = B.g_no_act + (size_t)g * MAX_NO_ACT;
    const int turns = uni(B.g_turns[g]);
    // visit counts (banned -> 0), max q over the non-banned edges
    int cnt[2];
    double maxq = -100.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        cnt[h] = 0;
        if (j < nm) {
            EdgeStat es{0.0, 0, CHILD_UNKNOWN};
            if (sb) es = sb[j];
            const int n = es.n;
            const uint16_t mv = pm[j];
            bool banned = false;
            for (int k = 0; k < n_no_act; ++k) banned = banned || (no_act[k] == mv);
            if (!banned) {
                cnt[h] = n;
                const double q = n ? es.w / (double)n : 0.0;
                maxq = q > maxq ? q : maxq;
            }
        }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_xor(maxq, d, 64);
        maxq = o > maxq ? o : maxq;
    }
    maxq = unid(maxq);
    if (maxq < P.resign_threshold && enable_resign && turns > P.min_resign_turn) return -1;   // :397-398
    if constexpr (SOLVE) {
        int won = -1;
        if (solve_root_decided(B, gv, &won) && won >= 0) return uni((int)pm[won]);
    }
    if (P.gumbel_m > 0) return gumbel_choose(P, B, gv);         // a Gumbel ply: no temperature, u is not used
    // order the edges by label (the policy vector is indexed by label)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        if (j < nm) {
            const uint16_t mv = pm[j];
            int rank = 0;
            for (int k = 0; k < nm; ++k) rank += pm[k] < mv;
            L.slab[rank] = mv;
            L.sn[rank] = cnt[h];
        }
    }
    wave_sync_global();
    // temperature (player.py:453-461)
    const double tau = ply_tau(P, turns, uni((int)B.g_increase_temp[g]));
    int chosen = 0;
    if constexpr (LCB) {
        if (tau == 0.0) {
            // (nothing is in flight here, so vn = n on every edge; no eligible edge: the most visited one, as below)
            const LcbEdges E = load_lcb_root(B, gv);
            double bound[2];
            const int pick = lcb_pick(E, Z.z, Z.ratio, bound);
            if (pick >= 0) {
                const int pn = pick < 64 ? __builtin_amdgcn_readlane(E.n[0], pick) : __builtin_amdgcn_readlane(E.n[1], pick - 64);
                const int pl = pick < 64 ? __builtin_amdgcn_readlane((int)E.lab[0], pick)
                                         : __builtin_amdgcn_readlane((int)E.lab[1], pick - 64);
                if (pn > 0) chosen = pl & 0x7FFF;
            }
            return chosen;
        }
    }
    if (tau == 0.0) {
        if (lane == 0) {
            int best = -1, bestn = -1;                       // np.argmax: first maximum in label order
            for (int k = 0; k < nm; ++k) if (L.sn[k] > bestn) { bestn = L.sn[k]; best = k; }
            chosen = (best >= 0 && bestn > 0) ? (int)L.slab[best] : 0;
        }
        wave_sync_global();
        return uni(chosen);
    }
    // policy ** (1 / tau), renormalised, then np.random.choice = cdf.searchsorted(u, side='right').  Everything that is
    // independent per move (the pow() calls above all: ~1 us each when one lane runs them back to back) is done one move
    // per lane; the float64 sums keep the order of the NumPy loops and stay on lane 0.
    long long total_n = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) if (lane + 64 * h < nm) total_n += L.sn[lane + 64 * h];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) total_n += __shfl_xor(total_n, d, 64);     // integers: any order
    const double inv = 1.0 / tau;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k = lane + 64 * h;
        if (k < nm) {
            const double pk = (double)L.sn[k] / (double)total_n;             // policy /= np.sum(policy)
            L.dsc[k] = L.sn[k] > 0 ? pow(pk, inv) : 0.0;
        }
    }
    wave_sync_global();
    double s = 0.0;
    if (lane == 0) for (int k = 0; k < nm; ++k) s += L.dsc[k];
    s = unid(s);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k = lane + 64 * h;
        if (k < nm) L.dsc[k] = L.dsc[k] / s;
    }
    wave_sync_global();
    double total = 0.0;
    if (lane == 0) {
        double c = 0.0;
        for (int k = 0; k < nm; ++k) { total += L.dsc[k]; c += L.dsc[k]; L.cdf[k] = c; }
    }
    total = unid(total);
    wave_sync_global();
    bool hit[2], pos[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k = lane + 64 * h;
        hit[h] = k < nm && L.cdf[k] / total > u;
        pos[h] = k < nm && L.dsc[k] > 0.0;
    }
    int pick = lowest_bit(__ballot(hit[0]), __ballot(hit[1]));          // first k with cdf[k] / total > u
    if (pick < 0) {                                                      // u beyond the last step: the last possible move
        const uint64_t p0 = __ballot(pos[0]), p1 = __ballot(pos[1]);
        pick = p1 ? 127 - __clzll((long long)p1) : (p0 ? 63 - __clzll((long long)p0) : -1);
    }
    chosen = pick >= 0 ? (int)L.slab[pick] : 0;
    wave_sync_global();
    return uni(chosen);
}

XQ_D void store_key(uint32_t* dst, const uint32_t* key)
{
    const int lane = lane_id();
    if (lane < KEY_WORDS) dst[lane] = key[lane];
}

XQ_D void set_init_board(int8_t* gb)
{
    // rkemsmekr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9/RKEMSMEKR (static_env.py:9)
    const int lane = lane_id();
    const int8_t back[9] = {ROOK, KNIGHT, ELEPHANT, ADVISOR, KING, ADVISOR, ELEPHANT, KNIGHT, ROOK};
    for (int s = lane; s < BOARD_LDS; s += 64) {
        int p = 0;
        if (s < NSQ) {
            const int x = s % 9, y = s / 9;
            if (y == 0) p = back[x];
            else if (y == 9) p = -back[x];
            else if (y == 2 && (x == 1 || x == 7)) p = CANNON;
            else if (y == 7 && (x == 1 || x == 7)) p = -CANNON;
            else if (y == 3 && (x % 2 == 0)) p = PAWN;
            else if (y == 6 && (x % 2 == 0)) p = -PAWN;
        }
        gb[s] = (int8_t)p;
    }
}

// Start position of game `game_id` (cz_search_set_book): the index into the book, or -1 for INIT_STATE.  A pure function
// of (seed, game_id, book): new_game and emit_record both ask it, no per-game state is kept.  Stream 0 draws 0 and 1 are the
// resign and store lotteries; rates 0 and 1 decide without a draw.
XQ_D int book_index(const SearchParams& P, uint32_t game_id)
{
    if (P.book_n <= 0 || !(P.book_rate > 0.0)) return -1;
    if (P.book_rate < 1.0 && !(philox_uniform(P.seed, game_id, 0, 2) < P.book_rate)) return -1;
    return (int)(game_id % (uint32_t)P.book_n);
}

XQ_D void set_book_board(int8_t* gb, const int8_t* src)
{
    const int lane = lane_id();
    for (int s = lane; s < BOARD_LDS; s += 64) gb[s] = s < NSQ ? src[s] : (int8_t)0;
}

// the rest of a game's start, its position being in g_board (new_game, new_script_game)
XQ_D void open_game(const SearchParams& P, const SearchBuffers& B, const GameView& gv, SearchLDS& L, uint32_t game_id)
{
    const int lane = lane_id();
    const int g = gv.g;
    wave_sync_global();
    const int8_t* gb = B.g_board + (size_t)g * BOARD_LDS;
    L.r.bd[1][lane] = gb[lane];
    if (lane < 32) L.r.bd[1][lane + 64] = gb[lane + 64];
    wave_sync_global();
    const uint64_t h0 = pack_key(L.r.bd[1], L.key);
    store_key(B.g_hist_key + (size_t)g * (P.max_plies + 2) * KEY_WORDS, L.key);
    if (lane == 0) B.g_hist_hash[(size_t)g * (P.max_plies + 2)] = h0;
    if (lane == 0) {
        B.g_game_id[g] = game_id;
        B.g_turns[g] = 0;
        B.g_no_eat[g] = 0;
        B.g_n_no_act[g] = 0;
        B.g_increase_temp[g] = 0;
        // enable_resign = random() > enable_resign_rate (self_play.py:102-105): stream 0, draw 0
        B.g_enable_resign[g] = philox_uniform(P.seed, game_id, 0, 0) > P.enable_resign_rate ? 1 : 0;
    }
    wave_sync_global();
    begin_search(P, B, gv, L);
}

// (re)start a self-play game in slot g (SelfPlayWorker.start_game, self_play.py:95-116; with a book the position its
// INIT_STATE stands for: turns, no_eat_count, history and "red = the first mover" as from the opening position)
XQ_D void new_game(const SearchParams& P, const SearchBuffers& B, const GameView& gv, SearchLDS& L, uint32_t game_id)
{
    const int g = gv.g;
    clear_tree(P, B, gv, L.chtab);
    const int bi = book_index(P, game_id);
    if (bi < 0) set_init_board(B.g_board + (size_t)g * BOARD_LDS);
    else set_book_board(B.g_board + (size_t)g * BOARD_LDS, P.book + (size_t)bi * NSQ);
    open_game(P, B, gv, L, game_id);
}

// (re)start slot g on a script (cz_search_set_script): game `game_id` walks script `game_id` from its own start position, like
// a book game; a slot whose next game id has no script has nothing left to play and goes PH_IDLE.
XQ_D void new_script_game(const SearchParams& P, const SearchBuffers& B, const GameView& gv, SearchLDS& L,
                          const ScriptState& X, uint32_t game_id)
{
    const int g = gv.g;
    clear_tree(P, B, gv, L.chtab);
    if (game_id >= (uint32_t)X.n) {
        if (lane_id() == 0) {
            B.g_game_id[g] = game_id;
            B.g_tasks_left[g] = 0;
            B.g_active[g] = 0;
            B.g_phase[g] = PH_IDLE;
        }
        wave_sync_global();
        return;
    }
    set_book_board(B.g_board + (size_t)g * BOARD_LDS, X.boards + (size_t)game_id * NSQ);
    open_game(P, B, gv, L, game_id);
}

// What a scripted game plays at ply `turns` instead of choose_action's move: the script's label; SCRIPT_END when the script is
// exhausted; SCRIPT_BAD when the label is not among the root's edges -- the position's legal moves, banned ones included --
// or the search left no root to ask: such a move never reaches step_board.
constexpr int SCRIPT_END = -1, SCRIPT_BAD = -3;
// off, len: the script's place in X.labels.
XQ_D int script_move(const SearchBuffers& B, const GameView& gv, const ScriptState& X, int off, int len, int turns)
{
    const int lane = lane_id();
    if (turns >= len) return SCRIPT_END;
    const uint16_t mv = (uint16_t)uni((int)X.labels[off + turns]);
    const int root = uni(B.g_root[gv.g]);
    if (root < 0) return SCRIPT_BAD;
    char* base = rec_ptr(gv, (uint32_t)root);
    const int nm = (int)(load_hdr(base).meta & 0xFF);
    const uint16_t* pm = node_mv(base, nm);
    const bool hit = (lane < nm && pm[lane] == mv) || (lane + 64 < nm && pm[lane + 64] == mv);
    return __ballot(hit) ? (int)mv : SCRIPT_BAD;
}

// searched: the first `searched` moves came from searches (the rest is the appended king capture): those of fast plies
// carry MOVE_FAST in the record; g_hist_act itself stays clean, the repetition scan reads it.
XQ_D void emit_record(const SearchParams& P, const SearchBuffers& B, const GameView& gv, int turns, int searched, int value,
                      bool store, bool resigned, uint32_t extra_flags)
{
    const int lane = lane_id();
    const int g = gv.g;
    unsigned int pos = 0;
    if (lane == 0) pos = atomicAdd(B.ring_tail, 1u);
    pos = uniu(pos);
    uint8_t* rec = B.ring + (size_t)(pos % (unsigned)P.ring_cap) * P.record_stride;
    if (lane == 0) {
        GameRecord* hdr = reinterpret_cast<GameRecord*>(rec);
        hdr->game_id = B.g_game_id[g];
        hdr->turns = turns;
        hdr->value = value;
        hdr->flags = (store ? 1u : 0u) | (resigned ? 2u : 0u) | extra_flags
                     | ((uint32_t)(book_index(P, B.g_game_id[g]) + 1) << GAME_BOOK_SHIFT);
    }
    uint16_t* mv = reinterpret_cast<uint16_t*>(rec + sizeof(GameRecord));
    const uint16_t* acts = B.g_hist_act + (size_t)g * (P.max_plies + 2);
    for (int i = lane; i < turns && i < P.max_plies + 2; i += 64) mv[i] = acts[i];
    if (P.fast_sims > 0) {                    // playout cap: one wave-uniform lottery per searched ply (cold: once a game)
        wave_sync_global();
        const uint32_t game_id = uniu(B.g_game_id[g]);
        for (int i = 0; i < searched && i < P.max_plies + 2; ++i)
            if (ply_is_fast(P, game_id, i) && lane == 0) mv[i] = (uint16_t)(acts[i] | MOVE_FAST);
    }
    count(gv, CT_GAMES);
    count(gv, value > 0 ? CT_RED_WINS : (value < 0 ? CT_BLACK_WINS : CT_DRAWS));
    if (resigned) count(gv, CT_RESIGNS);
}

}  // namespace
