// xq_search_selfplay.h -- part of xq_search.hip's translation unit; do not compile it into a second one.  Why: the same text as a
// unit of its own gave all eight k_sim* kernels 0.4-1.7 % more or fewer instructions (k_sim<false,false> 18 740 against
// 18 608, equal registers and scratch, nothing called out of line; cause not found).  The benchmark measures those kernels, so
// text only moves between these headers, and the proof of a move is the unit's device assembly, kernel by kernel
// (EXPERIMENTS.md, "the search unit's text in headers").
//
// The self-play game loop's one ply after a search: advance_game.
#pragma once
#include "xq_search_tree.h"
#include "xq_search_ply.h"
#include "xq_search_records.h"

namespace {

// One ply of SelfPlayWorker.start_game after the search finished (self_play.py:124-212).
// STOP (k_advance_stop, a stop rule is on): the visit entry of a ply that a rule ended says so (VISIT_EARLY, from S.cut).
// SCRIPT (k_advance_script, cz_search_set_script): the game walks script X[game_id].  The search's own choice is not made (no
// resignation test, no temperature, no draw from stream 1): the move is the script's, tested against the root's edges
// (script_move), and everything after it is the loop's.  The game ends where the rules end it -- the script then has nothing
// left but, possibly, the rules' final_move -- or where the script ends; its value is X.z, it is stored without a lottery and
// flagged GAME_SCRIPTED.  Anything else is a mismatch: GAME_SCRIPT_MISMATCH, store = 0, the next script.
// LCB (k_advance_lcb, cz_search_set_lcb): choose_action's; Z its state.
template <bool FULL, bool SOLVE = false, bool STOP = false, bool SCRIPT = false, bool LCB = false>   // (emit_visits', choose_action's)
XQ_D void advance_game(const SearchParams& P, const SearchBuffers& B, const GameView& gv, SearchLDS& L,
                       const VisitRing& V, const StopState& S = StopState{}, const ScriptState& X = ScriptState{},
                       const LcbState& Z = LcbState{})
{
    const int lane = lane_id();
    const int g = gv.g;
    const uint32_t game_id = uniu(B.g_game_id[g]);
    int turns = uni(B.g_turns[g]);
    int8_t* gb = B.g_board + (size_t)g * BOARD_LDS;
    uint32_t* hkeys = B.g_hist_key + (size_t)g * (P.max_plies + 2) * KEY_WORDS;
    uint16_t* hacts = B.g_hist_act + (size_t)g * (P.max_plies + 2);
    int action;
    int script_off = 0, script_len = 0;                                // (a game id beyond the scripts: an empty script)
    if constexpr (SCRIPT) {
        if (game_id < (uint32_t)X.n) {
            script_off = uni(X.offsets[game_id]);
            script_len = uni(X.offsets[game_id + 1]) - script_off;
        }
        action = script_move(B, gv, X, script_off, script_len, turns);
    } else {
        const double u = philox_uniform(P.seed, game_id, 1, (uint64_t)turns);
        action = choose_action<SOLVE, LCB>(P, B, gv, L, u, uni((int)B.g_enable_resign[g]) != 0, Z);
    }
    if (V.ring) {
        const bool fast = ply_is_fast(P, game_id, turns);
        bool early = false;
        if constexpr (STOP) early = uni((int)S.cut[g]) != 0;
        emit_visits<FULL>(P, B, gv, V, turns, action < 0, fast, P.forced_k > 0.0 && !fast, P.gumbel_m > 0, early);
    }
    count(gv, CT_PLIES);
    bool game_over = false, resigned = false;
    int value = 0;
    int final_move = NOMOVE;
    if (action < 0) {                                                  // resign, :126-129 (SCRIPT: its end, or a bad move)
        value = -1; game_over = true; resigned = !SCRIPT;
    } else {
        // state, no_eat = senv.new_step(state, action)  (:133-141)
        L.r.bd[0][lane] = gb[lane];
        if (lane < 32) L.r.bd[0][lane + 64] = (lane < 26) ? gb[lane + 64] : (int8_t)0;
        wave_sync_global();
        const int ft = label_ft(action);
        const int f = ft >> 8, t = ft & 0xFF;
        const bool no_eat = L.r.bd[0][t] == 0;
        step_board(L.r.bd[0], f, t, L.r.bd[3]);                         // bd[3] = new state, kept below
        if (lane == 0) hacts[turns] = (uint16_t)action;
        turns += 1;
        int no_eat_count = uni(B.g_no_eat[g]);
        no_eat_count = no_eat ? no_eat_count + 1 : 0;
        const uint64_t h = pack_key(L.r.bd[3], L.key);
        uint64_t* hhash = B.g_hist_hash + (size_t)g * (P.max_plies + 2);
        if (turns < P.max_plies + 2) {
            store_key(hkeys + (size_t)turns * KEY_WORDS, L.key);
            if (lane == 0) hhash[turns] = h;
        }
        int n_no_act = 0, inc = 0;
        if (no_eat_count >= 120 || turns >= 2 * P.max_game_length) {    // :149-151
            game_over = true; value = 0;
        } else {
            const DoneResult d = wave_done<true>(L.r.bd[3], L.r.bd[1], L.r.ml[0], L.r.ml[1], L.r.plist, true);   // :153
            game_over = d.over != 0; value = d.v; final_move = d.final_move;
            if (!game_over && !wave_has_attack(L.r.bd[3])) { game_over = true; value = 0; }  // :154-158
            if (!game_over && !d.check) {                               // :161-175
                int free_move = 0;
                // earlier states equal to this one, in order (both parities: the reference compares strings)
                // (64 earlier plies per step: lane l compares the 64-bit hash of ply base + l, one ballot lists the
                //  candidates, which are then verified word by word; a ply-at-a-time scan was 200 dependent memory
                //  round trips per move late in a game)
                for (int base = 0; base < turns && !game_over; base += 64) {
                  const int cmp_ply = base + lane;
                  uint64_t cand = __ballot(cmp_ply < turns && hhash[cmp_ply] == h);
                  while (cand && !game_over) {
                    const int i = base + __ffsll((long long)cand) - 1;
                    cand &= cand - 1;
                    const bool differs = lane < KEY_WORDS && hkeys[(size_t)i * KEY_WORDS + lane] != L.key[lane];
                    if (__ballot(differs)) continue;                  // a hash collision
                    const int mv = uni((int)hacts[i]);
                    // the rule helpers need the position in bd[0]
                    L.r.bd[0][lane] = L.r.bd[3][lane];
                    if (lane < 32) L.r.bd[0][lane + 64] = L.r.bd[3][lane + 64];
                    wave_sync_global();
                    if (wave_will_check_or_catch(L.r, L.r.bd[0], mv) == 1) {
                        if (n_no_act < MAX_NO_ACT) {
                            if (lane == 0) B.g_no_act[(size_t)g * MAX_NO_ACT + n_no_act] = (uint16_t)mv;
                            n_no_act += 1;
                        } else {
                            count(gv, CT_NO_ACT_TRUNCATED);           // (the reference's list is unbounded, self_play.py:161-175)
                        }
                    } else if (!wave_be_catched(L.r.bd[0], label_ft(mv) >> 8, L.r.bd[1], L.r.ml[0], L.r.plist)) {
                        inc = 1;
                        free_move += 1;
                        if (free_move >= 3) { game_over = true; value = 0; }
                    }
                  }
                }
            }
        }
        // commit the new position
        gb[lane] = L.r.bd[3][lane];
        if (lane < 32) gb[lane + 64] = (lane < 26) ? L.r.bd[3][lane + 64] : (int8_t)0;
        if (lane == 0) {
            B.g_turns[g] = turns;
            B.g_no_eat[g] = no_eat_count;
            B.g_n_no_act[g] = (uint8_t)n_no_act;
            B.g_increase_temp[g] = (uint8_t)inc;
        }
        wave_sync_global();
    }
    if (!game_over) {
        begin_search(P, B, gv, L);
        return;
    }
    bool mismatch = false;
    if constexpr (SCRIPT) {
        // the rules ended the game: the script may hold nothing more, or exactly their final_move (appended only then)
        const int rest = script_len - turns;
        bool capture = false;
        if (rest == 1 && final_move != NOMOVE) capture = uni((int)X.labels[script_off + turns]) == final_move;
        mismatch = action == SCRIPT_BAD || (action >= 0 && rest != 0 && !capture);
        if (!capture) final_move = NOMOVE;
    }
    const int searched = turns;
    if (final_move != NOMOVE) {                                         // :177-184
        if (lane == 0 && turns < P.max_plies + 2) hacts[turns] = (uint16_t)final_move;
        turns += 1;
        value = -value;
    }
    if (turns % 2 == 1) value = -value;                                 // :190-191
    bool store = true;
    if constexpr (SCRIPT) store = !mismatch;
    else if (turns < 10) store = philox_uniform(P.seed, game_id, 0, 1) > 0.9;   // :194-200
    wave_sync_global();
    uint32_t extra = 0u;
    if (V.ring) {                                                       // the next game in this slot starts complete
        int lost = 0;
        if (lane == 0) { lost = V.g_lost[g]; V.g_lost[g] = 0; }
        extra = uni(lost) ? GAME_VISITS_LOST : 0u;
    }
    if constexpr (SCRIPT) {
        value = game_id < (uint32_t)X.n ? uni((int)X.z[game_id]) : 0;
        extra |= GAME_SCRIPTED | (mismatch ? GAME_SCRIPT_MISMATCH : 0u);
        if (mismatch && lane == 0) atomicAdd(X.mismatches, 1ull);
        emit_record(P, B, gv, turns, searched, value, store, resigned, extra);
        new_script_game(P, B, gv, L, X, game_id + P.game_id_stride);
    } else {
        emit_record(P, B, gv, turns, searched, value, store, resigned, extra);
        new_game(P, B, gv, L, game_id + P.game_id_stride);
    }
}

}  // namespace
