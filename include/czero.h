/*
 * include/czero.h -- C-ABI of the MI355X-native Xiangqi self-play engine (libczero.so).
 *
 * The reference (NeymarL/ChineseChess-AlphaZero) is 100 % Python and has no FFI; this is the
 * seam a maintainer binds directly under its Python modules (ctypes stub: INTEGRATION.md).
 * Each entry point names the reference interface it replaces (paths relative to the
 * reference's cchess_alphazero/ package).
 *
 * Conventions
 *   - plain pointers and sizes only; every buffer is CALLER-OWNED DEVICE memory (e.g. a torch
 *     tensor's data_ptr()) unless the parameter is documented as host memory;
 *   - `stream` is a hipStream_t (NULL = the default stream); calls enqueue work and return;
 *   - return 0 (CZ_OK) or a negative CZ_ERR_* code, never throw; cz_last_error() is thread-local;
 *   - square s = y*9 + x (x 0..8, y 0..9, y = 0 is the side-to-move's back rank, as in
 *     environment/static_env.py:117-135); board = int8[90], 0 empty, +t mover / -t opponent,
 *     t = 1 pawn 2 cannon 3 rook 4 knight 5 elephant 6 advisor 7 king (Fen_2_Idx order + 1,
 *     environment/lookup_tables.py:27-42);
 *   - move = uint16 index into ActionLabelsRed (environment/lookup_tables.py:62-134), 0..2085;
 *     0xFFFF = none.
 */
#ifndef CZERO_H
#define CZERO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CZ_VERSION 2

#define CZ_OK 0
#define CZ_ERR_ARG (-1)
#define CZ_ERR_HIP (-2)
#define CZ_ERR_STATE (-3)
#define CZ_ERR_NOMEM (-4)

#define CZ_NSQ 90
#define CZ_NLABELS 2086
#define CZ_MAXMOVES 128
#define CZ_NOMOVE 0xFFFF

/* element type of the network-input planes written by the engine */
#define CZ_F32 0
#define CZ_F16 1
#define CZ_BF16 2
#define CZ_U8 3
#define CZ_F16C8 4   /* fp16 operand + c8 correction image (cz_conv3x3_c8): the residual-block entry points only */
#define CZ_F16C6 5   /* fp16 operand + c6 correction image (bf6 pieces; cz_conv3x3_c6_pack_weights): cz_resblock(_heads),
                        cz_input_resblock with 128 filters only */
#define CZ_F16C86 6  /* cz_resblock, 192 filters: the first c6 block of a tower whose input layer wrote a c8 image (x = c8 pair; first
                      * filter cz_conv3x3_c8_pack_weights', second cz_conv3x3_c6_pack_weights'; y = a c6 pair) */

int cz_version(void);
const char* cz_last_error(void);
int cz_device_count(void);

/* HOST buffers. label_of[90*90] (from*90+to -> label, 0xFFFF none), lab_ft[2086] (from<<8|to).
 * Replaces create_action_labels / ActionLabelsRed, environment/lookup_tables.py:62-134. */
int cz_label_tables(uint16_t* label_of, uint16_t* lab_ft);
/* HOST buffer. out[2086]: the label of the left-right mirrored move, "x0y0x1y1" -> "(8-x0)y0(8-x1)y1".  The label set is
 * closed under it; the map is an involution with 90 fixed points (the moves inside the centre file).  The table the
 * flagged rows of cz_gather_planes_m / cz_policy_value_loss_m follow. */
int cz_label_mirror(uint16_t* out);

/* ---- batched rules: one wavefront per board ------------------------------------------- */

/* get_legal_moves, environment/static_env.py:256-321 (pseudo-legal, reference emission order).
 * moves[n][128] (0xFFFF padded), counts[n]. */
int cz_movegen(const int8_t* boards, int n, uint16_t* moves, uint8_t* counts, void* stream);

/* done, environment/static_env.py:14-77.  over/v/final_move per board; check only when need_check
 * (may be NULL otherwise).  v is from the side to move's view. */
int cz_done(const int8_t* boards, int n, int need_check, int8_t* over, int8_t* v, uint16_t* final_move,
            uint8_t* check, void* stream);

/* step / new_step, environment/static_env.py:79-98: out = board after the move, flipped to the next
 * mover.  no_eat[i] = 1 no capture, 0 capture, 0xFF = the reference would raise ValueError (empty
 * source square or bad label; out = input board).  no_eat may be NULL. */
int cz_step(const int8_t* boards, const uint16_t* moves, int n, int8_t* out, uint8_t* no_eat, void* stream);

/* state_to_planes, environment/static_env.py:137-156: planes[n][14][10][9] of `dtype` (CZ_F32...). */
int cz_encode(const int8_t* boards, int n, void* planes, int dtype, void* stream);

/* will_check_or_catch, environment/static_env.py:390-421.  out[i] = 0/1, 0xFF = ValueError. */
int cz_check_or_catch(const int8_t* boards, const uint16_t* moves, int n, uint8_t* out, void* stream);

/* be_catched, environment/static_env.py:456-469. */
int cz_be_catched(const int8_t* boards, const uint16_t* moves, int n, uint8_t* out, void* stream);

/* has_attack_chessman, environment/static_env.py:471-479. */
int cz_has_attack(const int8_t* boards, int n, uint8_t* out, void* stream);

/* move-gen + done(need_check=True) + planes in one pass (the SURVEY 8(d) micro-suite kernel). */
int cz_rules_fused(const int8_t* boards, int n, uint16_t* moves, uint8_t* counts, int8_t* over, int8_t* v,
                   uint16_t* final_move, uint8_t* check, void* planes, int dtype, void* stream);

/* ---- batched PUCT-MCTS + self-play game loop: one wavefront per game ---------------------------
 * Replaces agent/player.py::CChessPlayer (action :145-196, MCTS_search :198-260,
 * select_action_q_and_u :262-320, expand_and_evaluate :322-338, update_tree :340-373, calc_policy
 * :375-406, apply_temperature :453-470) and worker/self_play.py::SelfPlayWorker.start_game :95-212
 * for n_games concurrent games.  The network stays with the caller: each cz_search_round() consumes the
 * policy/value rows of the previous round and writes the input planes of the new leaves; the evaluation
 * queue has one fixed slot per (game, simulation): slot = game * sims_per_round + sim.
 */
typedef struct cz_search cz_search;

typedef struct cz_search_cfg {
    int32_t n_games;                 /* G: concurrent games = wavefronts */
    int32_t sims_per_round;          /* K: config.play.search_threads (lock-step batch per game) */
    int32_t simulation_num_per_move; /* config.play.simulation_num_per_move */
    int32_t virtual_loss;            /* config.play.virtual_loss */
    int32_t max_nodes_per_game;      /* sizes a game's hash table and chunk table; 0 = (2 * max_game_length + 4) * sims,
                                        i.e. the tree of the longest game is kept whole (self_play.py:84,98-100) */
    int32_t pool_chunks;             /* tree memory shared by all games, in chunks of 1 MiB; 0 = what the games can use,
                                        at most 80 % of the device memory that is free at creation */
    int32_t max_depth;               /* longest path of one simulation: one that reaches an evaluated node with this many
                                        edges behind it backs up 0 (counter depth_overflow); 0 = 128, at most 128 */
    int32_t max_game_length;         /* config.play.max_game_length (full moves) */
    int32_t planes_dtype;            /* CZ_F32 / CZ_F16 / CZ_BF16 / CZ_U8 */
    int32_t min_resign_turn;         /* config.play.min_resign_turn */
    int32_t evaluate;                /* config.opts.evaluate */
    int32_t ring_capacity;           /* finished-game records kept on the device; 0 = 2 * n_games + 64 */
    double c_puct, noise_eps, dirichlet_alpha, tau_decay_rate, resign_threshold, enable_resign_rate;
    uint64_t seed;                   /* counter-based RNG key (Philox4x32-10): u(seed, game_id, stream, index) */
    int32_t use_history;             /* 28 input planes (CChessPlayer(use_history=True), static_env.py:158-194) */
    int32_t reserved;
} cz_search_cfg;

/* finished-game record in the ring: this header, then uint16 moves[max_plies + 2] (labels, mover frame) */
typedef struct cz_game_record {
    uint32_t game_id;
    int32_t turns;                   /* number of moves recorded */
    int32_t value;                   /* +1 red won, -1 black won, 0 draw (self_play.py:190-191); "red" = the side that
                                        made the game's first move, also when the game started from a book position */
    uint32_t flags;                  /* bit 0: store (self_play.py:194-200), bit 1: ended by resignation,
                                        bit 2: (visit recording on) the game has no complete visit record,
                                        bits 8-31: the game's start position: book index + 1, 0 = INIT_STATE
                                        (cz_search_set_book; written by the kernel, the host never redraws the lottery) */
} cz_game_record;
#define CZ_GAME_BOOK_SHIFT 8
#define CZ_BOOK_MAX ((1 << 24) - 2)  /* positions a book may hold: every index + 1 fits bits 8-31 of flags */
#define CZ_MOVE_FAST 0x8000          /* the record's uint16 moves[i], bit 15: ply i was a FAST search of the playout cap
                                        (cz_search_set_playout_cap); labels are below 2086.  Searched plies only: never
                                        set on the appended king capture.  Mask it out before reading the label */

int cz_search_create(const cz_search_cfg* cfg, cz_search** out);   /* allocates device memory on the current device */
int cz_search_destroy(cz_search* s);
size_t cz_search_bytes(const cz_search* s);
/* out[16]: G, K, sims, pool chunks, chunk-table entries per game, hash_cap, max_depth, max_plies, record_stride,
 * ring_cap, n_counters, input planes (14 / 28), chunks a game always keeps, longest no_act list, 0, 0 */
int cz_search_info(const cz_search* s, int32_t* out);
/* HOST out[8]: pool chunks, free chunks, chunks owned by games, ... by the largest game, tree bytes in use, ... of the
 * largest game, nodes in all trees, ... in the largest tree; synchronises the stream.
 * Tree memory: a game's tree is kept for the whole game (the reference's behaviour) in 1 MiB chunks taken from a pool
 * shared by all games; only when a ply cannot be reserved (pool empty) is that game's tree dropped -- counter
 * tree_resets; simulations that still find no room end with value 0 -- counter overflow_sims. */
int cz_search_memory_info(cz_search* s, int64_t* host_out, void* stream);

/* self-play mode: every slot plays games from INIT_STATE forever; slot g starts with game id
 * first_game_id + g and continues with + game_id_stride after each finished game (0 = n_games). */
int cz_search_start_selfplay(cz_search* s, uint64_t seed, uint32_t first_game_id, uint32_t game_id_stride, void* stream);

/* Start-position book of self-play.  boards [n][90] int8 in the MOVER's frame (+t the side to move, at rows 0-4, as in
 * cz_search_set_roots; a position with black to move is handed over flipped, static_env.fliped_state), host or device
 * memory; they are copied into memory the search object owns (n * 90 bytes), n <= CZ_BOOK_MAX.  n = 0 clears the book.
 * Game `game_id` starts from boards[game_id % n] iff philox_uniform(seed, game_id, stream 0, draw 2) < rate, otherwise
 * from INIT_STATE (draws 0 and 1 of stream 0 stay the resign and store lotteries; rate 0 and rate 1 draw nothing).  A
 * book game is SelfPlayWorker.start_game with INIT_STATE replaced: turns = 0, no_eat_count = 0, an empty history, and
 * the first mover plays the part of "red" -- tau decay, min_resign_turn, the < 10 plies store lottery, max_game_length,
 * the sign of `value` and the red_wins / black_wins counters all count from the book position.  The caller vouches for
 * the positions (one king each, not already over: cchess_alphazero/lib/book.py checks them).  Without a book every
 * kernel, record and counter is what it was.  Call it before cz_search_start_selfplay and before a graph capture (the
 * captured launches hold the book's address), like cz_search_record_visits; synchronises the stream.
 * CZ_ERR_ARG: n < 0, n > CZ_BOOK_MAX, boards NULL with n > 0, rate outside [0, 1] -- the object keeps its book. */
int cz_search_set_book(cz_search* s, const int8_t* boards, int n, double rate, void* stream);

/* Playout cap randomization of self-play (KataGo: Wu 2019, section 3.1; the reference has no such option).  With
 * fast_sims > 0 every ply of every self-play game is either a FULL search -- simulation_num_per_move simulations, root
 * noise as configured: what every ply is without this call -- or a FAST one: fast_sims simulations and NO root noise
 * (no Dirichlet rows are drawn for the game at that ply, its noise epoch does not advance).  Ply `turns` of game
 * `game_id` is full iff philox_uniform(seed, game_id, stream 2, draw turns) < full_rate (stream 0 holds the per-game
 * lotteries, stream 1 the move choice); full_rate >= 1 makes every ply full and full_rate <= 0 every ply fast, both
 * without a draw.  The ply's budget S replaces simulation_num_per_move in the reuse rule of CChessPlayer.action
 * (player.py:153-158): done = the reused root's visit count, reset to 0 by bans, increase_temp or done == S; the ply
 * runs max(0, S - done) simulations, so a fast ply whose reused root already has more than fast_sims visits searches
 * nothing and moves at once.  Move choice (temperature, resignation, bans), the game rules and the store lottery are
 * unchanged.  The finished-game record marks fast plies with CZ_MOVE_FAST in moves[i], a visit entry with
 * CZ_VISIT_FAST; fast plies still write their visit entry.  Chunk reservation stays sized by the full budget; no
 * counter is added.  fast_sims = 0 (the state after cz_search_create) switches it off: every kernel then produces the
 * bits it produced before.  Self-play only: external mode (cz_search_set_roots) never looks at it.  Call it before
 * cz_search_start_selfplay and before a graph capture (the captured launches hold the parameters), like
 * cz_search_set_book; synchronises the stream.  CZ_ERR_ARG: fast_sims < 0 or > simulation_num_per_move, full_rate
 * outside [0, 1] with fast_sims > 0 -- the object keeps its setting; cz_search_set_sims below fast_sims is refused. */
int cz_search_set_playout_cap(cz_search* s, int fast_sims, double full_rate, void* stream);

/* Forced playouts and policy target pruning (KataGo: Wu 2019, section 3.2, the companion of the playout cap; the
 * reference has no such option).  k = 0 (the state after cz_search_create) switches both off: every kernel then
 * produces the bits it produced before.  The paper uses k = 2.
 *
 * FORCED PLAYOUTS (search).  With k > 0 the selection at the ROOT (select_action_q_and_u with is_root_node,
 * player.py:286-320; no other node) treats an edge as forced when it is not banned, its score q + u is not rejected
 * (score >= -99999999), n > 0 and
 *       (double)n * (double)n < k * p_ * (double)sum_n                      [evaluated as (k * p_) * sum_n]
 * where n and sum_n are the values that selection reads -- virtual losses of simulations in flight included, sum_n
 * before this simulation's increment -- and p_ is the prior this simulation uses, root noise included.  That is
 * n < sqrt(k p_ sum_n) without a square root: exact in float64, nothing to contract.  A forced edge's score is
 * +infinity; everything else is unchanged: the proven-win shortcut (first edge with q > 1 - 1e-7) keeps precedence,
 * among several forced edges the `>=` arg-max takes the last in edge order, nodes with more than 64 moves included.
 * In self-play it applies on FULL plies only: a fast ply of the playout cap never forces (it has no noise).  In
 * external mode (cz_search_set_roots) it applies whenever it has been set -- which is how a single search is tested;
 * worker/evaluator.py (the arena), agent/player.py (CChessPlayer) and uci.py never set it.
 *
 * POLICY TARGET PRUNING (record).  Forcing spends visits the search would not have made on the move's merits; they
 * are removed from the recorded targets, not from the tree.  Given a root's edges -- labels with the banned bit
 * (0x8000), raw visit counts n, w (float64), float32 priors p WITHOUT noise (a noise row lives for one simulation),
 * c_puct and k -- all arithmetic in float64, in the order written:
 *   S   = sum of n_j over the non-banned edges (it must fit int32).  S == 0: nothing is pruned.
 *   c*  = the non-banned edge with the greatest n, ties to the LOWEST label: what cz_search_choose plays at tau = 0.
 *   sq  = sqrt((double)S), correctly rounded
 *   E*  = q* + ((c_puct * p*) * sq) / (1 + n*)                 with q = w / n
 *   for every other non-banned edge with n_j > 0:
 *     f_j    = floor(sqrt((k * p_j) * S))
 *     d_j    = E* - q_j
 *     need_j = n_j if d_j <= 0, otherwise ceil(((c_puct * p_j) * sq) / d_j - 1) clamped to [0, n_j] in float64 before
 *              the conversion to an integer
 *     m_j    = max(need_j, n_j - f_j)
 *     if m_j < n_j and m_j <= 1 then m_j = 0
 *   c* keeps n*; edges with n_j = 0 stay 0; banned edges keep their raw count and their flag.
 * (need_j is the smallest count at which the edge's own PUCT score no longer exceeds E*; at most f_j visits are
 * taken away; an edge cut down to a single visit is noise and goes altogether.)
 * In self-play, with k > 0, record_visits on and the ply not fast, the ply's visit entry holds the pruned counts, its
 * flags carry CZ_VISIT_PRUNED and its header word raw_total = S; when S == 0 (no move, every move banned) and on fast
 * plies and with k = 0 the entry is written byte for byte as before, raw_total = 0.  The move is still chosen from the
 * raw counts in the tree (temperature, resignation, bans); neither the tree nor the game loop changes; no counter is
 * added.
 *
 * Call it before cz_search_start_selfplay and before a graph capture (the captured launches hold the parameters), like
 * cz_search_set_playout_cap; synchronises the stream.  CZ_ERR_ARG: s NULL, k < 0 or not finite -- the object keeps its
 * setting. */
int cz_search_set_forced_playouts(cz_search* s, double k, void* stream);
/* The pruned counts of every current root, as a visit entry of that root would hold them: n [G][128] int32 (0 past the
 * root's edges), raw_total [G] int32 = S, both DEVICE.  Same inputs as cz_search_root_stats; the bans are those of the
 * current cz_search_set_roots; c_puct is the object's, k its cz_search_set_forced_playouts setting (k = 0: the raw
 * counts).  A root that is not in the tree reports zeros. */
int cz_search_root_targets(cz_search* s, int32_t* n, int32_t* raw_total, void* stream);
/* The pruning arithmetic on its own, one wavefront per row: labels / n / w / p [rows][128] and n_edges [rows] (<= 128),
 * out_n [rows][128] (0 past n_edges), out_raw_total [rows], all DEVICE.  Labels of a row are distinct.  CZ_ERR_ARG: a
 * NULL pointer, rows < 0, c_puct or k negative or not finite. */
int cz_policy_target_prune(const uint16_t* labels, const int32_t* n, const double* w, const float* p,
                           const uint8_t* n_edges, int rows, double c_puct, double k,
                           int32_t* out_n, int32_t* out_raw_total, void* stream);

/* Random leaf mirror (AlphaGo Zero's random symmetry at every evaluation, as Leela Zero and KataGo keep it; the
 * reference has no such option).  The left-right mirror image of a Xiangqi position (file x <-> 8 - x) is a symmetry of
 * the rules but not of a trained network; with rate > 0 every NEW leaf is shown to the network either as it is or in its
 * mirror image, so that over the leaves of a search the network's wing bias averages out of the visit counts, the
 * recorded targets, the search values and the surprise weights.
 *
 * THE COIN.  When a leaf is expanded (a new node record, the root of an empty tree included) it is evaluated mirrored
 * iff philox_uniform(seed, key, stream 3, index) < rate, with key = game_id + slot * 2654435761 (the key of the root
 * noise; game_id is 0 in external mode until a self-play run set it) and index = (turns of the current root << 32) | the
 * new node's record id.  Record ids are the tree's own addresses: no two nodes of a game's tree share one, so no two
 * leaves of a tree share a draw.  Streams 0, 1 and 2 stay the per-game lotteries, the move choice and the playout cap.
 * rate <= 0 and rate >= 1 decide without a draw.  The decision travels in the node's header beside its waiting flag
 * and is dropped when the priors are attached: nothing else ever sees it, and a leaf in flight keeps the decision it was
 * expanded with whatever is set afterwards.
 *
 * FRAMES.  A mirrored leaf's queue slot holds the MIRROR IMAGE of the position in every form the slot has: the input
 * planes in every planes_dtype, the second block of a 28-plane input (the earlier position mirrored too; a missing one
 * stays zeros) and the occupancy board of cz_search_leaf_masks, with or without the planes.  The network's policy row
 * for that slot is then in the mirrored frame: the search reads the entry of move `a` at column cz_label_mirror[a].
 * The value is taken as it is.  Priors, their float32 summation order (move order), the stored p[], the moves and every
 * record stay in the un-mirrored frame; a network that is exactly mirror-equivariant gives the same search bit for bit
 * at every rate.
 *
 * FLAGS.  flags_or_null: DEVICE uint8 [n_games * sims_per_round] owned by the caller, or NULL.  Whenever a leaf is
 * written to queue slot game * sims_per_round + sim, flags[slot] is written with it: 1 mirrored, 0 not (a compact queue
 * of cz_search_round_q names the slot in q_rows).  An evaluator that is not the plain network -- a test's stand-in, a
 * cache keyed by position -- needs it; the share of mirrored leaves is read from it, no counter is added.  A new array
 * starts as a copy of the previous one, or as zeros when there was none.
 *
 * rate = 0 (the state after cz_search_create) switches it off: nothing is drawn and every kernel produces the bits it
 * produced before.  Both modes; cz_search_set_roots and cz_search_start_selfplay keep the setting.  It may be called
 * between rounds; call it before a graph capture (the captured launches hold the rate and the array's address), like
 * cz_search_set_playout_cap; synchronises the stream.  CZ_ERR_ARG: s NULL, rate NaN or outside [0, 1] -- the object
 * keeps its setting. */
int cz_search_set_leaf_mirror(cz_search* s, double rate, uint8_t* flags_or_null, void* stream);

/* ---- cross-game evaluation cache (off by default; the reference has no such option; lc0's NNCache, KataGo's nnCache) ----
 * A table of network results keyed by position, shared by all games of the search object and kept across games:
 * cz_search_reset_trees, cz_search_set_roots and the start of a new self-play game do NOT empty it.  A new leaf whose
 * position the table holds takes no queue row: its priors are copied into the node, its value waits beside the slot,
 * and the next round attaches it at its place in simulation order with the evaluated leaves -- the node waits for that
 * attach exactly as an evaluated leaf does, and simulations that reach it park as they do now.  A row's network output
 * does not depend on its place in the batch and a node's priors are a function of its row and its move list, so THE
 * SEARCH WITH THE CACHE ON PRODUCES THE BITS OF THE SEARCH WITH IT OFF: visit counts, W, priors, records, counters
 * (`expansions` keeps counting tree growth; `hits` below says how many of them needed no row).  The caller must keep the
 * network a function of the row alone and empty the table (cz_search_eval_cache_clear) when the network changes.
 *
 * THE TABLE.  Direct-mapped, 2^log2_entries entries of CZ_EVAL_CACHE_STRIDE bytes: the 48-byte packed position, the
 * leaf-mirror bit the row was evaluated under (cz_search_set_leaf_mirror), the move count, the float32 value and
 * float p[128], the priors exactly as the attach writes them into the node.  A match is the full position plus the
 * mirror bit, never the hash alone; an entry is overwritten by the next position that maps to it.  The table is a
 * device allocation of its own, made by this call from what the chunk pool left (the pool takes at most 80 % of the
 * free memory); cz_search_bytes includes it while it is on.
 *
 * WHO TOUCHES IT WHEN.  Read only by the selection launch of a round (a leaf a resumed simulation creates in the backup
 * launch does not ask and is evaluated as before); written only by a launch of its own at the start of a round, from
 * the rows that round attaches, formed by the attach's own device functions; not touched by the backup launch.  All on
 * the search's stream: a reader only sees entries an earlier launch completed.  No lock, no fence, no wait.  Positions
 * asked for by several games in the SAME round are all evaluated (not merged).
 *
 * cz_search_set_eval_cache: log2_entries 0 switches it off and frees the table, otherwise CZ_EVAL_CACHE_MIN_LOG2 <=
 * log2_entries <= CZ_EVAL_CACHE_MAX_LOG2 (the size it has already: the table is emptied).  CZ_ERR_ARG: s NULL,
 * log2_entries outside that, or a search with 28 input planes (use_history: the second plane block depends on the
 * simulation's path and on the game history, so the input is not a function of the position).  CZ_ERR_NOMEM: the
 * allocation failed; the search stays usable with the cache off.  CZ_ERR_STATE: the table would go or change size while
 * leaves it answered wait for their attach -- change it between searches.  Call it after cz_search_create, before the
 * rounds and before a graph capture (the captured launches hold the table's address); synchronises the stream.
 * cz_search_policy_logits empties the table when it changes the mode (the meaning of a row changes).
 * cz_search_eval_cache_clear: empties the table and zeroes the numbers below (enqueued on the stream; leaves already
 * answered keep their values).  The rows of the ONE round that follows were evaluated before the call -- by the network
 * the caller is replacing -- and are not stored; the rounds after it store again.  cz_search_eval_cache_info: HOST out[4] = entries (0 = off), probes, hits, stores, summed
 * since the table was made or last emptied; synchronises the stream. */
#define CZ_EVAL_CACHE_STRIDE 576
#define CZ_EVAL_CACHE_MIN_LOG2 10
#define CZ_EVAL_CACHE_MAX_LOG2 24
int cz_search_set_eval_cache(cz_search* s, int log2_entries, void* stream);
int cz_search_eval_cache_clear(cz_search* s, void* stream);
int cz_search_eval_cache_info(cz_search* s, uint64_t* out, void* stream);

/* external mode (CChessPlayer.action): set the position to search for each game.  boards [G][90];
 * turns [G] or NULL; no_act [G][32] + n_no_act [G] or NULL (at most 32 banned moves per game); increase_temp / enable_resign [G] or NULL;
 * select_mask [G] or NULL (only games with a non-zero byte are touched).  Trees are kept (subtree reuse).
 * use_history only: hist_kind [G] or NULL = the `hist` argument of action(): 0 none, 1 prev_boards[g] ([G][90]) is
 * the game position two plies before the root, 2 a history shorter than 5 entries was passed. */
int cz_search_set_roots(cz_search* s, const int8_t* boards, const int32_t* turns, const uint16_t* no_act,
                        const uint8_t* n_no_act, const uint8_t* increase_temp, const uint8_t* enable_resign,
                        const uint8_t* select_mask, const int8_t* prev_boards, const uint8_t* hist_kind, void* stream);

/* one lock-step round for all games.  policy [G*K][2086] float32, value [G*K] float32 (results for the
 * planes written by the previous round; ignored for slots that had no leaf), planes [G*K][14 or 28][10][9]. */
int cz_search_round(cz_search* s, const float* policy, const float* value, void* planes, void* stream);

/* The same round with a COMPACT evaluation queue: only the slots that hold a new leaf are evaluated.  After the round
 * q_rows[0 .. *q_count) (int32 DEVICE, arbitrary order) lists those slots and *q_count (int32 DEVICE) their number; the
 * caller evaluates planes[q_rows[i]] and writes the result to policy[i] / value[i] -- row i, not the slot -- which the
 * NEXT cz_search_round_q consumes.  Nothing is copied to the host: run the network with the cz_*_q entry points, which
 * read the board count from q_count on the device (fixed launch shapes: the round still replays from a HIP graph).
 * The two forms may be mixed: a round consumes its results by compact row exactly when the PREVIOUS round of the
 * object was a cz_search_round_q.  In self-play 2-7 % of the slots carry no leaf (terminal / repeated positions, parked simulations), with
 * search_threads = 32-40 up to half of them. */
int cz_search_round_q(cz_search* s, const float* policy, const float* value, void* planes, int32_t* q_rows,
                      int32_t* q_count, void* stream);

/* simulations per search for the following cz_search_set_roots calls (CChessPlayer.action(depth=...), player.py:160) */
int cz_search_set_sims(cz_search* s, int simulation_num_per_move);
/* on = 1: the policy rows handed to cz_search_round(_q) are raw LOGITS, not probabilities.  The reference spreads the
 * softmax output over the legal moves, p_j / sum_legal p (agent/player.py:272-283); the softmax's own denominator cancels
 * there, so the priors are formed as exp(l_j - max over the node's moves) / their sum -- identical up to float32 rounding,
 * and the network's tail can skip normalising all 2086 columns (cz_heads_tail normalize = 0).  Default 0. */
int cz_search_policy_logits(cz_search* s, int on);
/* (round 5) masks [n_games * sims_per_round][96] uint32 DEVICE, caller-owned (NULL switches it off, the default): every new
 * leaf's position is ALSO written as an occupancy board into row `slot` -- word pos = plane position, bit c = plane c (0..13 the
 * position, 14..27 the history block of 28-plane searches) shows a piece there; state_to_planes / state_history_to_planes,
 * environment/static_env.py:137-194, in 384 bytes -- for cz_input_resblock_m.  The planes are written as before. */
int cz_search_leaf_masks(cz_search* s, uint32_t* masks);
/* (round 5) on = 0: while cz_search_leaf_masks is set, a new leaf is written as its occupancy board ONLY -- for a caller whose
 * network takes the boards (cz_input_resblock_m reads nothing else); the `planes` rows of cz_search_round(_q) are then left
 * untouched.  on = 1 (default) writes both.  CZ_ERR_ARG when switched off without masks; clearing the masks switches the
 * planes back on.  (state_to_planes, environment/static_env.py:137-156: the same information in 384 bytes.) */
int cz_search_leaf_planes(cz_search* s, int on);
int cz_search_reset_trees(cz_search* s, void* stream);
/* synchronises the stream; *host_out = number of games whose current search is unfinished */
int cz_search_pending(cz_search* s, int* host_out, void* stream);
/* After a cz_search_round: the queue rows (slot = game * K + sim) that hold a NEW leaf, i.e. the only rows whose
 * policy / value the next round will read.  rows [G*K] int32 DEVICE (compacted, arbitrary order), counts_dev [2] int32
 * DEVICE scratch; HOST host_out[0] = searches still running (as cz_search_pending), host_out[1] = rows written.
 * Synchronises the stream.  Lets a caller with few games (arena, UCI) evaluate only the rows that carry a position:
 * with K = 32 simulations per batch roughly half of a batch's rows are simulations parked on a leaf another one
 * already expanded (player.py:238-242). */
int cz_search_leaf_rows(cz_search* s, int32_t* rows, int32_t* counts_dev, int* host_out, void* stream);
/* root edges after a search: moves/n/w/p [G][128], sum_n [G], counts [G] (any may be NULL) */
int cz_search_root_stats(cz_search* s, uint16_t* moves, int32_t* n, double* w, float* p, int32_t* sum_n,
                         uint8_t* counts, void* stream);
/* the same for the node reached from each root along path[g][0 .. path_len) (DEVICE move labels, 0xFFFF ends a path
 * early; path_len = 0: the root).  A position that is not linked in the tree reports counts = 0.  This is what the
 * reference's callers read out of the search_tree dict they handed to the player (ponder move uci.py:312-318,
 * principal variation player.py:408-450). */
int cz_search_node_stats(cz_search* s, const uint16_t* path, int path_len, uint16_t* moves, int32_t* n, double* w,
                         float* p, int32_t* sum_n, uint8_t* counts, void* stream);
/* principal variation of every game in one launch (player.py:408-433: the most-visited edge at each node, `>=` keeps
 * the last maximum, the bans of the current search apply at the root): moves [G][max_len] uint16 (0xFFFF padded),
 * visits [G][max_len] int32, both DEVICE. */
int cz_search_pv(cz_search* s, int max_len, uint16_t* moves, int32_t* visits, void* stream);
/* stop starting simulations in every running search (UCI `stop`, CChessPlayer.close_and_return_action,
 * player.py:88-106): the next cz_search_round backs up what is in flight and the searches become idle */
int cz_search_stop(cz_search* s, void* stream);
/* calc_policy + apply_temperature + np.random.choice with the uniform draws u [G] (NULL = 0.5):
 * action [G] = label, or -1 when the player resigns */
int cz_search_choose(cz_search* s, const double* u, int32_t* action, void* stream);
/* HOST out[n_counters] (order: enum Counter in csrc/xq_search.h); synchronises the stream */
int cz_search_counters(cz_search* s, uint64_t* host_out, void* stream);
/* the same counters before the sum over games: HOST out[G][n_counters] (tuning: which game's wavefront a launch waits for,
 * tools/search_tail.py); synchronises the stream */
int cz_search_game_counters(cz_search* s, uint64_t* host_out, void* stream);
/* copies finished-game records (record_stride bytes each) written since *cursor into HOST memory */
int cz_search_drain_records(cz_search* s, unsigned int* cursor, void* host_buf, int max_records, int* n_out,
                            void* stream);
/* ---- root visit record of self-play (off by default) ----
 * on = 1: from now on every searched ply of a self-play game writes one entry -- the root's visit counts at the moment
 * the move is chosen (calc_policy, agent/player.py:375-406, before the temperature), the resignation ply included; an
 * appended king capture (self_play.py:177-184) is not searched and has none.  capacity = entries the device ring holds
 * (0 = 64 * n_games).  One round records at most 8 plies of a game (a search with nothing left to do ends in the same
 * launch), so a caller that drains at least every capacity / (8 * n_games) rounds loses nothing.  The ring is never
 * overwritten: an entry that finds it full is dropped and counted, and the game's finished-game record then carries
 * flag bit 2.  Games already under way when recording is switched on carry bit 2 as well; cz_search_start_selfplay
 * starts every game complete.  on = 0 frees the buffers.  Synchronises the stream; not while a captured graph that
 * holds the old buffers may still replay.  Device memory: capacity * 784 bytes + n_games + 256. */
int cz_search_record_visits(cz_search* s, int on, int capacity, void* stream);
/* one ring entry, 784 bytes: this header, then uint16 label[128] (the root's edges in edge order, get_legal_moves
 * order = the reference's node.a; mover frame like the record's moves; bit 15 set = banned at this ply, in its no_act
 * list), then int32 n[128] (exact visit counts, carried-over visits of the reused subtree included).  Entries of one
 * game appear in ply order, before the game's record. */
typedef struct cz_visit_entry {
    uint32_t game_id;
    uint16_t ply;                    /* turns when the move was chosen */
    uint8_t n_edges;
    uint8_t flags;                   /* bit 0: the player resigned at this ply; bit 1 (CZ_VISIT_FAST): the ply was a
                                        fast search of the playout cap (cz_search_set_playout_cap); bit 2
                                        (CZ_VISIT_PRUNED): n[] holds the pruned policy targets, not the raw counts
                                        (cz_search_set_forced_playouts); bit 3 (CZ_VISIT_GUMBEL): n[] holds the Gumbel
                                        policy target scaled to 65536 (cz_search_set_gumbel) */
    int32_t sum_n;                   /* the root's own visit count */
    uint32_t raw_total;              /* CZ_VISIT_PRUNED, CZ_VISIT_GUMBEL: sum of the RAW counts of the non-banned edges (S), so that
                                        raw_total - sum of the non-banned n[] = visits pruned; otherwise 0 (this word
                                        was `reserved`, always 0, before pruning existed) */
} cz_visit_entry;
#define CZ_VISIT_FAST 2u
#define CZ_VISIT_PRUNED 4u
/* Copies every entry written since the last call into HOST host_buf (784 bytes each) and frees their ring space;
 * *n_out = entries copied.  host_buf = NULL: *n_out = entries waiting, nothing is consumed.  CZ_ERR_ARG when more are
 * waiting than max_entries (nothing is consumed).  dropped_out (HOST, or NULL) = entries dropped since recording was
 * switched on.  Synchronises the stream. */
int cz_search_drain_visits(cz_search* s, void* host_buf, int max_entries, int* n_out, uint64_t* dropped_out,
                           void* stream);
/* ---- root value record of self-play (off by default; the reference has no such option) ----
 * The search's own estimate of the root position, recorded beside each visit entry so that a trainer can mix it with
 * the game result (Lc0's q_ratio).  on = 0 (the state after cz_search_create): no kernel, record, counter or entry
 * differs by a bit from what it was before this existed.
 *
 * THE ARITHMETIC.  Given a root's edges as a visit entry sees them -- labels with the banned bit (0x8000), the raw
 * statistics n_j (int32) and w_j (float64, from the root mover's view: the q = w / n that cz_search_choose takes its
 * maxq from) and m_j, the count the visit entry records for the edge (the PRUNED count when the entry is
 * CZ_VISIT_PRUNED, the raw count n_j otherwise) -- all arithmetic in float64:
 *       q_root = ( sum_j m_j * (w_j / n_j) ) / ( sum_j m_j )      over non-banned edges with n_j > 0
 * Each quotient and each product is rounded once; the numerator is summed in a fixed order (edge j and j + 64 in lane
 * j, then one ladder over the 64 lanes), so equal inputs give equal bits; the denominator is a sum of integers, exact.
 * Without pruning or bans this is sum w / sum n.  With forced playouts the visits that forcing added do not drag the
 * value towards moves the search rejected.  sum m_j = 0 -- no edge, every edge banned, a root that was never selected
 * from -- gives NaN: "no value".  Every backed-up value lies in [-2, 2] (a network value in [-1, 1], a terminal one
 * +-2, player.py:204-208) and a finished search has no virtual loss outstanding, so |w_j| <= 2 n_j and |q_root| <= 2.
 *
 * THE RING.  The 784-byte cz_visit_entry has no free word, so the values live in a ring of their own, double q[capacity],
 * indexed by the slot of the visit entry: the kernel writes both in one reservation, a dropped entry drops its value.
 * Needs cz_search_record_visits on (CZ_ERR_ARG otherwise, the object keeps its setting); every call of
 * cz_search_record_visits frees the value ring as well, so switch the values on after it.  Call it before
 * cz_search_start_selfplay and before a graph capture, like the other setters; synchronises the stream.  Entries
 * already waiting when it is switched on report NaN.  on = 0 frees the buffer.  Device memory: capacity * 8 bytes.
 * No counter is added; the move, the tree and the visit entries do not change. */
int cz_search_record_values(cz_search* s, int on, void* stream);
/* cz_search_drain_visits that also copies the entries' values into HOST q_buf[max_entries], q_buf[i] beside entry i.
 * host_buf = NULL counts (q_buf unused).  CZ_ERR_ARG also when host_buf is given and q_buf is NULL or the value record
 * is off.  cz_search_drain_visits itself keeps working with the values on; it drops the values of what it consumes. */
int cz_search_drain_visits_q(cz_search* s, void* host_buf, double* q_buf, int max_entries, int* n_out,
                             uint64_t* dropped_out, void* stream);
/* The value an entry of each current root would carry: q [G] float64 DEVICE.  Same inputs as cz_search_root_targets:
 * the bans of the current cz_search_set_roots, m = the counts cz_search_root_targets reports for the object's c_puct
 * and k (k = 0: the raw counts).  A root that is not in the tree reports NaN.  Works with the record off. */
int cz_search_root_value(cz_search* s, double* q, void* stream);
/* The arithmetic on its own, one wavefront per row: labels / m / n / w [rows][128] and n_edges [rows] (<= 128), out_q
 * [rows], all DEVICE.  CZ_ERR_ARG: a NULL pointer, rows < 0. */
int cz_root_value(const uint16_t* labels, const int32_t* m, const int32_t* n, const double* w, const uint8_t* n_edges,
                  int rows, double* out_q, void* stream);
/* ---- policy surprise record of self-play (off by default; the reference has no such option) ----
 * How far the search moved away from the network's prior at each recorded ply, so that a trainer can give the plies the
 * policy head learns most from more weight (KataGo's policy surprise weighting, Wu 2019).  on = 0 (the state after
 * cz_search_create): no kernel output, ring byte, record, counter or entry differs by a bit from what it was before
 * this existed.
 *
 * THE ARITHMETIC.  Given a root's edges as a visit entry sees them -- labels with the banned bit (0x8000), m_j, the
 * count the visit entry records for the edge (the PRUNED count when the entry is CZ_VISIT_PRUNED, the raw count
 * otherwise) and p_j, the float32 prior WITHOUT root noise -- all arithmetic in float64, every operation rounded once,
 * no fused multiply-add; the live edges are the non-banned j < n_edges:
 *       M = sum m_j (integers: exact)        P = sum (double) p_j                 over the live edges
 *       t_j = m_j / M                        r_j = max(p_j / P, 1e-30)
 *       s = sum t_j * log(t_j / r_j)         over the live edges with m_j > 0
 *       surprise = max(s, 0)
 * the Kullback-Leibler divergence of the recorded policy target from the normalised prior.  M = 0 or not P > 0 -- no
 * edge, every edge banned, a root that was never selected from -- gives NaN: "no surprise".  Each sum is taken in a
 * fixed order (edge j and j + 64 in lane j, then one ladder over the 64 lanes), so equal inputs give equal bits.
 * t_j <= 1 and r_j >= 1e-30 bound every logarithm by ln 1e30, and sum t_j = 1, so 0 <= surprise <= ln 1e30 = 69.08 <
 * CZ_SURPRISE_BOUND.  log is the device library's float64 logarithm (DESIGN.md names the routine and its accuracy).
 *
 * THE RING.  Like the value record: double s[capacity], indexed by the slot of the visit entry, written by the kernel
 * in the entry's reservation for every ply that gets an entry (fast plies of the playout cap included); a dropped
 * entry drops its surprise.  Needs cz_search_record_visits on (CZ_ERR_ARG otherwise, the object keeps its setting);
 * every call of cz_search_record_visits frees this ring as well, so switch it on after that.  Call it before
 * cz_search_start_selfplay and before a graph capture; synchronises the stream.  Entries already waiting when it is
 * switched on report NaN.  on = 0 frees the buffer.  Device memory: capacity * 8 bytes.  No counter is added; the move,
 * the tree, the visit entries and the value ring do not change. */
#define CZ_SURPRISE_BOUND 70
int cz_search_record_surprise(cz_search* s, int on, void* stream);
/* cz_search_drain_visits that also copies the entries' values into HOST q_buf[max_entries] and their surprises into
 * HOST s_buf[max_entries], beside entry i.  q_buf / s_buf = NULL: that ring is not copied (it has to be NULL when its
 * record is off: CZ_ERR_ARG otherwise).  host_buf = NULL counts.  cz_search_drain_visits and cz_search_drain_visits_q
 * keep working with the surprise record on; they drop the surprises of what they consume. */
int cz_search_drain_visits_qs(cz_search* s, void* host_buf, double* q_buf, double* s_buf, int max_entries, int* n_out,
                              uint64_t* dropped_out, void* stream);
/* The surprise an entry of each current root would carry: out [G] float64 DEVICE.  Same conventions as
 * cz_search_root_value: the bans of the current cz_search_set_roots, m = the counts cz_search_root_targets reports for
 * the object's c_puct and k (k = 0: the raw counts).  A root that is not in the tree reports NaN.  Works with the record
 * off. */
int cz_search_root_surprise(cz_search* s, double* out, void* stream);
/* The arithmetic on its own, one wavefront per row: labels / m / p [rows][128] (uint16 / int32 / float32) and n_edges
 * [rows] (<= 128), out [rows] float64, all DEVICE.  CZ_ERR_ARG: a NULL pointer, rows < 0. */
int cz_root_surprise(const uint16_t* labels, const int32_t* m, const float* p, const uint8_t* n_edges, int rows,
                     double* out, void* stream);
/* ---- Gumbel root search with sequential halving (off by default; the reference has no such option) ----
 * "Policy improvement by planning with Gumbel" (Danihelka et al., ICLR 2022) at the root: M candidate moves are sampled
 * without replacement through Gumbel noise, the ply's simulations are spent on them by sequential halving, the survivor
 * is played and the policy is trained towards softmax(log prior + sigma(completed Q)) instead of visit counts -- a target
 * that improves on the prior at any budget.  m = 0 (the state after cz_search_create): no kernel output, record, counter
 * or entry differs by a bit from what it was before this existed, and the per-game state below is not touched.
 *
 * Everything is float64 unless said otherwise.  "Edges" are the root's non-banned edges in edge order, p_j the stored
 * float32 prior WITHOUT noise, n_j / w_j the edge's statistics from the root mover's view.
 *
 * DRAWS.  g_j = -log(-log u_j), u_j = philox_uniform(seed, key, stream 4, turns << 32 | j) for edge index j (banned
 * edges keep their index), key = game id + game slot * 2654435761 like the root noise, so external mode has draws too;
 * u = 0 is replaced by 2^-53.  Drawn when the ply's search begins and fixed for the whole ply.
 *
 * SCHEDULE for m candidates and a budget of n simulations:
 *       seq(m, n): if m <= 1: return [0, 1, ..., n - 1]
 *                  L = ceil(log2 m); visits = [0] * m; k = m; out = []
 *                  while len(out) < n:
 *                      e = max(1, floor(n / (L * k)))
 *                      repeat e times: out += visits[:k]; visits[i] += 1 for i < k
 *                      k = max(2, k // 2)
 *                  return out[:n]
 * with m = min(M, number of edges) and n the simulations this ply runs: simulation_num_per_move less the visits the
 * reused root already has (the `tasks` of the ply).
 *
 * ROOT SELECTION.  started_j counts the selections of this ply that took edge j: per-game state, zeroed when the ply's
 * search begins, independent of the virtual loss and of visits inherited from a reused subtree -- which is why the
 * schedule is driven by it and not by n_j: with several simulations in flight n_j carries virtual losses, and a reused
 * root starts with unequal n_j, either of which would break the halving's "all survivors have equal counts".  The t-th
 * selection at the root, t = sum_j started_j, takes among the edges with started_j == seq(m, n)[t] the greatest
 *       g_j + log p_j + sigma(q01_j)
 *       q01_j = clamp((w_j / n_j + 1) / 2, 0, 1) where n_j > 0, else 0
 *       sigma(x) = ((c_visit + max_b n_b) * c_scale) * x           (max over the edges)
 * the LATER edge on a tie, as PUCT's `>=` does; p_j = 0 scores -infinity and loses to any finite score.  The first m
 * selections so pick the m greatest g_j + log p_j (+ sigma of what a reused root knows), the Gumbel top-m sample; from
 * then on only they are eligible.  The rule replaces the root's whole selection, the proven-win shortcut included;
 * below the root the search is PUCT as it is (cz_search_set_gumbel_full below replaces it there too).
 *
 * MOVE PLAYED.  Among the edges with the greatest started_j the greatest of the same score, w and n as they are after
 * the last backup.  cz_search_choose ignores u; the resign test is unchanged.  A Gumbel ply has no temperature and no
 * Dirichlet noise (no rows are drawn, as on a fast ply of the playout cap).
 *
 * POLICY TARGET, a pure function of a root row (labels, n, w, p) and (c_visit, c_scale):
 *       cq_j = q01_j where n_j > 0, else vbar = (sum_{n_b > 0} p_b q01_b) / (sum_{n_b > 0} p_b), 1/2 when that sum is not
 *              positive (nothing visited)
 *       pi'_j = p_j exp(sigma(cq_j) - max_b sigma(cq_b)) / sum over the edges
 *       m_j = floor(65536 pi'_j + 1/2); banned edges 0; all 0 when no edge has a positive prior
 * The paper also mixes the root's own network value into vbar with weight 1 / (1 + sum n); the node record holds no
 * value and that weight is below 6 % at 16 simulations, so it is LEFT OUT here (cz_search_set_gumbel_full, below, keeps
 * the value and puts it in).  exp and log are the device library's
 * float64 routines: m_j may differ by 1 from another implementation's.
 *
 * VISIT RECORD.  An entry of a Gumbel ply carries CZ_VISIT_GUMBEL, n[] holds m_j (a trainer that normalises n[] gets
 * pi') and raw_total the sum of the raw counts of the non-banned edges, as for CZ_VISIT_PRUNED.  The value and the
 * surprise record keep their definitions over the recorded n[].
 *
 * cz_search_set_gumbel: 0 <= m <= CZ_GUMBEL_MAX_M, c_visit and c_scale finite and >= 0 (the paper: 50 and 1), CZ_ERR_ARG
 * otherwise and when m > 0 while forced playouts or the playout cap are on (each defines its own root rule; their
 * setters refuse likewise while m > 0).  Call it before cz_search_start_selfplay / cz_search_set_roots and before a
 * graph capture; synchronises the stream.  Device memory: 1540 bytes per game, allocated at cz_search_create. */
#define CZ_VISIT_GUMBEL 8u
#define CZ_GUMBEL_MAX_M 128
int cz_search_set_gumbel(cz_search* s, int m, double c_visit, double c_scale, void* stream);
/* started [G][128] int32 DEVICE: the selections of the current ply per root edge, 0 for banned edges and beyond the
 * root's edges.  Meaningful once a ply has begun with the option on; before that it holds zeros. */
int cz_search_root_started(cz_search* s, int32_t* started, void* stream);
/* draws [G][128] float64 DEVICE: the current ply's g_j. */
int cz_search_gumbel_draws(cz_search* s, double* draws, void* stream);
/* What a CZ_VISIT_GUMBEL entry of each current root would hold: m [G][128] int32 and raw_total [G], DEVICE, with the
 * bans of the current cz_search_set_roots and the object's c_visit / c_scale.  Works with m = 0. */
int cz_search_gumbel_targets(cz_search* s, int32_t* m, int32_t* raw_total, void* stream);
/* The target arithmetic on its own, one wavefront per row: labels / n / w / p [rows][128] (uint16 with the banned bit /
 * int32 / float64 / float32) and n_edges [rows] (<= 128), out_m [rows][128], out_raw_total [rows], all DEVICE.
 * CZ_ERR_ARG: a NULL pointer, rows < 0, c_visit or c_scale negative or not finite. */
int cz_gumbel_policy_target(const uint16_t* labels, const int32_t* n, const double* w, const float* p,
                            const uint8_t* n_edges, int rows, double c_visit, double c_scale, int32_t* out_m,
                            int32_t* out_raw_total, void* stream);
/* ---- full Gumbel search: the rule below the root and v_mix (run.py self --gumbel-full) ------------------------------
 * The two parts of the paper that cz_search_set_gumbel leaves out; an option of it, off after cz_search_create.  With it
 * off no kernel output, record, counter or entry differs by a bit from what cz_search_set_gumbel alone gives.
 *
 * NODE VALUE.  While m > 0 (full on or off) every attach of an evaluated leaf keeps the leaf's network value in the
 * fourth word of the node header: the float32 the round was handed for the slot, from the node's mover's view -- the
 * value that is backed up; a leaf evaluated in its mirror image keeps the value as it came.  It costs no memory and no
 * load: the word was free and travels with the header.  A node attached while m = 0 carries 0.
 *
 * SELECTION BELOW THE ROOT.  With full on, at every node that is not the root the whole selection -- PUCT and the
 * proven-win shortcut -- is replaced by (float64; all edges of the node, only roots have bans; n_j, w_j as selection
 * reads them, virtual losses of simulations in flight included; p_j the float32 prior; v the node's stored value):
 *       N      = sum_j n_j
 *       vhat   = clamp((v + 1) / 2, 0, 1)
 *       A      = sum_{n_j > 0} p_j          B = sum_{n_j > 0} p_j q01_j
 *       v_mix  = (vhat + N (B / A)) / (1 + N) where A > 0, else vhat
 *       cq_j   = q01_j where n_j > 0, else v_mix
 *       s_j    = sigma(cq_j)                (max_b n_b over the node's edges)
 *       e_j    = p_j exp(s_j - max_b s_b)   T = sum_j e_j
 *       pi'_j  = e_j / T                    (0 for every j when T is not > 0)
 *       score_j = pi'_j - n_j / (1 + N)
 * and the edge of the greatest score is taken, the LATER edge on a tie.  No exploration constant: the visit counts of a
 * node follow pi'.  Nothing visited: pi' is the normalised prior.  Every prior 0: the least n_j wins.  The root keeps the
 * halving; virtual loss, sum_n, expansion, terminal and repeated positions and parking are what they were.  The sums
 * run over the lane's two edges and then one ladder over the 64 lanes; exp is the device library's float64 routine, so a
 * score may differ from another implementation's in its last places (1e-12 is generous).
 *
 * POLICY TARGET.  With full on vbar is replaced by v_mix of the root -- the formula above over the NON-BANNED edges with
 * the root's stored value -- which is the paper's target.  Nothing visited: cq_j = vhat for every edge and the target
 * is the prior.  The target feeds the visit entries, cz_search_root_targets and cz_search_gumbel_targets, and through
 * the recorded n[] the value and the surprise record, which keep their definitions.
 *
 * cz_search_set_gumbel_full: on is 0 or 1.  CZ_ERR_ARG when s is NULL, when on is anything else, or when on = 1 while
 * m = 0; the object keeps its setting.  cz_search_set_gumbel(m = 0) also switches it off.  Call it before
 * cz_search_start_selfplay / cz_search_set_roots and before a graph capture; synchronises the stream.  It does not
 * touch the trees: nodes attached while m = 0 carry the value 0 (vhat = 1/2), so a caller who grew trees before
 * switching the Gumbel search on should call cz_search_reset_trees first. */
int cz_search_set_gumbel_full(cz_search* s, int on, void* stream);
/* v [G] float32 DEVICE: the stored network value of the node cz_search_node_stats would report for the same path
 * (path NULL / path_len 0: the root); NaN when the position is not linked in the tree or is still waiting for its
 * evaluation.  0 for a node attached while m = 0. */
int cz_search_node_net_value(cz_search* s, const uint16_t* path, int path_len, float* v, void* stream);
/* cz_gumbel_policy_target with v [rows] float32 DEVICE, the rows' network values: the full search's target of
 * caller-supplied rows.  Same argument checks. */
int cz_gumbel_policy_target_v(const uint16_t* labels, const int32_t* n, const double* w, const float* p,
                              const uint8_t* n_edges, const float* v, int rows, double c_visit, double c_scale,
                              int32_t* out_m, int32_t* out_raw_total, void* stream);
/* The selection below the root on its own, one wavefront per row through the device function the search calls: n / w / p
 * [rows][128] (int32 / float64 / float32), n_edges [rows] (<= 128), v [rows] float32; out_pick [rows] int32, -1 for a
 * row without edges; out_score [rows][128] float64, every edge's score, 0 past n_edges.  All DEVICE.  CZ_ERR_ARG: a NULL
 * pointer, rows < 0, c_visit or c_scale negative or not finite. */
int cz_gumbel_interior_pick(const int32_t* n, const double* w, const float* p, const uint8_t* n_edges, const float* v,
                            int rows, double c_visit, double c_scale, int32_t* out_pick, double* out_score, void* stream);
/* ---- MCTS solver: forced wins and losses proven in the tree (off by default; the reference has no such option) --------
 * run.py self / eval --solver, the UCI option Solver.  The search stores that a move leads to a king capture in the edge
 * (a terminal child); with the solver on it draws the conclusions (Winands, Bjornsson, Saito: Monte-Carlo Tree Search
 * Solver, 2008; lc0's certainty propagation).  With it off no kernel output, record or counter differs by a bit, and the
 * kernels launched are the ones launched before it existed.
 *
 * STATUS.  A position s in a game's tree is OPEN, WIN(d) or LOSS(d) from its mover's view; d is the number of plies to a
 * terminal position along a line the tree holds -- a bound, not the shortest line -- and saturates at CZ_PROOF_DIST_MAX.
 *   terminal child   done(s') == (True, +1) counts as WIN(1), (True, -1) as LOSS(0).
 *   edge mark        an edge (s, a) carries the status of its child as last seen at a backup over that edge; terminal
 *                    children are marked by their code.  The edge is WINNING if the mark is LOSS, LOSING if it is WIN.
 *   marking          a simulation that ends on a terminal child or on a proven node marks the last edge of its path when
 *                    it is backed up.  Ordinary leaves, repetitions and overflow paths mark nothing.
 *   deriving         after an edge of an OPEN s was marked: s becomes WIN(1 + min d over its winning edges) if it has a
 *                    winning edge, LOSS(1 + max d over all edges) if every one of its nm > 0 edges is losing.  The first
 *                    proof of a node is final.  If s became proven the edge above it on the path is marked and its node
 *                    derived, and so on upward; the walk stops at the first node that stays OPEN.  Root bans play no part
 *                    in a status: it belongs to the position.
 *   arrival          a descent that steps onto a proven node at depth >= 1 ends there, after the repetition test, worth
 *                    +2 for WIN and -2 for LOSS from that node's mover (what the terminal at the end of the line is
 *                    worth); deferred and flushed like a terminal result, counted in proven_sims, no network row.
 * SELECTION, at the root and at OPEN nodes:
 *   1. among the non-banned edges a winning one is taken at once: the least d, the first in edge order on a tie;
 *   2. otherwise the reference's rule, its q > 1 - 1e-7 shortcut included, over the non-banned edges that are not losing;
 *   3. if every non-banned edge is losing, over all non-banned edges.
 * DECIDED ROOT.  A root is decided if it is LOSS, or WIN with a non-banned winning edge.  A decided root starts no further
 * simulation this ply -- tested before each batch, the first of a ply included -- and the ply is complete when the
 * simulations in flight are backed up.
 * MOVE CHOICE.  At a WIN root with a non-banned winning edge the played move is rule 1's edge, in self-play and in
 * cz_search_choose, whatever tau is; resignation is tested first.  Everything else is unchanged: the recorded visit
 * counts, q and surprise are what the tree holds.
 * COUNTERS, appended to cz_search_counters: proven_sims (arrivals), proofs (nodes that became WIN or LOSS), decided_plies
 * (plies whose remaining simulations a decided root cut).
 * Draws and repetition values (they depend on the path), the longest defence at a LOSS root and the shortest mate are
 * out of scope.
 *
 * WHERE IT LIVES.  The status sits in bits 10-11 and d in bits 16-23 of the node header's meta word, the edge mark in bits
 * 24-25 of the edge's child word (node ids use 24 bits); the distances of marked children are read from their headers.
 * No memory is added.  The trees keep their proofs when the solver is switched off; the search then ignores them.
 *
 * cz_search_set_solver: on is 0 or 1; CZ_ERR_ARG otherwise, when s is NULL, and when on = 1 while the Gumbel root search,
 * forced playouts or the evaluation cache are on (each has a root rule or a kernel instantiation of its own; their setters
 * refuse likewise while the solver is on).  Call it before cz_search_start_selfplay / cz_search_set_roots and before a
 * graph capture; synchronises the stream. */
#define CZ_PROOF_OPEN 0
#define CZ_PROOF_WIN 1
#define CZ_PROOF_LOSS 2
#define CZ_PROOF_DIST_MAX 255
int cz_search_set_solver(cz_search* s, int on, void* stream);
/* The proof state of the node cz_search_node_stats would report for the same path (path NULL / path_len 0: the root;
 * path_len at most 128): status [G] int8 (CZ_PROOF_*, -1 where the position is not linked in the tree) and dist [G] uint8;
 * mark [G][128] and mark_dist [G][128] uint8 (either may be NULL): per edge the status of its child as the edge holds it
 * and that child's d, 0 for an unmarked edge and past the node's edges.  All DEVICE.  Works with the solver off. */
int cz_search_node_proof(cz_search* s, const uint16_t* path, int path_len, int8_t* status, uint8_t* dist, uint8_t* mark,
                         uint8_t* mark_dist, void* stream);
/* out [G] uint8 DEVICE: 1 where the game's current root is decided, with the bans of the current ply. */
int cz_search_root_decided(cz_search* s, uint8_t* out, void* stream);
/* ---- network epilogue -----------------------------------------------------------------------------
 * x = relu?(x + bias[c] (+ residual)) in place over a channels-last activation x[rows][channels]
 * (n_elems = rows * channels, channels % 8 == 0, dtype CZ_F32 / CZ_F16 / CZ_BF16).  Replaces the separate
 * bias / add / ReLU passes that follow each trunk convolution of agent/model.py:68-83 (BatchNorm folded). */
int cz_bias_act(void* x, const void* bias, const void* residual, size_t n_elems, int channels, int dtype,
                int relu, void* stream);

/* ---- trunk convolution (hand-written MFMA kernel, csrc/xq_conv.hip) -------------------------------------------
 * Replaces Conv2D(F, 3, padding="same") -> BatchNorm -> (+ skip) -> ReLU of the residual tower
 * (agent/model.py:40-83, BatchNorm folded into w / bias) on channels-last 10x9 boards:
 *   y[n][pix][o] = act( sum_{ky,kx,c} w[o][c][ky][kx] * x[n][pix + (ky-1, kx-1)][c] + bias[o] (+ skip[n][pix][o]) )
 * Activations are [n_boards][90][channels] arrays of 2-byte elements (dtype CZ_BF16 or CZ_F16); fp32 accumulate.
 *   parts = 1: plain bf16 / fp16 operands (x_lo, skip_lo, y_lo unused).
 *   parts = 2: "split" operands -- every value is a pair hi + lo (lo = value - hi rounded again) and the kernel
 *              accumulates hi*hi + hi*lo + lo*hi: fp32-class results (product error ~2^-17) from three
 *              bf16 MFMAs.  Outputs are re-split into (y_hi, y_lo).
 * y_f32 != NULL: write the fp32 result there instead of y_hi / y_lo (last trunk layer, feeds the heads).
 * w_packed: device copy of what cz_conv3x3_pack_weights produced for the same channels / dtype / parts.
 * channels in {32, 128, 192, 256}.  skip_hi may be NULL (no residual). */
int cz_conv3x3(const void* x_hi, const void* x_lo, const void* w_packed, const float* bias, const void* skip_hi,
               const void* skip_lo, void* y_hi, void* y_lo, float* y_f32, int n_boards, int channels, int dtype,
               int parts, int relu, void* stream);
/* A whole residual block in one launch (csrc/xq_conv.hip, k_resblock):
 *   y = relu( conv3x3(relu(conv3x3(x, w1) + bias1), w2) + bias2 + x )          (agent/model.py:68-83)
 * The intermediate activation and the skip operand stay in LDS; HBM sees one read of x and one write of y.
 * Same layouts and `parts` as cz_conv3x3; y_f32 != NULL (parts = 2 only) writes the fp32 result instead of
 * (y_hi, y_lo); y may alias x.  Supported: 128 filters (parts 1 or 2), 192 / 256 filters (parts 1); anything else returns
 * CZ_ERR_ARG (use two cz_conv3x3 calls).  Bit-identical to the two-call form.
 * dtype CZ_F16C8 (128 or 192 filters, parts = 2): the c8 arithmetic -- x_lo / y_lo are c8 images, the filters are
 * cz_conv3x3_c8_pack_weights' (see cz_conv3x3_c8 below); bit-identical to two cz_conv3x3_c8 calls (k_resblock_c8,
 * k_resblock_ip_c8).  cz_input_conv (filters packed with CZ_F16, parts 2; u8 or fp32 planes) and the _q forms take the
 * same code at both filter counts, cz_resblock_heads and cz_input_resblock at 128 filters.
 * dtype CZ_F16 with parts = 2 ("f16x3": (hi, lo) fp16 pairs, 22 bits per operand) is the more exact sibling of the bf16
 * pairs at the same cost; it needs activations and folded filters inside fp16's range. */
int cz_resblock(const void* x_hi, const void* x_lo, const void* w1_packed, const float* bias1, const void* w2_packed,
                const float* bias2, void* y_hi, void* y_lo, float* y_f32, int n_boards, int channels, int dtype,
                int parts, void* stream);
/* The c8 tower arithmetic (csrc/xq_conv.hip, k_conv3x3_c8 / k_resblock_c8 / k_resblock_ip_c8, K loop csrc/xq_c8_kloop.h;
 * DESIGN section 7b; what the self-play engine requested by default until the end of round 4 -- now its bf6 sibling c6, below, with c8
 * next in the guard's chain -- and keeps where its load-time check against float64
 * allows -- a host binding these entry points directly owns that check): one 3x3 convolution, 128 or 192
 * filters (the shapes below are for 128), computed as  f16(w) f16(x) + e4m3(w) e4m3(x - f16(x)) + e4m3(w - f16(w)) e4m3(x)  (one fp16 and two block-scaled
 * fp8 matrix instructions per 64 input channels instead of three bf16 ones).  x_hi: f16 [n][90][128]; x_c8: bytes
 * [n][90][256] = e4m3(x_lo * 2^11) for the 128 channels, then e4m3(x) for them; y = conv + bias (+ skip pair) (ReLU if
 * relu), written as fp32 (y_f32) or as the operand pair (y_hi, y_c8).
 * The accumulators start at bias (+ the skip pair's value) and the products are added on top (round 4).
 * Reference arithmetic: Keras float32 (agent/model.py:32-83); per-product accuracy ~2^-16 (the split-bf16 form: 2^-17; the
 * fp16 pairs: 2^-21), two thirds of their matrix-pipe time.  Activations above 448 lose the w_lo x correction (e4m3
 * saturates): scale the folded network by a power of two first (agent/model.py choose_act_shift). */
/* Packed filter = fp16 fragments, correction fragments, 4 ints, then 2 x channels signed bytes: the correction operands'
 * power-of-two shifts PER OUTPUT CHANNEL (e4m3(w 2^s) with the row's largest magnitude in [128, 256), the same for
 * w - f16(w); c6: bf6, [8, 16)) -- the matrix instruction takes the filter operand's scale per row, so channels of very
 * different magnitude (folded BatchNorm scales) all keep their correction precision. */
size_t cz_conv3x3_c8_packed_bytes(int channels);
int cz_conv3x3_c8_pack_weights(const float* w_oihw, int channels, void* out_host);
int cz_conv3x3_c8(const void* x_hi, const void* x_c8, const void* w_packed, const float* bias,
                  const void* skip_hi, const void* skip_c8, void* y_hi, void* y_c8, float* y_f32,
                  int n_boards, int channels, int relu, void* stream);

/* The c6 tower arithmetic (round 4; k_resblock_c8<.., C6>; 128 and, since round 6, 192 filters; whole residual blocks only): the
 * c8 sum with the two correction operands in bf6 (e3m2) -- v_mfma_scale_f32_32x32x64_f8f6f4 retires bf6 operands in 32 cycles, e4m3 ones in
 * 64 (tools/probes/bf6_probe.hip), so a product costs 1.5 instead of 2.0 MFMA-equivalents; per-product accuracy ~2^-15
 * (measured on whole blocks against float64, tests/test_gpu_c6_elements.py: 2^-15.1, c8 2^-16.1, bf16x3 2^-17.3).
 * Activation images keep the c8 pair's shape (x_hi f16 [n][90][C], image bytes [n][90][2 C]); the image holds, per pixel
 * and 32-channel block, a 24-byte piece bf6((x - f16(x)) 2^(11 - k)) and a piece bf6(x 2^-k) (layout: csrc/xq_conv.hip,
 * namespace rb8), k = the image's exponent, 2^k * 28 >= max |x| (from calibration activations; the conversion rounds to
 * nearest even and saturates at 28 2^k, the lo piece at 28 2^(k - 11)).  Of a pixel's 2 C bytes the first C carry the lo
 * pieces, the last C the value pieces; piece w sits in the 24 bytes at 32 w of its half, element e (6 bits at bit 6 e) =
 * channel 32 w + 8 (e >> 3) + ((e >> 1) & 3) + 4 (e & 1).  The 8 bytes behind each piece belong to no piece: their content
 * is unspecified (kernels that stage the image in LDS copy what lies there) and no kernel reads them as data.  The value
 * the image stands for (the skip operand) is x_hi + lo6 2^(k - 11), an fp32 number; tests/c6_model.py encodes and decodes
 * the format, and the kernels' images are held to it byte for byte.
 * Filters: cz_conv3x3_c6_pack_weights(w, 128, x_exp, y_exp, out) -- same size as cz_conv3x3_c8_packed_bytes(128) -- with
 * the exponents of the image the convolution READS and of the one it WRITES; a block's w1 / w2 must agree on the
 * intermediate image's exponent, consecutive blocks on the stream image's.  Entry points (dtype CZ_F16C6): cz_resblock,
 * cz_resblock_heads, cz_input_resblock (whose gathered input image is c8: ITS w1 is cz_conv3x3_c8_pack_weights') and the
 * _q forms.  A host owns the accuracy check exactly as for c8 (agent/model.py guarded_inference_net: c6 -> c8 -> ...).
 * y_exp = 127 on a block's SECOND filter: the block writes a c8 image (y_lo of cz_resblock / cz_input_resblock is then read by
 * c8 blocks) -- the hand-over of a hybrid "c6>N" tower, whose first N blocks run c6 and the rest c8. */
int cz_conv3x3_c6_pack_weights(const float* w_oihw, int channels, int x_exp, int y_exp, void* out_host);

/* test / tuning hook: the 128-filter split residual block with operand-pair output has two schedules that give
 * bit-identical results -- k_resblock_pipe (default, 1): epilogue 2 of a board runs under the next board's first K
 * loop; k_resblock (0).  enable < 0 only queries.  Returns the previous setting. */
int cz_resblock_pipelined(int enable);
/* The LAST residual block of the tower with the two 1x1 head convolutions folded into its store pass (cz_resblock +
 * cz_head_convs in one launch; the block's activation never reaches HBM): split operands, 128 filters,
 * n_policy + n_value == 6.  Outputs as cz_head_convs. */
int cz_resblock_heads(const void* x_hi, const void* x_lo, const void* w1_packed, const float* bias1,
                      const void* w2_packed, const float* bias2, const float* head_w, const float* head_b,
                      float* policy_feat, float* value_feat, int n_boards, int channels, int dtype, int n_policy,
                      int n_value, void* stream);
/* The input layer AND the first residual block in one launch (128 filters; split operands, or dtype CZ_F16C8 with the c8
 * pair as output and cz_conv3x3_c8_pack_weights filters: k_resblock_c8<FIRST>): the 5x5 input convolution
 * (Conv2D(F, 5, "same") -> BatchNorm -> ReLU, agent/model.py:36-39) of the one-hot feature planes is a gather over the
 * occupied squares, computed in exact fp32 by the block's copy waves while its matrix waves run the previous board.
 *   planes_u8   [n_boards][in_planes][90] uint8, 0 / 1 (what the search kernel writes; in_planes 14 or 28)
 *   in_table    DEVICE fp32 [in_planes][25][128]: in_table[c][ky * 5 + kx][o] = w[o][c][ky][kx] (BatchNorm folded)
 *   in_bias     DEVICE fp32 [128]
 *   rows/n_dev  compact evaluation queue (may be NULL): board i = planes_u8[rows[i]], min(n_boards, *n_dev) boards
 * The rest as cz_resblock with operand-pair output.  Equal to cz_input_conv followed by cz_resblock up to the rounding of
 * the input layer (fp32 sums here, split-bf16 products there). */
int cz_input_resblock(const void* planes_u8, int in_planes, const float* in_table, const float* in_bias,
                      const void* w1_packed, const float* bias1, const void* w2_packed, const float* bias2, void* y_hi,
                      void* y_lo, int n_boards, int channels, int dtype, const int32_t* rows, const int32_t* n_dev,
                      void* stream);
/* (round 5) The same with the positions' OCCUPANCY BOARDS handed in: masks [n_boards or slots][96] uint32 DEVICE, word pos =
 * plane position i * 9 + j (words 90 .. 95 zero), bit c = plane c shows a piece there -- the planes' content in 384 bytes, which
 * is what the block's copy waves otherwise derive from the 1260 (2520) plane bytes before they can start the gather.
 * cz_search_leaf_masks() makes the search kernel write them beside the planes of every new leaf.  masks = NULL: exactly
 * cz_input_resblock; with masks, planes_u8 is not read (and may be NULL).  rows index both arrays alike. */
int cz_input_resblock_m(const void* planes_u8, const uint32_t* masks, int in_planes, const float* in_table,
                        const float* in_bias, const void* w1_packed, const float* bias1, const void* w2_packed,
                        const float* bias2, void* y_hi, void* y_lo, int n_boards, int channels, int dtype,
                        const int32_t* rows, const int32_t* n_dev, void* stream);
/* number of 2-byte elements of the packed filter (all parts, including the prefetch padding); 0 = bad argument */
size_t cz_conv3x3_packed_elems(int channels, int parts);
/* HOST: w_oihw[channels][channels][3][3] fp32 -> MFMA fragment order, split into parts; out_host holds
 * cz_conv3x3_packed_elems() elements */
int cz_conv3x3_pack_weights(const float* w_oihw, int channels, int dtype, int parts, void* out_host);
/* The input convolution of the network (csrc/xq_conv.hip, k_input_conv): Conv2D(F, 5, padding="same") -> BatchNorm ->
 * ReLU on the feature planes (agent/model.py:36-39), BatchNorm folded.  planes: [n_boards][in_planes][10][9] exactly as
 * cz_encode / the search kernel write them (planes_dtype CZ_F32 / CZ_F16 / CZ_BF16 / CZ_U8, in_planes 14 or 28);
 * output: the [n_boards][90][channels] operand (pair) the residual tower reads (dtype CZ_BF16 / CZ_F16, parts as in
 * cz_conv3x3 -- the 0/1 planes are exact in 2 bytes, so parts = 2 splits only the weights). */
int cz_input_conv(const void* planes, int planes_dtype, int in_planes, const void* w_packed, const float* bias,
                  void* y_hi, void* y_lo, int n_boards, int channels, int dtype, int parts, int relu, void* stream);
size_t cz_input_conv_packed_elems(int channels, int in_planes, int parts);
/* Compact-queue forms of the three kernels above (cz_search_round_q): the number of boards is min(n_boards, *n_dev)
 * with n_dev in DEVICE memory (n_boards = the capacity of the buffers = the launch shape), and the input convolution
 * reads board i from planes[rows[i]] (rows DEVICE int32, NULL = identity).  rows / n_dev may be NULL: then exactly the
 * plain function.  Threading: rows / n_dev travel to the launch through thread-local state inside the call, so each
 * call is self-contained on its thread; like every cz_* entry point these may be called from several host threads at
 * once as long as each thread uses its own stream. */
int cz_input_conv_q(const void* planes, int planes_dtype, int in_planes, const void* w_packed, const float* bias,
                    void* y_hi, void* y_lo, int n_boards, int channels, int dtype, int parts, int relu,
                    const int32_t* rows, const int32_t* n_dev, void* stream);
int cz_resblock_q(const void* x_hi, const void* x_lo, const void* w1_packed, const float* bias1, const void* w2_packed,
                  const float* bias2, void* y_hi, void* y_lo, float* y_f32, int n_boards, int channels, int dtype,
                  int parts, const int32_t* n_dev, void* stream);
/* (round 6) The chain for EVERY tower arithmetic.  A chain block's two images (the one its first convolution reads = the one the
 * block before wrote, and its intermediate image) each have a format: */
#define CZ_IMG_C8 0      /* f16 + e4m3 corrections (cz_conv3x3_c8_pack_weights filters read it) */
#define CZ_IMG_C6 1      /* f16 + bf6 pieces with an exponent (cz_conv3x3_c6_pack_weights) */
#define CZ_IMG_PAIR 2    /* (hi, lo) fp16 / bf16 pair (cz_conv3x3_pack_weights, parts = 2) */
#define CZ_EXIT_HEADS 3  /* exit only: the 1 x 1 head convolutions instead of an image */
/* cz_tower: n_blocks (1 .. 8) consecutive residual blocks of a 128-filter tower on the c8 OR the c6 arithmetic in ONE launch --
 * bit-identical to n_blocks calls of cz_resblock with the matching dtype, with the activations staying in the CU's LDS between
 * the blocks (HBM sees a board at the chain's entry and exit only).  Kernel: k_resblock_ip4_c8<128> -- a pair of boards per
 * workgroup with one LDS image each, both epilogues in place, FOUR matrix waves of two channel tiles (a pixel fragment from LDS
 * feeds two MFMAs, no copy waves).  w1_packed / bias1 / w2_packed / bias2: HOST arrays of n_blocks DEVICE pointers
 * (cz_conv3x3_c8_pack_weights / cz_conv3x3_c6_pack_weights filters; block b + 1 reads the image block b writes).  x / y: operand
 * pairs [n_boards][90][128] f16 + [n_boards][90][256] bytes.  fmt_x[b] / fmt_y[b] (HOST int arrays; NULL = all CZ_IMG_C6): the
 * format of the image block b's first / second filter reads -- one format per chain (all CZ_IMG_C8 or all CZ_IMG_C6; a hybrid
 * tower is one chain per arithmetic).  exit_fmt: what the last block's result becomes -- CZ_IMG_C6 / CZ_IMG_C8: that operand
 * pair in (y_hi, y_img) (a c6 chain whose last block carries y_exp = 127 ends on CZ_IMG_C8: the hand-over of a "c6>N" tower);
 * CZ_IMG_PAIR (c8 chains): (hi, lo) fp16 pairs, y_img = the lo array [n][90][128] f16: the hand-over of a "c8>N" tower to its
 * f16x3 blocks (cz_resblock's y_f32 + cz_split_bias_act in one); CZ_EXIT_HEADS: the head features (cz_resblock_heads'
 * outputs: policy_feat [n][n_policy * 90], value_feat [n][n_value * 90] fp32, ReLU'd; y_hi / y_img unused), the head dot
 * products summed over a pixel's four 32-channel partial sums: equal to cz_resblock_heads up to the rounding of that order.
 * n_dev: compact queue (DEVICE int32, may be NULL): min(n_boards, *n_dev) boards.  Replaces agent/model.py:41-43 for those
 * blocks. */
int cz_tower(const void* x_hi, const void* x_img, int n_blocks, const void* const* w1_packed, const float* const* bias1,
             const void* const* w2_packed, const float* const* bias2, const int* fmt_x, const int* fmt_y, int exit_fmt,
             void* y_hi, void* y_img, const float* head_w, const float* head_b, float* policy_feat, float* value_feat,
             int n_policy, int n_value, int n_boards, const int32_t* n_dev, void* stream);
/* cz_tower_pairs: the same for (hi, lo) pair blocks (f16x3 / bf16x3 arithmetic, dtype CZ_F16 / CZ_BF16; k_tower_pairs4<E, 128>,
 * the four-wave shape of k_resblock_ip4_c8): bit-identical to n_blocks calls of cz_resblock(parts = 2).  head_w != NULL: the chain ends on the tower's last block and
 * writes the head features (from hi + lo of the block's result) instead of (y_hi, y_lo). */
int cz_tower_pairs(const void* x_hi, const void* x_lo, int n_blocks, const void* const* w1_packed, const float* const* bias1,
                   const void* const* w2_packed, const float* const* bias2, void* y_hi, void* y_lo, const float* head_w,
                   const float* head_b, float* policy_feat, float* value_feat, int n_policy, int n_value, int n_boards,
                   int dtype, const int32_t* n_dev, void* stream);
/* cz_resblock_chain (round 6): n_blocks (1 .. 12) consecutive residual blocks of a 192-FILTER tower (the reference's deployed
 * width, configs/distribute.py:84-87) on one staged arithmetic -- dtype CZ_F16C8, or CZ_F16C6 (c6 blocks behind the tower's first
 * one, which reads the input layer's c8 image: cz_resblock with CZ_F16C86) -- in ONE launch: a workgroup takes a PAIR of boards
 * through all blocks, one LDS image per board (both epilogues in place), on four matrix waves of three channel tiles each -- six
 * channel tiles spread evenly over the CU's four SIMDs (k_resblock_ip4_c8; environment CZ_IP_PAIR=0: one board in two images on
 * six matrix waves, k_resblock_ip_c8).  HBM sees a board at the entry and the exit.  Bit-identical to n_blocks calls of cz_resblock.  y_f32 != NULL: the last block writes fp32 [n][90][192]
 * instead of the operand pair (the tower's last block / the hand-over of a c8>N tower).  dtype CZ_F16C86: a c6 chain that STARTS
 * the tower -- its block 0 reads the input layer's c8 image (first filter c8-packed, as for cz_resblock with CZ_F16C86), the
 * blocks behind it are c6 blocks: a 10 x 192 c6 tower is one launch.  dtype CZ_F16 / CZ_BF16: (hi, lo) PAIR
 * blocks (f16x3 / bf16x3 -- what the load-time guard gives a peaked-policy network at this width), x_img / y_img = the lo tensors
 * [n][90][192]; same shape of kernel (k_tower_pairs4<E, 192>). */
int cz_resblock_chain(const void* x_hi, const void* x_img, int n_blocks, const void* const* w1_packed, const float* const* bias1,
                      const void* const* w2_packed, const float* const* bias2, void* y_hi, void* y_img, float* y_f32, int n_boards,
                      int channels, int dtype, const int32_t* n_dev, void* stream);
/* cz_tower_plain (round 6): n_blocks (1 .. 24) consecutive residual blocks of a 256-FILTER tower on plain fp16 / bf16 operands
 * (dtype CZ_F16 / CZ_BF16, cz_conv3x3_pack_weights with parts = 1) in ONE launch -- BASELINE configs[4], the 20 x 256 fp16 tower,
 * is a single launch: a workgroup takes a PAIR of boards through all blocks with ONE LDS image per board (a filter fragment
 * feeds both boards; the intermediate activation overwrites the block's input, whose values wait as the skip operand in
 * registers / spare LDS; k_tower_plain2).  Bit-identical to n_blocks calls of
 * cz_resblock(parts = 1).  x / y: [n_boards][90][256]. */
int cz_tower_plain(const void* x, int n_blocks, const void* const* w1_packed, const float* const* bias1,
                   const void* const* w2_packed, const float* const* bias2, void* y, int n_boards, int channels, int dtype,
                   const int32_t* n_dev, void* stream);
int cz_resblock_heads_q(const void* x_hi, const void* x_lo, const void* w1_packed, const float* bias1,
                        const void* w2_packed, const float* bias2, const float* head_w, const float* head_b,
                        float* policy_feat, float* value_feat, int n_boards, int channels, int dtype, int n_policy,
                        int n_value, const int32_t* n_dev, void* stream);
/* HOST: w_oihw[channels][in_planes][5][5] fp32 -> MFMA fragment order (cz_input_conv_packed_elems() elements) */
int cz_input_conv_pack_weights(const float* w_oihw, int channels, int in_planes, int dtype, int parts, void* out_host);
/* fp32 activation x[rows][channels] (+ bias[c], may be NULL) -> ReLU? -> (y_hi, y_lo) operand pair (parts = 2) or
 * a plain bf16 / fp16 copy (parts = 1).  Used after the 5x5 input convolution. */
int cz_split_bias_act(const float* x, const float* bias, void* y_hi, void* y_lo, size_t n_elems, int channels,
                      int dtype, int parts, int relu, void* stream);

/* The two 1x1 head convolutions (policy Conv2D(4,1), value Conv2D(2,1), BatchNorm folded, ReLU; agent/model.py:56-63)
 * in one streaming pass over the trunk output x[n_boards][90][channels] (dtype CZ_F32 / CZ_F16 / CZ_BF16):
 *   w[n_policy + n_value][channels] fp32 (policy filters first), bias[n_policy + n_value] fp32;
 *   policy_feat[n_boards][n_policy * 90], value_feat[n_boards][n_value * 90] fp32 in channels-first Flatten order.
 * n_policy + n_value must be 6 (the reference's 4 + 2). */
int cz_head_convs(const void* x, int dtype, const float* w, const float* bias, float* policy_feat, float* value_feat,
                  int n_boards, int channels, int n_policy, int n_value, void* stream);

/* The dense tail of both heads (agent/model.py:58-59 and :64-66: Flatten -> Dense(2086, softmax); Flatten -> Dense(256,
 * relu) -> Dense(1, tanh)) on the head features cz_head_convs / cz_resblock_heads produce, in three launches of
 * hand-written kernels (csrc/xq_heads.hip: split-bf16 MFMA GEMM tiles of 64 positions with the softmax statistics
 * kept per lane, one normalising pass, the value head with its hidden layer in the accumulators).
 *   policy_feat[n][n_policy_feat], value_feat[n][n_value_feat]   fp32 (180 or 360 features each: 2 or 4 head filters)
 *   wp_packed / w1_packed    cz_fc_pack_weights() of the [n_labels][n_policy_feat] / [n_hidden][n_value_feat] matrices
 *   bias_p[n_labels], bias1[n_hidden], w2[n_hidden], b2          fp32 (n_labels even)
 *   policy[n][n_labels] (softmax), value[n] (tanh)               fp32 outputs
 *   stats_scratch            DEVICE scratch of 2 * n_boards floats (the rows' max / sum of exp between the launches)
 *   n_dev                    NULL, or the DEVICE int32 count of the compact evaluation queue: only the first
 *                            min(*n_dev, n_boards) rows are computed and written
 *   dtype                    the element type of the packed pairs (the one given to cz_fc_pack_weights): CZ_BF16 or CZ_F16
 *   normalize                1: policy = softmax (the reference's output).  0: policy keeps the raw LOGITS and the pass over
 *                            all n_labels columns is skipped -- for a queue consumed by a search with
 *                            cz_search_policy_logits(h, 1), which needs the legal moves' entries only
 * Precision: operands as (hi, lo) pairs, three MFMAs per product, fp32 accumulation -- the tower's arithmetic: 2^-17 per
 * product with bf16 pairs, 2^-21 class with fp16 pairs (22 bits per operand; the head features are O(1), well inside
 * fp16's range, and the matrix unit honours fp16 subnormals -- tools/f16x3_probe.py).
 * Range: the features are split into pairs inside the kernel and nothing checks them.  CZ_F16: |feature| < 65 504 (fp16's
 * largest value; a larger feature becomes inf and the row's outputs NaN); the per-element bounds are tested up to 3.0e4
 * (tests/test_gpu_heads.py).  CZ_BF16: fp32's whole range.  A search guard's activation_max covers the tower only, not these
 * features.  Shapes: n_labels may be any even number >= 2 and n_hidden any number >= 1 (partial and odd counts of 32-wide
 * label tiles included); only the feature counts are fixed to 180 or 360. */
int cz_heads_tail(const float* policy_feat, int n_policy_feat, const void* wp_packed, const float* bias_p,
                  int n_labels, const float* value_feat, int n_value_feat, const void* w1_packed, const float* bias1,
                  int n_hidden, const float* w2, float b2, float* policy, float* value, float* stats_scratch,
                  int n_boards, int dtype, int normalize, const int32_t* n_dev, void* stream);
/* number of 2-byte elements of a packed dense layer (0 = bad argument); HOST: w[n_out][n_in] fp32 -> (hi, lo) pairs of
 * `dtype` (CZ_BF16 / CZ_F16) in fragment order */
size_t cz_fc_packed_elems(int n_out, int n_in);
int cz_fc_pack_weights(const float* w, int n_out, int n_in, int dtype, void* out_host);

/* test hook: out[n] (DEVICE, float64) = n draws of the root noise np.random.dirichlet(alpha * ones(n_moves))[0]
 * (agent/player.py:304) from the generator the search kernel uses (k_noise; csrc/xq_noise.h: counter-based integer
 * hash keyed by seed / game_key, float32 Marsaglia-Tsang Gamma draws) */
int cz_debug_noise(uint64_t seed, uint32_t game_key, double alpha, int n_moves, double* out, int n, void* stream);
/* test hook: y[i] = sqrt((double)(x[i] + 1)) exactly as the PUCT kernel computes it */
int cz_debug_sqrt(const int32_t* x, double* y, int n, void* stream);

/* ---- trainer data path and loss (csrc/xq_train.hip; run.py opt, cchess_alphazero/worker/optimize.py) ----------------
 * Replaces the reference trainer's expanding_data / convert_to_trainging_data (worker/optimize.py:234-281) and the Keras
 * loss of compile_model (:139-146).  A "window" is n_pos positions in game-major order (game 0's plies, then game 1's ...:
 * the order expanding_data produces). */

/* Replay every game of a batch of records, one wavefront per game.  init_boards[n_games][90]: each game's initial board;
 * labels[n_pos]: the move labels of all games flat; offsets[n_games + 1] (DEVICE): game g owns positions
 * offsets[g] .. offsets[g+1]-1, offsets non-decreasing, offsets[n_games] <= n_pos.
 * Writes boards[n_pos][90] (the position BEFORE each move, flipped to its mover exactly as cz_step flips: the same
 * step_board code, so every board equals cz_step's bit for bit), prev[n_pos] (the index of the position two plies
 * earlier in the same game -- the history[-5] of state_history_to_planes --, -1 for a game's first two positions) and
 * bad_ply[n_games]: -1, or the ply (0-based within the game) of the first move with a bad label or an empty from-square
 * (the reference raises ValueError there); the game's later boards repeat the board at that ply.  bad_ply[g] = -2: the
 * game's offsets are out of order or beyond n_pos, nothing of it is written. */
int cz_replay_games(const int8_t* init_boards, const uint16_t* labels, const int32_t* offsets, int n_games, int n_pos,
                    int8_t* boards, int32_t* prev, int32_t* bad_ply, void* stream);

/* Minibatch gather fused with the encoding, one wavefront per row: planes[n_rows][depth][10][9] float32 for the window
 * positions idx[n_rows].  Planes 0-13 are state_to_planes of boards[idx[r]], bit-identical to cz_encode(CZ_F32) (the
 * same wave_encode); depth 28 adds planes 14-27 = the encoding of boards[prev[idx[r]]], zero when prev is -1
 * (state_history_to_planes).  An index outside [0, n_pos) gives zero planes.  prev may be NULL for depth 14. */
int cz_gather_planes(const int8_t* boards, const int32_t* prev, int n_pos, const int32_t* idx, int n_rows, int depth,
                     float* planes, void* stream);
/* The same kernel with a per-row mirror flag (run.py opt --augment mirror).  mirror[n_rows] (DEVICE, uint8) or NULL = no
 * row flagged = cz_gather_planes, bit for bit.  A row with a nonzero flag gets the planes of the left-right mirrored
 * position: planes_m[r][p][y][x] == planes[r][p][y][8 - x] for all 14 or 28 planes, exactly (the board is mirrored in LDS
 * and encoded by the same wave_encode; at depth 28 the position two plies back is mirrored too, a missing one stays
 * zero).  An index outside [0, n_pos) gives zero planes whatever its flag. */
int cz_gather_planes_m(const int8_t* boards, const int32_t* prev, int n_pos, const int32_t* idx, const uint8_t* mirror,
                       int n_rows, int depth, float* planes, void* stream);

/* Policy / value loss of a minibatch and its gradients, one wavefront per row, no atomics: per-row outputs, so a sum
 * over them on the host side is deterministic.
 *   logits[n_rows][ld] fp32 (ld >= 2086), v[n_rows] = the value head after tanh, idx[n_rows] = window positions;
 *   window targets: played[n_pos] (labels), z[n_pos] (values), and for mode 1 the visit counts in CSR form:
 *   row_ptr[n_pos + 1], vis_label[nnz], vis_count[nnz] (>= 0; the labels of one row distinct).  With nnz = 0 the three
 *   may be NULL and every row takes the one-hot; a row whose span row_ptr[i] .. row_ptr[i+1] is not inside [0, nnz)
 *   counts as a row without visits (nothing outside the arrays is read).
 * Target t: mode 1 (visits) on a row whose counts sum to more than 0: t_k = count_k / sum, divided in float64 and rounded
 * once to float32 (the bits of lib/record_decoder._visit_targets); otherwise (mode 0 played, or no visits) the one-hot
 * of played.  p = softmax(logits) in fp32 after subtracting the row max; eps = 1e-7f, hi = float(1 - 1e-7).
 *   policy_loss[r] = -sum_k t_k log(clip(p_k, eps, hi))      (Keras 2.0.8 categorical_crossentropy of the softmax)
 *   value_sqerr[r] = (v - z)^2
 *   grad_logits[r][2086] = (w_p / n_rows) (p_j S - t_j m_j), m_j = 1 where eps < p_j < hi else 0, S = sum_k t_k m_k
 *                          (the exact gradient of the clipped loss through the softmax)
 *   grad_v[r] = w_v 2 (v - z) / n_rows
 * The gradients are those of w_p mean(policy_loss) + w_v mean(value_sqerr).  An index outside [0, n_pos) gives zeros. */
int cz_policy_value_loss(const float* logits, int ld, const float* v, const int32_t* idx, int n_rows, int n_pos,
                         const int32_t* row_ptr, const uint16_t* vis_label, const int32_t* vis_count, int nnz,
                         const uint16_t* played, const float* z, int mode, float w_p, float w_v, float* policy_loss,
                         float* value_sqerr, float* grad_logits, float* grad_v, void* stream);
/* The same kernel with the per-row mirror flag of cz_gather_planes_m (mirror[n_rows] DEVICE uint8, or NULL = no row flagged =
 * cz_policy_value_loss, bit for bit).  A flagged row's policy target is the unflagged row's with every label sent through
 * cz_label_mirror's map: the played label in mode 0 and in the no-visits fallback, every vis_label entry in mode 1; the
 * counts, their float64 total and the quotients are untouched, and so are the value target, the clip, the softmax and the
 * gradient formulas.  So a flagged row gives the bits of an unflagged row of a window holding the mirrored game's record. */
int cz_policy_value_loss_m(const float* logits, int ld, const float* v, const int32_t* idx, const uint8_t* mirror, int n_rows,
                           int n_pos, const int32_t* row_ptr, const uint16_t* vis_label, const int32_t* vis_count, int nnz,
                           const uint16_t* played, const float* z, int mode, float w_p, float w_v, float* policy_loss,
                           float* value_sqerr, float* grad_logits, float* grad_v, void* stream);
/* The same kernel with a mixed value target (run.py opt --q-ratio L; the value record of cz_search_record_values):
 * q[n_pos] (DEVICE float32, NaN = the position has no search value) and q_ratio = L.  The row's value target is
 *       t = z + L * (q - z)
 * formed in float32 as a rounded difference, a rounded product and a rounded sum -- no fused multiply-add, so NumPy
 * float32 reproduces it bit for bit -- and t = z where q is NaN; value_sqerr = (v - t)^2, grad_v = w_v 2 (v - t) / n_rows.
 * q = NULL or q_ratio = 0 takes the path of cz_policy_value_loss_m, bit for bit; the two entries above forward here
 * with NULL.  The policy outputs never depend on q, and q does not change under the mirror.  CZ_ERR_ARG also for a
 * q_ratio outside [0, 1] (NaN included). */
int cz_policy_value_loss_q(const float* logits, int ld, const float* v, const int32_t* idx, const uint8_t* mirror, int n_rows,
                           int n_pos, const int32_t* row_ptr, const uint16_t* vis_label, const int32_t* vis_count, int nnz,
                           const uint16_t* played, const float* z, const float* q, float q_ratio, int mode, float w_p,
                           float w_v, float* policy_loss, float* value_sqerr, float* grad_logits, float* grad_v,
                           void* stream);
/* The same kernel with a training weight per row (run.py opt --surprise-weight A): row_w[n_pos] (DEVICE float32,
 * indexed by window position like z and q).  The weight scales the row's share of the gradients only: the scale of row
 * r with i = idx[r] is __fmul_rn(w_p / n_rows, row_w[i]) for grad_logits and grad_v[r] is its unweighted value times
 * row_w[i], each one rounded product -- a weight of 1.0f gives the unweighted bits.  policy_loss[r] and value_sqerr[r]
 * stay the row's unweighted values.  The division stays by n_rows, not by the sum of the weights: the weights average 1
 * over a game, which matches replicating rows in proportion to their weight in expectation.  row_w = NULL takes the
 * path of cz_policy_value_loss_q, bit for bit; the entries above forward here with NULL.  A weight that is negative or
 * not finite is the caller's error and is not checked here. */
int cz_policy_value_loss_w(const float* logits, int ld, const float* v, const int32_t* idx, const uint8_t* mirror, int n_rows,
                           int n_pos, const int32_t* row_ptr, const uint16_t* vis_label, const int32_t* vis_count, int nnz,
                           const uint16_t* played, const float* z, const float* q, float q_ratio, const float* row_w, int mode,
                           float w_p, float w_v, float* policy_loss, float* value_sqerr, float* grad_logits, float* grad_v,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
