// xq_search.h -- device-side data layout of the batched PUCT-MCTS engine (gfx950).
//
// One wavefront per game tree.  The reference keeps a game's whole tree for the whole game
// (worker/self_play.py:84,98-100); 4096 games x 800 simulations x ~150 plies is ~130 GB of tree, which is what
// the 288 GB of HBM are for.  Trees live in a POOL of 1 MiB chunks shared by all games of the search object:
//   * a game owns a list of chunks (g_chunk_tab) and bump-allocates variable-size records in them; a record is
//     addressed by a 32-bit id = local chunk number << 16 | 16-byte granule inside the chunk;
//   * NODE record  = 48 B packed position | 16 B header {sum_n, move count | flags, stat id, net value} | float p[nm] |
//     uint16 move[nm]: everything a wave needs to price a node's edges is one contiguous run;
//   * STAT block   = nm x 16 B {double W, int32 N, int32 child}: allocated only when a node is first selected
//     FROM (two nodes in three are leaves that never are), edge j of a node = granule stat + j, so an edge id is a
//     record id as well and a path entry is one word; while the moves-left utility is on (cz_search_set_moves_left) the
//     block is 2 nm granules: nm M records {int64 ksum, int32 mn, int32 spare} follow, edge j's at granule stat + nm + j
//     (xq_search_ml.h), and header word 3 holds the node's own prediction in quanta instead of the net value; while the
//     draw average is on (cz_search_set_draw) the same granules hold nm D records {int64 dsum, int32 dn, int32 spare}
//     and the same word the node's own draw probability in quanta (xq_search_draw.h); while the lower-confidence-bound move
//     choice is on (cz_search_set_lcb) they hold nm V records {double s2, int32 vn, int32 spare} (xq_search_var.h): the three
//     options exclude each other;
//   * chunks are taken from / returned to a device-side free ring (pool_* below) between plies and between games,
//     never inside the simulation kernel: begin_search reserves the worst case of the coming ply.
// The hot scratch (boards, ordered move lists, the current path, the game's chunk table) lives in LDS.
//
// Reference objects replaced (cchess_alphazero/agent/player.py):
//   VisitState (:17-25)  -> node record          ActionState (:28-33) -> p / move in the node record + stat block
//   tree = defaultdict keyed by state string (:49) -> per-game open-addressing hash on the packed board
//   history lists of MCTS_search (:198-260)        -> s_path_* per simulation slot
#pragma once
#include <stdint.h>

namespace xq {

constexpr int KEY_WORDS = 12;          // 90 squares x 4 bit, padded to 48 B
constexpr int MAX_NO_ACT = 32;         // banned root moves per ply (self_play.py:161-175); longer lists are refused by the host
constexpr int CHUNK_SHIFT = 16;        // granules (16 B) per chunk = 65536 -> 1 MiB chunks
constexpr int CHUNK_GRANULES = 1 << CHUNK_SHIFT;
constexpr size_t CHUNK_BYTES = (size_t)CHUNK_GRANULES * 16;
constexpr int MAX_CHUNKS = 256;        // per game (LDS copy of the chunk table): 256 MiB of tree per game at most
constexpr int NODE_HDR_GRANULES = 4;   // key (3) + header (1)
constexpr int RESERVE_MOVES = 80;      // moves per new node the per-ply reservation assumes (observed maximum 70)
constexpr int CHILD_UNKNOWN = -1;
constexpr int CHILD_TERM_WIN = -2;     // done() == (True, +1): value for the child's mover +1 -> x2
constexpr int CHILD_TERM_LOSS = -3;    // done() == (True, -1)
// MCTS solver (cz_search_set_solver): a child link that names a node (>= 0) is a 24-bit node id (MAX_CHUNKS x 65536
// granules) with the edge mark above it -- the Proof of the child as last seen at a backup over the edge.  Every reader of
// `child` strips the mark (child_id in xq_search_solver.h); the terminal codes are their own marks.
constexpr int CHILD_ID_MASK = 0x00FFFFFF;
constexpr int CHILD_MARK_SHIFT = 24;
enum Proof : int { PROOF_OPEN = 0, PROOF_WIN = 1, PROOF_LOSS = 2 };   // a position's status, from its mover's view
constexpr int PROOF_DIST_MAX = 255;    // plies to the terminal position along a line the tree holds: saturates here
static_assert(MAX_CHUNKS * CHUNK_GRANULES <= CHILD_ID_MASK + 1, "a node id has to fit below the edge mark");

enum SimState : uint8_t { SIM_IDLE = 0, SIM_LEAF = 1, SIM_PARKED = 2,
                          SIM_DEFERRED = 3,     // ended on a terminal / repeated position; backed up when the phase's descents are over (never outlives a launch)
                          SIM_CACHED = 4 };     // a new leaf whose evaluation the cache held (cz_search_set_eval_cache): priors in the node, value in
                                                // s_cval; no queue row, attached with the SIM_LEAF slots of the next round

enum NodeFlag : uint32_t { NODE_WAITING = 1u << 8,      // low 8 bits of node_meta = move count
                           NODE_MIRRORED = 1u << 9 };   // set beside NODE_WAITING: the leaf is evaluated in its mirror image
                                                        // (cz_search_set_leaf_mirror); cleared with it when the priors attach
// MCTS solver: the node's Proof in bits 10-11 of node_meta and its distance in bits 16-23, written once (a first proof is
// final) by lane 0 like the rest of the header; 0 = OPEN, so a tree grown with the solver off holds OPEN nodes only
constexpr int NODE_PROOF_SHIFT = 10, NODE_DIST_SHIFT = 16;

enum GameMode : int { MODE_EXTERNAL = 0, MODE_SELFPLAY = 1 };

enum GamePhase : uint8_t {
    PH_IDLE = 0,        // nothing to do (external mode: waiting for set_roots / choose)
    PH_SEARCH = 1,      // simulations outstanding for the current root
    PH_READY = 2,       // search of the current root complete (external mode: results can be read)
};

// per-game counters (uint64 each); summed on the host
enum Counter : int {
    CT_SIMS = 0, CT_EXPANSIONS, CT_TERMINAL_SIMS, CT_REPETITION_SIMS, CT_PARKED, CT_SUM_DEPTH, CT_MAX_DEPTH,
    CT_EDGES_VISITED, CT_LEAF_MOVES, CT_PLIES, CT_GAMES, CT_RED_WINS, CT_BLACK_WINS, CT_DRAWS, CT_RESIGNS,
    CT_TREE_RESETS, CT_OVERFLOW_SIMS, CT_DEPTH_OVERFLOW, CT_ROOT_REUSED_SIMS, CT_RING_DROPPED, CT_CHUNKS_TAKEN,
    CT_STAT_BLOCKS,
    CT_NO_ACT_TRUNCATED,    // self-play: a perpetual-check ban that did not fit the MAX_NO_ACT list of the ply (dropped, counted)
    CT_PROVEN_SIMS,         // MCTS solver: descents that ended on a proven node (worth +-2, no network row)
    CT_PROOFS,              // MCTS solver: nodes that became WIN or LOSS
    CT_DECIDED_PLIES,       // MCTS solver: plies whose remaining simulations a decided root cut
    CT_KLD_PLIES,           // KLD-gain stop (cz_search_set_kld_gain): plies it ended
    CT_KLD_SIMS_CUT,        // ... and the simulations of those plies that were never started
    CT_LEAD_PLIES,          // unreachable-lead stop (cz_search_set_smart_pruning): plies it ended
    CT_LEAD_SIMS_CUT,       // ... and the simulations of those plies that were never started
#ifdef CZ_SIM_PROFILE       // tuning build (tools/ab_search.sh): shader-clock cycles of wave time per section of a simulation
    CT_CYC_SELECT, CT_CYC_RULES, CT_CYC_HASH, CT_CYC_EXPAND, CT_CYC_REP, CT_CYC_ATTACH, CT_CYC_RESUME_LOAD,
    CT_CYC_KERNEL_SELECT, CT_CYC_KERNEL_BACKUP,
#endif
    CT_COUNT
};
// Counters a running kernel accumulates in LDS (SearchLDS.ctr; counters_begin / counters_flush walk them).  The stop rules'
// four count at most once per ply and go straight to the game's global block (count_direct), so the LDS layout -- and with
// it the text of every kernel that existed before them -- stays what it was.  The tuning build keeps everything in LDS.
#ifdef CZ_SIM_PROFILE
constexpr int CT_LDS_COUNT = CT_COUNT;
#else
constexpr int CT_LDS_COUNT = CT_KLD_PLIES;
#endif

struct SearchParams {
    // sizes
    int G, K, sims, vl;
    int hash_cap, max_depth, max_plies;
    int n_chunks;           // chunks in the pool
    int max_chunks;         // chunk-table entries per game (<= MAX_CHUNKS)
    int keep_chunks;        // chunks a game never gives back: enough for one full search on an empty tree
    int max_batches;        // lock-step batches one k_sim launch may start for a game
    int planes_dtype;
    int in_planes;          // 14, or 28 with use_history
    int mode;
    // PUCT / game parameters (reference config.play.*)
    double c_puct;
    float c_puct_f32;
    double noise_eps;
    float one_minus_eps_f32;
    double dirichlet_alpha;
    double tau_decay_rate;
    double resign_threshold;
    int min_resign_turn;
    int evaluate;
    int max_game_length;
    double enable_resign_rate;
    uint64_t seed;
    uint32_t game_id_stride;
    int ring_cap;
    int record_stride;      // bytes per finished-game record
    int policy_logits;      // the network rows hold raw LOGITS (cz_search_policy_logits): priors = exp(l - max over the
                            // node's moves), then the usual renormalisation over them
    // start-position book of self-play (cz_search_set_book); read by new_game / emit_record only
    int book_n;             // positions in the book, 0 = none: every game starts from INIT_STATE
    double book_rate;       // a game starts from the book iff philox_uniform(seed, game_id, 0, 2) < book_rate
    const int8_t* book;     // [book_n][90] boards in the mover's frame, owned by the search object
    // playout cap randomization of self-play (cz_search_set_playout_cap); read through ply_is_fast only
    int fast_sims;          // simulations of a fast ply, 0 = off: every ply is a full search of `sims`
    double full_rate;       // ply `turns` is a full search iff philox_uniform(seed, game_id, 2, turns) < full_rate
    // forced playouts + policy target pruning (cz_search_set_forced_playouts); read by k_sim's root context, emit_visits
    // and k_root_records only
    double forced_k;        // 0 = off; a tried root child is visited at least sqrt(forced_k * p * N) times
    // random leaf mirror (cz_search_set_leaf_mirror); read through leaf_coin only
    double leaf_mirror;     // 0 = off; a new leaf is evaluated mirrored iff philox_uniform(seed, key, 3, turns << 32 | node id) < leaf_mirror
    // Gumbel root search with sequential halving (cz_search_set_gumbel); read by begin_search, k_sim's root context,
    // k_noise, choose_action, emit_visits and k_root_records only
    int gumbel_m;           // 0 = off; candidates sampled without replacement at the root (<= GUMBEL_MAX_M)
    double gumbel_visit;    // c_visit of sigma(x) = (c_visit + max_b n_b) * c_scale * x
    double gumbel_scale;    // c_scale
    // full Gumbel search (cz_search_set_gumbel_full).  On the device only select_edge<GUM> reads it (the GUM
    // instantiations of k_sim); the host reads it to launch the FULL instantiations of k_advance and k_root_records, which
    // hold the full target (search_round_impl, launch_root_records).  While gumbel_m > 0 every attach keeps the leaf's
    // network value in word 3 of the node header (float32, the node's mover's view; a node attached while gumbel_m = 0
    // keeps expand_node's 0).
    int gumbel_full;        // 0 = off; 1: below the root argmax pi'(a) - N(a) / (1 + sum N) replaces PUCT, and the policy
                            // target completes the unvisited edges with v_mix instead of the visited edges' mean
    // MCTS solver (cz_search_set_solver); read by the host alone, which launches the SOLVE instantiations of k_sim, k_advance
    // and k_choose while it is on
    int solver;             // 0 = off
    // c_puct schedule (cz_search_set_cpuct_schedule); read through cpuct_of only: select_edge, select_solve and the callers of
    // prune_targets
    double cpuct_factor;    // F, 0 = off: the exploration constant is c_puct at every visit count
    double cpuct_base;      // B >= 1
    // policy temperature (cz_search_set_policy_temperature); read where a logit row becomes weights (prior_norm's callers)
    float inv_temp;         // (float)(1 / T), 1 = off
};
constexpr int GUMBEL_MAX_M = 128;

struct SearchBuffers {
    // ---- optional caller-owned output (cz_search_leaf_masks): one 96-word occupancy board per queue slot ----
    uint32_t* leaf_masks;   // [G*K][96] or NULL
    int leaf_planes_off;    // cz_search_leaf_planes(0): with leaf_masks set, the planes of a new leaf are NOT written
    // ---- optional caller-owned output (cz_search_set_leaf_mirror): 1 = the slot's leaf was written mirrored ----
    uint8_t* leaf_flags;    // [G*K] or NULL
    // ---- trees ----
    char* pool;             // [n_chunks] x 1 MiB
    uint32_t* pool_ring;    // [n_chunks] free chunk numbers; entries [head, tail) are free
    unsigned int* pool_head;     // [1] chunks ever taken      (monotonic; ring index = value % n_chunks)
    unsigned int* pool_tail;     // [1] chunks ever returned + the initial fill
    unsigned int* pool_tail_vis; // [1] pool_tail as of the last kernel boundary: takers stay below it
    uint32_t* g_chunk_tab;  // [G][max_chunks] pool chunk number of the game's local chunk i
    int32_t* g_nchunks;     // [G]
    uint32_t* g_heap_top;   // [G] next free granule (record id); 1 on an empty tree (id 0 = none)
    uint64_t* hash_tab;     // [G][hash_cap]  tag << 32 | node id + 1, 0 = empty
    int32_t* g_node_count;  // [G]
    // ---- search state, per game ----
    int32_t* g_root;        // [G] node index of the root, -1 = not in the tree yet
    int8_t* g_board;        // [G][96] current root position (int8 board)
    int32_t* g_tasks_left;  // [G] simulations of this ply not yet launched
    int32_t* g_active;      // [G] simulations of the current batch that have not backed up
    uint8_t* g_phase;       // [G]
    int32_t* g_turns;       // [G]
    uint16_t* g_no_act;     // [G][MAX_NO_ACT]
    uint8_t* g_n_no_act;    // [G]
    uint8_t* g_increase_temp;  // [G]
    // ---- simulation slots, per game x K ----
    uint8_t* s_state;       // [G][K]
    int32_t* s_depth;       // [G][K]
    int32_t* s_node;        // [G][K]  leaf / parked node
    int32_t* s_path_node;   // [G][K][max_depth]
    int32_t* s_path_edge;   // [G][K][max_depth]
    // ---- game loop (self-play mode), per game ----
    uint32_t* g_game_id;    // [G]
    uint8_t* g_enable_resign;  // [G]
    int32_t* g_no_eat;      // [G]
    uint32_t* g_hist_key;   // [G][max_plies + 2][12]
    uint64_t* g_hist_hash;  // [G][max_plies + 2] hash of the key (repetition scan: 64 plies per ballot)
    uint16_t* g_hist_act;   // [G][max_plies + 2]
    // ---- outputs ----
    unsigned long long* counters;   // [G][CT_COUNT]
    uint8_t* ring;          // [ring_cap][record_stride]
    unsigned int* ring_tail;       // [1] total records ever written
    int32_t* g_last_action; // [G] external mode: result of choose
    int32_t* pending;       // [1] scratch for cz_search_pending
    double* noise;          // [G][K][128] Dirichlet(alpha)[0] draws for the root edges, refreshed by k_noise
    uint32_t* g_noise_epoch;   // [G]
    int8_t* g_prev_board;   // [G][96] game position two plies before the root (action(hist=...), 28-plane input)
    uint8_t* g_hist_kind;   // [G] 0 no game history, 1 g_prev_board valid, 2 history too short
    int32_t* s_qrow;        // [G][K] compact evaluation-queue row of the slot's leaf (cz_search_round_q), -1 none
    // ---- Gumbel root search (cz_search_set_gumbel), per game; untouched while the option is off ----
    int32_t* g_started;     // [G][128] selections of this ply that took root edge j (zeroed by begin_search)
    double* g_gumbel;       // [G][128] the ply's Gumbel draws g_j, drawn by begin_search
    int32_t* g_budget;      // [G] the ply's simulation budget n: `tasks` of begin_search
};

// finished-game record header (followed by uint16 moves[max_plies + 2])
struct GameRecord {
    uint32_t game_id;
    int32_t turns;
    int32_t value;      // from red's view: +1 red won, -1 black won, 0 draw (self_play.py:190-191)
    uint32_t flags;     // bit 0 store, bit 1 resigned, bit 2 (visit recording on only) an entry of the game was dropped;
                        // bits 3-4 (a script set only) GAME_SCRIPTED, GAME_SCRIPT_MISMATCH;
                        // bits 8-31: book index + 1 of the game's start position, 0 = INIT_STATE (cz_search_set_book)
};
constexpr uint32_t GAME_VISITS_LOST = 4u;
constexpr uint32_t GAME_SCRIPTED = 8u;          // flags bit 3: the game walked a script (cz_search_set_script)
constexpr uint32_t GAME_SCRIPT_MISMATCH = 16u;  // flags bit 4: ... and ended on a mismatch (store = 0)
constexpr int GAME_BOOK_SHIFT = 8;
constexpr int BOOK_MAX = (1 << 24) - 2;    // positions a book may hold: what the 24-bit index + 1 field can name
constexpr uint16_t MOVE_FAST = 0x8000;     // record moves[i], bit 15: ply i was a fast search (cz_search_set_playout_cap);
                                           // labels are below 2086.  Never set on the appended king capture

// ---- root visit record of self-play (cz_search_record_visits) ----
// One entry per searched ply, written by k_advance right after the move is chosen: the root's edges in edge order
// (get_legal_moves order, the reference's node.a), each with its exact visit count.  Fixed-stride entries in a ring
// that is never overwritten: an entry that finds the ring full is dropped and counted.  The buffers reach k_advance
// as an argument of its own (SearchParams / SearchBuffers go to every search kernel and stay as they are).
constexpr int VISIT_MAX_EDGES = 128;               // = MAXMOVES
constexpr uint16_t VISIT_BANNED = 0x8000;          // label bit: the edge is in the ply's no_act list
constexpr uint32_t VISIT_RESIGN = 1u;              // entry flag: the player resigned at this ply
constexpr uint32_t VISIT_FAST = 2u;                // entry flag: the ply was a fast search (cz_search_set_playout_cap)
constexpr uint32_t VISIT_PRUNED = 4u;              // entry flag: n[] holds the PRUNED counts (cz_search_set_forced_playouts)
constexpr uint32_t VISIT_GUMBEL = 8u;              // entry flag: n[] holds the Gumbel policy target scaled to 65536 (cz_search_set_gumbel)
constexpr uint32_t VISIT_EARLY = 16u;              // entry flag: a stop rule ended the ply before its budget (cz_search_set_kld_gain, _smart_pruning)
constexpr uint32_t VISIT_NO_RESIGN = 32u;          // entry flag (max-q record on only): the game plays on without resignation (cz_search_record_maxq)
struct VisitEntryHdr {                             // followed by uint16 label[128], then int32 n[128]
    uint32_t game_id;
    uint16_t ply;       // turns when the move was chosen
    uint8_t n_edges;
    uint8_t flags;
    int32_t sum_n;      // the root's own visit count
    uint32_t raw_total; // VISIT_PRUNED / VISIT_GUMBEL: sum of the raw counts of the non-banned edges; otherwise 0
};
constexpr int VISIT_STRIDE = (int)sizeof(VisitEntryHdr) + 2 * VISIT_MAX_EDGES + 4 * VISIT_MAX_EDGES;   // 784 B
constexpr double SURPRISE_R_FLOOR = 1e-30;          // floor of the normalised prior in root_surprise (czero.h): s <= ln 1e30 < 70

struct VisitRing {
    uint8_t* ring;                  // [cap][VISIT_STRIDE]; NULL = recording off
    unsigned int* ctl;              // [0] entries ever reserved, [1] entries the host has drained (written between launches)
    unsigned long long* dropped;    // [1] entries that found the ring full
    uint8_t* g_lost;                // [G] the game in slot g lost an entry (or started before recording was switched on)
    unsigned int cap;
    // value record (cz_search_record_values): the root's search value of the entry in the same slot, a ring of its own
    // because the 784-byte entry has no free word; written by emit_visits in the entry's reservation
    double* q;                      // [cap]; NULL = off
    // surprise record (cz_search_record_surprise): KL(recorded counts || noise-free priors) of the same entry, likewise
    double* s;                      // [cap]; NULL = off
    // max-q record (cz_search_record_maxq): the number the ply's resignation test compared, likewise; while it is on the
    // entries of games that play on without resignation carry VISIT_NO_RESIGN
    double* mq;                     // [cap]; NULL = off
};

// ---- early stop of a settled ply (cz_search_set_kld_gain, cz_search_set_smart_pruning; csrc/xq_search_stop.h) ----
// The rules' parameters and their per-game state, allocated only while a rule is on.  Like the visit ring it reaches the
// kernels that use it (k_sim_stop, k_advance_stop, k_stop_reset) as an argument of its own.
struct StopState {
    double gain;            // G of the KLD-gain rule, 0 = that rule is off
    int interval;           // I: new root visits between two checkpoints
    int lead;               // 1 = the unreachable-lead rule is on
    int32_t* prev_n;        // [G][128] m_j: the root's visit counts at the ply's last checkpoint, in edge order
    int32_t* prev_sum;      // [G] M, their sum; -1 = the snapshot is empty
    int32_t* start_tasks;   // [G] g_tasks_left at the ply's first test point; -1 = the ply has not reached one yet
    double* last_gain;      // [G] the last measured g of the ply, NaN = none
    int32_t* checks;        // [G] checkpoints of the ply, the one that took the first snapshot included
    uint8_t* cut;           // [G] the rule that ended the ply: 0 none, 1 KLD gain, 2 unreachable lead
};

// ---- scripted games (cz_search_set_script; advance_game<SCRIPT>, new_script_game) ----
// Game id i < n walks script i: from boards[i] it plays labels[offsets[i] .. offsets[i + 1]) and ends with z[i].  Device copies
// the search object owns.  Like the visit ring it reaches the kernels that use it (k_advance_script, k_start_script) as an
// argument of its own.
struct ScriptState {
    const int8_t* boards;       // [n][90], first mover's frame
    const uint16_t* labels;     // [offsets[n]]
    const int32_t* offsets;     // [n + 1]
    const int8_t* z;            // [n] the game's result from its first mover's view
    unsigned long long* mismatches;   // [1] the counter script_mismatch: games that ended on a move their position does not have
                                      // or on moves left over after the rules ended them.  Beside the scripts like the visit
                                      // ring's `dropped`: enum Counter is what every kernel's counter block is sized by
    int n;                      // 0 = off
};

}  // namespace xq
