// xq_search.hip -- batched PUCT-MCTS + self-play game loop for gfx950, one wavefront per game.
//
// Replaces, for thousands of concurrent games, the reference's per-game Python objects:
//   CChessPlayer.action / MCTS_search / select_action_q_and_u / expand_and_evaluate / update_tree /
//   calc_policy / apply_temperature      (cchess_alphazero/agent/player.py:145-470)
//   SelfPlayWorker.start_game            (cchess_alphazero/worker/self_play.py:95-212)
//
// cz_search_round() is one lock-step ROUND for every game, three launches on one stream:
//   k_sim(BACKUP)  1. attach the network results of the previous round to their leaves and back them up,
//                  2. resume simulations that were parked on those leaves;
//   k_advance      3. where a search is complete: pick the move, apply the game rules, start the next
//                     search / the next game (self-play) or mark the game READY (external mode);
//   k_sim(SELECT)  4. where a batch of K simulations is complete start the next one; every new leaf writes
//                     its input planes into its fixed slot (game * K + sim) of the evaluation queue.
// With the evaluation cache on (cz_search_set_eval_cache) a fourth launch comes first: k_cache_fill stores the rows step 1
// is about to attach, and the k_sim launches are the k_sim_cached instantiations, whose new leaves ask the table in step 4.
// With the moves-left utility on (cz_search_set_moves_left) the k_sim launches are the k_sim_ml instantiations, and k_reserve_ml
// runs between k_advance and k_sim(SELECT): the statistics blocks are twice the size, and it reserves the difference.
// With the draw average on (cz_search_set_draw) they are the k_sim_draw instantiations, with k_reserve_ml in the same place.
// With the lower-confidence-bound move choice on (cz_search_set_lcb) they are the k_sim_var instantiations, likewise, and
// k_advance is k_advance_lcb.
// With the schedule of c_puct on (cz_search_set_cpuct_schedule) every one of these k_sim kernels is its SCHED instantiation,
// whose selection computes the exploration constant from the node's visit count; the policy temperature
// (cz_search_set_policy_temperature) is a factor in the attach of the same kernels.
// The host then runs ONE network forward over the whole queue.
// There is no host decision inside a round and no device->host copy, so a round (kernel + network
// forward) can be replayed from a HIP graph.
//
// Arithmetic follows the reference bit for bit: priors float32 (summed in move order),
// sqrt / Q / U in float64 with the float32 product c_puct*p for non-root nodes, W float64.
// Build with -ffp-contract=off.
//
// The device side is in internal headers, all of them parts of this one translation unit (each says why), in include order:
//   xq_search_tree.h      SearchLDS, EdgeStat, GameView, node and edge accessors, counters, the generator, keys and hash, backup
//   xq_search_attach.h    prior spreading and the attach of an evaluated leaf (prior_norm, attach_policy, attach_and_backup)
//   xq_search_ml.h        the moves-left utility: MovesLeftState, MRec, ml_quanta, wave_add_i64, backup_m, ml_edge_d, ml_utility
//   xq_search_draw.h      the draw average: DrawState, DRec, draw_quanta, backup_d, draw_sigma, draw_term
//   xq_search_var.h       the lower-confidence-bound move choice: LcbState, VRec, backup_v, LcbEdges, lcb_pick
//   xq_search_select.h    RootCtx and PUCT at the root, the Gumbel helpers, gumbel_interior, select_gumbel, select_edge
//   xq_search_solver.h    the MCTS solver: its bit fields, solve_*, select_solve
//   xq_search_sim.h       one simulation: Deferred, write_planes, expand_node, the cache probe, run_sim, flush_deferred
//   xq_search_records.h   RootEdges, gumbel_choose, gumbel_targets, prune_targets, root_value, root_surprise, root_maxq, emit_visits
//   xq_search_ply.h       the chunk pool, reserve_ply, ply_is_fast, begin_search, choose_action, new_game, the book, emit_record,
//                         new_script_game, script_move
//   xq_search_selfplay.h  advance_game
//   xq_search_stop.h      the early stop of a settled ply: stop_reset, ply_settled
//   xq_search_round.h     sim_body, k_sim / k_sim_cached / k_sim_solve / k_sim_stop / k_sim_ml / k_sim_draw, k_reserve_ml,
//                         k_cache_fill, k_advance, k_advance_stop, k_advance_script, k_stop_reset, k_noise
//   xq_search_aux.h       every other kernel (k_start_selfplay, k_start_script .. k_debug_sqrt) and walk_path
// This file keeps the includes and the host side: the opaque search object and the C-ABI entry points.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include "xq_rules.h"
#include "xq_search.h"
#include "xq_noise.h"
#include "xq_mirror.h"
#include "xq_evalcache.h"
#include "../../include/czero.h"

using namespace xq;

extern "C" void czi_set_error(const char* msg);   // xq_kernels.hip

#include "xq_search_tree.h"
#include "xq_search_attach.h"
#include "xq_search_ml.h"
#include "xq_search_draw.h"
#include "xq_search_var.h"
#include "xq_search_select.h"
#include "xq_search_solver.h"
#include "xq_search_sim.h"
#include "xq_search_records.h"
#include "xq_search_ply.h"
#include "xq_search_selfplay.h"
#include "xq_search_stop.h"
#include "xq_search_round.h"
#include "xq_search_aux.h"

// ---- host side: the opaque search object ----------------------------------------------------------------------
struct cz_search {
    SearchParams P;
    SearchBuffers B;
    void* slab = nullptr;             // everything but the chunk pool
    void* pool = nullptr;             // n_chunks x 1 MiB
    size_t bytes = 0;                 // slab + pool
    int device = 0;
    int prev_compact = 0;             // the previous round built a compact queue: its results are indexed by compact row
    int keep_chunks_created = 0;      // P.keep_chunks as sized at creation (cz_search_set_sims never goes below it)
    VisitRing V{};                    // root visit record (cz_search_record_visits); V.ring NULL = off
    void* vis_mem = nullptr;          // ring + control words + per-game flags, allocated only while recording is on
    void* book_mem = nullptr;         // the start-position book (cz_search_set_book): P.book points here
    EvalCache C{};                    // evaluation cache (cz_search_set_eval_cache); C.tab NULL = off
    void* ec_mem = nullptr;           // its bookkeeping (s_cval, stamp, counters), allocated only while the cache is on
    size_t ec_ctr_bytes = 0;          // the counters at its start: what cz_search_eval_cache_clear zeroes
    StopState S{};                    // early stop of a settled ply (cz_search_set_kld_gain, cz_search_set_smart_pruning)
    void* stop_mem = nullptr;         // its per-game state, allocated only while a rule is on; S.prev_sum NULL = both off
    size_t stop_bytes = 0;
    ScriptState X{};                  // scripted games (cz_search_set_script); X.n 0 = off
    void* script_mem = nullptr;       // boards, labels, offsets and z, in one allocation
    MovesLeftState M{};               // moves-left utility (cz_search_set_moves_left); M.slope 0 = off
    DrawState D{};                    // draw average (cz_search_set_draw); D.on 0 = off
    LcbState Z{};                     // lower-confidence-bound move choice (cz_search_set_lcb); Z.on 0 = off
};

namespace {

int serr(int code, const char* what)
{
    czi_set_error(what);
    return code;
}
int serr_hip(const char* what, hipError_t e)
{
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
    czi_set_error(buf);
    return CZ_ERR_HIP;
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

template <typename T>
void carve(char*& cur, T*& ptr, size_t count, bool dry)
{
    if (!dry) ptr = reinterpret_cast<T*>(cur);
    cur += align_up(sizeof(T) * count);
}

size_t layout(cz_search* s, char* base, bool dry)
{
    const SearchParams& P = s->P;
    SearchBuffers& B = s->B;
    char* cur = base;
    const size_t G = (size_t)P.G, H = (size_t)P.hash_cap;
    const size_t K = (size_t)P.K, D = (size_t)P.max_depth, PL = (size_t)P.max_plies + 2;
    carve(cur, B.hash_tab, G * H, dry);                  // first: the only part that has to be zeroed per game
    carve(cur, B.pool_ring, (size_t)P.n_chunks, dry);
    carve(cur, B.pool_head, 1, dry);
    carve(cur, B.pool_tail, 1, dry);
    carve(cur, B.pool_tail_vis, 1, dry);
    carve(cur, B.g_chunk_tab, G * (size_t)P.max_chunks, dry);
    carve(cur, B.g_nchunks, G, dry);
    carve(cur, B.g_heap_top, G, dry);
    carve(cur, B.g_node_count, G, dry);
    carve(cur, B.g_root, G, dry);
    carve(cur, B.g_board, G * BOARD_LDS, dry);
    carve(cur, B.g_tasks_left, G, dry);
    carve(cur, B.g_active, G, dry);
    carve(cur, B.g_phase, G, dry);
    carve(cur, B.g_turns, G, dry);
    carve(cur, B.g_no_act, G * MAX_NO_ACT, dry);
    carve(cur, B.g_n_no_act, G, dry);
    carve(cur, B.g_increase_temp, G, dry);
    carve(cur, B.s_state, G * K, dry);
    carve(cur, B.s_depth, G * K, dry);
    carve(cur, B.s_node, G * K, dry);
    carve(cur, B.s_path_node, G * K * D, dry);
    carve(cur, B.s_path_edge, G * K * D, dry);
    carve(cur, B.g_game_id, G, dry);
    carve(cur, B.g_enable_resign, G, dry);
    carve(cur, B.g_no_eat, G, dry);
    carve(cur, B.g_hist_key, G * PL * KEY_WORDS, dry);
    carve(cur, B.g_hist_hash, G * PL, dry);
    carve(cur, B.g_hist_act, G * PL, dry);
    carve(cur, B.counters, G * CT_COUNT, dry);
    carve(cur, B.ring, (size_t)P.ring_cap * P.record_stride, dry);
    carve(cur, B.ring_tail, 1, dry);
    carve(cur, B.g_last_action, G, dry);
    carve(cur, B.pending, 1, dry);
    carve(cur, B.noise, G * K * MAXMOVES, dry);
    carve(cur, B.g_noise_epoch, G, dry);
    carve(cur, B.g_prev_board, G * BOARD_LDS, dry);
    carve(cur, B.g_hist_kind, G, dry);
    carve(cur, B.s_qrow, G * K, dry);
    carve(cur, B.g_started, G * MAXMOVES, dry);
    carve(cur, B.g_gumbel, G * MAXMOVES, dry);
    carve(cur, B.g_budget, G, dry);
    return (size_t)(cur - base);
}

// The larger statistics blocks are in use: the moves-left utility, the draw average or the lower-confidence-bound move choice is
// on (at most one of them: FEATURES), a block carries one M / D / V record per edge (reserve_ply<true>, k_reserve_ml).
bool larger_blocks(const cz_search* s) { return s->M.slope > 0.0 || s->D.on != 0 || s->Z.on != 0; }

// chunks a game needs for one full search on an empty tree (what it keeps through resets and between games)
// larger: with the larger statistics blocks
int keep_chunks_for(int sims, bool larger = false)
{
    const long long PER_TASK = NODE_HDR_GRANULES + (6 * RESERVE_MOVES + 15) / 16 + (larger ? 2 : 1) * RESERVE_MOVES;
    const long long USABLE = CHUNK_GRANULES - (larger ? 2 : 1) * MAXMOVES;
    const long long need = (long long)(sims + 1) * PER_TASK + 1;
    return (int)((need + USABLE - 1) / USABLE);
}

// P.keep_chunks for P.sims simulations with the blocks in use now: what one full search needs, within what a game can own and
// never fewer than it was created with (the initial pool layout gave every game that many).
void set_keep_chunks(cz_search* s)
{
    int keep = keep_chunks_for(s->P.sims, larger_blocks(s));
    if (keep > s->P.max_chunks) keep = s->P.max_chunks;
    s->P.keep_chunks = keep > s->keep_chunks_created ? keep : s->keep_chunks_created;
}

// The pool is sized at creation (raised to the plain blocks' floor, games x keep_chunks + 1) and never grows.  An option that
// doubles the statistics blocks may need more chunks for one full search: where the pool is below the floor of the larger
// blocks the option's setter refuses to switch it on, so that a game that dropped its tree always holds one full search.
// Returns false after setting the error text.
bool pool_holds_larger_blocks(const cz_search* s, const char* me)
{
    int keep = keep_chunks_for(s->P.sims, true);
    if (keep > s->P.max_chunks) keep = s->P.max_chunks;
    if (keep < s->keep_chunks_created) keep = s->keep_chunks_created;
    const long long floor_chunks = (long long)s->P.G * keep + 1;
    if (floor_chunks <= (long long)s->P.n_chunks) return true;
    char buf[200];
    snprintf(buf, sizeof(buf), "%s: the pool of %d chunks is below the floor of the larger statistics blocks, games x keep_chunks"
             " + 1 = %lld", me, s->P.n_chunks, floor_chunks);
    serr(CZ_ERR_ARG, buf);
    return false;
}

// The readers of the larger blocks' records while their option is off (the trees hold no such records): every output that is
// given is zeroed.
struct ZeroOut { void* ptr; size_t bytes; };
template <size_t N>
int zero_outputs(const ZeroOut (&outs)[N], const char* entry, void* stream)
{
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < N && e == hipSuccess; ++i)
        if (outs[i].ptr) e = hipMemsetAsync(outs[i].ptr, 0, outs[i].bytes, (hipStream_t)stream);
    return e == hipSuccess ? CZ_OK : serr_hip(entry, e);
}

// initial state of the pool: game g owns chunks [g * keep, (g + 1) * keep), the rest is free
int init_pool(cz_search* s)
{
    const SearchParams& P = s->P;
    const size_t G = (size_t)P.G;
    const int owned = P.G * P.keep_chunks;
    uint32_t* tab = new (std::nothrow) uint32_t[G * P.max_chunks]();
    uint32_t* ring = new (std::nothrow) uint32_t[(size_t)P.n_chunks]();
    int32_t* nch = new (std::nothrow) int32_t[G];
    uint32_t* top = new (std::nothrow) uint32_t[G];
    hipError_t e = hipSuccess;
    if (!tab || !ring || !nch || !top) e = hipErrorOutOfMemory;
    else {
        for (size_t g = 0; g < G; ++g) {
            for (int i = 0; i < P.keep_chunks; ++i) tab[g * P.max_chunks + i] = (uint32_t)(g * P.keep_chunks + i);
            nch[g] = P.keep_chunks;
            top[g] = 1u;
        }
        for (int i = owned; i < P.n_chunks; ++i) ring[i - owned] = (uint32_t)i;
        const unsigned int head = 0u, tail = (unsigned int)(P.n_chunks - owned);
        e = hipMemcpy(s->B.g_chunk_tab, tab, sizeof(uint32_t) * G * P.max_chunks, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(s->B.pool_ring, ring, sizeof(uint32_t) * (size_t)P.n_chunks, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(s->B.g_nchunks, nch, sizeof(int32_t) * G, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(s->B.g_heap_top, top, sizeof(uint32_t) * G, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(s->B.pool_head, &head, sizeof(head), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(s->B.pool_tail, &tail, sizeof(tail), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(s->B.pool_tail_vis, &tail, sizeof(tail), hipMemcpyHostToDevice);
    }
    delete[] tab; delete[] ring; delete[] nch; delete[] top;
    return e == hipSuccess ? CZ_OK : serr_hip("cz_search_create: pool initialisation", e);
}

// The side columns of a visit entry (czero.h), in CZ_VISIT_COL_* order: the column's ring, its name in error texts, and
// whether it excludes a script (cz_search_set_script).  VisitRing keeps its named fields: it is a kernel argument.
struct VisitCol {
    double* VisitRing::* ring;
    const char* name;
    bool no_script;
};
const VisitCol VISIT_COLS[CZ_VISIT_COLS] = {
    {&VisitRing::q, "value", false}, {&VisitRing::s, "surprise", false}, {&VisitRing::mq, "max-q", true}};
static_assert(CZ_VISIT_COL_Q == 0 && CZ_VISIT_COL_S == 1 && CZ_VISIT_COL_MAXQ == 2, "czero.h: the order of VISIT_COLS");

}  // namespace

extern "C" {

int cz_search_create(const cz_search_cfg* c, cz_search** out)
{
    if (!c || !out) return serr(CZ_ERR_ARG, "cz_search_create: null argument");
    if (c->n_games < 1 || c->sims_per_round < 1 || c->simulation_num_per_move < 1)
        return serr(CZ_ERR_ARG, "cz_search_create: n_games, sims_per_round, simulation_num_per_move must be >= 1");
    cz_search* s = new (std::nothrow) cz_search();
    if (!s) return serr(CZ_ERR_NOMEM, "cz_search_create: host allocation failed");
    SearchParams& P = s->P;
    P.G = c->n_games;
    P.K = c->sims_per_round;
    P.sims = c->simulation_num_per_move;
    P.vl = c->virtual_loss;
    P.max_depth = c->max_depth > 0 ? c->max_depth : MAXD_LDS;      // simulations deeper than this are cut (counted)
    if (P.max_depth > MAXD_LDS) P.max_depth = MAXD_LDS;
    P.max_game_length = c->max_game_length > 0 ? c->max_game_length : 100;
    P.max_plies = 2 * P.max_game_length + 2;
    // the most nodes one game's tree is sized for: every simulation of every ply of the longest game expands one
    long long max_nodes = c->max_nodes_per_game > 0 ? c->max_nodes_per_game : (long long)(P.max_plies + 2) * P.sims;
    if (max_nodes < P.sims + 2) max_nodes = P.sims + 2;
    if (max_nodes > (1ll << 23)) max_nodes = 1ll << 23;
    int h = 128;
    while ((long long)h * 2 < max_nodes * 3) h <<= 1;              // load factor <= 2/3 at max_nodes
    P.hash_cap = h;
    P.keep_chunks = keep_chunks_for(P.sims);
    s->keep_chunks_created = P.keep_chunks;
    // lock-step batches one k_sim launch may START for a game: 1.  (A batch whose simulations all end on terminal or
    // repeated positions needs no evaluation and could be followed by the next at once, but then the whole launch
    // waits for the few waves that chain batches of the slowest kind of simulation: with 3, the sustained k_sim(SELECT)
    // launch was 0.78 ms mean / 2.3 ms p99 against a 0.64 ms median.)
    P.max_batches = 1;
    if (const char* e = getenv("CZ_MAX_BATCHES")) { const int v = atoi(e); if (v >= 1 && v <= 16) P.max_batches = v; }
    // chunk table: the whole-game tree at ~420 B per node (node record + its share of statistics blocks)
    const long long game_chunks = (max_nodes * 420 + (long long)CHUNK_BYTES - 1) / (long long)CHUNK_BYTES;
    long long mc = game_chunks + P.keep_chunks;
    if (mc < P.keep_chunks + 1) mc = P.keep_chunks + 1;
    if (mc > MAX_CHUNKS) mc = MAX_CHUNKS;
    if (P.keep_chunks > MAX_CHUNKS) { delete s; return serr(CZ_ERR_ARG, "cz_search_create: simulation_num_per_move too large for one game's chunk table"); }
    P.max_chunks = (int)mc;
    P.planes_dtype = c->planes_dtype;
    P.in_planes = c->use_history ? 28 : 14;
    P.mode = MODE_EXTERNAL;
    P.c_puct = c->c_puct;
    P.c_puct_f32 = (float)c->c_puct;
    P.noise_eps = c->noise_eps;
    P.one_minus_eps_f32 = (float)(1.0 - c->noise_eps);
    P.dirichlet_alpha = c->dirichlet_alpha;
    P.tau_decay_rate = c->tau_decay_rate;
    P.resign_threshold = c->resign_threshold;
    P.min_resign_turn = c->min_resign_turn;
    P.evaluate = c->evaluate;
    P.enable_resign_rate = c->enable_resign_rate;
    P.seed = c->seed;
    P.game_id_stride = (uint32_t)P.G;
    P.gumbel_visit = 50.0;
    P.gumbel_scale = 1.0;
    P.cpuct_factor = 0.0;
    P.cpuct_base = 19652.0;
    P.inv_temp = 1.0f;
    P.ring_cap = c->ring_capacity > 0 ? c->ring_capacity : 2 * P.G + 64;
    P.record_stride = (int)((sizeof(GameRecord) + sizeof(uint16_t) * (size_t)(P.max_plies + 2) + 15) & ~(size_t)15);
    if (P.planes_dtype < CZ_F32 || P.planes_dtype > CZ_U8) { delete s; return serr(CZ_ERR_ARG, "cz_search_create: planes_dtype"); }
    hipError_t e = hipGetDevice(&s->device);
    if (e != hipSuccess) { delete s; return serr_hip("cz_search_create: hipGetDevice", e); }
    // pool size: what the games can use at most, bounded by the memory that is free now (the caller's network and
    // queue buffers come later: leave a fifth of it), never less than what the games keep
    const long long floor_chunks = (long long)P.G * P.keep_chunks + 1;
    long long want = c->pool_chunks > 0 ? c->pool_chunks : (long long)P.G * P.max_chunks;
    if (c->pool_chunks <= 0) {
        size_t free_b = 0, total_b = 0;
        e = hipMemGetInfo(&free_b, &total_b);
        if (e != hipSuccess) { delete s; return serr_hip("cz_search_create: hipMemGetInfo", e); }
        P.n_chunks = 0;
        const size_t fixed = layout(s, nullptr, true);             // (n_chunks = 0: the ring is added below, 4 B per chunk)
        const long long avail = ((long long)(free_b / 5 * 4) - (long long)fixed) / (long long)(CHUNK_BYTES + 4);
        if (want > avail) want = avail;
    }
    if (want < floor_chunks) want = floor_chunks;
    if (want > 0x7fffff00ll) want = 0x7fffff00ll;
    P.n_chunks = (int)want;
    const size_t slab_bytes = layout(s, nullptr, true);
    e = hipMalloc(&s->slab, slab_bytes);
    if (e != hipSuccess) { delete s; return serr_hip("cz_search_create: hipMalloc", e); }
    e = hipMalloc(&s->pool, (size_t)P.n_chunks * CHUNK_BYTES + 4096);   // (+ slack: speculative reads past a record)
    if (e != hipSuccess) { (void)hipFree(s->slab); delete s; return serr_hip("cz_search_create: hipMalloc (chunk pool)", e); }
    s->bytes = slab_bytes + (size_t)P.n_chunks * CHUNK_BYTES;
    e = hipMemset(s->slab, 0, slab_bytes);
    if (e != hipSuccess) { (void)cz_search_destroy(s); return serr_hip("cz_search_create: hipMemset", e); }
    layout(s, (char*)s->slab, false);
    s->B.pool = (char*)s->pool;
    const int rc = init_pool(s);
    if (rc != CZ_OK) { (void)cz_search_destroy(s); return rc; }
    *out = s;
    return CZ_OK;
}

int cz_search_destroy(cz_search* s)
{
    if (!s) return CZ_OK;
    (void)hipFree(s->vis_mem);
    for (const VisitCol& c : VISIT_COLS) (void)hipFree(s->V.*c.ring);
    (void)hipFree(s->book_mem);
    (void)hipFree(s->C.tab);
    (void)hipFree(s->ec_mem);
    (void)hipFree(s->stop_mem);
    (void)hipFree(s->script_mem);
    (void)hipFree(s->pool);
    (void)hipFree(s->slab);
    delete s;
    return CZ_OK;
}

size_t cz_search_bytes(const cz_search* s)
{
    if (!s) return 0;
    return s->bytes + (s->C.tab ? (size_t)ec_table_bytes(s->C.log2) : 0)      // (the evaluation cache's table, while it is on)
           + s->stop_bytes;                                                    // (the stop rules' state, while one is on)
}

int cz_search_info(const cz_search* s, int32_t* out)
{
    if (!s || !out) return serr(CZ_ERR_ARG, "cz_search_info: null argument");
    out[0] = s->P.G; out[1] = s->P.K; out[2] = s->P.sims; out[3] = s->P.n_chunks; out[4] = s->P.max_chunks;
    out[5] = s->P.hash_cap; out[6] = s->P.max_depth; out[7] = s->P.max_plies; out[8] = s->P.record_stride;
    out[9] = s->P.ring_cap; out[10] = CT_COUNT; out[11] = s->P.in_planes; out[12] = s->P.keep_chunks;
    out[13] = MAX_NO_ACT; out[14] = 0; out[15] = 0;
    return CZ_OK;
}

int cz_search_memory_info(cz_search* s, int64_t* host_out, void* stream)
{
    if (!s || !host_out) return serr(CZ_ERR_ARG, "cz_search_memory_info: null argument");
    const size_t G = (size_t)s->P.G;
    int32_t* nch = new (std::nothrow) int32_t[G];
    uint32_t* top = new (std::nothrow) uint32_t[G];
    int32_t* cnt = new (std::nothrow) int32_t[G];
    unsigned int ht[2] = {0u, 0u};
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = (nch && top && cnt) ? hipSuccess : hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipMemcpyAsync(nch, s->B.g_nchunks, sizeof(int32_t) * G, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(top, s->B.g_heap_top, sizeof(uint32_t) * G, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(cnt, s->B.g_node_count, sizeof(int32_t) * G, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&ht[0], s->B.pool_head, sizeof(unsigned int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&ht[1], s->B.pool_tail, sizeof(unsigned int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
        int64_t held = 0, held_max = 0, used = 0, used_max = 0, nodes = 0, nodes_max = 0;
        for (size_t g = 0; g < G; ++g) {
            held += nch[g];
            if (nch[g] > held_max) held_max = nch[g];
            const int64_t u = (int64_t)(top[g] >> CHUNK_SHIFT) * (int64_t)CHUNK_BYTES + (int64_t)(top[g] & (CHUNK_GRANULES - 1)) * 16;
            used += u;
            if (u > used_max) used_max = u;
            nodes += cnt[g];
            if (cnt[g] > nodes_max) nodes_max = cnt[g];
        }
        host_out[0] = s->P.n_chunks;                  // pool size (chunks of 1 MiB)
        host_out[1] = (int64_t)(unsigned int)(ht[1] - ht[0]);     // free chunks
        host_out[2] = held;                           // chunks owned by games
        host_out[3] = held_max;                       // ... by the largest game
        host_out[4] = used;                           // tree bytes in use (all games)
        host_out[5] = used_max;                       // ... of the largest game
        host_out[6] = nodes;
        host_out[7] = nodes_max;
    }
    delete[] nch; delete[] top; delete[] cnt;
    if (e != hipSuccess) return serr_hip("cz_search_memory_info", e);
    return CZ_OK;
}

#define S_LAUNCH_CHECK(name)                                         \
    do {                                                             \
        hipError_t e_ = hipGetLastError();                           \
        if (e_ != hipSuccess) return serr_hip(name, e_);             \
    } while (0)

int cz_search_start_selfplay(cz_search* s, uint64_t seed, uint32_t first_game_id, uint32_t game_id_stride, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_start_selfplay: null handle");
    s->P.mode = MODE_SELFPLAY;
    s->P.seed = seed;
    s->P.game_id_stride = game_id_stride ? game_id_stride : (uint32_t)s->P.G;
    hipError_t e = hipMemsetAsync(s->B.ring_tail, 0, sizeof(unsigned int), (hipStream_t)stream);
    if (e == hipSuccess && s->V.ring)                 // the games start now: their visit records will be complete
        e = hipMemsetAsync(s->V.g_lost, 0, (size_t)s->P.G, (hipStream_t)stream);
    if (e != hipSuccess) return serr_hip("cz_search_start_selfplay", e);
    hipLaunchKernelGGL(k_pool_commit, dim3(1), dim3(1), 0, (hipStream_t)stream, s->B);
    if (s->X.n > 0) hipLaunchKernelGGL(k_start_script, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B, s->X, first_game_id);
    else hipLaunchKernelGGL(k_start_selfplay, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B, first_game_id);
    if (s->stop_mem)                                  // every game's first search begins: empty snapshots
        hipLaunchKernelGGL(k_stop_reset, dim3((s->P.G + 255) / 256), dim3(256), 0, (hipStream_t)stream, s->S, s->P.G,
                           (const uint8_t*)nullptr);
    S_LAUNCH_CHECK("cz_search_start_selfplay");
    return CZ_OK;
}

int cz_search_set_roots(cz_search* s, const int8_t* boards, const int32_t* turns, const uint16_t* no_act,
                        const uint8_t* n_no_act, const uint8_t* increase_temp, const uint8_t* enable_resign,
                        const uint8_t* select_mask, const int8_t* prev_boards, const uint8_t* hist_kind, void* stream)
{
    if (!s || !boards) return serr(CZ_ERR_ARG, "cz_search_set_roots: null argument");
    s->P.mode = MODE_EXTERNAL;
    hipLaunchKernelGGL(k_pool_commit, dim3(1), dim3(1), 0, (hipStream_t)stream, s->B);
    hipLaunchKernelGGL(k_set_roots, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B, boards, turns, no_act,
                       n_no_act, increase_temp, enable_resign, select_mask, prev_boards, hist_kind);
    if (s->stop_mem)                                  // the selected games' searches begin: empty snapshots
        hipLaunchKernelGGL(k_stop_reset, dim3((s->P.G + 255) / 256), dim3(256), 0, (hipStream_t)stream, s->S, s->P.G,
                           select_mask);
    S_LAUNCH_CHECK("cz_search_set_roots");
    return CZ_OK;
}

static int search_round_impl(cz_search* s, const float* policy, const float* value, void* planes, int32_t* q_rows,
                             int32_t* q_count, void* stream)
{
    const dim3 grid(s->P.G), block(64);
    hipStream_t st = (hipStream_t)stream;
    const bool noise = s->P.noise_eps != 0.0 && s->P.gumbel_m == 0;
    const int compact = q_rows ? 1 : 0;
    // the rows consumed now were written after the PREVIOUS round: by compact row if that round built a compact queue
    const int consume_compact = s->prev_compact;
    s->prev_compact = compact;
    const dim3 nblock(256);
    const bool hist = s->P.in_planes == 28;
    const bool gum = s->P.gumbel_m > 0;
    const bool cache = s->C.tab != nullptr;
    const bool solve = s->P.solver != 0;                        // (never with gum or cache: cz_search_set_solver)
    const bool stop = s->stop_mem != nullptr;                   // (never with gum, cache or solve: cz_search_set_kld_gain)
    const bool script = s->X.n > 0 && s->P.mode == MODE_SELFPLAY;   // (never with gum, solve or stop: cz_search_set_script)
    const bool ml = s->M.slope > 0.0;                           // (never with gum, solve, stop, cache or a script: cz_search_set_moves_left)
    const bool draw = s->D.on != 0;                             // (never with ml or what ml is never with: cz_search_set_draw)
    const bool lcb = s->Z.on != 0;                              // (never with ml, draw or what they are never with: cz_search_set_lcb)
    const bool sched = s->P.cpuct_factor > 0.0;                 // (beside every one of them: the SCHED instantiation of the same kernel)
    auto sim = [&](int mask, int cq) {
        if (lcb) {
            if (hist) hipLaunchKernelGGL((sched ? k_sim_var<true, true> : k_sim_var<true>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count);
            else hipLaunchKernelGGL((sched ? k_sim_var<false, true> : k_sim_var<false>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count);
        } else if (draw) {
            if (hist) hipLaunchKernelGGL((sched ? k_sim_draw<true, true> : k_sim_draw<true>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count, s->D);
            else hipLaunchKernelGGL((sched ? k_sim_draw<false, true> : k_sim_draw<false>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count, s->D);
        } else if (ml) {
            if (hist) hipLaunchKernelGGL((sched ? k_sim_ml<true, true> : k_sim_ml<true>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count, s->M);
            else hipLaunchKernelGGL((sched ? k_sim_ml<false, true> : k_sim_ml<false>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count, s->M);
        } else if (stop) {
            if (hist) hipLaunchKernelGGL((sched ? k_sim_stop<true, true> : k_sim_stop<true>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count, s->S);
            else hipLaunchKernelGGL((sched ? k_sim_stop<false, true> : k_sim_stop<false>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count, s->S);
        } else if (solve) {
            if (hist) hipLaunchKernelGGL((sched ? k_sim_solve<true, true> : k_sim_solve<true>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count);
            else hipLaunchKernelGGL((sched ? k_sim_solve<false, true> : k_sim_solve<false>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count);
        } else if (cache) {         // (14 planes: cz_search_set_eval_cache refuses the history input)
            if (gum) hipLaunchKernelGGL((sched ? k_sim_cached<true, true> : k_sim_cached<true>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count, s->C);
            else hipLaunchKernelGGL((sched ? k_sim_cached<false, true> : k_sim_cached<false>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count, s->C);
        } else if (gum) {
            if (hist) hipLaunchKernelGGL((sched ? k_sim<true, true, true> : k_sim<true, true>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count);
            else hipLaunchKernelGGL((sched ? k_sim<false, true, true> : k_sim<false, true>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count);
        } else {
            if (hist) hipLaunchKernelGGL((sched ? k_sim<true, false, true> : k_sim<true, false>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count);
            else hipLaunchKernelGGL((sched ? k_sim<false, false, true> : k_sim<false, false>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count);
        }
    };
    // evaluation cache: the rows the BACKUP launch is about to attach go into the table first (its only writer)
    if (cache)
        hipLaunchKernelGGL(k_cache_fill, dim3(s->P.G * s->P.K), block, 0, st, s->P, s->B, s->C, policy, value, consume_compact);
    sim(SIM_BACKUP, consume_compact);
    if (script) hipLaunchKernelGGL(k_advance_script, grid, block, 0, st, s->P, s->B, s->V, s->X);
    else if (stop) hipLaunchKernelGGL(k_advance_stop, grid, block, 0, st, s->P, s->B, s->V, s->S);
    else if (gum && s->P.gumbel_full) hipLaunchKernelGGL(k_advance<true>, grid, block, 0, st, s->P, s->B, s->V);
    else if (solve) hipLaunchKernelGGL((k_advance<false, true>), grid, block, 0, st, s->P, s->B, s->V);
    else if (lcb) hipLaunchKernelGGL(k_advance_lcb, grid, block, 0, st, s->P, s->B, s->V, s->Z);
    else hipLaunchKernelGGL(k_advance<false>, grid, block, 0, st, s->P, s->B, s->V);
    if (larger_blocks(s)) hipLaunchKernelGGL(k_reserve_ml, grid, block, 0, st, s->P, s->B);   // the larger statistics blocks of the searches that go on
    if (noise) hipLaunchKernelGGL(k_noise, grid, nblock, 0, st, s->P, s->B);
    sim(SIM_SELECT, compact);
    S_LAUNCH_CHECK("cz_search_round");
    return CZ_OK;
}

int cz_search_round(cz_search* s, const float* policy, const float* value, void* planes, void* stream)
{
    if (!s || !planes || !policy || !value) return serr(CZ_ERR_ARG, "cz_search_round: null argument");
    return search_round_impl(s, policy, value, planes, nullptr, nullptr, stream);
}

int cz_search_round_q(cz_search* s, const float* policy, const float* value, void* planes, int32_t* q_rows,
                      int32_t* q_count, void* stream)
{
    if (!s || !planes || !policy || !value || !q_rows || !q_count)
        return serr(CZ_ERR_ARG, "cz_search_round_q: null argument");
    return search_round_impl(s, policy, value, planes, q_rows, q_count, stream);
}

int cz_search_set_sims(cz_search* s, int simulation_num_per_move)
{
    if (!s || simulation_num_per_move < 1) return serr(CZ_ERR_ARG, "cz_search_set_sims: bad argument");
    if (simulation_num_per_move < s->P.fast_sims)
        return serr(CZ_ERR_ARG, "cz_search_set_sims: below the playout cap's fast_sims (cz_search_set_playout_cap)");
    // (a search longer than the chunks a game can own ends in counted overflow_sims, it is not refused here)
    s->P.sims = simulation_num_per_move;
    // a game that has to drop its tree keeps enough chunks for one full search of the NEW length
    set_keep_chunks(s);
    return CZ_OK;
}

int cz_search_leaf_masks(cz_search* s, uint32_t* masks)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_leaf_masks: null handle");
    s->B.leaf_masks = masks;
    if (!masks) s->B.leaf_planes_off = 0;
    return CZ_OK;
}

int cz_search_leaf_planes(cz_search* s, int on)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_leaf_planes: null handle");
    if (!on && !s->B.leaf_masks) return serr(CZ_ERR_ARG, "cz_search_leaf_planes: the planes can only be switched off while cz_search_leaf_masks is set");
    s->B.leaf_planes_off = on ? 0 : 1;
    return CZ_OK;
}

int cz_search_policy_logits(cz_search* s, int on)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_policy_logits: null handle");
    const int mode = on ? 1 : 0;
    if (!mode && s->P.inv_temp != 1.0f)
        return serr(CZ_ERR_ARG, "cz_search_policy_logits: a policy temperature is set (cz_search_set_policy_temperature), it needs "
                                "logit rows");
    if (mode != s->P.policy_logits && s->C.tab) {
        // the meaning of a row changes: what the evaluation cache holds was formed under the other one.  This entry has no
        // stream of its own, so the table is emptied between two device synchronisations.
        hipError_t e = hipDeviceSynchronize();
        if (e != hipSuccess) return serr_hip("cz_search_policy_logits", e);
        const int rc = cz_search_eval_cache_clear(s, nullptr);
        if (rc != CZ_OK) return rc;
        e = hipDeviceSynchronize();
        if (e != hipSuccess) return serr_hip("cz_search_policy_logits", e);
    }
    s->P.policy_logits = mode;
    return CZ_OK;
}

// ---- features that cannot run beside each other (include/czero.h has the matrix and the reasons) -------------------------
// Host only.  A refused setter names the first excluder that is on, in this order; each phrase stands here once.
// cchess_alphazero/search_options.py states the same pairs for the layers above (tests/test_gpu_search_options.py).
// The last three are the options with the larger statistics blocks (larger_blocks): each excludes the other two, whose records
// lie in the same granules, and F_BLOCKS_EXCLUDE, the features with a k_sim instantiation or a use of the blocks' words of their own.
enum Feature : int { F_FORCED, F_CAP, F_GUMBEL, F_SOLVER, F_KLD, F_LEAD, F_CACHE, F_SCRIPT, F_ML, F_DRAW, F_LCB, F_COUNT };
constexpr unsigned fbit(Feature f) { return 1u << f; }
constexpr unsigned F_BLOCKS = fbit(F_ML) | fbit(F_DRAW) | fbit(F_LCB);
constexpr unsigned F_BLOCKS_EXCLUDE = fbit(F_GUMBEL) | fbit(F_SOLVER) | fbit(F_KLD) | fbit(F_LEAD) | fbit(F_CACHE) | fbit(F_SCRIPT);
constexpr struct { bool (*on)(const cz_search*); const char* phrase; unsigned excludes; } FEATURES[F_COUNT] = {
    {[](const cz_search* s) { return s->P.forced_k > 0.0; }, "forced playouts are on (cz_search_set_forced_playouts)",
     fbit(F_GUMBEL) | fbit(F_SOLVER)},
    {[](const cz_search* s) { return s->P.fast_sims > 0; }, "the playout cap is on (cz_search_set_playout_cap)", fbit(F_GUMBEL)},
    {[](const cz_search* s) { return s->P.gumbel_m > 0; }, "the Gumbel root search is on (cz_search_set_gumbel)",
     fbit(F_FORCED) | fbit(F_CAP) | fbit(F_SOLVER) | fbit(F_KLD) | fbit(F_LEAD) | fbit(F_SCRIPT) | F_BLOCKS},
    {[](const cz_search* s) { return s->P.solver != 0; }, "the MCTS solver is on (cz_search_set_solver)",
     fbit(F_FORCED) | fbit(F_GUMBEL) | fbit(F_KLD) | fbit(F_LEAD) | fbit(F_CACHE) | fbit(F_SCRIPT) | F_BLOCKS},
    {[](const cz_search* s) { return s->S.gain > 0.0; }, "the KLD-gain stop is on (cz_search_set_kld_gain)",
     fbit(F_GUMBEL) | fbit(F_SOLVER) | fbit(F_CACHE) | fbit(F_SCRIPT) | F_BLOCKS},
    {[](const cz_search* s) { return s->S.lead != 0; }, "the unreachable-lead stop is on (cz_search_set_smart_pruning)",
     fbit(F_GUMBEL) | fbit(F_SOLVER) | fbit(F_CACHE) | fbit(F_SCRIPT) | F_BLOCKS},
    {[](const cz_search* s) { return s->C.tab != nullptr; }, "the evaluation cache is on (cz_search_set_eval_cache)",
     fbit(F_SOLVER) | fbit(F_KLD) | fbit(F_LEAD) | F_BLOCKS},
    {[](const cz_search* s) { return s->X.n > 0; }, "a script is set (cz_search_set_script)",
     fbit(F_GUMBEL) | fbit(F_SOLVER) | fbit(F_KLD) | fbit(F_LEAD) | F_BLOCKS},
    {[](const cz_search* s) { return s->M.slope > 0.0; }, "the moves-left utility is on (cz_search_set_moves_left)",
     F_BLOCKS_EXCLUDE | fbit(F_DRAW) | fbit(F_LCB)},
    {[](const cz_search* s) { return s->D.on != 0; }, "the draw average is on (cz_search_set_draw)",
     F_BLOCKS_EXCLUDE | fbit(F_ML) | fbit(F_LCB)},
    {[](const cz_search* s) { return s->Z.on != 0; }, "the lower-confidence-bound move choice is on (cz_search_set_lcb)",
     F_BLOCKS_EXCLUDE | fbit(F_ML) | fbit(F_DRAW)},
};
constexpr bool features_symmetric()
{
    for (int a = 0; a < F_COUNT; ++a)
        for (int b = 0; b <= a; ++b)
            if ((FEATURES[a].excludes >> b & 1) != (a == b ? 0 : FEATURES[b].excludes >> a & 1)) return false;
    return true;
}
static_assert(features_symmetric(), "the exclusion matrix is symmetric and no feature excludes itself");

// What a setter of feature f does between its argument checks and its assignment.  Switching on is refused beside an excluder:
// CZ_ERR_ARG, "<entry>: <phrase of the first one that is on>".  grows (a setter of F_BLOCKS that steps from off to on): then
// the host-only pool test, pool_holds_larger_blocks.  Then the stream is idle: launches in flight keep the setting (the table)
// they started with.
static int admit(const cz_search* s, Feature f, bool on, const char* entry, void* stream, bool grows = false)
{
    for (int o = 0; on && o < F_COUNT; ++o)
        if ((FEATURES[f].excludes >> o & 1) && FEATURES[o].on(s)) {
            char buf[160];
            snprintf(buf, sizeof(buf), "%s: %s", entry, FEATURES[o].phrase);
            return serr(CZ_ERR_ARG, buf);
        }
    if (grows && !pool_holds_larger_blocks(s, entry)) return CZ_ERR_ARG;
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    return e == hipSuccess ? CZ_OK : serr_hip(entry, e);
}

// What a setter of F_BLOCKS does after its assignment: where it went on or off the statistics blocks change size, so the trees
// start over, and a game keeps the chunks of one full search of the new size.
static int blocks_changed(cz_search* s, bool was, bool on, void* stream)
{
    if (was == on) return CZ_OK;
    set_keep_chunks(s);
    return cz_search_reset_trees(s, stream);
}

// ---- evaluation cache (include/czero.h; csrc/xq_evalcache.h has the layout and who touches the table when) ----
static_assert(CZ_EVAL_CACHE_STRIDE == EC_STRIDE && CZ_EVAL_CACHE_MIN_LOG2 == EC_MIN_LOG2 && CZ_EVAL_CACHE_MAX_LOG2 == EC_MAX_LOG2,
              "czero.h: evaluation cache");
static_assert(EC_KEY_WORDS == KEY_WORDS && EC_MAX_MOVES == MAXMOVES, "xq_evalcache.h: entry layout");

int cz_search_eval_cache_clear(cz_search* s, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_eval_cache_clear: null handle");
    if (!s->C.tab) return CZ_OK;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(s->C.tab, 0, (size_t)ec_table_bytes(s->C.log2), st);
    // The counters go and the stamp starts over at 0: the rows of the round that follows were evaluated BEFORE the table was
    // emptied (by the network the caller is replacing), so that round's fill stores nothing; its k_sim(BACKUP) launch steps
    // the stamp to 1 and the fills go on.  s_cval stays: slots the cache answered in the last round wait for their attach.
    if (e == hipSuccess) e = hipMemsetAsync(s->ec_mem, 0, s->ec_ctr_bytes, st);
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)s->C.stamp, 0, 1, st);
    if (e != hipSuccess) return serr_hip("cz_search_eval_cache_clear", e);
    return CZ_OK;
}

int cz_search_set_eval_cache(cz_search* s, int log2_entries, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_eval_cache: null handle");
    if (log2_entries != 0 && (log2_entries < EC_MIN_LOG2 || log2_entries > EC_MAX_LOG2))
        return serr(CZ_ERR_ARG, "cz_search_set_eval_cache: log2_entries must be 0 (off) or 10 .. 24");
    if (log2_entries != 0 && s->P.in_planes == 28)
        return serr(CZ_ERR_ARG, "cz_search_set_eval_cache: refused with the 28-plane history input: its second plane block "
                                "depends on the simulation's path and the game history, so the network input is not a "
                                "function of the position");
    if (const int rc = admit(s, F_CACHE, log2_entries != 0, "cz_search_set_eval_cache", stream)) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    if (s->C.tab && log2_entries == s->C.log2) return cz_search_eval_cache_clear(s, stream);
    const size_t G = (size_t)s->P.G, slots = G * (size_t)s->P.K;
    if (s->C.tab) {
        // a slot the cache answered keeps its value in s_cval until the next round attaches it, and only the cached
        // kernels attach it: the table goes or changes size between searches
        uint8_t* st8 = new (std::nothrow) uint8_t[slots];
        if (!st8) return serr(CZ_ERR_NOMEM, "cz_search_set_eval_cache: host allocation failed");
        e = hipMemcpy(st8, s->B.s_state, slots, hipMemcpyDeviceToHost);
        bool waiting = false;
        for (size_t i = 0; e == hipSuccess && i < slots; ++i) waiting = waiting || st8[i] == SIM_CACHED;
        delete[] st8;
        if (e != hipSuccess) return serr_hip("cz_search_set_eval_cache", e);
        if (waiting)
            return serr(CZ_ERR_STATE, "cz_search_set_eval_cache: leaves the cache answered wait for their attach; switch it "
                                      "off or resize it between searches (after cz_search_reset_trees, cz_search_set_roots "
                                      "or cz_search_start_selfplay)");
    }
    (void)hipFree(s->C.tab);
    (void)hipFree(s->ec_mem);
    s->C = EvalCache{};
    s->ec_mem = nullptr;
    s->ec_ctr_bytes = 0;
    if (log2_entries == 0) return CZ_OK;
    const size_t off_stores = 0, off_probes = off_stores + align_up(8 * slots), off_hits = off_probes + align_up(8 * G),
                 off_cval = off_hits + align_up(8 * G), off_stamp = off_cval + align_up(4 * slots);
    const size_t aux = off_stamp + align_up(4);
    void* tab = nullptr;
    void* mem = nullptr;
    e = hipMalloc(&tab, (size_t)ec_table_bytes(log2_entries));
    if (e == hipSuccess) e = hipMalloc(&mem, aux);
    if (e != hipSuccess) {
        (void)hipFree(tab);
        (void)hipGetLastError();
        czi_set_error("cz_search_set_eval_cache: out of device memory for the table (the cache stays off)");
        return e == hipErrorOutOfMemory ? CZ_ERR_NOMEM : serr_hip("cz_search_set_eval_cache: hipMalloc", e);
    }
    e = hipMemset(mem, 0, aux);
    if (e != hipSuccess) { (void)hipFree(tab); (void)hipFree(mem); return serr_hip("cz_search_set_eval_cache: hipMemset", e); }
    char* m = (char*)mem;
    s->ec_mem = mem;
    s->ec_ctr_bytes = off_cval;
    s->C.tab = (EvalCacheEntry*)tab;
    s->C.log2 = log2_entries;
    s->C.s_stores = (unsigned long long*)(m + off_stores);
    s->C.g_probes = (unsigned long long*)(m + off_probes);
    s->C.g_hits = (unsigned long long*)(m + off_hits);
    s->C.s_cval = (float*)(m + off_cval);
    s->C.stamp = (uint32_t*)(m + off_stamp);
    const int rc = cz_search_eval_cache_clear(s, stream);
    if (rc == CZ_OK) e = hipStreamSynchronize(st);
    if (rc != CZ_OK || e != hipSuccess) {
        (void)hipFree(tab);
        (void)hipFree(mem);
        s->C = EvalCache{};
        s->ec_mem = nullptr;
        s->ec_ctr_bytes = 0;
        return rc != CZ_OK ? rc : serr_hip("cz_search_set_eval_cache", e);
    }
    return CZ_OK;
}

int cz_search_eval_cache_info(cz_search* s, uint64_t* out, void* stream)
{
    if (!s || !out) return serr(CZ_ERR_ARG, "cz_search_eval_cache_info: null argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!s->C.tab) return CZ_OK;
    const size_t G = (size_t)s->P.G, slots = G * (size_t)s->P.K;
    unsigned long long* host = new (std::nothrow) unsigned long long[slots + 2 * G];
    if (!host) return serr(CZ_ERR_NOMEM, "cz_search_eval_cache_info: host allocation failed");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(host, s->C.s_stores, 8 * slots, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(host + slots, s->C.g_probes, 8 * G, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(host + slots + G, s->C.g_hits, 8 * G, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
        out[0] = 1ull << s->C.log2;
        for (size_t g = 0; g < G; ++g) { out[1] += host[slots + g]; out[2] += host[slots + G + g]; }
        for (size_t i = 0; i < slots; ++i) out[3] += host[i];
    }
    delete[] host;
    if (e != hipSuccess) return serr_hip("cz_search_eval_cache_info", e);
    return CZ_OK;
}

static_assert(sizeof(cz_visit_entry) == sizeof(VisitEntryHdr) && VISIT_STRIDE == 784, "czero.h: visit entry layout");
static_assert(VISIT_MAX_EDGES == MAXMOVES, "a root has at most MAXMOVES edges");

// Switch side column `col` of the visit ring (VISIT_COLS: one double per slot) on or off; `what` names the entry point in errors
static int record_col(cz_search* s, int col, int on, void* stream, const char* what)
{
    char where[96];
    const auto refuse = [&](const char* why) {
        snprintf(where, sizeof(where), "%s: %s", what, why);
        return serr(CZ_ERR_ARG, where);
    };
    if (!s) return refuse("null handle");
    if (on && !s->V.ring) return refuse("needs cz_search_record_visits on");
    if (on && VISIT_COLS[col].no_script && s->X.n > 0) return refuse("a script is set (cz_search_set_script)");
    double*& ring = s->V.*VISIT_COLS[col].ring;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipStreamSynchronize(st);             // no launch in flight may still use the old buffer
    if (e != hipSuccess) return serr_hip(what, e);
    if (on && ring) return CZ_OK;                        // already on: the ring and what waits in it stay
    (void)hipFree(ring);
    ring = nullptr;
    if (!on) return CZ_OK;
    void* mem = nullptr;
    const size_t bytes = (size_t)s->V.cap * sizeof(double);
    e = hipMalloc(&mem, bytes);
    snprintf(where, sizeof(where), "%s: hipMalloc", what);
    if (e != hipSuccess) return serr_hip(where, e);
    // entries already waiting in the visit ring were written without this record: NaN, "none"
    e = hipMemsetAsync(mem, 0xFF, bytes, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipFree(mem); return serr_hip(what, e); }
    ring = (double*)mem;
    return CZ_OK;
}

int cz_search_record_visits(cz_search* s, int on, int capacity, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_record_visits: null handle");
    if (capacity < 0) return serr(CZ_ERR_ARG, "cz_search_record_visits: capacity < 0");
    if (!on && s->X.n > 0) return serr(CZ_ERR_ARG, "cz_search_record_visits: a script is set (cz_search_set_script)");
    hipStream_t st = (hipStream_t)stream;
    // the side columns share the visit ring's slots: they go with it.  record_col waits for the stream: no launch in
    // flight may still use the old buffers
    for (int k = 0; k < CZ_VISIT_COLS; ++k)
        if (const int rc = record_col(s, k, 0, stream, "cz_search_record_visits")) return rc;
    hipError_t e = hipSuccess;
    (void)hipFree(s->vis_mem);
    s->vis_mem = nullptr;
    s->V = VisitRing{};
    if (!on) return CZ_OK;
    // default: 64 entries per game -- one k_advance launch records at most 8 plies of a game (the loop in k_advance),
    // so a caller that drains at least every 8 rounds never loses an entry
    const long long cap = capacity > 0 ? capacity : 64ll * s->P.G;
    if (cap > 0x7fffffffll) return serr(CZ_ERR_ARG, "cz_search_record_visits: capacity too large");
    const size_t ring_b = align_up((size_t)cap * VISIT_STRIDE), ctl_b = 256, G = (size_t)s->P.G;
    e = hipMalloc(&s->vis_mem, ring_b + ctl_b + align_up(G));
    if (e != hipSuccess) { s->vis_mem = nullptr; return serr_hip("cz_search_record_visits: hipMalloc", e); }
    char* base = (char*)s->vis_mem;
    e = hipMemsetAsync(base + ring_b, 0, ctl_b, st);
    // games already under way lack their earlier plies: they are reported without visits
    if (e == hipSuccess) e = hipMemsetAsync(base + ring_b + ctl_b, s->P.mode == MODE_SELFPLAY ? 1 : 0, G, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipFree(s->vis_mem);
        s->vis_mem = nullptr;
        return serr_hip("cz_search_record_visits", e);
    }
    s->V.ring = (uint8_t*)base;
    s->V.ctl = (unsigned int*)(base + ring_b);
    s->V.dropped = (unsigned long long*)(base + ring_b + 16);   // (cz_search_drain_visits reads ctl and dropped in one copy)
    s->V.g_lost = (uint8_t*)(base + ring_b + ctl_b);
    s->V.cap = (unsigned int)cap;
    return CZ_OK;
}

static_assert(BOOK_MAX + 1 < (1 << 24), "the book index + 1 has to fit bits 8-31 of cz_game_record.flags");
static_assert(CZ_BOOK_MAX == BOOK_MAX, "czero.h: book capacity");

int cz_search_set_book(cz_search* s, const int8_t* boards, int n, double rate, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_book: null handle");
    if (n < 0 || n > BOOK_MAX) return serr(CZ_ERR_ARG, "cz_search_set_book: n outside 0 .. CZ_BOOK_MAX");
    if (n > 0 && !boards) return serr(CZ_ERR_ARG, "cz_search_set_book: null boards");
    if (!(rate >= 0.0 && rate <= 1.0)) return serr(CZ_ERR_ARG, "cz_search_set_book: rate outside [0, 1]");
    if (n > 0 && s->X.n > 0) return serr(CZ_ERR_ARG, "cz_search_set_book: a script is set (cz_search_set_script)");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipStreamSynchronize(st);             // no launch in flight may still read the old book
    if (e != hipSuccess) return serr_hip("cz_search_set_book", e);
    void* mem = nullptr;
    if (n > 0) {                                         // the new book is complete before the old one goes
        e = hipMalloc(&mem, (size_t)n * NSQ);
        if (e != hipSuccess) return serr_hip("cz_search_set_book: hipMalloc", e);
        e = hipMemcpyAsync(mem, boards, (size_t)n * NSQ, hipMemcpyDefault, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { (void)hipFree(mem); return serr_hip("cz_search_set_book", e); }
    }
    (void)hipFree(s->book_mem);
    s->book_mem = mem;
    s->P.book = (const int8_t*)mem;
    s->P.book_n = n;
    s->P.book_rate = n > 0 ? rate : 0.0;
    return CZ_OK;
}

static_assert(CZ_GAME_SCRIPTED == GAME_SCRIPTED && CZ_GAME_SCRIPT_MISMATCH == GAME_SCRIPT_MISMATCH, "czero.h: script flags");

int cz_search_set_script(cz_search* s, const int8_t* init_boards, const uint16_t* labels, const int32_t* offsets,
                         const int8_t* z, int n, void* stream)
{
    const char* const me = "cz_search_set_script";
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_script: null handle");
    if (n < 0) return serr(CZ_ERR_ARG, "cz_search_set_script: n < 0");
    if (n > 0 && (!init_boards || !offsets || !z)) return serr(CZ_ERR_ARG, "cz_search_set_script: null argument");
    if (n > 0) {
        // a script defines the start position, the move and the end of every game: not beside what defines one of them too
        if (!s->V.ring) return serr(CZ_ERR_ARG, "cz_search_set_script: needs cz_search_record_visits on");
        if (s->P.book_n > 0) return serr(CZ_ERR_ARG, "cz_search_set_script: a book is set (cz_search_set_book)");
        for (const VisitCol& c : VISIT_COLS)
            if (c.no_script && s->V.*c.ring) {
                char buf[96];
                snprintf(buf, sizeof(buf), "cz_search_set_script: the %s record is on", c.name);
                return serr(CZ_ERR_ARG, buf);
            }
        if (offsets[0] != 0) return serr(CZ_ERR_ARG, "cz_search_set_script: offsets[0] != 0");
        for (int i = 0; i < n; ++i) {
            if (offsets[i + 1] < offsets[i]) return serr(CZ_ERR_ARG, "cz_search_set_script: offsets decrease");
            if (z[i] < -1 || z[i] > 1) return serr(CZ_ERR_ARG, "cz_search_set_script: z outside -1 .. 1");
        }
        if (offsets[n] > 0 && !labels) return serr(CZ_ERR_ARG, "cz_search_set_script: null labels");
    }
    if (const int rc = admit(s, F_SCRIPT, n > 0, me, stream)) return rc;   // (then no launch in flight reads the old script)
    hipStream_t st = (hipStream_t)stream;
    void* mem = nullptr;
    ScriptState X{};
    if (n > 0) {                                         // the new script is complete before the old one goes
        const size_t total = (size_t)offsets[n];
        const size_t off_lab = align_up((size_t)n * NSQ), off_off = off_lab + align_up(2 * total),
                     off_z = off_off + align_up(4 * ((size_t)n + 1)), off_ctr = off_z + align_up((size_t)n);
        hipError_t e = hipMalloc(&mem, off_ctr + align_up(8));
        if (e != hipSuccess) return serr_hip("cz_search_set_script: hipMalloc", e);
        char* m = (char*)mem;
        e = hipMemsetAsync(m + off_ctr, 0, 8, st);
        if (e == hipSuccess) e = hipMemcpyAsync(m, init_boards, (size_t)n * NSQ, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && total) e = hipMemcpyAsync(m + off_lab, labels, 2 * total, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(m + off_off, offsets, 4 * ((size_t)n + 1), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(m + off_z, z, (size_t)n, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { (void)hipFree(mem); return serr_hip(me, e); }
        X = ScriptState{(const int8_t*)m, (const uint16_t*)(m + off_lab), (const int32_t*)(m + off_off), (const int8_t*)(m + off_z),
                        (unsigned long long*)(m + off_ctr), n};
    }
    (void)hipFree(s->script_mem);
    s->script_mem = mem;
    s->X = X;
    return CZ_OK;
}

int cz_search_script_mismatches(cz_search* s, uint64_t* host_out, void* stream)
{
    if (!s || !host_out) return serr(CZ_ERR_ARG, "cz_search_script_mismatches: null argument");
    *host_out = 0;
    if (s->X.n == 0) return CZ_OK;
    hipError_t e = hipMemcpyAsync(host_out, s->X.mismatches, 8, hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    return e == hipSuccess ? CZ_OK : serr_hip("cz_search_script_mismatches", e);
}

static_assert(CZ_MOVE_FAST == MOVE_FAST && CZ_VISIT_FAST == VISIT_FAST, "czero.h: playout cap flags");

int cz_search_set_playout_cap(cz_search* s, int fast_sims, double full_rate, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_playout_cap: null handle");
    if (fast_sims < 0 || fast_sims > s->P.sims)
        return serr(CZ_ERR_ARG, "cz_search_set_playout_cap: fast_sims outside 0 .. simulation_num_per_move");
    if (fast_sims > 0 && !(full_rate >= 0.0 && full_rate <= 1.0))
        return serr(CZ_ERR_ARG, "cz_search_set_playout_cap: full_rate outside [0, 1]");
    if (const int rc = admit(s, F_CAP, fast_sims > 0, "cz_search_set_playout_cap", stream)) return rc;
    s->P.fast_sims = fast_sims;
    s->P.full_rate = fast_sims > 0 ? full_rate : 0.0;
    return CZ_OK;
}

static_assert(CZ_VISIT_PRUNED == VISIT_PRUNED && sizeof(cz_visit_entry) == sizeof(VisitEntryHdr), "czero.h: visit entry");

static bool finite_nonneg(double x) { return x >= 0.0 && x <= 1.7976931348623157e308; }   // (false for NaN and infinity)

int cz_search_set_forced_playouts(cz_search* s, double k, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_forced_playouts: null handle");
    if (!finite_nonneg(k)) return serr(CZ_ERR_ARG, "cz_search_set_forced_playouts: k negative or not finite");
    if (const int rc = admit(s, F_FORCED, k > 0.0, "cz_search_set_forced_playouts", stream)) return rc;
    s->P.forced_k = k;
    return CZ_OK;
}

static_assert(CZ_VISIT_GUMBEL == VISIT_GUMBEL && CZ_GUMBEL_MAX_M == GUMBEL_MAX_M, "czero.h: Gumbel root search");

// k_root_records, the instantiation of the object's setting (cz_search_set_gumbel_full)
static void launch_root_records(cz_search* s, hipStream_t st, const SearchParams& P, const SearchBuffers& B, int32_t* n,
                                int32_t* raw_total, double* q, double* sv, int gumbel, double* mq = nullptr)
{
    if (P.gumbel_m > 0 && P.gumbel_full)
        hipLaunchKernelGGL(k_root_records<true>, dim3(s->P.G), dim3(64), 0, st, P, B, n, raw_total, q, sv, gumbel, mq);
    else
        hipLaunchKernelGGL(k_root_records<false>, dim3(s->P.G), dim3(64), 0, st, P, B, n, raw_total, q, sv, gumbel, mq);
}

int cz_search_set_gumbel(cz_search* s, int m, double c_visit, double c_scale, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_gumbel: null handle");
    if (m < 0 || m > GUMBEL_MAX_M) return serr(CZ_ERR_ARG, "cz_search_set_gumbel: m outside 0 .. 128");
    if (!finite_nonneg(c_visit) || !finite_nonneg(c_scale))
        return serr(CZ_ERR_ARG, "cz_search_set_gumbel: c_visit or c_scale negative or not finite");
    if (const int rc = admit(s, F_GUMBEL, m > 0, "cz_search_set_gumbel", stream)) return rc;
    s->P.gumbel_m = m;
    s->P.gumbel_visit = c_visit;
    s->P.gumbel_scale = c_scale;
    if (m == 0) s->P.gumbel_full = 0;                           // (the full search is an option of the Gumbel root search)
    return CZ_OK;
}

// ---- MCTS solver (include/czero.h) ---------------------------------------------------------------------------------------
static_assert(CZ_PROOF_OPEN == PROOF_OPEN && CZ_PROOF_WIN == PROOF_WIN && CZ_PROOF_LOSS == PROOF_LOSS &&
              CZ_PROOF_DIST_MAX == PROOF_DIST_MAX, "czero.h: MCTS solver");

int cz_search_set_solver(cz_search* s, int on, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_solver: null handle");
    if (on != 0 && on != 1) return serr(CZ_ERR_ARG, "cz_search_set_solver: on is neither 0 nor 1");
    if (const int rc = admit(s, F_SOLVER, on != 0, "cz_search_set_solver", stream)) return rc;
    s->P.solver = on;
    return CZ_OK;
}

int cz_search_node_proof(cz_search* s, const uint16_t* path, int path_len, int8_t* status, uint8_t* dist, uint8_t* mark,
                         uint8_t* mark_dist, void* stream)
{
    if (!s || path_len < 0 || path_len > MAXD_LDS || (path_len > 0 && !path) || !status || !dist)
        return serr(CZ_ERR_ARG, "cz_search_node_proof: bad argument");
    hipLaunchKernelGGL(k_node_proof, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B, path, path_len, status, dist,
                       mark, mark_dist);
    S_LAUNCH_CHECK("cz_search_node_proof");
    return CZ_OK;
}

int cz_search_root_decided(cz_search* s, uint8_t* out, void* stream)
{
    if (!s || !out) return serr(CZ_ERR_ARG, "cz_search_root_decided: null argument");
    hipLaunchKernelGGL(k_root_decided, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B, out);
    S_LAUNCH_CHECK("cz_search_root_decided");
    return CZ_OK;
}

// ---- moves-left utility (include/czero.h) --------------------------------------------------------------------------------
int cz_search_set_moves_left(cz_search* s, double slope, double cap, const float* x_rows, void* stream)
{
    const char* const me = "cz_search_set_moves_left";
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_moves_left: null handle");
    if (!finite_nonneg(slope) || !finite_nonneg(cap))
        return serr(CZ_ERR_ARG, "cz_search_set_moves_left: slope or cap negative or not finite");
    const bool on = slope > 0.0;
    if (on && !x_rows) return serr(CZ_ERR_ARG, "cz_search_set_moves_left: x_rows is NULL");
    const bool was = s->M.slope > 0.0;
    if (const int rc = admit(s, F_ML, on, me, stream, on && !was)) return rc;
    s->M.slope = slope;
    s->M.cap = cap;
    s->M.x = on ? x_rows : nullptr;
    return blocks_changed(s, was, on, stream);
}

int cz_search_node_moves_left(cz_search* s, const uint16_t* path, int path_len, int64_t* ksum, int32_t* mn, int32_t* k_net,
                              uint8_t* counts, void* stream)
{
    if (!s || path_len < 0 || path_len > MAXD_LDS || (path_len > 0 && !path))
        return serr(CZ_ERR_ARG, "cz_search_node_moves_left: bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (!(s->M.slope > 0.0)) {                                  // off: the trees hold no M records
        const size_t G = (size_t)s->P.G;
        const ZeroOut outs[] = {{ksum, sizeof(int64_t) * G * MAXMOVES}, {mn, sizeof(int32_t) * G * MAXMOVES},
                                {k_net, sizeof(int32_t) * G}, {counts, G}};
        return zero_outputs(outs, "cz_search_node_moves_left", stream);
    }
    hipLaunchKernelGGL(k_node_moves_left, dim3(s->P.G), dim3(64), 0, st, s->P, s->B, path, path_len, (long long*)ksum, mn, k_net,
                       counts);
    S_LAUNCH_CHECK("cz_search_node_moves_left");
    return CZ_OK;
}

int cz_moves_left_quanta(const float* x, int32_t* k, int n, void* stream)
{
    if (!x || !k || n < 0) return serr(CZ_ERR_ARG, "cz_moves_left_quanta: null argument or n < 0");
    if (n == 0) return CZ_OK;
    hipLaunchKernelGGL(k_ml_quanta, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, k, n);
    S_LAUNCH_CHECK("cz_moves_left_quanta");
    return CZ_OK;
}

// ---- draw average (include/czero.h) ----------------------------------------------------------------------------------------
int cz_search_set_draw(cz_search* s, int on_, double score, const float* wdl_rows, void* stream)
{
    const char* const me = "cz_search_set_draw";
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_draw: null handle");
    if (!(score >= -1.0 && score <= 1.0)) return serr(CZ_ERR_ARG, "cz_search_set_draw: score outside [-1, 1] or not finite");
    const bool on = on_ != 0;
    if (on && !wdl_rows) return serr(CZ_ERR_ARG, "cz_search_set_draw: wdl_rows is NULL");
    const bool was = s->D.on != 0;
    if (const int rc = admit(s, F_DRAW, on, me, stream, on && !was)) return rc;
    s->D.on = on ? 1 : 0;
    s->D.score = on ? score : 0.0;
    s->D.wdl = on ? wdl_rows : nullptr;
    return blocks_changed(s, was, on, stream);
}

int cz_search_node_draws(cz_search* s, const uint16_t* path, int path_len, int64_t* dsum, int32_t* dn, int32_t* dq_net,
                         uint8_t* counts, void* stream)
{
    if (!s || path_len < 0 || path_len > MAXD_LDS || (path_len > 0 && !path))
        return serr(CZ_ERR_ARG, "cz_search_node_draws: bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (!s->D.on) {                                             // off: the trees hold no D records
        const size_t G = (size_t)s->P.G;
        const ZeroOut outs[] = {{dsum, sizeof(int64_t) * G * MAXMOVES}, {dn, sizeof(int32_t) * G * MAXMOVES},
                                {dq_net, sizeof(int32_t) * G}, {counts, G}};
        return zero_outputs(outs, "cz_search_node_draws", stream);
    }
    hipLaunchKernelGGL(k_node_draws, dim3(s->P.G), dim3(64), 0, st, s->P, s->B, path, path_len, (long long*)dsum, dn, dq_net, counts);
    S_LAUNCH_CHECK("cz_search_node_draws");
    return CZ_OK;
}

int cz_draw_quanta(const float* d, int stride, int32_t* dq, int n, void* stream)
{
    if (!d || !dq || n < 0 || stride < 1) return serr(CZ_ERR_ARG, "cz_draw_quanta: null argument, n < 0 or stride < 1");
    if (n == 0) return CZ_OK;
    hipLaunchKernelGGL(k_draw_quanta, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d, stride, dq, n);
    S_LAUNCH_CHECK("cz_draw_quanta");
    return CZ_OK;
}

// ---- lower-confidence-bound move choice (include/czero.h) ------------------------------------------------------------------
int cz_search_set_lcb(cz_search* s, double z, double min_ratio, void* stream)
{
    const char* const me = "cz_search_set_lcb";
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_lcb: null handle");
    if (!finite_nonneg(z)) return serr(CZ_ERR_ARG, "cz_search_set_lcb: z negative or not finite");
    if (!(min_ratio >= 0.0 && min_ratio <= 1.0)) return serr(CZ_ERR_ARG, "cz_search_set_lcb: min_ratio outside [0, 1] or not finite");
    const bool on = z > 0.0;
    const bool was = s->Z.on != 0;
    if (const int rc = admit(s, F_LCB, on, me, stream, on && !was)) return rc;
    s->Z.on = on ? 1 : 0;
    s->Z.z = on ? z : 0.0;
    s->Z.ratio = min_ratio;
    return blocks_changed(s, was, on, stream);
}

int cz_search_node_values(cz_search* s, const uint16_t* path, int path_len, double* s2, int32_t* vn, uint8_t* counts,
                          void* stream)
{
    if (!s || path_len < 0 || path_len > MAXD_LDS || (path_len > 0 && !path))
        return serr(CZ_ERR_ARG, "cz_search_node_values: bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (!s->Z.on) {                                             // off: the trees hold no V records
        const size_t G = (size_t)s->P.G;
        const ZeroOut outs[] = {{s2, sizeof(double) * G * MAXMOVES}, {vn, sizeof(int32_t) * G * MAXMOVES}, {counts, G}};
        return zero_outputs(outs, "cz_search_node_values", stream);
    }
    hipLaunchKernelGGL(k_node_values, dim3(s->P.G), dim3(64), 0, st, s->P, s->B, path, path_len, s2, vn, counts);
    S_LAUNCH_CHECK("cz_search_node_values");
    return CZ_OK;
}

int cz_search_root_lcb(cz_search* s, double* lcb, int32_t* pick, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_root_lcb: null handle");
    if (!s->Z.on) return serr(CZ_ERR_ARG, "cz_search_root_lcb: the lower-confidence-bound move choice is off (cz_search_set_lcb)");
    hipLaunchKernelGGL(k_root_lcb, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B, s->Z, lcb, pick);
    S_LAUNCH_CHECK("cz_search_root_lcb");
    return CZ_OK;
}

int cz_lcb_pick(const uint16_t* labels, const int32_t* n, const double* w, const double* s2, const int32_t* vn,
                const uint8_t* n_edges, int rows, double z, double min_ratio, double* out_lcb, int32_t* out_pick, void* stream)
{
    if (!labels || !n || !w || !s2 || !vn || !n_edges || rows < 0) return serr(CZ_ERR_ARG, "cz_lcb_pick: null argument or rows < 0");
    if (!finite_nonneg(z) || !(min_ratio >= 0.0 && min_ratio <= 1.0))
        return serr(CZ_ERR_ARG, "cz_lcb_pick: z negative or not finite, or min_ratio outside [0, 1]");
    if (rows == 0) return CZ_OK;
    hipLaunchKernelGGL(k_lcb_rows, dim3(rows), dim3(64), 0, (hipStream_t)stream, labels, n, w, s2, vn, n_edges, rows, z, min_ratio,
                       out_lcb, out_pick);
    S_LAUNCH_CHECK("cz_lcb_pick");
    return CZ_OK;
}

// ---- early stop of a settled ply (include/czero.h) ----------------------------------------------------------------------
static_assert(CZ_VISIT_EARLY == VISIT_EARLY, "czero.h: stop rules");

// The per-game state exists exactly while a rule is on (s->S.gain > 0 or s->S.lead); the stream is idle when this runs.
static int stop_state_update(cz_search* s, hipStream_t st, const char* what)
{
    const bool want = s->S.gain > 0.0 || s->S.lead != 0;
    if (want == (s->stop_mem != nullptr)) return CZ_OK;
    const auto no_state = [s] {
        s->S.prev_n = nullptr; s->S.prev_sum = nullptr; s->S.start_tasks = nullptr; s->S.last_gain = nullptr;
        s->S.checks = nullptr; s->S.cut = nullptr;
    };
    if (!want) {
        (void)hipFree(s->stop_mem);
        s->stop_mem = nullptr;
        s->stop_bytes = 0;
        no_state();
        return CZ_OK;
    }
    const size_t G = (size_t)s->P.G;
    const size_t off_gain = 0, off_prev = off_gain + align_up(8 * G), off_sum = off_prev + align_up(4 * G * MAXMOVES),
                 off_start = off_sum + align_up(4 * G), off_checks = off_start + align_up(4 * G),
                 off_cut = off_checks + align_up(4 * G), bytes = off_cut + align_up(G);
    void* mem = nullptr;
    hipError_t e = hipMalloc(&mem, bytes);
    if (e != hipSuccess) return serr_hip(what, e);
    e = hipMemsetAsync(mem, 0, bytes, st);
    if (e != hipSuccess) { (void)hipFree(mem); return serr_hip(what, e); }
    char* m = (char*)mem;
    s->S.last_gain = (double*)(m + off_gain);
    s->S.prev_n = (int32_t*)(m + off_prev);
    s->S.prev_sum = (int32_t*)(m + off_sum);
    s->S.start_tasks = (int32_t*)(m + off_start);
    s->S.checks = (int32_t*)(m + off_checks);
    s->S.cut = (uint8_t*)(m + off_cut);
    // searches under way count as begun now: empty snapshots, the first test point they reach starts their count
    hipLaunchKernelGGL(k_stop_reset, dim3((s->P.G + 255) / 256), dim3(256), 0, st, s->S, s->P.G, (const uint8_t*)nullptr);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipFree(mem);
        no_state();
        return serr_hip(what, e);
    }
    s->stop_mem = mem;
    s->stop_bytes = bytes;
    return CZ_OK;
}

int cz_search_set_kld_gain(cz_search* s, double gain, int interval, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_kld_gain: null handle");
    if (!finite_nonneg(gain)) return serr(CZ_ERR_ARG, "cz_search_set_kld_gain: gain negative or not finite");
    if (interval < 1) return serr(CZ_ERR_ARG, "cz_search_set_kld_gain: interval < 1");
    if (const int rc0 = admit(s, F_KLD, gain > 0.0, "cz_search_set_kld_gain", stream)) return rc0;
    const double old_gain = s->S.gain;
    const int old_interval = s->S.interval;
    s->S.gain = gain;
    s->S.interval = interval;
    const int rc = stop_state_update(s, (hipStream_t)stream, "cz_search_set_kld_gain");
    if (rc != CZ_OK) { s->S.gain = old_gain; s->S.interval = old_interval; }
    return rc;
}

int cz_search_set_smart_pruning(cz_search* s, int on, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_smart_pruning: null handle");
    if (on != 0 && on != 1) return serr(CZ_ERR_ARG, "cz_search_set_smart_pruning: on is neither 0 nor 1");
    if (const int rc0 = admit(s, F_LEAD, on != 0, "cz_search_set_smart_pruning", stream)) return rc0;
    const int old = s->S.lead;
    s->S.lead = on;
    const int rc = stop_state_update(s, (hipStream_t)stream, "cz_search_set_smart_pruning");
    if (rc != CZ_OK) s->S.lead = old;
    return rc;
}

int cz_search_root_kld(cz_search* s, double* gain, int32_t* checks, void* stream)
{
    if (!s || !gain || !checks) return serr(CZ_ERR_ARG, "cz_search_root_kld: null argument");
    const size_t G = (size_t)s->P.G;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (s->stop_mem) {
        e = hipMemcpyAsync(gain, s->S.last_gain, sizeof(double) * G, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(checks, s->S.checks, sizeof(int32_t) * G, hipMemcpyDeviceToDevice, st);
    } else {                                                    // both rules off: nothing measured (NaN), no checkpoint
        e = hipMemsetAsync(gain, 0xFF, sizeof(double) * G, st);
        if (e == hipSuccess) e = hipMemsetAsync(checks, 0, sizeof(int32_t) * G, st);
    }
    return e == hipSuccess ? CZ_OK : serr_hip("cz_search_root_kld", e);
}

int cz_search_set_gumbel_full(cz_search* s, int on, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_gumbel_full: null handle");
    if (on != 0 && on != 1) return serr(CZ_ERR_ARG, "cz_search_set_gumbel_full: on is neither 0 nor 1");
    if (on && s->P.gumbel_m == 0)
        return serr(CZ_ERR_ARG, "cz_search_set_gumbel_full: the Gumbel root search is off (cz_search_set_gumbel)");
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);   // launches in flight keep the setting they started with
    if (e != hipSuccess) return serr_hip("cz_search_set_gumbel_full", e);
    s->P.gumbel_full = on;
    return CZ_OK;
}

int cz_search_node_net_value(cz_search* s, const uint16_t* path, int path_len, float* v, void* stream)
{
    if (!s || !v || path_len < 0 || (path_len > 0 && !path)) return serr(CZ_ERR_ARG, "cz_search_node_net_value: bad argument");
    hipLaunchKernelGGL(k_node_net_value, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B, path, path_len, v);
    S_LAUNCH_CHECK("cz_search_node_net_value");
    return CZ_OK;
}

int cz_search_root_started(cz_search* s, int32_t* started, void* stream)
{
    if (!s || !started) return serr(CZ_ERR_ARG, "cz_search_root_started: null argument");
    hipError_t e = hipMemcpyAsync(started, s->B.g_started, sizeof(int32_t) * (size_t)s->P.G * MAXMOVES,
                                  hipMemcpyDeviceToDevice, (hipStream_t)stream);
    return e == hipSuccess ? CZ_OK : serr_hip("cz_search_root_started", e);
}

int cz_search_gumbel_draws(cz_search* s, double* draws, void* stream)
{
    if (!s || !draws) return serr(CZ_ERR_ARG, "cz_search_gumbel_draws: null argument");
    hipError_t e = hipMemcpyAsync(draws, s->B.g_gumbel, sizeof(double) * (size_t)s->P.G * MAXMOVES,
                                  hipMemcpyDeviceToDevice, (hipStream_t)stream);
    return e == hipSuccess ? CZ_OK : serr_hip("cz_search_gumbel_draws", e);
}

int cz_search_gumbel_targets(cz_search* s, int32_t* m, int32_t* raw_total, void* stream)
{
    if (!s || !m || !raw_total) return serr(CZ_ERR_ARG, "cz_search_gumbel_targets: null argument");
    launch_root_records(s, (hipStream_t)stream, s->P, s->B, m, raw_total,
                       (double*)nullptr, (double*)nullptr, 1);
    S_LAUNCH_CHECK("cz_search_gumbel_targets");
    return CZ_OK;
}

int cz_gumbel_policy_target(const uint16_t* labels, const int32_t* n, const double* w, const float* p,
                            const uint8_t* n_edges, int rows, double c_visit, double c_scale, int32_t* out_m,
                            int32_t* out_raw_total, void* stream)
{
    if (!labels || !n || !w || !p || !n_edges || !out_m || !out_raw_total || rows < 0)
        return serr(CZ_ERR_ARG, "cz_gumbel_policy_target: null argument or rows < 0");
    if (!finite_nonneg(c_visit) || !finite_nonneg(c_scale))
        return serr(CZ_ERR_ARG, "cz_gumbel_policy_target: c_visit or c_scale negative or not finite");
    if (rows == 0) return CZ_OK;
    hipLaunchKernelGGL(k_gumbel_rows<false>, dim3(rows), dim3(64), 0, (hipStream_t)stream, labels, n, w, p, n_edges, rows,
                       c_visit, c_scale, out_m, out_raw_total, (const float*)nullptr);
    S_LAUNCH_CHECK("cz_gumbel_policy_target");
    return CZ_OK;
}

int cz_gumbel_policy_target_v(const uint16_t* labels, const int32_t* n, const double* w, const float* p,
                              const uint8_t* n_edges, const float* v, int rows, double c_visit, double c_scale,
                              int32_t* out_m, int32_t* out_raw_total, void* stream)
{
    if (!labels || !n || !w || !p || !n_edges || !v || !out_m || !out_raw_total || rows < 0)
        return serr(CZ_ERR_ARG, "cz_gumbel_policy_target_v: null argument or rows < 0");
    if (!finite_nonneg(c_visit) || !finite_nonneg(c_scale))
        return serr(CZ_ERR_ARG, "cz_gumbel_policy_target_v: c_visit or c_scale negative or not finite");
    if (rows == 0) return CZ_OK;
    hipLaunchKernelGGL(k_gumbel_rows<true>, dim3(rows), dim3(64), 0, (hipStream_t)stream, labels, n, w, p, n_edges, rows,
                       c_visit, c_scale, out_m, out_raw_total, v);
    S_LAUNCH_CHECK("cz_gumbel_policy_target_v");
    return CZ_OK;
}

int cz_gumbel_interior_pick(const int32_t* n, const double* w, const float* p, const uint8_t* n_edges, const float* v,
                            int rows, double c_visit, double c_scale, int32_t* out_pick, double* out_score, void* stream)
{
    if (!n || !w || !p || !n_edges || !v || !out_pick || !out_score || rows < 0)
        return serr(CZ_ERR_ARG, "cz_gumbel_interior_pick: null argument or rows < 0");
    if (!finite_nonneg(c_visit) || !finite_nonneg(c_scale))
        return serr(CZ_ERR_ARG, "cz_gumbel_interior_pick: c_visit or c_scale negative or not finite");
    if (rows == 0) return CZ_OK;
    hipLaunchKernelGGL(k_gumbel_interior_rows, dim3(rows), dim3(64), 0, (hipStream_t)stream, n, w, p, n_edges, v, rows,
                       c_visit, c_scale, out_pick, out_score);
    S_LAUNCH_CHECK("cz_gumbel_interior_pick");
    return CZ_OK;
}

// ---- the schedule of c_puct and the policy temperature (include/czero.h) ---------------------------------------------------
// Plain parameters of the kernels that are launched anyway: no entry in FEATURES, nothing excludes them.
static bool cpuct_schedule_ok(double factor, double base) { return finite_nonneg(factor) && finite_nonneg(base) && base >= 1.0; }

int cz_search_set_cpuct_schedule(cz_search* s, double factor, double base, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_cpuct_schedule: null handle");
    if (!cpuct_schedule_ok(factor, base))
        return serr(CZ_ERR_ARG, "cz_search_set_cpuct_schedule: factor negative or not finite, or base below 1 or not finite");
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream);   // launches in flight keep the schedule they started with
    if (e != hipSuccess) return serr_hip("cz_search_set_cpuct_schedule", e);
    s->P.cpuct_factor = factor;
    s->P.cpuct_base = base;
    return CZ_OK;
}

int cz_search_set_policy_temperature(cz_search* s, double T, void* stream)
{
    const char* const me = "cz_search_set_policy_temperature";
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_policy_temperature: null handle");
    if (!(T >= 0.1 && T <= 10.0)) return serr(CZ_ERR_ARG, "cz_search_set_policy_temperature: T outside [0.1, 10] or not finite");
    const float inv_t = (float)(1.0 / T);
    if (inv_t != 1.0f && !s->P.policy_logits)
        return serr(CZ_ERR_ARG, "cz_search_set_policy_temperature: the policy rows are probabilities, a temperature needs logit rows "
                                "(cz_search_policy_logits)");
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return serr_hip(me, e);
    if (inv_t == s->P.inv_temp) return CZ_OK;
    s->P.inv_temp = inv_t;
    // the stored priors were formed at the old temperature: the trees start over and the evaluation cache is emptied
    int rc = cz_search_reset_trees(s, stream);
    if (rc == CZ_OK) rc = cz_search_eval_cache_clear(s, stream);
    if (rc != CZ_OK) return rc;
    e = hipStreamSynchronize((hipStream_t)stream);
    return e == hipSuccess ? CZ_OK : serr_hip(me, e);
}

int cz_debug_cpuct(const int32_t* sum_n, int rows, double c_puct, double factor, double base, double* out_c, float* out_c32,
                   void* stream)
{
    if (!sum_n || !out_c || !out_c32 || rows < 0) return serr(CZ_ERR_ARG, "cz_debug_cpuct: null argument or rows < 0");
    if (!finite_nonneg(c_puct) || !cpuct_schedule_ok(factor, base))
        return serr(CZ_ERR_ARG, "cz_debug_cpuct: c_puct or factor negative or not finite, or base below 1 or not finite");
    if (rows == 0) return CZ_OK;
    hipLaunchKernelGGL(k_cpuct_rows, dim3(rows), dim3(64), 0, (hipStream_t)stream, sum_n, rows, c_puct, factor,
                       base, out_c, out_c32);
    S_LAUNCH_CHECK("cz_debug_cpuct");
    return CZ_OK;
}

int cz_search_set_leaf_mirror(cz_search* s, double rate, uint8_t* flags_or_null, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_leaf_mirror: null handle");
    if (!(rate >= 0.0 && rate <= 1.0)) return serr(CZ_ERR_ARG, "cz_search_set_leaf_mirror: rate outside [0, 1]");   // (NaN too)
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipStreamSynchronize(st);   // launches in flight keep the rate and the flag array they started with
    if (e == hipSuccess && flags_or_null && flags_or_null != s->B.leaf_flags) {
        // a new array starts as the old one (the leaves in flight keep their flags), or as zeros where there was none
        const size_t n = (size_t)s->P.G * (size_t)s->P.K;
        e = s->B.leaf_flags ? hipMemcpyAsync(flags_or_null, s->B.leaf_flags, n, hipMemcpyDeviceToDevice, st)
                            : hipMemsetAsync(flags_or_null, 0, n, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) return serr_hip("cz_search_set_leaf_mirror", e);
    s->P.leaf_mirror = rate;
    s->B.leaf_flags = flags_or_null;
    return CZ_OK;
}

int cz_search_root_targets(cz_search* s, int32_t* n, int32_t* raw_total, void* stream)
{
    if (!s || !n || !raw_total) return serr(CZ_ERR_ARG, "cz_search_root_targets: null argument");
    launch_root_records(s, (hipStream_t)stream, s->P, s->B, n, raw_total,
                       (double*)nullptr, (double*)nullptr, 0);
    S_LAUNCH_CHECK("cz_search_root_targets");
    return CZ_OK;
}

int cz_policy_target_prune(const uint16_t* labels, const int32_t* n, const double* w, const float* p,
                           const uint8_t* n_edges, int rows, double c_puct, double k, int32_t* out_n,
                           int32_t* out_raw_total, void* stream)
{
    if (!labels || !n || !w || !p || !n_edges || !out_n || !out_raw_total || rows < 0)
        return serr(CZ_ERR_ARG, "cz_policy_target_prune: null argument or rows < 0");
    if (!finite_nonneg(k) || !finite_nonneg(c_puct))
        return serr(CZ_ERR_ARG, "cz_policy_target_prune: k or c_puct negative or not finite");
    if (rows == 0) return CZ_OK;
    hipLaunchKernelGGL(k_row_records, dim3(rows), dim3(64), 0, (hipStream_t)stream, labels, (const int32_t*)nullptr, n, w, p,
                       n_edges, rows, c_puct, k, out_n, out_raw_total, (double*)nullptr, (double*)nullptr, (double*)nullptr);
    S_LAUNCH_CHECK("cz_policy_target_prune");
    return CZ_OK;
}

int cz_search_record_values(cz_search* s, int on, void* stream)
{
    return record_col(s, CZ_VISIT_COL_Q, on, stream, "cz_search_record_values");
}

int cz_search_root_value(cz_search* s, double* q, void* stream)
{
    if (!s || !q) return serr(CZ_ERR_ARG, "cz_search_root_value: null argument");
    launch_root_records(s, (hipStream_t)stream, s->P, s->B, (int32_t*)nullptr,
                       (int32_t*)nullptr, q, (double*)nullptr, 0);
    S_LAUNCH_CHECK("cz_search_root_value");
    return CZ_OK;
}

int cz_root_value(const uint16_t* labels, const int32_t* m, const int32_t* n, const double* w, const uint8_t* n_edges,
                  int rows, double* out_q, void* stream)
{
    if (!labels || !m || !n || !w || !n_edges || !out_q || rows < 0)
        return serr(CZ_ERR_ARG, "cz_root_value: null argument or rows < 0");
    if (rows == 0) return CZ_OK;
    hipLaunchKernelGGL(k_row_records, dim3(rows), dim3(64), 0, (hipStream_t)stream, labels, m, n, w, (const float*)nullptr,
                       n_edges, rows, 0.0, 0.0, (int32_t*)nullptr, (int32_t*)nullptr, out_q, (double*)nullptr, (double*)nullptr);
    S_LAUNCH_CHECK("cz_root_value");
    return CZ_OK;
}

static_assert(CZ_SURPRISE_BOUND == 70 && SURPRISE_R_FLOOR == 1e-30, "czero.h: ln(1 / the floor) = 69.08 < the bound");

int cz_search_record_surprise(cz_search* s, int on, void* stream)
{
    return record_col(s, CZ_VISIT_COL_S, on, stream, "cz_search_record_surprise");
}

int cz_search_root_surprise(cz_search* s, double* out, void* stream)
{
    if (!s || !out) return serr(CZ_ERR_ARG, "cz_search_root_surprise: null argument");
    launch_root_records(s, (hipStream_t)stream, s->P, s->B, (int32_t*)nullptr,
                       (int32_t*)nullptr, (double*)nullptr, out, 0);
    S_LAUNCH_CHECK("cz_search_root_surprise");
    return CZ_OK;
}

int cz_root_surprise(const uint16_t* labels, const int32_t* m, const float* p, const uint8_t* n_edges, int rows,
                     double* out, void* stream)
{
    if (!labels || !m || !p || !n_edges || !out || rows < 0)
        return serr(CZ_ERR_ARG, "cz_root_surprise: null argument or rows < 0");
    if (rows == 0) return CZ_OK;
    hipLaunchKernelGGL(k_row_records, dim3(rows), dim3(64), 0, (hipStream_t)stream, labels, m, (const int32_t*)nullptr,
                       (const double*)nullptr, p, n_edges, rows, 0.0, 0.0, (int32_t*)nullptr, (int32_t*)nullptr,
                       (double*)nullptr, out, (double*)nullptr);
    S_LAUNCH_CHECK("cz_root_surprise");
    return CZ_OK;
}

static_assert(CZ_VISIT_NO_RESIGN == VISIT_NO_RESIGN, "czero.h: max-q record flag");

int cz_search_record_maxq(cz_search* s, int on, void* stream)
{
    return record_col(s, CZ_VISIT_COL_MAXQ, on, stream, "cz_search_record_maxq");
}

int cz_search_root_maxq(cz_search* s, double* out, void* stream)
{
    if (!s || !out) return serr(CZ_ERR_ARG, "cz_search_root_maxq: null argument");
    launch_root_records(s, (hipStream_t)stream, s->P, s->B, (int32_t*)nullptr,
                       (int32_t*)nullptr, (double*)nullptr, (double*)nullptr, 0, out);
    S_LAUNCH_CHECK("cz_search_root_maxq");
    return CZ_OK;
}

int cz_root_maxq(const uint16_t* labels, const int32_t* n, const double* w, const uint8_t* n_edges, int rows, double* out,
                 void* stream)
{
    if (!labels || !n || !w || !n_edges || !out || rows < 0)
        return serr(CZ_ERR_ARG, "cz_root_maxq: null argument or rows < 0");
    if (rows == 0) return CZ_OK;
    hipLaunchKernelGGL(k_row_records, dim3(rows), dim3(64), 0, (hipStream_t)stream, labels, (const int32_t*)nullptr, n, w,
                       (const float*)nullptr, n_edges, rows, 0.0, 0.0, (int32_t*)nullptr, (int32_t*)nullptr,
                       (double*)nullptr, (double*)nullptr, out);
    S_LAUNCH_CHECK("cz_root_maxq");
    return CZ_OK;
}

int cz_search_set_resign_threshold(cz_search* s, double t, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_resign_threshold: null handle");
    if (!(t >= -1.7976931348623157e308 && t <= 1.7976931348623157e308))                   // (false for NaN and infinity)
        return serr(CZ_ERR_ARG, "cz_search_set_resign_threshold: t not finite");
    const hipError_t e = hipStreamSynchronize((hipStream_t)stream);   // launches in flight keep the threshold they started with
    if (e != hipSuccess) return serr_hip("cz_search_set_resign_threshold", e);
    s->P.resign_threshold = t;
    return CZ_OK;
}

int cz_search_drain_visits_cols(cz_search* s, void* host_buf, double* const cols[CZ_VISIT_COLS], int max_entries, int* n_out,
                                uint64_t* dropped_out, void* stream)
{
    if (!s || !n_out || max_entries < 0) return serr(CZ_ERR_ARG, "cz_search_drain_visits_cols: bad argument");
    if (!s->V.ring) return serr(CZ_ERR_ARG, "cz_search_drain_visits_cols: visit recording is off");
    if (!host_buf) cols = nullptr;                       // a count copies nothing
    for (int c = 0; cols && c < CZ_VISIT_COLS; ++c)
        if (cols[c] && !(s->V.*VISIT_COLS[c].ring)) {
            char buf[96];
            snprintf(buf, sizeof(buf), "cz_search_drain_visits_cols: the %s record is off", VISIT_COLS[c].name);
            return serr(CZ_ERR_ARG, buf);
        }
    hipStream_t st = (hipStream_t)stream;
    unsigned int ctl[6] = {0u, 0u, 0u, 0u, 0u, 0u};        // tail, head, -, -, dropped (64 bit): one copy
    static_assert(sizeof(unsigned long long) == 8, "dropped counter is 64-bit");
    hipError_t e = hipMemcpyAsync(ctl, s->V.ctl, sizeof(ctl), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return serr_hip("cz_search_drain_visits_cols", e);
    unsigned long long dropped = 0ull;
    memcpy(&dropped, &ctl[4], sizeof(dropped));
    const unsigned int tail = ctl[0], head = ctl[1], cap = s->V.cap;
    // reservations at or beyond head + cap were dropped by the kernel (and counted): the valid entries are [head, head + cap)
    const unsigned int valid = tail - head < cap ? tail - head : cap;
    if (dropped_out) *dropped_out = (uint64_t)dropped;
    if (!host_buf) { *n_out = (int)valid; return CZ_OK; }
    // all or nothing: a partial drain would have to remember where the dropped reservations lie
    if (valid > (unsigned int)max_entries)
        return serr(CZ_ERR_ARG, "cz_search_drain_visits_cols: host_buf holds fewer entries than are waiting (ask with host_buf = NULL)");
    const unsigned int k = valid;
    unsigned int done = 0;
    while (done < k && e == hipSuccess) {                // at most two runs: the ring may wrap once
        const unsigned int at = (head + done) % cap;
        const unsigned int run = (cap - at) < (k - done) ? (cap - at) : (k - done);
        e = hipMemcpyAsync((char*)host_buf + (size_t)done * VISIT_STRIDE, s->V.ring + (size_t)at * VISIT_STRIDE,
                           (size_t)run * VISIT_STRIDE, hipMemcpyDeviceToHost, st);
        for (int c = 0; cols && c < CZ_VISIT_COLS; ++c)
            if (cols[c] && e == hipSuccess)
                e = hipMemcpyAsync(cols[c] + done, s->V.*VISIT_COLS[c].ring + at, (size_t)run * sizeof(double),
                                   hipMemcpyDeviceToHost, st);
        done += run;
    }
    const unsigned int new_head = tail;
    if (e == hipSuccess) e = hipMemcpyAsync(s->V.ctl + 1, &new_head, sizeof(new_head), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return serr_hip("cz_search_drain_visits_cols", e);
    *n_out = (int)k;
    return CZ_OK;
}

int cz_search_drain_visits(cz_search* s, void* host_buf, int max_entries, int* n_out, uint64_t* dropped_out, void* stream)
{
    return cz_search_drain_visits_cols(s, host_buf, nullptr, max_entries, n_out, dropped_out, stream);
}

int cz_search_reset_trees(cz_search* s, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_reset_trees: null handle");
    hipLaunchKernelGGL(k_pool_commit, dim3(1), dim3(1), 0, (hipStream_t)stream, s->B);
    hipLaunchKernelGGL(k_reset_trees, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B);
    S_LAUNCH_CHECK("cz_search_reset_trees");
    return CZ_OK;
}

int cz_search_pending(cz_search* s, int* host_out, void* stream)
{
    if (!s || !host_out) return serr(CZ_ERR_ARG, "cz_search_pending: null argument");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(s->B.pending, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return serr_hip("cz_search_pending", e);
    hipLaunchKernelGGL(k_pending, dim3((s->P.G + 255) / 256), dim3(256), 0, st, s->P, s->B);
    S_LAUNCH_CHECK("cz_search_pending");
    int32_t v = 0;
    e = hipMemcpyAsync(&v, s->B.pending, sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return serr_hip("cz_search_pending", e);
    *host_out = v;
    return CZ_OK;
}

int cz_search_leaf_rows(cz_search* s, int32_t* rows, int32_t* counts_dev, int* host_out, void* stream)
{
    if (!s || !rows || !counts_dev || !host_out) return serr(CZ_ERR_ARG, "cz_search_leaf_rows: null argument");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(counts_dev, 0, 2 * sizeof(int32_t), st);
    if (e != hipSuccess) return serr_hip("cz_search_leaf_rows", e);
    const int n = s->P.G * s->P.K;
    hipLaunchKernelGGL(k_leaf_rows, dim3((n + 255) / 256), dim3(256), 0, st, s->P, s->B, rows, counts_dev);
    S_LAUNCH_CHECK("cz_search_leaf_rows");
    int32_t v[2] = {0, 0};
    e = hipMemcpyAsync(v, counts_dev, sizeof(v), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return serr_hip("cz_search_leaf_rows", e);
    host_out[0] = v[0];
    host_out[1] = v[1];
    return CZ_OK;
}

int cz_search_root_stats(cz_search* s, uint16_t* moves, int32_t* n, double* w, float* p, int32_t* sum_n,
                         uint8_t* counts, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_root_stats: null handle");
    hipLaunchKernelGGL(k_root_stats, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B, (const uint16_t*)nullptr, 0,
                       moves, n, w, p, sum_n, counts);
    S_LAUNCH_CHECK("cz_search_root_stats");
    return CZ_OK;
}

int cz_search_stop(cz_search* s, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_stop: null handle");
    hipLaunchKernelGGL(k_stop, dim3((s->P.G + 255) / 256), dim3(256), 0, (hipStream_t)stream, s->P, s->B);
    S_LAUNCH_CHECK("cz_search_stop");
    return CZ_OK;
}

int cz_search_node_stats(cz_search* s, const uint16_t* path, int path_len, uint16_t* moves, int32_t* n, double* w,
                         float* p, int32_t* sum_n, uint8_t* counts, void* stream)
{
    if (!s || path_len < 0 || (path_len > 0 && !path)) return serr(CZ_ERR_ARG, "cz_search_node_stats: bad argument");
    hipLaunchKernelGGL(k_root_stats, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B, path, path_len, moves, n, w,
                       p, sum_n, counts);
    S_LAUNCH_CHECK("cz_search_node_stats");
    return CZ_OK;
}

int cz_search_pv(cz_search* s, int max_len, uint16_t* moves, int32_t* visits, void* stream)
{
    if (!s || !moves || !visits || max_len < 1) return serr(CZ_ERR_ARG, "cz_search_pv: bad argument");
    if (s->Z.on) hipLaunchKernelGGL(k_pv_lcb, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B, max_len, moves, visits, s->Z);
    else hipLaunchKernelGGL(k_pv, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B, max_len, moves, visits);
    S_LAUNCH_CHECK("cz_search_pv");
    return CZ_OK;
}

int cz_search_choose(cz_search* s, const double* u, int32_t* action, void* stream)
{
    if (!s || !action) return serr(CZ_ERR_ARG, "cz_search_choose: null argument");
    if (s->Z.on) hipLaunchKernelGGL(k_choose_lcb, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B, u, action, s->Z);
    else if (s->P.solver) hipLaunchKernelGGL(k_choose<true>, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B, u, action);
    else hipLaunchKernelGGL(k_choose<false>, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B, u, action);
    S_LAUNCH_CHECK("cz_search_choose");
    return CZ_OK;
}

int cz_search_counters(cz_search* s, uint64_t* host_out, void* stream)
{
    if (!s || !host_out) return serr(CZ_ERR_ARG, "cz_search_counters: null argument");
    const size_t n = (size_t)s->P.G * CT_COUNT;
    unsigned long long* tmp = new (std::nothrow) unsigned long long[n];
    if (!tmp) return serr(CZ_ERR_NOMEM, "cz_search_counters: host allocation failed");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(tmp, s->B.counters, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { delete[] tmp; return serr_hip("cz_search_counters", e); }
    for (int c = 0; c < CT_COUNT; ++c) host_out[c] = 0;
    for (int g = 0; g < s->P.G; ++g)
        for (int c = 0; c < CT_COUNT; ++c) {
            const unsigned long long v = tmp[(size_t)g * CT_COUNT + c];
            if (c == CT_MAX_DEPTH) { if (v > host_out[c]) host_out[c] = v; }
            else host_out[c] += v;
        }
    delete[] tmp;
    return CZ_OK;
}

int cz_search_game_counters(cz_search* s, uint64_t* host_out, void* stream)
{
    if (!s || !host_out) return serr(CZ_ERR_ARG, "cz_search_game_counters: null argument");
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "counters are 64-bit");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(host_out, s->B.counters, (size_t)s->P.G * CT_COUNT * sizeof(uint64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return serr_hip("cz_search_game_counters", e);
    return CZ_OK;
}

int cz_search_drain_records(cz_search* s, unsigned int* cursor, void* host_buf, int max_records, int* n_out, void* stream)
{
    if (!s || !cursor || !host_buf || !n_out) return serr(CZ_ERR_ARG, "cz_search_drain_records: null argument");
    hipStream_t st = (hipStream_t)stream;
    unsigned int tail = 0;
    hipError_t e = hipMemcpyAsync(&tail, s->B.ring_tail, sizeof(tail), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return serr_hip("cz_search_drain_records", e);
    unsigned int cur = *cursor;
    if (tail - cur > (unsigned)s->P.ring_cap) cur = tail - (unsigned)s->P.ring_cap;   // overwritten records are lost
    int n = 0;
    while (cur != tail && n < max_records) {
        const size_t off = (size_t)(cur % (unsigned)s->P.ring_cap) * s->P.record_stride;
        e = hipMemcpyAsync((char*)host_buf + (size_t)n * s->P.record_stride, s->B.ring + off, s->P.record_stride,
                           hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) return serr_hip("cz_search_drain_records", e);
        ++cur; ++n;
    }
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return serr_hip("cz_search_drain_records", e);
    *cursor = cur;
    *n_out = n;
    return CZ_OK;
}

int cz_debug_noise(uint64_t seed, uint32_t game_key, double alpha, int n_moves, double* out, int n, void* stream)
{
    if (n <= 0) return CZ_OK;
    if (!out || n_moves < 1 || n_moves > MAXMOVES || !(alpha > 0.0)) return serr(CZ_ERR_ARG, "cz_debug_noise: bad argument");
    hipLaunchKernelGGL(k_debug_noise, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed, game_key, (float)alpha,
                       n_moves, out, n);
    S_LAUNCH_CHECK("cz_debug_noise");
    return CZ_OK;
}

int cz_debug_sqrt(const int32_t* x, double* y, int n, void* stream)
{
    if (n <= 0) return CZ_OK;
    hipLaunchKernelGGL(k_debug_sqrt, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, y, n);
    S_LAUNCH_CHECK("cz_debug_sqrt");
    return CZ_OK;
}

}  // extern "C"
