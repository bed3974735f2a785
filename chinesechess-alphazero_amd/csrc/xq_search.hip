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
// The host then runs ONE network forward over the whole queue.
// There is no host decision inside a round and no device->host copy, so a round (kernel + network
// forward) can be replayed from a HIP graph.
//
// Arithmetic follows the reference bit for bit: priors float32 (summed in move order),
// sqrt / Q / U in float64 with the float32 product c_puct*p for non-root nodes, W float64.
// Build with -ffp-contract=off.
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

namespace {

constexpr int MAXD_LDS = 128;          // LDS copy of the current path; SearchParams.max_depth <= this
constexpr int INIT_NIB_WORDS = KEY_WORDS;


struct SearchLDS {
    RulesLDS r;
    uint32_t key[KEY_WORDS + 4];
    int32_t path_node[MAXD_LDS];
    int32_t path_edge[MAXD_LDS];
    unsigned long long ctr[CT_COUNT];  // counter accumulators of the running kernel
    uint8_t codes[BOARD_LDS];          // plane codes of the leaf being encoded
    double dsc[MAXMOVES];              // sampling scratch
    double cdf[MAXMOVES];
    float pr[MAXMOVES];                // prior gather scratch
    uint16_t slab[MAXMOVES];           // labels sorted
    int32_t sn[MAXMOVES];              // visit counts sorted by label
    uint32_t chtab[MAX_CHUNKS];        // the game's chunk table (pool chunk number of local chunk i)
};

// one edge's visit statistics (ActionState n / w + the child link); edge j of a node = granule stat + j
struct __attribute__((aligned(16))) EdgeStat {
    double w;
    int32_t n;
    int32_t child;          // node id; CHILD_UNKNOWN / CHILD_TERM_*
};
static_assert(sizeof(EdgeStat) == 16, "one granule per edge");

// node record: key[12] | {sum_n, meta, stat, -} | float p[nm] | uint16 mv[nm]
constexpr int NODE_OFF_HDR = 48, NODE_OFF_P = 64;

// pointers into one game's state
struct GameView {
    char* pool;
    const uint32_t* chtab;  // LDS copy of the chunk table
    uint64_t* hash;
    int32_t* path_node;     // [K][max_depth]
    int32_t* path_edge;
    uint8_t* s_state;
    int32_t* s_depth;
    int32_t* s_node;
    unsigned long long* ctr;     // global per-game counters
    unsigned long long* lctr;    // this kernel's LDS accumulators
    int g;
};

XQ_D int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
XQ_D uint32_t uniu(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
XQ_D uint64_t uni64(uint64_t v)
{
    const uint32_t lo = uniu((uint32_t)v), hi = uniu((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
XQ_D double unid(double v) { return __longlong_as_double((long long)uni64((uint64_t)__double_as_longlong(v))); }

// `chtab` = LDS array of MAX_CHUNKS words that receives the game's chunk table
XQ_D GameView make_view(const SearchBuffers& B, const SearchParams& P, int g, unsigned long long* lctr, uint32_t* chtab)
{
    GameView v;
    v.lctr = lctr;
    v.pool = B.pool;
    const int nch = uni(B.g_nchunks[g]);
    for (int i = lane_id(); i < nch; i += 64) chtab[i] = B.g_chunk_tab[(size_t)g * P.max_chunks + i];
    v.chtab = chtab;
    v.hash = B.hash_tab + (size_t)g * P.hash_cap;
    v.path_node = B.s_path_node + (size_t)g * P.K * P.max_depth;
    v.path_edge = B.s_path_edge + (size_t)g * P.K * P.max_depth;
    v.s_state = B.s_state + (size_t)g * P.K;
    v.s_depth = B.s_depth + (size_t)g * P.K;
    v.s_node = B.s_node + (size_t)g * P.K;
    v.ctr = B.counters + (size_t)g * CT_COUNT;
    v.g = g;
    wave_sync();
    return v;
}

// record id -> address (ids of one record never straddle a chunk)
XQ_D char* rec_ptr(const GameView& gv, uint32_t id)
{
    return gv.pool + ((size_t)gv.chtab[id >> CHUNK_SHIFT] << 20) + ((size_t)(id & (uint32_t)(CHUNK_GRANULES - 1)) << 4);
}
XQ_D const uint32_t* node_key(const GameView& gv, int node) { return reinterpret_cast<const uint32_t*>(rec_ptr(gv, (uint32_t)node)); }
XQ_D float* node_p(char* base) { return reinterpret_cast<float*>(base + NODE_OFF_P); }
XQ_D uint16_t* node_mv(char* base, int nm) { return reinterpret_cast<uint16_t*>(base + NODE_OFF_P + 4 * nm); }
XQ_D EdgeStat* edge_ptr(const GameView& gv, uint32_t edge) { return reinterpret_cast<EdgeStat*>(rec_ptr(gv, edge)); }

// ---- MCTS solver (include/czero.h, cz_search_set_solver): what the words say ------------------------------------------
// An edge's child link without its mark: what every reader that follows the link uses.  The codes (< 0) stay as they are.
XQ_D int child_id(int c) { return c < 0 ? c : (c & CHILD_ID_MASK); }
// The edge mark: the Proof of the child.  A terminal child is marked by its code: (True, +1) is WIN(1), (True, -1) LOSS(0).
XQ_D int child_mark(int c)
{
    if (c >= 0) return (c >> CHILD_MARK_SHIFT) & 3;
    return c == CHILD_TERM_WIN ? PROOF_WIN : (c == CHILD_TERM_LOSS ? PROOF_LOSS : PROOF_OPEN);
}
XQ_D int meta_proof(uint32_t meta) { return (int)(meta >> NODE_PROOF_SHIFT) & 3; }
XQ_D int meta_dist(uint32_t meta) { return (int)(meta >> NODE_DIST_SHIFT) & 0xFF; }
// d of a MARKED child, fetched from the child's header (a first proof is final, so the header still says what the mark was
// made from).  Any lane may ask: the header is lane 0's word, and every store of a proof is followed by a fence (solve_walk).
XQ_D int child_dist(const GameView& gv, int c)
{
    if (c < 0) return c == CHILD_TERM_WIN ? 1 : 0;
    return meta_dist(*reinterpret_cast<const uint32_t*>(rec_ptr(gv, (uint32_t)(c & CHILD_ID_MASK)) + NODE_OFF_HDR + 4));
}

// Counters accumulate in LDS while a kernel runs (no global round trip per event) and are flushed once.
XQ_D void count(const GameView& gv, int which, unsigned long long by = 1)
{
    if (lane_id() == 0) gv.lctr[which] += by;
}
XQ_D void count_max(const GameView& gv, int which, unsigned long long val)
{
    if (lane_id() == 0 && gv.lctr[which] < val) gv.lctr[which] = val;
}
#ifdef CZ_SIM_PROFILE
#define PROF_BEGIN() long long prof_t = clock64()
#define PROF(which) do { const long long t_ = clock64(); count(gv, which, (unsigned long long)(t_ - prof_t)); prof_t = t_; } while (0)
#else
#define PROF_BEGIN() do { } while (0)
#define PROF(which) do { } while (0)
#endif
XQ_D void counters_begin(const GameView& gv)
{
    for (int i = lane_id(); i < CT_COUNT; i += 64) gv.lctr[i] = 0;
    wave_sync();
}
XQ_D void counters_flush(const GameView& gv)
{
    wave_sync_global();
    for (int i = lane_id(); i < CT_COUNT; i += 64) {
        const unsigned long long v = gv.lctr[i];
        if (v == 0) continue;
        if (i == CT_MAX_DEPTH) { if (gv.ctr[i] < v) gv.ctr[i] = v; }
        else gv.ctr[i] += v;
    }
}

// ---- counter-based RNG (Philox4x32-10), same stream as oracle/xq_mcts.c ------------------------
XQ_D double philox_uniform(uint64_t seed, uint32_t game_id, uint32_t stream, uint64_t idx)
{
    uint32_t c0 = (uint32_t)idx, c1 = (uint32_t)(idx >> 32), c2 = stream, c3 = game_id;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return ((double)(c0 >> 5) * 67108864.0 + (double)(c1 >> 6)) / 9007199254740992.0;
}

// ---- random leaf mirror (cz_search_set_leaf_mirror) ---------------------------------------------
// M(label) in one read (the attach side sits in a chain of dependent loads: leaf_pre_b).  Built at compile time from
// label_of / lab_ft, the tables cz_label_mirror reads.
static __device__ const MirrorTab d_mirror = make_mirror_tab();
XQ_D int row_col(int label, bool mirrored) { return mirrored ? (int)d_mirror.m[label] : label; }

// Is the new leaf `id` (its node record's id: no two nodes of a tree share one) evaluated in its mirror image?  Stream 3
// of the generator (0: the per-game lotteries, 1: the move choice, 2: the playout cap), keyed like the root noise by game
// id and game slot, draw (turns of the root << 32 | id); rates 0 and 1 decide without a draw.  Wave-uniform.
XQ_D bool leaf_coin(const SearchParams& P, const SearchBuffers& B, int g, uint32_t id)
{
    if (!(P.leaf_mirror > 0.0)) return false;
    if (P.leaf_mirror >= 1.0) return true;
    const uint32_t key = uniu(B.g_game_id[g]) + (uint32_t)g * 2654435761u;
    const uint64_t idx = ((uint64_t)uniu((uint32_t)B.g_turns[g]) << 32) | id;
    return philox_uniform(P.seed, key, 3, idx) < P.leaf_mirror;
}

// (the root noise generator -- NoiseRng, gamma_draw, dirichlet0 -- lives in xq_noise.h: host + device, CPU-tested)

// ---- packed keys and the transposition hash ----------------------------------------------------
// board (LDS) -> key words in L.key (lanes 0..11), returns the 64-bit hash (wave-uniform)
XQ_D uint64_t pack_key(const int8_t* b, uint32_t* key)
{
    const int lane = lane_id();
    uint64_t h = 0;
    if (lane < KEY_WORDS) {
        uint32_t w = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int s = lane * 8 + j;
            const int p = s < NSQ ? b[s] : 0;
            w |= nib_of(p) << (4 * j);
        }
        key[lane] = w;
        h = mix64((uint64_t)w + 0x9E3779B97F4A7C15ULL * (uint64_t)(lane + 1));
    }
    // xor of the twelve word hashes (lanes 12 .. 15 hold 0): a DPP scan of the first row, no LDS permute
    const uint32_t lo = row0_xor_u32((uint32_t)h), hi = row0_xor_u32((uint32_t)(h >> 32));
    wave_sync();
    h = ((uint64_t)hi << 32) | lo;
    return mix64(h);
}

// hash of an already packed key (same value pack_key returns for that position)
XQ_D uint64_t hash_of_key(const uint32_t* key)
{
    const int lane = lane_id();
    uint64_t h = 0;
    if (lane < KEY_WORDS) h = mix64((uint64_t)key[lane] + 0x9E3779B97F4A7C15ULL * (uint64_t)(lane + 1));
    const uint32_t lo = row0_xor_u32((uint32_t)h), hi = row0_xor_u32((uint32_t)(h >> 32));
    h = ((uint64_t)hi << 32) | lo;
    return mix64(h);
}

XQ_D void unpack_key(const uint32_t* __restrict__ gkey, int8_t* b)
{
    const int lane = lane_id();
    {
        const uint32_t w = gkey[lane >> 3];
        b[lane] = (int8_t)piece_of_nib((w >> (4 * (lane & 7))) & 15u);
    }
    if (lane < 26) {
        const int s = lane + 64;
        const uint32_t w = gkey[s >> 3];
        b[s] = (int8_t)piece_of_nib((w >> (4 * (s & 7))) & 15u);
    }
    if (lane >= 26 && lane < 32) b[lane + 64] = 0;
    wave_sync();
}

// returns node index or -1; *slot_out = where to insert
XQ_D int hash_lookup(const GameView& gv, const SearchParams& P, const uint32_t* key, uint64_t h, int* slot_out)
{
    const int lane = lane_id();
    const uint32_t mask = (uint32_t)P.hash_cap - 1u;
    uint32_t slot = (uint32_t)h & mask;
    const uint32_t tag = (uint32_t)(h >> 32) | 1u;
    for (int probe = 0; probe < P.hash_cap; ++probe) {
        const uint64_t e = uni64(gv.hash[slot]);
        if (e == 0) { *slot_out = (int)slot; return -1; }
        if ((uint32_t)(e >> 32) == tag) {
            const int idx = (int)((uint32_t)e) - 1;
            const bool ne = lane < KEY_WORDS && node_key(gv, idx)[lane] != key[lane];
            if (!__ballot(ne)) { *slot_out = (int)slot; return idx; }
        }
        slot = (slot + 1) & mask;
    }
    *slot_out = -1;
    return -1;
}

// ---- backup: update_tree, player.py:357-366 ------------------------------------------------------
// levels are independent (a path never holds the same edge twice), so lane i updates level i
XQ_D void backup(const SearchParams& P, const GameView& gv, const SearchLDS& L, int depth, double v)
{
    const int lane = lane_id();
    for (int i = lane; i < depth; i += 64) {
        EdgeStat* e = edge_ptr(gv, (uint32_t)L.path_edge[i]);
        const double vi = ((depth - i) & 1) ? -v : v;        // v = -v once per level walking up
        const EdgeStat cur = *e;                             // one 16-byte load
        e->n = cur.n + (1 - P.vl);
        e->w = cur.w + (vi + (double)P.vl);
    }
    count(gv, CT_SIMS);
    count(gv, CT_SUM_DEPTH, (unsigned long long)depth);
    count_max(gv, CT_MAX_DEPTH, (unsigned long long)depth);
    wave_sync_global();
}

// sum_n / (move count | flags) / stat block / network value of a node: one 16-byte load
struct NodeHdr {
    int sum_n;
    uint32_t meta, stat;
    uint32_t val;       // the bits of the float32 network value (store_net_value); read by the full Gumbel search only
};
XQ_D NodeHdr load_hdr(char* base)
{
    // lane 0 is also the only lane that ever writes these words, so its load sees its own earlier stores
    // without a fence
    int4 v = make_int4(0, 0, 0, 0);
    if (lane_id() == 0) v = *reinterpret_cast<const int4*>(base + NODE_OFF_HDR);
    NodeHdr h;
    h.sum_n = __builtin_amdgcn_readfirstlane(v.x);
    h.meta = (uint32_t)__builtin_amdgcn_readfirstlane(v.y);
    h.stat = (uint32_t)__builtin_amdgcn_readfirstlane(v.z);
    h.val = (uint32_t)__builtin_amdgcn_readfirstlane(v.w);
    return h;
}
XQ_D void store_sum_n(char* base, int v) { *reinterpret_cast<int32_t*>(base + NODE_OFF_HDR) = v; }
XQ_D void store_meta(char* base, uint32_t v) { *reinterpret_cast<uint32_t*>(base + NODE_OFF_HDR + 4) = v; }
XQ_D void store_stat(char* base, uint32_t v) { *reinterpret_cast<uint32_t*>(base + NODE_OFF_HDR + 8) = v; }
// The leaf's network value, from its mover's view, as the round was handed it (a mirrored leaf's as it is): written by
// lane 0 beside the store_meta of the attach, and only while the Gumbel root search is on (GUM instantiations of k_sim).
// A node attached while it was off keeps the 0 of expand_node.
XQ_D void store_net_value(char* base, float v) { *reinterpret_cast<float*>(base + NODE_OFF_HDR + 12) = v; }

// ---- prior spreading: select_action_q_and_u, player.py:272-284 ----------------------------------
// Network rows as raw logits (cz_search_policy_logits): the reference spreads the softmax output over the legal moves,
// p_j / sum_legal p (player.py:272-283), in which the softmax's own denominator cancels -- so only the legal moves' logits
// matter: p_j := exp(l_j - max over the node's moves).  (The engine's own queue then skips the normalising pass over all
// 2086 columns: 546 MB of traffic per round for the 4 % of the entries that are read.)
XQ_D void logits_to_weights(float& q0, float& q1, int nm)
{
    const int lane = lane_id();
    const bool h0 = lane < nm, h1 = lane + 64 < nm;
    float m = h0 ? q0 : -3.0e38f;
    if (h1 && q1 > m) m = q1;
    m = wave_max_f32(m);
    q0 = h0 ? __expf(q0 - m) : 0.0f;
    q1 = h1 ? __expf(q1 - m) : 0.0f;
}

// The priors of a node from its row's entries, lane j holding move j in p0 and move j + 64 in p1 (0 past the node's nm
// moves): prior j = (p0 or p1 after the call) / the returned sum.  Raw logits first become weights relative to the largest
// legal one; the sum is the float32 accumulation in move order (select_action_q_and_u, player.py:272-284), the terms read
// straight from the lanes' registers (a loop over an LDS copy paid an LDS round trip per term).  The one place the priors
// are formed: the attach of an evaluated leaf and the evaluation cache's fill (k_cache_fill) both call it, so a cached
// entry holds the attach's bits by construction.
XQ_D float prior_norm(float& p0, float& p1, int nm, bool logits)
{
    if (logits) logits_to_weights(p0, p1, nm);             // (raw logits: weights relative to the largest legal one)
    float all_p = 0.0f;
    if (nm > 0) {
        all_p = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p0), 0));          // int 0 + float32
        const int n0 = nm < 64 ? nm : 64;
        for (int j = 1; j < n0; ++j) all_p = all_p + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p0), j));
        for (int j = 64; j < nm; ++j) all_p = all_p + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p1), j - 64));
    }
    if (all_p == 0.0f) all_p = 1.0f;
    return all_p;
}

// keep_v: the leaf's network value v goes into the node header as well (k_sim's keep_v: constant false outside the GUM
// instantiations, so their text does not hold the store)
XQ_D void attach_policy(const GameView& gv, SearchLDS& L, int node, const float* __restrict__ prow, bool logits,
                        bool keep_v, float v)
{
    const int lane = lane_id();
    char* base = rec_ptr(gv, (uint32_t)node);
    const NodeHdr hdr = load_hdr(base);
    const uint32_t meta = hdr.meta;
    const int nm = (int)(meta & 0xFF);
    float* pp = node_p(base);
    const uint16_t* pm = node_mv(base, nm);
    // a mirrored leaf's row is in the mirrored frame: the entry of move a is column M(a); p[] and the moves stay as they are
    const bool mir = (meta & NODE_MIRRORED) != 0u;
    float q0 = 0.0f, q1 = 0.0f;
    if (lane < nm) q0 = prow[row_col(pm[lane], mir)];
    if (lane + 64 < nm) q1 = prow[row_col(pm[lane + 64], mir)];
    const float all_p = prior_norm(q0, q1, nm, logits);
    if (lane < nm) pp[lane] = q0 / all_p;
    if (lane + 64 < nm) pp[lane + 64] = q1 / all_p;
    // p[j] is written and later read (select_edge) by the same lane, the header by lane 0: no global fence
    if (lane == 0) store_meta(base, meta & ~(uint32_t)(NODE_WAITING | NODE_MIRRORED));
    if (keep_v && lane == 0) store_net_value(base, v);
    wave_sync();
}

// attach_policy + load_path + backup of one evaluated leaf with their independent loads issued together: the move labels
// with the path's edge ids, then the priors of those labels with the statistics of those edges -- two dependent memory
// round trips per leaf instead of five (the BACKUP launch is nothing but such chains, eight leaves one after the other).
// Same arithmetic, same lanes writing the same words as the three functions it replaces.  depth <= 64.
// (round 5) The part of a leaf's chain that does not depend on the tree -- its move labels, its path's edge ids, the network
// row's entries for those labels -- is fetched one leaf AHEAD (LeafPre: leaf_pre_a, then leaf_pre_b once the labels are
// back), under the previous leaf's edge update and fence; what stays in a leaf's serial chain is the edge statistics' load,
// the arithmetic and the store fence: two memory round trips per leaf instead of three.
struct LeafPre {
    uint16_t m0, m1;
    int e;
    float p0, p1;
};
XQ_D void leaf_pre_a(const GameView& gv, LeafPre& lp, int node, uint32_t meta, int depth, const int32_t* __restrict__ hp_edge)
{
    const int lane = lane_id();
    char* base = rec_ptr(gv, (uint32_t)node);
    const int nm = (int)(meta & 0xFF);
    const uint16_t* pm = node_mv(base, nm);
    lp.m0 = 0; lp.m1 = 0; lp.e = 0;
    if (lane < nm) lp.m0 = pm[lane];
    if (lane + 64 < nm) lp.m1 = pm[lane + 64];
    if (lane < depth) lp.e = hp_edge[lane];
}
XQ_D void leaf_pre_b(LeafPre& lp, uint32_t meta, const float* __restrict__ prow)
{
    const int lane = lane_id();
    const int nm = (int)(meta & 0xFF);
    lp.p0 = 0.0f; lp.p1 = 0.0f;
    const bool mir = (meta & NODE_MIRRORED) != 0u;             // (the row of a mirrored leaf: column M(label), one table read)
    if (lane < nm) lp.p0 = prow[row_col(lp.m0, mir)];
    if (lane + 64 < nm) lp.p1 = prow[row_col(lp.m1, mir)];
}

// `lp`: this leaf's prefetched labels / edge ids / row entries.  `next`: issued between this leaf's edge-statistics load and
// its arithmetic -- the caller's prefetch of the following leaf.
// keep_v: as attach_policy's; v is float(v) of the slot's float32, so the cast back is exact.
template <typename Next>
XQ_D void attach_and_backup(const SearchParams& P, const GameView& gv, SearchLDS& L, int node, uint32_t meta, int depth,
                            const LeafPre& lp, double v, bool logits, bool keep_v, Next&& next)
{
    const int lane = lane_id();
    char* base = rec_ptr(gv, (uint32_t)node);
    const int nm = (int)(meta & 0xFF);
    float* pp = node_p(base);
    float p0 = lp.p0, p1 = lp.p1;
    EdgeStat cur{0.0, 0, 0};
    EdgeStat* ep = nullptr;
    if (lane < depth) { ep = edge_ptr(gv, (uint32_t)lp.e); cur = *ep; }
    next();
    const float all_p = prior_norm(p0, p1, nm, logits);    // prior spreading (select_action_q_and_u, player.py:272-284)
    if (lane < nm) pp[lane] = p0 / all_p;
    if (lane + 64 < nm) pp[lane + 64] = p1 / all_p;
    if (lane == 0) store_meta(base, meta & ~(uint32_t)(NODE_WAITING | NODE_MIRRORED));
    if (keep_v && lane == 0) store_net_value(base, (float)v);
    // update_tree (player.py:357-366): lane i = level i
    if (lane < depth) {
        const double vi = ((depth - lane) & 1) ? -v : v;
        ep->n = cur.n + (1 - P.vl);
        ep->w = cur.w + (vi + (double)P.vl);
    }
    count(gv, CT_SIMS);
    count(gv, CT_SUM_DEPTH, (unsigned long long)depth);
    count_max(gv, CT_MAX_DEPTH, (unsigned long long)depth);
    wave_sync_global();
}

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
XQ_D double root_u(const SearchParams& P, double p_, double xx, int n) { return P.c_puct * p_ * xx / (double)(1 + n); }

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
// so their registers and their text are what they were without it.  net_value: the header's fourth word (GUM only).
template <bool GUM>
XQ_D Picked select_edge(const SearchParams& P, const SearchBuffers& B, int g, char* base, const EdgeStat* sb, int sum_n,
                        int nm, const RootCtx& rc, uint32_t net_value)
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
    const float* pp = node_p(base);
    const uint16_t* pm = node_mv(base, nm);
    int n0 = 0, child0 = CHILD_UNKNOWN, mv0 = 0;           // this lane's edge of the first half
    double w0 = 0.0;
    double best_s = -1.0e300;
    int best_j = -1;
    bool win0 = false, win1 = false;
    const int halves = nm > 64 ? 2 : 1;                     // almost every position has <= 64 moves
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
                u = root_u(P, root_prior(P, rc, p, j), xx, n);
            } else {
                const float a = P.c_puct_f32 * p;
                u = (double)a * xx / (double)(1 + n);
            }
            if (valid) {
                score = q + u;
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
            if (!(es.w / (double)n + root_u(P, p_, xx, n) >= -99999999.0)) continue;
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

// ---- MCTS solver: selection, marking and deriving (include/czero.h, cz_search_set_solver) -------------------------------
// Rule 1's edge among the lanes' winning edges (win[h]: edge lane + 64 h is winning and may be taken; ch[h] its child
// word): the least d, the first in edge order on a tie; -1 without one.  The distances come from the child headers, which
// is why this runs only once a winning edge exists.  Wave-uniform.
XQ_D int solve_least(const GameView& gv, const bool win[2], const int ch[2])
{
    if ((__ballot(win[0]) | __ballot(win[1])) == 0ull) return -1;
    const int lane = lane_id();
    double key = -1.0e300;                                     // max of -(d * 128 + j) = the least (d, j)
#pragma unroll
    for (int h = 0; h < 2; ++h)
        if (win[h]) {
            const double k = -(double)(child_dist(gv, ch[h]) * MAXMOVES + lane + 64 * h);
            key = k > key ? k : key;
        }
    return (int)(-wave_max_f64(key)) & (MAXMOVES - 1);
}

// Rule 1 at a root: the non-banned winning edge of least d of the node at `base` (nm moves, statistics sb or nullptr), -1
// without one.  The move choice (choose_action) and the decided-root test ask it.  All 64 lanes call it.
XQ_D int solve_root_edge(const GameView& gv, char* base, const EdgeStat* sb, int nm, int n_no_act, const uint16_t* no_act)
{
    const int lane = lane_id();
    const uint16_t* pm = node_mv(base, nm);
    bool win[2] = {false, false};
    int ch[2] = {CHILD_UNKNOWN, CHILD_UNKNOWN};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        if (j >= nm || !sb) continue;
        ch[h] = sb[j].child;
        bool banned = false;
        for (int k = 0; k < n_no_act; ++k) banned = banned || (no_act[k] == pm[j]);
        win[h] = !banned && child_mark(ch[h]) == PROOF_LOSS;
    }
    return solve_least(gv, win, ch);
}

// Is the game's root decided -- LOSS, or WIN with a non-banned winning edge?  Then no further simulation starts this ply.
// *edge (optional): rule 1's edge at such a WIN root, else -1.  All 64 lanes call it; wave-uniform.
XQ_D bool solve_root_decided(const SearchBuffers& B, const GameView& gv, int* edge)
{
    if (edge) *edge = -1;
    const int root = uni(B.g_root[gv.g]);
    if (root <= 0) return false;                                // (-1: not in the tree; 0, "none": an object never given a root)
    char* base = rec_ptr(gv, (uint32_t)root);
    const NodeHdr hdr = load_hdr(base);
    const int st = meta_proof(hdr.meta);
    if (st == PROOF_LOSS) return true;
    if (st != PROOF_WIN) return false;
    const int nm = (int)(hdr.meta & 0xFF);
    const int j = solve_root_edge(gv, base, hdr.stat ? edge_ptr(gv, hdr.stat) : nullptr, nm, uni((int)B.g_n_no_act[gv.g]),
                                  B.g_no_act + (size_t)gv.g * MAX_NO_ACT);
    if (edge) *edge = j;
    return j >= 0;
}

// select_edge with the solver on, at the root and at OPEN nodes (the SOLVE instantiations of k_sim call it instead):
//   1. among the non-banned edges a winning one is taken at once, the least d, the first in edge order on a tie;
//   2. otherwise select_edge's rule -- the same expressions in the same order, the q > 1 - 1e-7 shortcut included -- over
//      the non-banned edges that are not losing;
//   3. every non-banned edge losing: over all non-banned edges.
// Edge j is loaded by the lane that owns it (j & 63), both halves held at once: the marks come with the 16-byte load.
XQ_D int select_solve(const SearchParams& P, const GameView& gv, char* base, const EdgeStat* sb, int sum_n, int nm,
                      const RootCtx& rc)
{
    const int lane = lane_id();
    const double xx = __dsqrt_rn((double)(sum_n + 1));
    const float* pp = node_p(base);
    const uint16_t* pm = node_mv(base, nm);
    bool nb[2] = {false, false}, live[2] = {false, false}, win[2] = {false, false}, sure[2] = {false, false};
    int ch[2] = {CHILD_UNKNOWN, CHILD_UNKNOWN}, mk[2] = {PROOF_OPEN, PROOF_OPEN};
    double sc[2] = {-1.0e300, -1.0e300};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int j = lane + 64 * h;
        if (j >= nm) continue;
        EdgeStat es{0.0, 0, CHILD_UNKNOWN};
        if (sb) es = sb[j];
        const float p = pp[j];
        const uint16_t mv = pm[j];
        const int n = es.n;
        const double w = es.w;
        const double q = n ? w / (double)n : 0.0;
        bool valid = true;
        double u;
        if (rc.is_root) {
            if (rc.n_no_act) valid = !root_banned(rc, mv);
            u = root_u(P, root_prior(P, rc, p, j), xx, n);
        } else {
            const float a = P.c_puct_f32 * p;
            u = (double)a * xx / (double)(1 + n);
        }
        if (!valid) continue;
        nb[h] = true;
        ch[h] = es.child;
        mk[h] = child_mark(es.child);
        win[h] = mk[h] == PROOF_LOSS;
        const double score = q + u;
        live[h] = score >= -99999999.0;                         // (a rejected score leaves the edge out, as it does there)
        sc[h] = score;
        sure[h] = live[h] && q > (1.0 - 1e-7);
    }
    const int won = solve_least(gv, win, ch);                   // rule 1
    if (won >= 0) return won;
    // rules 2 and 3: the losing edges stay out unless every non-banned edge is one
    const bool all_losing = (__ballot(nb[0] && mk[0] != PROOF_WIN) | __ballot(nb[1] && mk[1] != PROOF_WIN)) == 0ull;
    double best_s = -1.0e300;
    int best_j = -1;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        live[h] = live[h] && (all_losing || mk[h] != PROOF_WIN);
        sure[h] = sure[h] && live[h];
        if (live[h] && sc[h] >= best_s) { best_s = sc[h]; best_j = lane + 64 * h; }   // h = 1 has the larger index: wins ties
    }
    const int first_win = lowest_bit(__ballot(sure[0]), __ballot(sure[1]));     // player.py:309-311
    if (first_win >= 0) return first_win;
    const double m = wave_max_f64(best_s);                      // player.py:312-314: the LAST maximum, select_edge's vote
    const bool top = best_j >= 0 && best_s == m;
    const uint64_t t1 = __ballot(top && best_j >= 64), t0 = __ballot(top);
    return t1 ? 64 + (63 - __clzll((long long)t1)) : (t0 ? 63 - __clzll((long long)t0) : -1);
}

// The second step of a backup, after the level-parallel one and only for a value of +-2: the simulation whose path (depth
// entries) is in L.path_* ended on a terminal child or on a proven node.  Its last edge is marked with that position's
// status, the node above derived if it is OPEN, and while a node becomes proven the walk goes on one level up; it stops at
// the first node that stays OPEN (or was proven before).  Sequential over the levels; each level is one scan of the
// node's edges over both halves, every edge read and written by its owner lane (j & 63), the header by lane 0.  The
// distances of the marked children come from their headers, any lane asking: hence the fence after every proof stored.
XQ_D void solve_walk(const GameView& gv, const SearchLDS& L, int depth)
{
    if (depth <= 0) return;
    const int lane = lane_id();
    int st;
    {
        const int c = uni(edge_ptr(gv, (uint32_t)L.path_edge[depth - 1])->child);
        st = child_mark(c);                                     // a terminal child: its code
        if (c >= 0) st = meta_proof(load_hdr(rec_ptr(gv, (uint32_t)child_id(c))).meta);
    }
    for (int i = depth - 1; i >= 0 && st != PROOF_OPEN; --i) {
        const int e = L.path_edge[i];
        char* base = rec_ptr(gv, (uint32_t)L.path_node[i]);
        const NodeHdr hdr = load_hdr(base);
        const int nm = (int)(hdr.meta & 0xFF);
        const int je = (int)((uint32_t)e - hdr.stat);
        EdgeStat* sb = edge_ptr(gv, hdr.stat);
        if (lane == (je & 63)) {                                // marking
            const int c = sb[je].child;
            if (c >= 0) sb[je].child = (c & CHILD_ID_MASK) | (st << CHILD_MARK_SHIFT);
        }
        if (meta_proof(hdr.meta) != PROOF_OPEN) break;          // a first proof is final
        bool win[2] = {false, false}, lose[2] = {false, false};
        double near = -1.0e300, far = -1.0;                     // max of -d over the winning edges, max of d over the losing
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = lane + 64 * h;
            if (j >= nm) continue;
            const int c = sb[j].child;
            const int mk = child_mark(c);
            if (mk == PROOF_OPEN) continue;
            const double d = (double)child_dist(gv, c);
            win[h] = mk == PROOF_LOSS;
            lose[h] = mk == PROOF_WIN;
            if (win[h]) near = -d > near ? -d : near;
            else far = d > far ? d : far;
        }
        int d;
        if (__ballot(win[0]) | __ballot(win[1])) {
            st = PROOF_WIN;
            d = 1 + (int)(-wave_max_f64(near));
        } else if (nm > 0 && __popcll(__ballot(lose[0])) + __popcll(__ballot(lose[1])) == nm) {
            st = PROOF_LOSS;
            d = 1 + (int)wave_max_f64(far);
        } else break;
        d = d < PROOF_DIST_MAX ? d : PROOF_DIST_MAX;
        if (lane == 0)
            store_meta(base, hdr.meta | ((uint32_t)st << NODE_PROOF_SHIFT) | ((uint32_t)d << NODE_DIST_SHIFT));
        count(gv, CT_PROOFS);
        wave_sync_global();
    }
    wave_sync_global();
}

// ---- simulation bookkeeping --------------------------------------------------------------------------
XQ_D void sim_finish(const GameView& gv, int sim, int* active)
{
    if (lane_id() == 0) gv.s_state[sim] = SIM_IDLE;
    *active -= 1;
}

// ---- deferred terminal / repetition results -----------------------------------------------------------------------
// MCTS_search does not apply a terminal or repetition value itself: it SUBMITS update_tree to the executor
// (player.py:206, :228-232), behind the search tasks of the batch that were queued first (:173-174), and a search
// thread runs its descent to the end before the interpreter switches.  So the descents of a phase (a fresh batch, or
// the simulations resumed after an evaluation) see each other's virtual losses but not each other's terminal results;
// those are applied when the descents are over, in index order (oracle: finish / flush_deferred
// in xq_mcts.c; tests/golden/kgt1_spread.json is the evidence that this is what the reference does).
// The slot keeps (value, depth) until the flush: written and read back by lane 0 only (its own stores, no fence).
struct Deferred {
    uint64_t lo;       // simulations < 64 waiting for their backup, one bit each (wave-uniform)
    int hi;            // how many with an index >= 64 (found by scanning the slots)
};
XQ_D void defer_result(const GameView& gv, int sim, int depth, int value, Deferred& df)
{
    if (lane_id() == 0) { gv.s_state[sim] = SIM_DEFERRED; gv.s_node[sim] = value; gv.s_depth[sim] = depth; }
    if (sim < 64) df.lo |= 1ull << sim;
    else df.hi += 1;
    wave_sync();
}

XQ_D int find_in_path(const SearchLDS& L, int depth, int node)
{
    const int lane = lane_id();
    for (int base = 0; base < depth; base += 64) {
        const uint64_t m = __ballot(base + lane < depth && L.path_node[base + lane] == node);
        if (m) return base + __ffsll((long long)m) - 1;
    }
    return -1;
}

struct RoundIO {
    void* planes;
    int planes_dtype;
    int in_planes;
    uint32_t* masks;       // cz_search_leaf_masks: [slots][96] occupancy boards, or NULL
    bool planes_off;       // cz_search_leaf_planes(0): only the occupancy boards are written
    uint8_t* flags;        // cz_search_set_leaf_mirror: [slots] 1 = the slot's leaf was written mirrored, or NULL
};

// occupancy-board word of plane position pos (row i = pos / 9 of the planes shows rank y = 9 - i): bit `shift` + plane of the
// piece on that square, 0 for an empty square or pos >= 90 (state_to_planes, static_env.py:137-156)
// `mirror`: the word of the mirror image, which shows file 8 - j at column j.
XQ_D uint32_t mask_word(const int8_t* b, int pos, int shift, bool mirror)
{
    if (pos >= NSQ) return 0u;
    const int i = pos / 9, j = pos - i * 9;
    const int p = b[(9 - i) * 9 + (mirror ? 8 - j : j)];
    return p == 0 ? 0u : 1u << (shift + (p > 0 ? p - 1 : 6 - p));
}

XQ_D void encode_block(int dtype, const int8_t* b, uint8_t* codes, char* out, bool mirror)
{
    switch (dtype) {
    case CZ_F32: wave_encode_codes<0>(b, codes, out, mirror); break;
    case CZ_F16: wave_encode_codes<1>(b, codes, out, mirror); break;
    case CZ_BF16: wave_encode_codes<2>(b, codes, out, mirror); break;
    default: wave_encode_codes<3>(b, codes, out, mirror); break;
    }
}

// the leaf's input planes into its queue slot: 14 planes (state_to_planes), or 28 with the position two plies
// earlier (`prev`, NULL = none: zeros) as the second block (state_history_to_planes, static_env.py:158-194).
// `mirror` (wave-uniform): the slot holds the mirror image of both positions instead, in all its forms, and says so in the
// slot's flag.  The mirror is in the index the boards are read with: b and prev are only read, the caller goes on using them.
template <bool HIST>
XQ_D void write_planes(const RoundIO& io, const int8_t* b, uint8_t* codes, size_t slot, const int8_t* prev, bool mirror)
{
    if (io.flags && lane_id() == 0) io.flags[slot] = mirror ? (uint8_t)1 : (uint8_t)0;
    const size_t esz = io.planes_dtype == CZ_F32 ? 4 : (io.planes_dtype == CZ_U8 ? 1 : 2);
    char* out = (char*)io.planes + slot * (size_t)io.in_planes * 90 * esz;
    // (round 5) a caller whose network reads the occupancy boards alone (cz_input_resblock_m) switches the planes off
    // (cz_search_leaf_planes): the leaf then costs the code row + two word stores instead of the 1260-element encoder pass
    const bool only_masks = io.masks && io.planes_off;
    if (only_masks) {
        // boards only: one LDS read and a shift per word, straight from the position(s) -- no code row, no encoder pass
        const int lane = lane_id();
        uint32_t m0 = mask_word(b, lane, 0, mirror), m1 = mask_word(b, 64 + lane, 0, mirror);
        if (HIST && prev) { m0 |= mask_word(prev, lane, 14, mirror); m1 |= mask_word(prev, 64 + lane, 14, mirror); }
        uint32_t* mo = io.masks + slot * 96;
        mo[lane] = m0;
        if (lane < 32) mo[64 + lane] = m1;
        return;
    }
    encode_block(io.planes_dtype, b, codes, out, mirror);
    // the same position as an occupancy board (cz_search_leaf_masks): word pos = plane position i * 9 + j, bit c = plane c shows
    // a piece there -- `codes` holds exactly that channel per position after the encoder's pass
    const int lane = lane_id();
    uint32_t m0 = 0u, m1 = 0u;
    if (io.masks) {
        const uint32_t c0 = codes[lane], c1 = lane < 26 ? codes[64 + lane] : 0xFFu;
        m0 = c0 == 0xFFu ? 0u : 1u << c0;
        m1 = c1 == 0xFFu ? 0u : 1u << c1;
    }
    if (HIST) {
        char* out2 = out + 1260 * esz;
        if (prev) {
            encode_block(io.planes_dtype, prev, codes, out2, mirror);
            if (io.masks) {
                const uint32_t c0 = codes[lane], c1 = lane < 26 ? codes[64 + lane] : 0xFFu;
                m0 |= c0 == 0xFFu ? 0u : 1u << (14 + c0);
                m1 |= c1 == 0xFFu ? 0u : 1u << (14 + c1);
            }
        } else {
            for (int q = lane_id(); q < 315 * (int)esz; q += 64) reinterpret_cast<uint32_t*>(out2)[q] = 0u;
        }
    }
    if (io.masks) {
        uint32_t* mo = io.masks + slot * 96;
        mo[lane] = m0;
        if (lane < 32) mo[64 + lane] = m1;
    }
}

// second plane block of a new leaf (expand_and_evaluate, player.py:322-338): simulations started by action() with a
// real game history use the game position two plies before the ROOT whatever their depth (the reference never
// clears `is_root_node` while descending, :217); every other simulation uses its own search path.
XQ_D const int8_t* history_board(const SearchParams& P, const SearchBuffers& B, const GameView& gv, SearchLDS& L,
                                 bool fresh, int depth)
{
    if (P.in_planes != 28) return nullptr;
    const int lane = lane_id();
    const int kind = uni((int)B.g_hist_kind[gv.g]);
    if (fresh && kind != 0) {
        if (kind != 1) return nullptr;                                // a history shorter than 5 entries
        const int8_t* pb = B.g_prev_board + (size_t)gv.g * BOARD_LDS;
        L.r.bd[2][lane] = pb[lane];
        if (lane < 32) L.r.bd[2][lane + 64] = (lane < 26) ? pb[lane + 64] : (int8_t)0;
        wave_sync();
        return L.r.bd[2];
    }
    if (depth < 2) return nullptr;
    unpack_key(node_key(gv, L.path_node[depth - 2]), L.r.bd[2]);
    return L.r.bd[2];
}

// The game's heap while a kernel runs: bump pointer + owned chunks, held in registers (wave-uniform).
struct Arena {
    uint32_t top;           // next free granule (record id)
    int nchunks;            // chunks the game owns (reserved by begin_search for the whole ply)
    int ncount;             // nodes in the tree
};

// `granules` <= 128 contiguous granules inside one chunk; 0 = the game's chunks are used up
XQ_D uint32_t heap_alloc(Arena& ar, int granules)
{
    uint32_t top = ar.top;
    if ((int)(top & (uint32_t)(CHUNK_GRANULES - 1)) + granules > CHUNK_GRANULES)
        top = ((top >> CHUNK_SHIFT) + 1u) << CHUNK_SHIFT;            // records never straddle chunks
    if ((int)(top >> CHUNK_SHIFT) >= ar.nchunks) return 0u;
    ar.top = top + (uint32_t)granules;
    return top;
}

// create a node for the position whose packed key is in L.key and whose ordered move list is in `ml` (nm moves);
// returns the node id or -1 when the game's chunks (or its hash table) are full.  `mirrored`: the new leaf's coin
// (leaf_coin), which the node carries in its header until its priors are attached.
XQ_D int expand_node(const SearchParams& P, const SearchBuffers& B, const GameView& gv, SearchLDS& L,
                     const MoveList& ml, int nm, int hash_slot, uint64_t h, Arena& ar, bool& mirrored)
{
    const int lane = lane_id();
    nm = nm < MAXMOVES ? nm : MAXMOVES;
    if (hash_slot < 0) return -1;
    const uint32_t id = heap_alloc(ar, NODE_HDR_GRANULES + (6 * nm + 15) / 16);
    if (id == 0u) return -1;
    char* base = rec_ptr(gv, id);
    mirrored = leaf_coin(P, B, gv.g, id);
    if (lane < KEY_WORDS) reinterpret_cast<uint32_t*>(base)[lane] = L.key[lane];
    float* pp = node_p(base);
    uint16_t* pm = node_mv(base, nm);
    for (int j = lane; j < nm; j += 64) {
        pp[j] = 0.0f;
        pm[j] = ml.lab[j];
    }
    if (lane == 0) {
        // sum_n = 1 (player.py:213), no statistics yet: they are allocated when the node is first selected from
        *reinterpret_cast<int4*>(base + NODE_OFF_HDR) = make_int4(1, (int)((uint32_t)nm | NODE_WAITING | (mirrored ? (uint32_t)NODE_MIRRORED : 0u)), 0, 0);
        gv.hash[hash_slot] = ((uint64_t)((uint32_t)(h >> 32) | 1u) << 32) | (uint32_t)(id + 1u);
    }
    ar.ncount += 1;
    count(gv, CT_EXPANSIONS);
    count(gv, CT_LEAF_MOVES, (unsigned long long)nm);
    // p / move are written by the lane that reads them in select_edge, the header and the hash slot by lane 0,
    // the key words by the lanes that compare them in hash_lookup: no global fence
    wave_sync();
    return (int)id;
}

// ---- evaluation cache (cz_search_set_eval_cache): the probe of a new leaf -------------------------------------------
// Called right after expand_node made `node` for the position whose key is in L.key (hash h, coin `mirrored`), in the
// k_sim(SELECT) launch only; the table is read, never written (k_cache_fill, an earlier launch, is the only writer).  A hit
// is the full key plus the mirror bit and the move count: the lanes that own p[j] in select_edge (j & 63) copy the entry's
// priors into the node record, lane 0 leaves the value in the slot's s_cval.  The node stays NODE_WAITING: the caller
// marks the slot SIM_CACHED and the next round's attach takes it in simulation order with the evaluated leaves.
XQ_D bool cache_probe(const EvalCache& C, const GameView& gv, const uint32_t* key, uint64_t h, bool mirrored, int nm,
                      int node, size_t slot)
{
    const int lane = lane_id();
    nm = nm < MAXMOVES ? nm : MAXMOVES;
    const EvalCacheEntry* e = C.tab + ec_slot(h, mirrored, C.log2);
    bool ne = false;
    if (lane < KEY_WORDS) ne = e->key[lane] != key[lane];
    else if (lane == KEY_WORDS) ne = e->meta != ec_meta(nm, mirrored);
    const bool hit = __ballot(ne) == 0ull;
    if (lane == 0) {                                        // (this game's wave is the words' only writer)
        C.g_probes[gv.g] += 1ull;
        if (hit) C.g_hits[gv.g] += 1ull;
    }
    if (!hit) return false;
    float* pp = node_p(rec_ptr(gv, (uint32_t)node));
    if (lane < nm) pp[lane] = e->p[lane];
    if (lane + 64 < nm) pp[lane + 64] = e->p[lane + 64];
    if (lane == 0) C.s_cval[slot] = e->value;
    return true;
}

// the attach of a SIM_CACHED slot: the priors are in the node already (cache_probe), what is left of attach_policy is the
// header -- the flags go, the value stays with keep_v
XQ_D void cached_attach(const GameView& gv, int node, bool keep_v, float v)
{
    char* base = rec_ptr(gv, (uint32_t)node);
    if (lane_id() == 0) {
        const uint32_t meta = *reinterpret_cast<const uint32_t*>(base + NODE_OFF_HDR + 4);
        store_meta(base, meta & ~(uint32_t)(NODE_WAITING | NODE_MIRRORED));
        if (keep_v) store_net_value(base, v);
    }
    wave_sync();
}

// move label of path entry (node, edge): edge - stat block = index into the node's move list (rare: repetitions)
XQ_D int edge_move(const GameView& gv, int node, int edge)
{
    char* base = rec_ptr(gv, (uint32_t)node);
    const NodeHdr hdr = load_hdr(base);
    const int nm = (int)(hdr.meta & 0xFF);
    return uni((int)node_mv(base, nm)[(uint32_t)edge - hdr.stat]);
}

// One descent of simulation `sim` starting at `node` with `depth` path entries already in L.path_*
// (MCTS_search, player.py:198-260).  `node` < 0 means the root position is not in the tree yet.
// CACHE: the evaluation cache is on (cz_search_set_eval_cache); `probe` (the SELECT launch): a new leaf asks the table C
// before it takes a queue row.
// SOLVE: the MCTS solver is on (cz_search_set_solver): the arrival on a proven node and select_solve; likewise an
// instantiation of its own.
template <bool HIST, bool GUM, bool CACHE, bool SOLVE = false>
XQ_D void run_sim(const SearchParams& P, const SearchBuffers& B, const GameView& gv, SearchLDS& L,
                  const RoundIO& io, const RootCtx& rc0, int root, int sim, int node, int depth, int* active,
                  Arena& ar, bool fresh, Deferred& df, const EvalCache& C, bool probe)
{
    const int lane = lane_id();
    const int g = gv.g;
    int32_t* hp_node = gv.path_node + (size_t)sim * P.max_depth;
    int32_t* hp_edge = gv.path_edge + (size_t)sim * P.max_depth;
    if (node < 0) {
        // root expansion (player.py:211-221 with history == [state]); the position is in g_board
        const int8_t* gb = B.g_board + (size_t)g * BOARD_LDS;
        L.r.bd[1][lane] = gb[lane];
        if (lane < 32) L.r.bd[1][lane + 64] = (lane < 26) ? gb[lane + 64] : (int8_t)0;
        wave_sync();
        const int nm = wave_movegen<true>(L.r.bd[1], L.r.ml[0], L.r.plist);
        const uint64_t h = pack_key(L.r.bd[1], L.key);
        int slot;
        int idx = hash_lookup(gv, P, L.key, h, &slot);
        bool mir = false;
        const bool made = idx < 0;
        if (idx < 0) idx = expand_node(P, B, gv, L, L.r.ml[0], nm, slot, h, ar, mir);
        else mir = (load_hdr(rec_ptr(gv, (uint32_t)idx)).meta & NODE_MIRRORED) != 0u;   // (the frame its attach will read)
        if (idx < 0) { count(gv, CT_OVERFLOW_SIMS); backup(P, gv, L, 0, 0.0); sim_finish(gv, sim, active); return; }
        bool hit = false;
        if constexpr (CACHE) {
            if (probe && made) hit = cache_probe(C, gv, L.key, h, mir, nm, idx, (size_t)g * P.K + sim);
        }
        if (lane == 0) {
            B.g_root[g] = idx;
            gv.s_state[sim] = hit ? SIM_CACHED : SIM_LEAF; gv.s_node[sim] = idx; gv.s_depth[sim] = 0;
        }
        if (!hit) write_planes<HIST>(io, L.r.bd[1], L.codes, (size_t)g * P.K + sim, HIST ? history_board(P, B, gv, L, fresh, 0) : nullptr, mir);
        wave_sync();
        return;
    }
    PROF_BEGIN();
    for (;;) {
        // state in history[:-1] (player.py:223-236)
        const int rep = find_in_path(L, depth, node);
        if (rep >= 0) {
            unpack_key(node_key(gv, node), L.r.bd[0]);
            const int mv = edge_move(gv, L.path_node[rep], L.path_edge[rep]);
            int v;
            if (wave_will_check_or_catch(L.r, L.r.bd[0], mv) == 1) v = -1;
            else if (wave_be_catched(L.r.bd[0], label_ft(mv) >> 8, L.r.bd[1], L.r.ml[0], L.r.plist)) v = 1;
            else v = 0;
            count(gv, CT_REPETITION_SIMS);
            defer_result(gv, sim, depth, v, df);                     // update_tree is a queued task (player.py:228-232)
            PROF(CT_CYC_REP);
            return;
        }
        char* base = rec_ptr(gv, (uint32_t)node);
        const NodeHdr hdr = load_hdr(base);
        const uint32_t meta = hdr.meta;
        if constexpr (SOLVE) {
            // arrival: the descent stepped onto a proven node (below the root: a proven root that is searched is not
            // decided).  Worth what the terminal at the end of its line is worth, from this node's mover; deferred and
            // flushed like a terminal result, no network row.
            if (depth >= 1 && meta_proof(meta) != PROOF_OPEN) {
                count(gv, CT_PROVEN_SIMS);
                defer_result(gv, sim, depth, meta_proof(meta) == PROOF_WIN ? 2 : -2, df);
                return;
            }
        }
        if (meta & NODE_WAITING) {                                  // player.py:238-242
            if (lane == 0) { gv.s_state[sim] = SIM_PARKED; gv.s_node[sim] = node; gv.s_depth[sim] = depth; }
            count(gv, CT_PARKED);
            wave_sync();
            return;
        }
        if (depth >= P.max_depth) {
            count(gv, CT_DEPTH_OVERFLOW);
            backup(P, gv, L, depth, 0.0);
            sim_finish(gv, sim, active);
            return;
        }
        const int nm = (int)(meta & 0xFF);
        // the node's statistics block: allocated on the first selection FROM the node (most nodes stay leaves)
        uint32_t stat = hdr.stat;
        const bool fresh_stat = stat == 0u && nm > 0;
        if (fresh_stat) {
            stat = heap_alloc(ar, nm);
            if (stat == 0u) {
                count(gv, CT_OVERFLOW_SIMS);
                backup(P, gv, L, depth, 0.0);
                sim_finish(gv, sim, active);
                return;
            }
            if (lane == 0) store_stat(base, stat);
            count(gv, CT_STAT_BLOCKS);
        }
        EdgeStat* sb = nm > 0 ? edge_ptr(gv, stat) : nullptr;
        if (fresh_stat) {
            // edge j is initialised by the lane that owns it in select_edge (j & 63): no fence before its later loads
            for (int j = lane; j < nm; j += 64) sb[j] = EdgeStat{0.0, 0, CHILD_UNKNOWN};
        }
        RootCtx rc = rc0;
        rc.is_root = (node == root);                                // player.py:266
        rc.sim = sim;
        Picked pk;
        if constexpr (SOLVE) {                                      // (have = false: the edge is reloaded below)
            pk = Picked{select_solve(P, gv, base, fresh_stat ? nullptr : sb, hdr.sum_n, nm, rc), false, 0, CHILD_UNKNOWN, 0, 0.0};
        } else {
            pk = select_edge<GUM>(P, B, g, base, fresh_stat ? nullptr : sb, hdr.sum_n, nm, rc, hdr.val);
        }
        if (pk.j < 0) {                                             // "Best action is None": cannot happen
            backup(P, gv, L, depth, 0.0);
            sim_finish(gv, sim, active);
            return;
        }
        EdgeStat* ep = sb + pk.j;
        const int e = (int)(stat + (uint32_t)pk.j);                 // edge id = granule of its statistics
        const int owner = pk.j & 63;        // the lane that loads this edge in select_edge: its own stores are
                                            // visible to it in program order, no global fence per level
        if (lane == owner) {                                        // player.py:245-252
            if (pk.have) {                                          // the values select just read: no reload
                ep->n = pk.n + P.vl;
                ep->w = pk.w - (double)P.vl;
            } else {
                ep->n += P.vl;
                ep->w = ep->w - (double)P.vl;
            }
        }
        if (lane == 0) {
            store_sum_n(base, hdr.sum_n + 1);
            L.path_node[depth] = node; L.path_edge[depth] = e;
            hp_node[depth] = node; hp_edge[depth] = e;
        }
        count(gv, CT_EDGES_VISITED, (unsigned long long)nm);
        depth += 1;
        wave_sync();
        int child = child_id(pk.have ? pk.child : uni(ep->child));  // (without the solver's mark)
        PROF(CT_CYC_SELECT);
        if (child == CHILD_UNKNOWN) {
            // (the table load of the move's squares is issued before the key's so that the two round trips overlap)
            const int ft = label_ft(pk.have ? pk.mv : uni((int)node_mv(base, nm)[pk.j]));
            unpack_key(reinterpret_cast<const uint32_t*>(base), L.r.bd[0]);
            step_board(L.r.bd[0], ft >> 8, ft & 0xFF, L.r.bd[1]);
            const DoneResult d = wave_done<true>(L.r.bd[1], L.r.bd[2], L.r.ml[0], L.r.ml[1], L.r.plist, false);   // player.py:204
            PROF(CT_CYC_RULES);
            if (d.over) {
                child = d.v > 0 ? CHILD_TERM_WIN : CHILD_TERM_LOSS;
                if (lane == owner) ep->child = child;
            } else {
                const uint64_t h = pack_key(L.r.bd[1], L.key);
                int slot;
                int idx = hash_lookup(gv, P, L.key, h, &slot);
                PROF(CT_CYC_HASH);
                if (idx >= 0) {
                    if (lane == owner) ep->child = idx;
                    child = idx;
                } else {
                    bool mir;
                    idx = expand_node(P, B, gv, L, L.r.ml[0], d.nmoves, slot, h, ar, mir);     // player.py:211-221
                    if (idx < 0) {
                        count(gv, CT_OVERFLOW_SIMS);
                        backup(P, gv, L, depth, 0.0);
                        sim_finish(gv, sim, active);
                        return;
                    }
                    if (lane == owner) ep->child = idx;
                    bool hit = false;
                    if constexpr (CACHE) {
                        if (probe) hit = cache_probe(C, gv, L.key, h, mir, d.nmoves, idx, (size_t)g * P.K + sim);
                    }
                    if (lane == 0) { gv.s_state[sim] = hit ? SIM_CACHED : SIM_LEAF; gv.s_node[sim] = idx; gv.s_depth[sim] = depth; }
                    if (!hit) write_planes<HIST>(io, L.r.bd[1], L.codes, (size_t)g * P.K + sim, HIST ? history_board(P, B, gv, L, fresh, depth) : nullptr, mir);
                    wave_sync();
                    PROF(CT_CYC_EXPAND);
                    return;
                }
            }
            wave_sync();
        }
        if (child == CHILD_TERM_WIN || child == CHILD_TERM_LOSS) {  // player.py:204-208: value doubled
            count(gv, CT_TERMINAL_SIMS);
            defer_result(gv, sim, depth, child == CHILD_TERM_WIN ? 2 : -2, df);     // queued update_tree (player.py:206)
            return;
        }
        node = child;
    }
}

// reload a suspended simulation's path into LDS
XQ_D void load_path(const SearchParams& P, const GameView& gv, SearchLDS& L, int sim, int depth)
{
    const int lane = lane_id();
    const int32_t* hp_node = gv.path_node + (size_t)sim * P.max_depth;
    const int32_t* hp_edge = gv.path_edge + (size_t)sim * P.max_depth;
    wave_sync();
    for (int i = lane; i < depth; i += 64) { L.path_node[i] = hp_node[i]; L.path_edge[i] = hp_edge[i]; }
    wave_sync();
}

// apply the deferred terminal / repetition values of the phase that just ended, in index order
// SOLVE: a value of +-2 (a terminal child, or the solver's arrival on a proven node) is followed by solve_walk
template <bool SOLVE = false>
XQ_D void flush_deferred(const SearchParams& P, const GameView& gv, SearchLDS& L, Deferred& df, int* active)
{
    if (df.lo == 0 && df.hi == 0) return;
    wave_sync_global();                  // lane 0's path stores of this launch are complete before the lanes reload paths
    auto one = [&](int i) {
        const int depth = uni(gv.s_depth[i]);
        const double v = (double)uni(gv.s_node[i]);
        load_path(P, gv, L, i, depth);
        backup(P, gv, L, depth, v);
        if constexpr (SOLVE) {
            if (v == 2.0 || v == -2.0) solve_walk(gv, L, depth);
        }
        sim_finish(gv, i, active);
    };
    while (df.lo) {
        const int i = __ffsll((long long)df.lo) - 1;
        df.lo &= df.lo - 1;
        one(i);
    }
    if (df.hi) {
        for (int i = 64; i < P.K; ++i)
            if (uni((int)gv.s_state[i]) == SIM_DEFERRED) one(i);
        df.hi = 0;
    }
}

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
// exhausted.
XQ_D bool reserve_ply(const SearchParams& P, const SearchBuffers& B, const GameView& gv, uint32_t* chtab, int tasks)
{
    const int g = gv.g;
    const uint32_t top = uniu(B.g_heap_top[g]);
    int nch = uni(B.g_nchunks[g]);
    const int ncount = uni(B.g_node_count[g]);
    if ((long long)ncount + tasks + 1 > (long long)P.hash_cap * 7 / 8) return false;      // open addressing: keep it sparse
    constexpr int PER_TASK = NODE_HDR_GRANULES + (6 * RESERVE_MOVES + 15) / 16 + RESERVE_MOVES;
    constexpr int USABLE = CHUNK_GRANULES - MAXMOVES;                 // a record that does not fit moves to the next chunk
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

XQ_D int gumbel_choose(const SearchParams& P, const SearchBuffers& B, const GameView& gv);

// ---- calc_policy + apply_temperature + choice (player.py:375-406, 453-470, :195) ---------------------
// returns the chosen label, or -1 when the player resigns.  u is the uniform draw of np.random.choice.
// SOLVE (the MCTS solver is on, an instantiation of its own): at a WIN root with a non-banned winning edge the move is
// that edge (rule 1 of select_solve), whatever tau is; resignation is tested first.
template <bool SOLVE = false>
XQ_D int choose_action(const SearchParams& P, const SearchBuffers& B, const GameView& gv, SearchLDS& L, double u,
                       bool enable_resign)
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
    const int inc = uni((int)B.g_increase_temp[g]);
    double tau = 0.0;
    if (turns < 30 && P.tau_decay_rate != 0.0) tau = pow(P.tau_decay_rate, (double)(turns + 1));
    if (tau < 0.1 || (turns >= 4 && P.evaluate)) tau = 0.0;
    if (inc && !P.evaluate) tau = 0.5;
    int chosen = 0;
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

// (re)start a self-play game in slot g (SelfPlayWorker.start_game, self_play.py:95-116; with a book the position its
// INIT_STATE stands for: turns, no_eat_count, history and "red = the first mover" as from the opening position)
XQ_D void new_game(const SearchParams& P, const SearchBuffers& B, const GameView& gv, SearchLDS& L, uint32_t game_id)
{
    const int lane = lane_id();
    const int g = gv.g;
    clear_tree(P, B, gv, L.chtab);
    const int bi = book_index(P, game_id);
    if (bi < 0) set_init_board(B.g_board + (size_t)g * BOARD_LDS);
    else set_book_board(B.g_board + (size_t)g * BOARD_LDS, P.book + (size_t)bi * NSQ);
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
XQ_D int prune_targets(int nm, const uint16_t lab[2], int n[2], const double w[2], const float p[2], double c_puct, double k)
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

// Root visit record (cz_search_record_visits): the root's edges as choose_action saw them -- edge order, exact
// counts, banned edges flagged (calc_policy zeroes them, player.py:375-406) -- for the ply that just chose its move.
// prune (forced playouts on, a full ply): the counts are the pruned policy targets, the entry says so (VISIT_PRUNED,
// raw_total); the tree keeps the raw counts and choose_action has already used them.
// FULL: a Gumbel ply's target is the full search's (gumbel_targets<true> with the root's stored value).
template <bool FULL>
XQ_D void emit_visits(const SearchParams& P, const SearchBuffers& B, const GameView& gv, const VisitRing& V, int turns,
                      bool resigned, bool fast, bool prune, bool gumbel)
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
                                 : (prune ? prune_targets(nm, E.lab, m, E.w, E.p, P.c_puct, P.forced_k) : 0);
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
    if (lane == 0) {
        VisitEntryHdr* h = reinterpret_cast<VisitEntryHdr*>(e);
        h->game_id = B.g_game_id[g];
        h->ply = (uint16_t)turns;
        h->n_edges = (uint8_t)nm;
        h->flags = (uint8_t)((resigned ? VISIT_RESIGN : 0u) | (fast ? VISIT_FAST : 0u) | (pruned ? VISIT_PRUNED : 0u) |
                               (gumbel ? VISIT_GUMBEL : 0u));
        h->sum_n = E.sum_n;
        h->raw_total = (uint32_t)raw_total;
    }
}

// One ply of SelfPlayWorker.start_game after the search finished (self_play.py:124-212).
template <bool FULL, bool SOLVE = false>        // (emit_visits', choose_action's)
XQ_D void advance_game(const SearchParams& P, const SearchBuffers& B, const GameView& gv, SearchLDS& L,
                       const VisitRing& V)
{
    const int lane = lane_id();
    const int g = gv.g;
    const uint32_t game_id = uniu(B.g_game_id[g]);
    int turns = uni(B.g_turns[g]);
    int8_t* gb = B.g_board + (size_t)g * BOARD_LDS;
    uint32_t* hkeys = B.g_hist_key + (size_t)g * (P.max_plies + 2) * KEY_WORDS;
    uint16_t* hacts = B.g_hist_act + (size_t)g * (P.max_plies + 2);
    const double u = philox_uniform(P.seed, game_id, 1, (uint64_t)turns);
    const int action = choose_action<SOLVE>(P, B, gv, L, u, uni((int)B.g_enable_resign[g]) != 0);
    if (V.ring) {
        const bool fast = ply_is_fast(P, game_id, turns);
        emit_visits<FULL>(P, B, gv, V, turns, action < 0, fast, P.forced_k > 0.0 && !fast, P.gumbel_m > 0);
    }
    count(gv, CT_PLIES);
    bool game_over = false, resigned = false;
    int value = 0;
    int final_move = NOMOVE;
    if (action < 0) {                                                  // resign, :126-129
        value = -1; game_over = true; resigned = true;
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
    const int searched = turns;
    if (final_move != NOMOVE) {                                         // :177-184
        if (lane == 0 && turns < P.max_plies + 2) hacts[turns] = (uint16_t)final_move;
        turns += 1;
        value = -value;
    }
    if (turns % 2 == 1) value = -value;                                 // :190-191
    bool store = true;
    if (turns < 10) store = philox_uniform(P.seed, game_id, 0, 1) > 0.9;   // :194-200
    wave_sync_global();
    uint32_t extra = 0u;
    if (V.ring) {                                                       // the next game in this slot starts complete
        int lost = 0;
        if (lane == 0) { lost = V.g_lost[g]; V.g_lost[g] = 0; }
        extra = uni(lost) ? GAME_VISITS_LOST : 0u;
    }
    emit_record(P, B, gv, turns, searched, value, store, resigned, extra);
    new_game(P, B, gv, L, game_id + P.game_id_stride);
}

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
template <bool HIST, bool GUM, bool CACHE, bool SOLVE = false>
XQ_D void sim_body(SearchLDS& L, const SearchParams& P, const SearchBuffers& B, const float* __restrict__ policy,
                   const float* __restrict__ value, void* planes, int mask, int compact,
                   int32_t* __restrict__ q_rows, int32_t* __restrict__ q_count, const EvalCache& C)
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
        if (rest) {
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
            if (CACHE && ((cached >> i) & 1ull)) {
                cached_attach(gv, node, keep_v, (float)v);
                load_path(P, gv, L, i, depth);
                backup(P, gv, L, depth, v);
                if (i_next >= 0) { pre_a(nx, i_next); pre_b(nx, i_next); }
            } else if (depth <= 64) {
                attach_and_backup(P, gv, L, node, (uint32_t)__builtin_amdgcn_readlane((int)my_meta, i), depth, lp, v,
                                  P.policy_logits != 0, keep_v, [&]() {
                                      if (i_next >= 0) { pre_a(nx, i_next); pre_b(nx, i_next); }
                                  });
            } else {
                attach_policy(gv, L, node, policy + slot * NLABELS, P.policy_logits != 0, keep_v, (float)v);
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
            attach_policy(gv, L, node, policy + slot * NLABELS, P.policy_logits != 0, keep_v, value[slot]);
            load_path(P, gv, L, i, depth);
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
            flush_deferred<SOLVE>(P, gv, L, df, &active);
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
        run_sim<HIST, GUM, CACHE, SOLVE>(P, B, gv, L, io, rc, uni(B.g_root[g]), sim, node, depth, &active, ar, fresh, df, C,
                                         (mask & SIM_SELECT) != 0);
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

template <bool HIST, bool GUM>
__global__ __launch_bounds__(64, 4) void k_sim(SearchParams P, SearchBuffers B, const float* __restrict__ policy,
                                           const float* __restrict__ value, void* planes, int mask, int compact,
                                           int32_t* __restrict__ q_rows, int32_t* __restrict__ q_count)
{
    __shared__ SearchLDS L;
    sim_body<HIST, GUM, false>(L, P, B, policy, value, planes, mask, compact, q_rows, q_count, EvalCache{});
}

// k_sim with the evaluation cache on (14 input planes only: cz_search_set_eval_cache refuses the history input)
template <bool GUM>
__global__ __launch_bounds__(64, 4) void k_sim_cached(SearchParams P, SearchBuffers B, const float* __restrict__ policy,
                                                  const float* __restrict__ value, void* planes, int mask, int compact,
                                                  int32_t* __restrict__ q_rows, int32_t* __restrict__ q_count, EvalCache C)
{
    __shared__ SearchLDS L;
    sim_body<false, GUM, true>(L, P, B, policy, value, planes, mask, compact, q_rows, q_count, C);
}

// k_sim with the MCTS solver on (cz_search_set_solver refuses the Gumbel search, forced playouts and the evaluation cache)
template <bool HIST>
__global__ __launch_bounds__(64, 4) void k_sim_solve(SearchParams P, SearchBuffers B, const float* __restrict__ policy,
                                                 const float* __restrict__ value, void* planes, int mask, int compact,
                                                 int32_t* __restrict__ q_rows, int32_t* __restrict__ q_count)
{
    __shared__ SearchLDS L;
    sim_body<HIST, false, false, true>(L, P, B, policy, value, planes, mask, compact, q_rows, q_count, EvalCache{});
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
    char* base = B.pool + ((size_t)chunk << 20) + ((size_t)(node & (uint32_t)(CHUNK_GRANULES - 1)) << 4);   // (rec_ptr)
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
    const float all_p = prior_norm(p0, p1, nm, P.policy_logits != 0);
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
        const char* rbase = B.pool + ((size_t)B.g_chunk_tab[(size_t)g * P.max_chunks + ((uint32_t)root >> CHUNK_SHIFT)] << 20)
                            + ((size_t)((uint32_t)root & (uint32_t)(CHUNK_GRANULES - 1)) << 4);
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
// _root_value, _root_surprise): the pruned counts n [G][128] and their raw total, the search value q, the policy
// surprise s.  A NULL output is not computed.  One wavefront per game.
// gumbel (or the option on): the counts are the Gumbel policy targets, as a VISIT_GUMBEL entry holds them; FULL: the full
// search's (launched while cz_search_set_gumbel_full is on).
template <bool FULL>
__global__ __launch_bounds__(64) void k_root_records(SearchParams P, SearchBuffers B, int32_t* __restrict__ n,
                                                    int32_t* __restrict__ raw_total, double* __restrict__ q,
                                                    double* __restrict__ s, int gumbel)
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
                                             : prune_targets(E.nm, E.lab, m, E.w, E.p, P.c_puct, P.forced_k);
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
}

// cz_policy_target_prune, cz_root_value, cz_root_surprise: the same arithmetic on caller-supplied rows [rows][128], one
// wavefront per row.  out_n (with out_raw_total): the counts n are pruned; otherwise m holds the recorded counts.  A
// NULL input reads as zeros, a NULL output is not computed.
__global__ __launch_bounds__(64) void k_row_records(const uint16_t* __restrict__ labels, const int32_t* __restrict__ m_in,
                                                   const int32_t* __restrict__ n, const double* __restrict__ w,
                                                   const float* __restrict__ p, const uint8_t* __restrict__ n_edges,
                                                   int rows, double c_puct, double k, int32_t* __restrict__ out_n,
                                                   int32_t* __restrict__ out_raw_total, double* __restrict__ out_q,
                                                   double* __restrict__ out_s)
{
    const int r = blockIdx.x;
    if (r >= rows) return;
    const int lane = lane_id();
    const RootEdges E = load_row_edges(labels, n, w, p, n_edges, r);
    int m[2] = {E.n[0], E.n[1]};
    if (out_n) {
        const int S = prune_targets(E.nm, E.lab, m, E.w, E.p, c_puct, k);
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

// chunks a game needs for one full search on an empty tree (what it keeps through resets and between games)
int keep_chunks_for(int sims)
{
    constexpr long long PER_TASK = NODE_HDR_GRANULES + (6 * RESERVE_MOVES + 15) / 16 + RESERVE_MOVES;
    constexpr long long USABLE = CHUNK_GRANULES - MAXMOVES;
    const long long need = (long long)(sims + 1) * PER_TASK + 1;
    return (int)((need + USABLE - 1) / USABLE);
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
    (void)hipFree(s->V.q);
    (void)hipFree(s->V.s);
    (void)hipFree(s->book_mem);
    (void)hipFree(s->C.tab);
    (void)hipFree(s->ec_mem);
    (void)hipFree(s->pool);
    (void)hipFree(s->slab);
    delete s;
    return CZ_OK;
}

size_t cz_search_bytes(const cz_search* s)
{
    if (!s) return 0;
    return s->bytes + (s->C.tab ? (size_t)ec_table_bytes(s->C.log2) : 0);     // (the evaluation cache's table, while it is on)
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
    hipLaunchKernelGGL(k_start_selfplay, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B, first_game_id);
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
    auto sim = [&](int mask, int cq) {
        if (solve) {
            if (hist) hipLaunchKernelGGL((k_sim_solve<true>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count);
            else hipLaunchKernelGGL((k_sim_solve<false>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count);
        } else if (cache) {         // (14 planes: cz_search_set_eval_cache refuses the history input)
            if (gum) hipLaunchKernelGGL((k_sim_cached<true>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count, s->C);
            else hipLaunchKernelGGL((k_sim_cached<false>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count, s->C);
        } else if (gum) {
            if (hist) hipLaunchKernelGGL((k_sim<true, true>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count);
            else hipLaunchKernelGGL((k_sim<false, true>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count);
        } else {
            if (hist) hipLaunchKernelGGL((k_sim<true, false>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count);
            else hipLaunchKernelGGL((k_sim<false, false>), grid, block, 0, st, s->P, s->B, policy, value, planes, mask, cq, q_rows, q_count);
        }
    };
    // evaluation cache: the rows the BACKUP launch is about to attach go into the table first (its only writer)
    if (cache)
        hipLaunchKernelGGL(k_cache_fill, dim3(s->P.G * s->P.K), block, 0, st, s->P, s->B, s->C, policy, value, consume_compact);
    sim(SIM_BACKUP, consume_compact);
    if (gum && s->P.gumbel_full) hipLaunchKernelGGL(k_advance<true>, grid, block, 0, st, s->P, s->B, s->V);
    else if (solve) hipLaunchKernelGGL((k_advance<false, true>), grid, block, 0, st, s->P, s->B, s->V);
    else hipLaunchKernelGGL(k_advance<false>, grid, block, 0, st, s->P, s->B, s->V);
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
    // a game that has to drop its tree keeps enough chunks for one full search of the NEW length (never fewer than it
    // was created with: the initial pool layout gave every game that many)
    int keep = keep_chunks_for(simulation_num_per_move);
    if (keep > s->P.max_chunks) keep = s->P.max_chunks;
    if (keep > s->keep_chunks_created) s->P.keep_chunks = keep;
    else s->P.keep_chunks = s->keep_chunks_created;
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
    if (log2_entries != 0 && s->P.solver)
        return serr(CZ_ERR_ARG, "cz_search_set_eval_cache: the MCTS solver is on (cz_search_set_solver)");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipStreamSynchronize(st);             // no launch that holds the old table is still running
    if (e != hipSuccess) return serr_hip("cz_search_set_eval_cache", e);
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

// Switch a side ring of the visit ring (one double per slot: V.q, V.s) on or off; `what` names the caller in errors
static int side_ring(cz_search* s, double*& ring, int on, hipStream_t st, const char* what)
{
    hipError_t e = hipStreamSynchronize(st);             // no launch in flight may still use the old buffer
    if (e != hipSuccess) return serr_hip(what, e);
    if (on && ring) return CZ_OK;                        // already on: the ring and what waits in it stay
    (void)hipFree(ring);
    ring = nullptr;
    if (!on) return CZ_OK;
    void* mem = nullptr;
    const size_t bytes = (size_t)s->V.cap * sizeof(double);
    e = hipMalloc(&mem, bytes);
    char where[64];
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
    hipStream_t st = (hipStream_t)stream;
    // the value and the surprise ring share the visit ring's slots: they go with it.  side_ring waits for the stream:
    // no launch in flight may still use the old buffers
    if (side_ring(s, s->V.q, 0, st, "cz_search_record_visits") != CZ_OK
        || side_ring(s, s->V.s, 0, st, "cz_search_record_visits") != CZ_OK)
        return CZ_ERR_HIP;
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

static_assert(CZ_MOVE_FAST == MOVE_FAST && CZ_VISIT_FAST == VISIT_FAST, "czero.h: playout cap flags");

int cz_search_set_playout_cap(cz_search* s, int fast_sims, double full_rate, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_playout_cap: null handle");
    if (fast_sims < 0 || fast_sims > s->P.sims)
        return serr(CZ_ERR_ARG, "cz_search_set_playout_cap: fast_sims outside 0 .. simulation_num_per_move");
    if (fast_sims > 0 && !(full_rate >= 0.0 && full_rate <= 1.0))
        return serr(CZ_ERR_ARG, "cz_search_set_playout_cap: full_rate outside [0, 1]");
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);   // launches in flight keep the schedule they started with
    if (e != hipSuccess) return serr_hip("cz_search_set_playout_cap", e);
    if (fast_sims > 0 && s->P.gumbel_m > 0)
        return serr(CZ_ERR_ARG, "cz_search_set_playout_cap: the Gumbel root search is on (cz_search_set_gumbel)");
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
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);   // launches in flight keep the setting they started with
    if (e != hipSuccess) return serr_hip("cz_search_set_forced_playouts", e);
    if (k > 0.0 && s->P.gumbel_m > 0)
        return serr(CZ_ERR_ARG, "cz_search_set_forced_playouts: the Gumbel root search is on (cz_search_set_gumbel)");
    if (k > 0.0 && s->P.solver)
        return serr(CZ_ERR_ARG, "cz_search_set_forced_playouts: the MCTS solver is on (cz_search_set_solver)");
    s->P.forced_k = k;
    return CZ_OK;
}

static_assert(CZ_VISIT_GUMBEL == VISIT_GUMBEL && CZ_GUMBEL_MAX_M == GUMBEL_MAX_M, "czero.h: Gumbel root search");

// k_root_records, the instantiation of the object's setting (cz_search_set_gumbel_full)
static void launch_root_records(cz_search* s, hipStream_t st, const SearchParams& P, const SearchBuffers& B, int32_t* n,
                                int32_t* raw_total, double* q, double* sv, int gumbel)
{
    if (P.gumbel_m > 0 && P.gumbel_full)
        hipLaunchKernelGGL(k_root_records<true>, dim3(s->P.G), dim3(64), 0, st, P, B, n, raw_total, q, sv, gumbel);
    else
        hipLaunchKernelGGL(k_root_records<false>, dim3(s->P.G), dim3(64), 0, st, P, B, n, raw_total, q, sv, gumbel);
}

int cz_search_set_gumbel(cz_search* s, int m, double c_visit, double c_scale, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_set_gumbel: null handle");
    if (m < 0 || m > GUMBEL_MAX_M) return serr(CZ_ERR_ARG, "cz_search_set_gumbel: m outside 0 .. 128");
    if (!finite_nonneg(c_visit) || !finite_nonneg(c_scale))
        return serr(CZ_ERR_ARG, "cz_search_set_gumbel: c_visit or c_scale negative or not finite");
    if (m > 0 && (s->P.forced_k > 0.0 || s->P.fast_sims > 0))
        return serr(CZ_ERR_ARG, "cz_search_set_gumbel: forced playouts or the playout cap are on, each defines its own root rule");
    if (m > 0 && s->P.solver)
        return serr(CZ_ERR_ARG, "cz_search_set_gumbel: the MCTS solver is on (cz_search_set_solver)");
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);   // launches in flight keep the setting they started with
    if (e != hipSuccess) return serr_hip("cz_search_set_gumbel", e);
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
    if (on && s->P.gumbel_m > 0)
        return serr(CZ_ERR_ARG, "cz_search_set_solver: the Gumbel root search is on (cz_search_set_gumbel)");
    if (on && s->P.forced_k > 0.0)
        return serr(CZ_ERR_ARG, "cz_search_set_solver: forced playouts are on (cz_search_set_forced_playouts)");
    if (on && s->C.tab)
        return serr(CZ_ERR_ARG, "cz_search_set_solver: the evaluation cache is on (cz_search_set_eval_cache)");
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);   // launches in flight keep the setting they started with
    if (e != hipSuccess) return serr_hip("cz_search_set_solver", e);
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
                       n_edges, rows, c_puct, k, out_n, out_raw_total, (double*)nullptr, (double*)nullptr);
    S_LAUNCH_CHECK("cz_policy_target_prune");
    return CZ_OK;
}

int cz_search_record_values(cz_search* s, int on, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_record_values: null handle");
    if (on && !s->V.ring) return serr(CZ_ERR_ARG, "cz_search_record_values: needs cz_search_record_visits on");
    return side_ring(s, s->V.q, on, (hipStream_t)stream, "cz_search_record_values");
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
                       n_edges, rows, 0.0, 0.0, (int32_t*)nullptr, (int32_t*)nullptr, out_q, (double*)nullptr);
    S_LAUNCH_CHECK("cz_root_value");
    return CZ_OK;
}

static_assert(CZ_SURPRISE_BOUND == 70 && SURPRISE_R_FLOOR == 1e-30, "czero.h: ln(1 / the floor) = 69.08 < the bound");

int cz_search_record_surprise(cz_search* s, int on, void* stream)
{
    if (!s) return serr(CZ_ERR_ARG, "cz_search_record_surprise: null handle");
    if (on && !s->V.ring) return serr(CZ_ERR_ARG, "cz_search_record_surprise: needs cz_search_record_visits on");
    return side_ring(s, s->V.s, on, (hipStream_t)stream, "cz_search_record_surprise");
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
                       (double*)nullptr, out);
    S_LAUNCH_CHECK("cz_root_surprise");
    return CZ_OK;
}

// cz_search_drain_visits, _q and _qs: q_buf / s_buf NULL = that ring is not copied
static int drain_visits(cz_search* s, void* host_buf, double* q_buf, double* s_buf, int max_entries, int* n_out,
                        uint64_t* dropped_out, void* stream)
{
    if (!s || !n_out || max_entries < 0) return serr(CZ_ERR_ARG, "cz_search_drain_visits: bad argument");
    if (!s->V.ring) return serr(CZ_ERR_ARG, "cz_search_drain_visits: visit recording is off");
    if (q_buf && !s->V.q) return serr(CZ_ERR_ARG, "cz_search_drain_visits_q: value recording is off");
    if (s_buf && !s->V.s) return serr(CZ_ERR_ARG, "cz_search_drain_visits_qs: surprise recording is off");
    hipStream_t st = (hipStream_t)stream;
    unsigned int ctl[6] = {0u, 0u, 0u, 0u, 0u, 0u};        // tail, head, -, -, dropped (64 bit): one copy
    static_assert(sizeof(unsigned long long) == 8, "dropped counter is 64-bit");
    hipError_t e = hipMemcpyAsync(ctl, s->V.ctl, sizeof(ctl), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return serr_hip("cz_search_drain_visits", e);
    unsigned long long dropped = 0ull;
    memcpy(&dropped, &ctl[4], sizeof(dropped));
    const unsigned int tail = ctl[0], head = ctl[1], cap = s->V.cap;
    // reservations at or beyond head + cap were dropped by the kernel (and counted): the valid entries are [head, head + cap)
    const unsigned int valid = tail - head < cap ? tail - head : cap;
    if (dropped_out) *dropped_out = (uint64_t)dropped;
    if (!host_buf) { *n_out = (int)valid; return CZ_OK; }
    // all or nothing: a partial drain would have to remember where the dropped reservations lie
    if (valid > (unsigned int)max_entries)
        return serr(CZ_ERR_ARG, "cz_search_drain_visits: host_buf holds fewer entries than are waiting (ask with host_buf = NULL)");
    const unsigned int k = valid;
    unsigned int done = 0;
    while (done < k && e == hipSuccess) {                // at most two runs: the ring may wrap once
        const unsigned int at = (head + done) % cap;
        const unsigned int run = (cap - at) < (k - done) ? (cap - at) : (k - done);
        e = hipMemcpyAsync((char*)host_buf + (size_t)done * VISIT_STRIDE, s->V.ring + (size_t)at * VISIT_STRIDE,
                           (size_t)run * VISIT_STRIDE, hipMemcpyDeviceToHost, st);
        if (q_buf && e == hipSuccess)
            e = hipMemcpyAsync(q_buf + done, s->V.q + at, (size_t)run * sizeof(double), hipMemcpyDeviceToHost, st);
        if (s_buf && e == hipSuccess)
            e = hipMemcpyAsync(s_buf + done, s->V.s + at, (size_t)run * sizeof(double), hipMemcpyDeviceToHost, st);
        done += run;
    }
    const unsigned int new_head = tail;
    if (e == hipSuccess) e = hipMemcpyAsync(s->V.ctl + 1, &new_head, sizeof(new_head), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return serr_hip("cz_search_drain_visits", e);
    *n_out = (int)k;
    return CZ_OK;
}

int cz_search_drain_visits(cz_search* s, void* host_buf, int max_entries, int* n_out, uint64_t* dropped_out, void* stream)
{
    return drain_visits(s, host_buf, nullptr, nullptr, max_entries, n_out, dropped_out, stream);
}

int cz_search_drain_visits_q(cz_search* s, void* host_buf, double* q_buf, int max_entries, int* n_out,
                             uint64_t* dropped_out, void* stream)
{
    if (host_buf && !q_buf) return serr(CZ_ERR_ARG, "cz_search_drain_visits_q: null q_buf");
    return drain_visits(s, host_buf, host_buf ? q_buf : nullptr, nullptr, max_entries, n_out, dropped_out, stream);
}

int cz_search_drain_visits_qs(cz_search* s, void* host_buf, double* q_buf, double* s_buf, int max_entries, int* n_out,
                              uint64_t* dropped_out, void* stream)
{
    return drain_visits(s, host_buf, host_buf ? q_buf : nullptr, host_buf ? s_buf : nullptr, max_entries, n_out,
                        dropped_out, stream);
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
    hipLaunchKernelGGL(k_pv, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B, max_len, moves, visits);
    S_LAUNCH_CHECK("cz_search_pv");
    return CZ_OK;
}

int cz_search_choose(cz_search* s, const double* u, int32_t* action, void* stream)
{
    if (!s || !action) return serr(CZ_ERR_ARG, "cz_search_choose: null argument");
    if (s->P.solver) hipLaunchKernelGGL(k_choose<true>, dim3(s->P.G), dim3(64), 0, (hipStream_t)stream, s->P, s->B, u, action);
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
