// xq_search_tree.h -- part of xq_search.hip's translation unit; do not compile it into a second one.  Why: the same text as a
// unit of its own gave all eight k_sim* kernels 0.4-1.7 % more or fewer instructions (k_sim<false,false> 18 740 against
// 18 608, equal registers and scratch, nothing called out of line; cause not found).  The benchmark measures those kernels, so
// text only moves between these headers, and the proof of a move is the unit's device assembly, kernel by kernel
// (EXPERIMENTS.md, "the search unit's text in headers").
//
// The tree as one wavefront sees it: the LDS scratch (SearchLDS), an edge's statistics (EdgeStat), the pointers into one game's
// state (GameView, make_view), the wave-uniform readers (uni*), the node and edge accessors, the counters and PROF, the
// counter-based generator (philox_uniform), the leaf-mirror table and coin, packed keys and the transposition hash
// (hash_lookup), backup, the node header (NodeHdr).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "xq_rules.h"
#include "xq_search.h"
#include "xq_mirror.h"

using namespace xq;

namespace {

constexpr int MAXD_LDS = 128;          // LDS copy of the current path; SearchParams.max_depth <= this
constexpr int INIT_NIB_WORDS = KEY_WORDS;


struct SearchLDS {
    RulesLDS r;
    uint32_t key[KEY_WORDS + 4];
    int32_t path_node[MAXD_LDS];
    int32_t path_edge[MAXD_LDS];
    unsigned long long ctr[CT_LDS_COUNT];  // counter accumulators of the running kernel
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

// record id -> address (ids of one record never straddle a chunk); `chunk`: the pool chunk number of the id's local chunk
XQ_D char* rec_addr(char* pool, uint32_t chunk, uint32_t id)
{
    return pool + ((size_t)chunk << 20) + ((size_t)(id & (uint32_t)(CHUNK_GRANULES - 1)) << 4);
}
XQ_D char* rec_ptr(const GameView& gv, uint32_t id) { return rec_addr(gv.pool, gv.chtab[id >> CHUNK_SHIFT], id); }
XQ_D const uint32_t* node_key(const GameView& gv, int node) { return reinterpret_cast<const uint32_t*>(rec_ptr(gv, (uint32_t)node)); }
XQ_D float* node_p(char* base) { return reinterpret_cast<float*>(base + NODE_OFF_P); }
XQ_D uint16_t* node_mv(char* base, int nm) { return reinterpret_cast<uint16_t*>(base + NODE_OFF_P + 4 * nm); }
XQ_D EdgeStat* edge_ptr(const GameView& gv, uint32_t edge) { return reinterpret_cast<EdgeStat*>(rec_ptr(gv, edge)); }

// Counters accumulate in LDS while a kernel runs (no global round trip per event) and are flushed once.
XQ_D void count(const GameView& gv, int which, unsigned long long by = 1)
{
    if (lane_id() == 0) gv.lctr[which] += by;
}
// a counter at or beyond CT_LDS_COUNT has no LDS accumulator: straight to the game's global block (lane 0 is its only writer)
XQ_D void count_direct(const GameView& gv, int which, unsigned long long by = 1)
{
    if (lane_id() == 0) {
        if (which < CT_LDS_COUNT) gv.lctr[which] += by;
        else gv.ctr[which] += by;
    }
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
    for (int i = lane_id(); i < CT_LDS_COUNT; i += 64) gv.lctr[i] = 0;
    wave_sync();
}
XQ_D void counters_flush(const GameView& gv)
{
    wave_sync_global();
    for (int i = lane_id(); i < CT_LDS_COUNT; i += 64) {
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

}  // namespace
