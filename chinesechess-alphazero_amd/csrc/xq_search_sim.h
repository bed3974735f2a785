// xq_search_sim.h -- part of xq_search.hip's translation unit; do not compile it into a second one.  Why: the same text as a
// unit of its own gave all eight k_sim* kernels 0.4-1.7 % more or fewer instructions (k_sim<false,false> 18 740 against
// 18 608, equal registers and scratch, nothing called out of line; cause not found).  The benchmark measures those kernels, so
// text only moves between these headers, and the proof of a move is the unit's device assembly, kernel by kernel
// (EXPERIMENTS.md, "the search unit's text in headers").
//
// One simulation: slot bookkeeping (sim_finish), the deferred results (Deferred, defer_result), find_in_path, the evaluation
// queue's slot (RoundIO, write_planes), history_board, the game's heap (Arena, heap_alloc) and expand_node, the evaluation
// cache's probe (cache_probe, cached_attach), edge_move, run_sim, load_path, flush_deferred.
#pragma once
#include "xq_search_tree.h"
#include "xq_search_select.h"
#include "xq_search_ml.h"
#include "xq_search_draw.h"
#include "xq_search_var.h"
#include "xq_search_solver.h"
#include "xq_evalcache.h"
#include "../../include/czero.h"

namespace {

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

// backup() of a simulation that ends without a network row; ML: m goes up too, with k = 0; DRAW: d goes up too, with dq (0
// for every such end but a repetition worth 0: flush_deferred); VAR: v * v goes up too (backup_v)
template <bool ML, bool DRAW = false, bool VAR = false>
XQ_D void backup_end(const SearchParams& P, const GameView& gv, const SearchLDS& L, int depth, double v, int dq = 0)
{
    if constexpr (ML) backup_m(gv, L, depth, 0);
    if constexpr (DRAW) backup_d(gv, L, depth, dq);
    if constexpr (VAR) backup_v(gv, L, depth, v);
    backup(P, gv, L, depth, v);
}

// One descent of simulation `sim` starting at `node` with `depth` path entries already in L.path_*
// (MCTS_search, player.py:198-260).  `node` < 0 means the root position is not in the tree yet.
// CACHE: the evaluation cache is on (cz_search_set_eval_cache); `probe` (the SELECT launch): a new leaf asks the table C
// before it takes a queue row.
// SOLVE: the MCTS solver is on (cz_search_set_solver): the arrival on a proven node and select_solve; likewise an
// instantiation of its own.
// ML: the moves-left utility is on (cz_search_set_moves_left): a statistics block carries its M records, the selection reads
// them (select_edge<GUM, ML>), a backup made here takes m up with k = 0; likewise an instantiation of its own.
// DRAW: the draw average is on (cz_search_set_draw): a statistics block carries its D records in the M records' place, the
// selection reads them with the sign of the node's depth, a backup made here takes d up with dq = 0; likewise.
// VAR: the lower-confidence-bound move choice is on (cz_search_set_lcb): a statistics block carries its V records in the same
// place, the selection is the plain one, a backup made here takes its squared value up (backup_v); likewise.
// SCHED: the schedule of c_puct is on (cz_search_set_cpuct_schedule): the selection computes c(sum_n); likewise.
template <bool HIST, bool GUM, bool CACHE, bool SOLVE = false, bool ML = false, bool DRAW = false, bool VAR = false,
          bool SCHED = false>
XQ_D void run_sim(const SearchParams& P, const SearchBuffers& B, const GameView& gv, SearchLDS& L,
                  const RoundIO& io, const RootCtx& rc0, int root, int sim, int node, int depth, int* active,
                  Arena& ar, bool fresh, Deferred& df, const EvalCache& C, bool probe,
                  const MovesLeftState& M = MovesLeftState{}, const DrawState& D = DrawState{})
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
        if (idx < 0) { count(gv, CT_OVERFLOW_SIMS); backup_end<ML, DRAW, VAR>(P, gv, L, 0, 0.0); sim_finish(gv, sim, active); return; }
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
            backup_end<ML, DRAW, VAR>(P, gv, L, depth, 0.0);
            sim_finish(gv, sim, active);
            return;
        }
        const int nm = (int)(meta & 0xFF);
        // the node's statistics block: allocated on the first selection FROM the node (most nodes stay leaves)
        uint32_t stat = hdr.stat;
        const bool fresh_stat = stat == 0u && nm > 0;
        if (fresh_stat) {
            stat = heap_alloc(ar, (ML || DRAW || VAR) ? 2 * nm : nm);   // (ML / DRAW / VAR: the M / D / V records directly behind the statistics)
            if (stat == 0u) {
                count(gv, CT_OVERFLOW_SIMS);
                backup_end<ML, DRAW, VAR>(P, gv, L, depth, 0.0);
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
            if constexpr (ML || DRAW || VAR) {                      // (a D record is an M record's bytes; a V record's zero too)
                MRec* mb = m_block(sb, nm);
                for (int j = lane; j < nm; j += 64) mb[j] = MRec{0, 0, 0};
            }
        }
        RootCtx rc = rc0;
        rc.is_root = (node == root);                                // player.py:266
        rc.sim = sim;
        Picked pk;
        if constexpr (SOLVE) {                                      // (have = false: the edge is reloaded below)
            pk = Picked{select_solve<SCHED>(P, gv, base, fresh_stat ? nullptr : sb, hdr.sum_n, nm, rc), false, 0, CHILD_UNKNOWN, 0, 0.0};
        } else {
            pk = select_edge<GUM, ML, DRAW, SCHED>(P, B, g, base, fresh_stat ? nullptr : sb, hdr.sum_n, nm, rc, hdr.val, M,
                                            DRAW ? draw_sigma(D, depth) : 0.0);
        }
        if (pk.j < 0) {                                             // "Best action is None": cannot happen
            backup_end<ML, DRAW, VAR>(P, gv, L, depth, 0.0);
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
                        backup_end<ML, DRAW, VAR>(P, gv, L, depth, 0.0);
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
// ML: m goes up with k = 0, as after every end without a network row
// DRAW: d goes up too: a deferred value of 0 is a repetition that is a draw (the only deferred value that is 0), dq = 2^20;
// every other one (a terminal child, a repetition worth +-1) has dq = 0
// VAR: the squared value goes up too: 4 for a terminal child, 0 or 1 for a repetition
template <bool SOLVE = false, bool ML = false, bool DRAW = false, bool VAR = false>
XQ_D void flush_deferred(const SearchParams& P, const GameView& gv, SearchLDS& L, Deferred& df, int* active)
{
    if (df.lo == 0 && df.hi == 0) return;
    wave_sync_global();                  // lane 0's path stores of this launch are complete before the lanes reload paths
    auto one = [&](int i) {
        const int depth = uni(gv.s_depth[i]);
        const double v = (double)uni(gv.s_node[i]);
        load_path(P, gv, L, i, depth);
        backup_end<ML, DRAW, VAR>(P, gv, L, depth, v, (DRAW && v == 0.0) ? DRAW_QUANTA : 0);
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

}  // namespace
