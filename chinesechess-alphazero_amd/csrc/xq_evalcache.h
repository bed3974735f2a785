// xq_evalcache.h -- layout and slot function of the cross-game evaluation cache (host + device).
//
// cz_search_set_eval_cache (include/czero.h): a direct-mapped table of network results keyed by position, shared by all
// games of one search object and kept across games, tree resets and new roots.  A row's network output does not depend on
// its place in the batch, and a node's priors are a function of its logits row and its move list, so an entry holds
// exactly what the attach of an evaluated leaf would have written: a search with the table on produces the bits of the
// search with it off.
//
// Who touches the table when: READ only by the k_sim(SELECT) launch (the probe of a new leaf: cache_probe, csrc/xq_search_sim.h),
// WRITTEN only by k_cache_fill (csrc/xq_search_round.h), the first launch of a round, NOT touched by the k_sim(BACKUP) launch.  All on the search's
// one stream: a reader only ever sees entries an earlier launch completed.  No lock, no fence, no wait.
//
// Everything here is XQ_HD so that tests/test_eval_cache_cpu.py checks the same text (tests/evalcache_harness.cpp).
#pragma once
#include <stdint.h>
#include "xq_lane.h"

namespace xq {

constexpr int EC_MIN_LOG2 = 10, EC_MAX_LOG2 = 24;   // cz_search_set_eval_cache: 0 = off, else this range
constexpr int EC_KEY_WORDS = 12;                    // = KEY_WORDS (xq_search.h): the 48-byte packed position
constexpr int EC_MAX_MOVES = 128;                   // = MAXMOVES
constexpr uint32_t EC_MIRROR = 1u << 8;             // entry meta: the row was evaluated in the mirror image (the low 8 bits of
                                                    // meta are the move count, as in a node's header)
constexpr uint32_t EC_VALID = 1u << 31;             // entry meta: the entry holds a result (a cleared table is all zero)

// One entry.  A match is all twelve key words and meta == move count | mirror bit | EC_VALID, never the hash alone.
struct EvalCacheEntry {
    uint32_t key[EC_KEY_WORDS];     // the packed position (pack_key)
    uint32_t claim;                 // stamp of the round whose fill last claimed the entry (one writer per entry and round)
    uint32_t meta;                  // move count | EC_MIRROR | EC_VALID
    float value;                    // the network value of the row, as the round was handed it
    uint32_t pad;
    float p[EC_MAX_MOVES];          // the priors exactly as the attach writes them into the node record
};
constexpr int EC_STRIDE = (int)sizeof(EvalCacheEntry);
static_assert(EC_STRIDE == 576 && EC_STRIDE <= 640 && EC_STRIDE % 64 == 0, "include/czero.h: CZ_EVAL_CACHE_STRIDE");

XQ_HD uint32_t ec_meta(int n_moves, bool mirrored)
{
    return (uint32_t)n_moves | (mirrored ? EC_MIRROR : 0u) | EC_VALID;
}

// The entry of a position: the 64-bit hash pack_key returns, mixed with the mirror bit (a position and its mirror-bit twin
// do not compete for one entry), top log2_entries bits.
XQ_HD uint32_t ec_slot(uint64_t hash, bool mirrored, int log2_entries)
{
    const uint64_t x = mix64(hash ^ (mirrored ? 0xD6E8FEB86659FD93ULL : 0ULL));
    return (uint32_t)(x >> (64 - log2_entries));
}

XQ_HD uint64_t ec_table_bytes(int log2_entries) { return (uint64_t)EC_STRIDE << log2_entries; }

// the table and its bookkeeping as the kernels get them (an argument of its own: SearchParams / SearchBuffers stay as
// they are)
struct EvalCache {
    EvalCacheEntry* tab;            // [1 << log2]; NULL = off
    int log2;
    float* s_cval;                  // [G*K] the value of a slot whose leaf hit the table (SIM_CACHED)
    uint32_t* stamp;                // [1] the current round's claim stamp; stepped by the k_sim(BACKUP) launch
    unsigned long long* g_probes;   // [G] probes of game g's wave (written by that wave alone)
    unsigned long long* g_hits;     // [G] ... of which hit
    unsigned long long* s_stores;   // [G*K] entries written for queue slot i (written by that slot's fill wave alone)
};

}  // namespace xq
