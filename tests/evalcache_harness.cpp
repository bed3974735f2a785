// tests/evalcache_harness.cpp -- CPU build of the evaluation cache's layout and slot function
// (chinesechess-alphazero_amd/csrc/xq_evalcache.h), the same text the search kernels compile.  Built with g++ by
// tests/test_eval_cache_cpu.py.
#include <stddef.h>
#include <stdint.h>
#include "../chinesechess-alphazero_amd/csrc/xq_evalcache.h"

using namespace xq;

extern "C" {

// stride, offsets of key / claim / meta / value / p, the size limits
void ec_layout(int32_t* out)
{
    out[0] = EC_STRIDE;
    out[1] = (int32_t)offsetof(EvalCacheEntry, key);
    out[2] = (int32_t)offsetof(EvalCacheEntry, claim);
    out[3] = (int32_t)offsetof(EvalCacheEntry, meta);
    out[4] = (int32_t)offsetof(EvalCacheEntry, value);
    out[5] = (int32_t)offsetof(EvalCacheEntry, p);
    out[6] = EC_MIN_LOG2;
    out[7] = EC_MAX_LOG2;
}

uint64_t ec_bytes(int log2_entries) { return ec_table_bytes(log2_entries); }

void ec_slots(const uint64_t* hashes, int n, int mirrored, int log2_entries, uint32_t* out)
{
    for (int i = 0; i < n; ++i) out[i] = ec_slot(hashes[i], mirrored != 0, log2_entries);
}

uint32_t ec_meta_word(int n_moves, int mirrored) { return ec_meta(n_moves, mirrored != 0); }

}
