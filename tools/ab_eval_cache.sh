#!/bin/bash
# GPU: what the cross-game evaluation cache (cz_search_set_eval_cache) costs and gains.
#  1. the default benchmark on the parent build (variants/libczero_parent.so, selected with CZ_LIB as in
#     tools/ab_leaf_mirror.sh) and on this tree's build, alternating on one box, the cache off (bench.py never switches it
#     on): the off rate must lie within the spread the repeated parent legs show -- the kernels launched with the cache off
#     are the ones launched before;
#  2. sustained legs off / on of this build at `normal` (tools/eval_cache_rate.py): expansions/s, hit rates, stores, the
#     table's bytes, the fill kernel's time, the share of in-round duplicate rows;
#  3. the same with --sims 64, and with a 16-position book (BOOK, default tests/golden/book.txt).
# Stops at the first run that fails.
#   usage: [OUT=dir] [PARENT=lib] [BOOK=file] bash tools/ab_eval_cache.sh [REPS] [ROUNDS] [LOG2]
#          -> $OUT/ab_eval_cache.log, $OUT/eval_cache_rate{,_sims64,_book16}.json (+ .err: one line per leg as it ends)
#             (OUT defaults to profiles/)
set -o pipefail
out=${OUT:-profiles}
parent=${PARENT:-$PWD/variants/libczero_parent.so}
book=${BOOK:-tests/golden/book.txt}
reps=${1:-3}
rounds=${2:-3000}
log2=${3:-22}
mkdir -p $out
log=$out/ab_eval_cache.log
: > $log
one() {     # name, then environment assignments
  local name=$1; shift
  echo "run=$name" >> $log
  env "$@" timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 4 2>/dev/null | tail -1 >> $log || { echo "FAILED: $name" >> $log; cat $log; exit 1; }
}
for rep in $(seq 1 $reps); do
  one parent_$rep CZ_LIB=$parent
  one branch_$rep CZ_LIB=
done
cat $log
rate() {    # name, then the tool's extra arguments
  local name=$1; shift
  timeout -k 10 1100 python tools/eval_cache_rate.py --rounds $rounds --log2 $log2 --out $out/$name.json "$@" 2>$out/$name.err | tail -1 || { echo "FAILED: $name"; tail -5 $out/$name.err; exit 1; }
}
rate eval_cache_rate
rate eval_cache_rate_sims64 --sims 64
rate eval_cache_rate_book16 --book $book --book-n 16
