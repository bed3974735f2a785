#!/bin/bash
# GPU: the default benchmark on the parent build (variants/libczero_parent.so, selected with CZ_LIB as in tools/ab_search.sh)
# and on this tree's build, alternating on one box, no book set; then one run of this build with a book at rate 1
# (informational: game lengths differ, so expansions/s is not comparable).  Stops at the first run that fails.
#   usage: [OUT=dir] bash tools/ab_book.sh [REPS]      -> $OUT/ab_book.log  (OUT defaults to profiles/)
set -o pipefail
out=${OUT:-profiles}
mkdir -p $out
log=$out/ab_book.log
: > $log
one() {     # name, then environment assignments
  local name=$1; shift
  echo "run=$name" >> $log
  env "$@" timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 4 2>/dev/null | tail -1 >> $log || { echo "FAILED: $name" >> $log; cat $log; exit 1; }
}
for rep in $(seq 1 ${1:-3}); do
  one parent_$rep CZ_LIB=$PWD/variants/libczero_parent.so
  one branch_$rep CZ_LIB=
done
one branch_book_rate1 CZ_LIB= CZ_BOOK=$PWD/tests/golden/book.txt
cat $log
