#!/bin/bash
# GPU: the default benchmark on the parent build (variants/libczero_parent.so, selected with CZ_LIB as in
# tools/ab_record_q.sh) and on this tree's build, alternating on one box, the surprise record off (bench.py never
# switches it on): k_advance with a NULL surprise ring must cost nothing.  Stops at the first run that fails.
#   usage: [OUT=dir] [LOG=name] bash tools/ab_surprise.sh [REPS] [bp]   -> $OUT/ab_surprise.log  (OUT defaults to profiles/)
#   a second argument "bp" runs this tree's build first in every pair: two logs, one of each order, cancel a drift
set -o pipefail
out=${OUT:-profiles}
mkdir -p $out
log=$out/${LOG:-ab_surprise.log}
: > $log
one() {     # name, then environment assignments
  local name=$1; shift
  echo "run=$name" >> $log
  env "$@" timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 4 2>/dev/null | tail -1 >> $log || { echo "FAILED: $name" >> $log; cat $log; exit 1; }
}
for rep in $(seq 1 ${1:-3}); do
  [ "$2" = bp ] && one branch_$rep CZ_LIB=
  one parent_$rep CZ_LIB=$PWD/variants/libczero_parent.so
  [ "$2" = bp ] || one branch_$rep CZ_LIB=
done
grep -o 'run=[a-z_0-9]*\|"value":[0-9.]*' $log
