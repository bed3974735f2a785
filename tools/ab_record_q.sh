#!/bin/bash
# GPU: the default benchmark on the parent build (variants/libczero_parent.so, selected with CZ_LIB as in
# tools/ab_forced_playouts.sh) and on this tree's build, alternating on one box, the value record off (bench.py never
# switches it on): k_advance with a NULL value ring must cost nothing.  Stops at the first run that fails.
#   usage: [OUT=dir] bash tools/ab_record_q.sh [REPS]      -> $OUT/ab_record_q.log  (OUT defaults to profiles/)
set -o pipefail
out=${OUT:-profiles}
mkdir -p $out
log=$out/ab_record_q.log
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
cat $log
