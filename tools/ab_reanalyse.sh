#!/bin/bash
# GPU: the default benchmark on the parent build (variants/libczero_parent.so, selected with CZ_LIB as in
# tools/ab_forced_playouts.sh) and on this tree's build, alternating on one box, no script set (bench.py never sets one): the
# scripted game loop is a kernel instantiation of its own (k_advance_script), so every kernel the benchmark launches is the
# parent's.  The comparison is with the parent's own range on the same box.  Stops at the first run that fails.
#   usage: [OUT=dir] bash tools/ab_reanalyse.sh [REPS]      -> $OUT/ab_reanalyse.log  (OUT defaults to profiles/; REPS to 5)
set -o pipefail
out=${OUT:-profiles}
mkdir -p $out
log=$out/ab_reanalyse.log
: > $log
one() {     # name, then environment assignments
  local name=$1; shift
  echo "run=$name" >> $log
  env "$@" timeout -k 10 300 python bench.py --gpus 1 --steps 20 --warmup 4 2>/dev/null | tail -1 >> $log || { echo "FAILED: $name" >> $log; cat $log; exit 1; }
}
for rep in $(seq 1 ${1:-5}); do
  one parent_$rep CZ_LIB=$PWD/variants/libczero_parent.so
  one branch_$rep CZ_LIB=
done
cat $log
