#!/bin/bash
# GPU: the default benchmark on the parent build (variants/libczero_parent.so, selected with CZ_LIB as in
# tools/ab_forced_playouts.sh) and on this tree's build, alternating on one box, the max-q record off (bench.py never
# switches it on): k_advance with a NULL max-q ring must cost nothing, and the k_sim* kernels are the parent's.  The
# comparison is with the parent's own range on the same box.  Stops at the first run that fails.
#   usage: [OUT=dir] bash tools/ab_resign_audit.sh [REPS]      -> $OUT/ab_resign_audit.log  (OUT defaults to profiles/; REPS to 5)
set -o pipefail
out=${OUT:-profiles}
mkdir -p $out
log=$out/ab_resign_audit.log
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
