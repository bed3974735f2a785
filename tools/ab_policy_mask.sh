#!/bin/bash
# GPU: what `run.py opt --policy-mask legal` costs.
#  1. the default benchmark on the parent build (variants/libczero_parent.so, selected with CZ_LIB as in
#     tools/ab_moves_left.sh) and on this tree's build, alternating on one box: the search and network kernels are
#     untouched and bench.py trains nothing -- a check, not a gate;
#  2. one training step at the `normal` batch size with the loss over all labels and over the legal moves, alternated legs of
#     this build (tools/train_rate.py --policy-mask legal): the loss launch's time and the whole step's.
# Stops at the first run that fails.
#   usage: [OUT=dir] bash tools/ab_policy_mask.sh [REPS] [LEGS]
#          -> $OUT/ab_policy_mask.log, $OUT/policy_mask_rate.json  (OUT defaults to profiles/)
set -o pipefail
out=${OUT:-profiles}
mkdir -p $out
log=$out/ab_policy_mask.log
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
timeout -k 10 400 python tools/train_rate.py --policy-mask legal --repeats ${2:-3} 2>/dev/null | tail -1 > $out/policy_mask_rate.json || { echo "FAILED: train_rate"; exit 1; }
cat $out/policy_mask_rate.json
