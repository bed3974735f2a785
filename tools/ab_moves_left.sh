#!/bin/bash
# GPU: what the moves-left output costs.
#  1. the default benchmark on the parent build (variants/libczero_parent.so, selected with CZ_LIB as in
#     tools/ab_wdl_head.sh) and on this tree's build, alternating on one box: bench.py asks no network for the output, so
#     both run cz_heads_tail, whose kernels are the instantiations the parent launches -- a check, not a gate;
#  2. the dense tail at 32 768 rows with and without the output, both value heads, alternating legs
#     (tools/moves_left_tail_cost.py).
# Stops at the first run that fails.
#   usage: [OUT=dir] bash tools/ab_moves_left.sh [REPS] [LEGS]
#          -> $OUT/ab_moves_left.log, $OUT/moves_left_tail_cost.json  (OUT defaults to profiles/)
set -o pipefail
out=${OUT:-profiles}
mkdir -p $out
log=$out/ab_moves_left.log
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
timeout -k 10 300 python tools/moves_left_tail_cost.py --legs ${2:-7} --out $out/moves_left_tail_cost.json 2>/dev/null | tail -1 || { echo "FAILED: moves_left_tail_cost"; exit 1; }
