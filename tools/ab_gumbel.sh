#!/bin/bash
# GPU: what the Gumbel root search (cz_search_set_gumbel) costs.
#  1. the default benchmark on the parent build (variants/libczero_parent.so, selected with CZ_LIB as in
#     tools/ab_leaf_mirror.sh) and on this tree's build, alternating on one box, the option off (bench.py never switches
#     it on): the default instantiations of the simulation kernel do not hold the option's code, so the rate must not move;
#  2. expansions/s of this build with the option off and with M = 16 at the configuration's simulations
#     (tools/gumbel_cost.py).
# Stops at the first run that fails.
#   usage: [OUT=dir] bash tools/ab_gumbel.sh [REPS] [COST_ROUNDS]
#          -> $OUT/ab_gumbel.log, $OUT/gumbel_cost.json  (OUT defaults to profiles/)
set -o pipefail
out=${OUT:-profiles}
mkdir -p $out
log=$out/ab_gumbel.log
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
timeout -k 10 600 python tools/gumbel_cost.py --rounds ${2:-1500} --out $out/gumbel_cost.json 2>/dev/null | tail -1 || { echo "FAILED: gumbel_cost"; exit 1; }
