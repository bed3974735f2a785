#!/bin/bash
# GPU: what the MCTS solver (cz_search_set_solver) costs.
#  1. the default benchmark on the parent build (variants/libczero_parent.so, selected with CZ_LIB as in
#     tools/ab_leaf_mirror.sh) and on this tree's build, alternating on one box, the solver off (bench.py never switches
#     it on): the kernels launched are the instantiations the parent launches, plus the mark strip of the descent;
#  2. expansions/s of this build with the solver off and on, and what the solver found (tools/solver_cost.py).
# Stops at the first run that fails.
#   usage: [OUT=dir] bash tools/ab_solver.sh [REPS] [COST_ROUNDS]
#          -> $OUT/ab_solver.log, $OUT/solver_cost.json  (OUT defaults to profiles/)
set -o pipefail
out=${OUT:-profiles}
mkdir -p $out
log=$out/ab_solver.log
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
timeout -k 10 600 python tools/solver_cost.py --rounds ${2:-1500} --out $out/solver_cost.json 2>/dev/null | tail -1 || { echo "FAILED: solver_cost"; exit 1; }
