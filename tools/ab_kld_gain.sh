#!/bin/bash
# GPU: what the stop rules (cz_search_set_kld_gain, cz_search_set_smart_pruning) cost while they are off, and what the
# KLD-gain stop yields.
#  1. the default benchmark on the parent build (variants/libczero_parent.so, selected with CZ_LIB as in
#     tools/ab_solver.sh) and on this tree's build, alternating on one box, both rules off (bench.py never switches them
#     on): the kernels launched are the instantiations the parent launches;
#  2. expansions/s, plies/s, simulations per ply and the share of plies cut, the rule off, on without ever firing, and over a
#     sweep of gains (tools/kld_gain_cost.py).
# Stops at the first run that fails.
#   usage: [OUT=dir] bash tools/ab_kld_gain.sh [REPS] [COST_ROUNDS] [COST_REPS]
#          -> $OUT/ab_kld_gain.log, $OUT/kld_gain_cost.json  (OUT defaults to profiles/)
set -o pipefail
out=${OUT:-profiles}
mkdir -p $out
log=$out/ab_kld_gain.log
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
timeout -k 10 900 python tools/kld_gain_cost.py --rounds ${2:-1500} --reps ${3:-2} --out $out/kld_gain_cost.json 2>/dev/null | tail -1 || { echo "FAILED: kld_gain_cost"; exit 1; }
