#!/bin/bash
# GPU: what the c_puct schedule and the policy temperature cost while they are OFF, which is what the benchmark runs.
#   The default benchmark on the parent build (variants/libczero_parent.so, selected with CZ_LIB as in tools/ab_lcb.sh) and
#   on this tree's build, alternating on one box, LEGS legs each (default 5).  bench.py never switches either on, so both run
#   the same k_sim / k_advance instantiations; the attach multiplies by 1.0f where it did not multiply (EXPERIMENTS.md has the
#   kernel-by-kernel comparison).  Expectation: every branch leg inside the parent legs' own range.
# The cost of the options ON is tools/puct_schedule_cost.py's.  Stops at the first run that fails.
#   usage: [OUT=dir] bash tools/ab_puct_schedule.sh [LEGS]
#          -> $OUT/ab_puct_schedule.log  (OUT defaults to profiles/)
set -o pipefail
out=${OUT:-profiles}
mkdir -p $out
log=$out/ab_puct_schedule.log
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
