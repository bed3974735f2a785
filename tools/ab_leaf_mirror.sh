#!/bin/bash
# GPU: what the random leaf mirror (cz_search_set_leaf_mirror) costs.
#  1. the default benchmark on the parent build (variants/libczero_parent.so, selected with CZ_LIB as in
#     tools/ab_record_q.sh) and on this tree's build, alternating on one box, the mirror off (bench.py never switches it
#     on): the mirrored index of the board write and the flag test of the attach side must cost nothing at rate 0;
#  2. expansions/s of this build at rates 0 / 0.5 / 1 (tools/leaf_mirror_cost.py);
#  3. the sustained search round of tools/search_probe.py at the same three rates.
# Stops at the first run that fails.
#   usage: [OUT=dir] bash tools/ab_leaf_mirror.sh [REPS] [COST_ROUNDS] [PROBE_ROUNDS]
#          -> $OUT/ab_leaf_mirror.log, $OUT/leaf_mirror_cost.json, $OUT/leaf_mirror_probe.log  (OUT defaults to profiles/)
set -o pipefail
out=${OUT:-profiles}
mkdir -p $out
log=$out/ab_leaf_mirror.log
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
timeout -k 10 600 python tools/leaf_mirror_cost.py --rounds ${2:-1500} --out $out/leaf_mirror_cost.json 2>/dev/null | tail -1 || { echo "FAILED: leaf_mirror_cost"; exit 1; }
probe=$out/leaf_mirror_probe.log
: > $probe
for rate in 0 0.5 1; do
  timeout -k 10 300 python tools/search_probe.py --rounds ${3:-3000} --masks-only 1 --leaf-mirror $rate 2>/dev/null | tail -1 >> $probe || { echo "FAILED: search_probe $rate" >> $probe; cat $probe; exit 1; }
done
cat $probe
