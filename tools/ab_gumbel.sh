#!/bin/bash
# GPU: what the Gumbel root search (cz_search_set_gumbel) costs.
#  1. the default benchmark on the parent build (variants/libczero_parent.so, selected with CZ_LIB as in
#     tools/ab_leaf_mirror.sh) and on this tree's build, alternating on one box, the option off (bench.py never switches
#     it on): the default instantiations of the simulation kernel do not hold the option's code, so the rate must not move;
#  2. expansions/s of this build with the option off and with M = 16 at the configuration's simulations
#     (tools/gumbel_cost.py).
#  3. FULL=1: the same for the full Gumbel search (cz_search_set_gumbel_full) -- the log is gumbel_full_ab.log, and the
#     cost leg is M = 16 at 32 simulations with full off and on (tools/gumbel_cost.py --full).
# Stops at the first run that fails.
#   usage: [OUT=dir] [FULL=1] bash tools/ab_gumbel.sh [REPS] [COST_ROUNDS]
#          -> $OUT/ab_gumbel.log, $OUT/gumbel_cost.json  (OUT defaults to profiles/; FULL=1: gumbel_full_ab.log,
#             gumbel_full_cost.json)
set -o pipefail
out=${OUT:-profiles}
mkdir -p $out
log=$out/ab_gumbel.log
[ -n "$FULL" ] && log=$out/gumbel_full_ab.log
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
# FULL=1: mean and span (max - min) of the parent's runs and of this build's, appended to the log (ab_gumbel.log stays
# the raw lines it was)
[ -n "$FULL" ] && python - $log <<'PY' | tee -a $log
import json, sys
runs, name = {}, None
for line in open(sys.argv[1]):
    if line.startswith("run="):
        name = line[4:].split("_")[0]
    elif line.startswith("{") and name:
        runs.setdefault(name, []).append(json.loads(line)["value"])
for k, v in runs.items():
    print(f"summary {k}: runs {len(v)} mean {sum(v) / len(v):.0f} span {max(v) - min(v):.0f} expansions/s")
PY
if [ -n "$FULL" ]; then
  timeout -k 10 600 python tools/gumbel_cost.py --full --rounds ${2:-1500} --out $out/gumbel_full_cost.json 2>/dev/null | tail -1 || { echo "FAILED: gumbel_cost --full"; exit 1; }
else
  timeout -k 10 600 python tools/gumbel_cost.py --rounds ${2:-1500} --out $out/gumbel_cost.json 2>/dev/null | tail -1 || { echo "FAILED: gumbel_cost"; exit 1; }
fi
