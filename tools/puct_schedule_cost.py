#!/usr/bin/env python3
"""Cost of the c_puct schedule (engine.cpuct_factor / cpuct_base, cz_search_set_cpuct_schedule) and of the policy temperature
(engine.policy_temp, cz_search_set_policy_temperature) on the `normal` benchmark engine with a random network.

    python tools/puct_schedule_cost.py [--rounds 1500] [--reps 2] [--factor 3.894] [--base 38739] [--temp 1.4]
    -> one JSON line, also written to --out (default profiles/puct_schedule_cost.json)

Legs alternate off / schedule on / temperature on, --reps times over, in ONE process, each a fresh engine (same seed, same
network), driven the way the self-play worker drives it: HIP graph replays, drained every report_every_rounds (200).  Reports
per leg expansions/s.  The off legs run the kernels that ran before the options existed; the schedule legs run the SCHED
instantiations of k_sim (one wave-uniform float64 logarithm per selection); the temperature legs run the same kernels as the
off legs with another value of one float32 factor in the attach.  The games of the three settings differ from the first ply.  A
random network shows no playing effect: no strength claim is made here."""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "chinesechess-alphazero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SETTINGS = ("off", "schedule", "temperature")


def leg(setting, args):
    import torch
    import bench
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.engine import SelfPlayEngine
    cfg = bench.build_config(types.SimpleNamespace(config="normal", games=None, sims_per_round=None, dtype=None,
                                                   trunk=None))
    torch.manual_seed(0)
    net = CChessNet.from_model_config(cfg.model)
    kw = dict(schedule=dict(cpuct_factor=args.factor, cpuct_base=args.base), temperature=dict(policy_temp=args.temp)).get(setting, {})
    eng = SelfPlayEngine(cfg, cfg.engine.games_per_gpu, net=net, dtype=getattr(torch, cfg.engine.net_dtype), seed=20261021, **kw)
    try:
        assert eng.cpuct_on == (setting == "schedule") and eng.policy_temp_on == (setting == "temperature")
        eng.start(0, 0)
        eng.prewarm()
        for _ in range(20):
            eng.step()
        eng.capture_graph(warmup=0)
        games = 0
        torch.cuda.synchronize()
        c0 = eng.counters()
        t0 = time.perf_counter()
        for r in range(1, args.rounds + 1):
            eng.step()
            if r % args.every == 0:
                games += len(eng.drain())
        games += len(eng.drain())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        c1 = eng.counters()
        d = {k: c1.get(k, 0) - c0.get(k, 0) for k in ("sims", "expansions", "plies", "tree_resets", "overflow_sims")}
        return dict(setting=setting, rounds=args.rounds, seconds=dt, expansions_per_s=d["expansions"] / dt, games=games,
                    plies=d["plies"], sims=d["sims"], tree_resets=d["tree_resets"], overflow_sims=d["overflow_sims"],
                    mean_depth=(c1["sum_depth"] - c0["sum_depth"]) / max(1, d["sims"]))
    finally:
        eng.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--factor", type=float, default=3.894)
    ap.add_argument("--base", type=float, default=38739.0)
    ap.add_argument("--temp", type=float, default=1.4)
    ap.add_argument("--every", type=int, default=200, help="drain cadence (rounds), the worker's report_every_rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "puct_schedule_cost.json"))
    args = ap.parse_args()
    legs = []
    for _ in range(args.reps):
        for setting in SETTINGS:
            legs.append(leg(setting, args))
            print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    by = {}
    for name in SETTINGS:
        xs = [x["expansions_per_s"] for x in legs if x["setting"] == name]
        by[name] = dict(expansions_per_s=xs, mean=sum(xs) / len(xs), spread=(max(xs) - min(xs)) / (sum(xs) / len(xs)),
                        mean_depth=sum(x["mean_depth"] for x in legs if x["setting"] == name) / len(xs))
    for name in SETTINGS[1:]:
        by[name]["over_off"] = by[name]["mean"] / by["off"]["mean"]
    out = dict(factor=args.factor, base=args.base, temp=args.temp, by_setting=by, legs=legs)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
