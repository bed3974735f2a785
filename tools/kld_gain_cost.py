#!/usr/bin/env python3
"""Cost and yield of the KLD-gain stop (engine.kld_gain, cz_search_set_kld_gain) on the `normal` benchmark engine.

    python tools/kld_gain_cost.py [--rounds 1500] [--reps 2] [--gains 1e-5,1e-4,1e-3] [--interval 100]
    -> one JSON line, also written to --out (default profiles/kld_gain_cost.json)

Legs run in ONE process, each a fresh engine (same seed, same random network), driven the way the self-play worker drives
it: HIP graph replays, drained every report_every_rounds (200).  The legs of one repetition: the rule off; the rule on with a
gain so small (1e-300) that it never fires, which prices the checks alone; then the sweep of gains.  Reported per leg:
expansions/s, plies/s, the mean simulations per ply, the share of plies the rule ended and games/hour.  The off legs run the
kernels that ran before the option existed; what the rule adds sits in k_sim_stop and k_advance_stop alone.  A random
network's visit distributions settle differently from a trained one's: the sweep says what this workload does."""
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

NEVER = 1e-300                    # a gain below which no measured value falls: the checks run, nothing is cut


def leg(gain, interval, rounds, every):
    import torch
    import bench
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.engine import SelfPlayEngine
    cfg = bench.build_config(types.SimpleNamespace(config="normal", games=None, sims_per_round=None, dtype=None,
                                                   trunk=None))
    torch.manual_seed(0)
    net = CChessNet.from_model_config(cfg.model)
    eng = SelfPlayEngine(cfg, cfg.engine.games_per_gpu, net=net, dtype=getattr(torch, cfg.engine.net_dtype), seed=20261020,
                         kld_gain=gain, kld_interval=interval)
    try:
        eng.start(0, 0)
        eng.prewarm()
        for _ in range(20):
            eng.step()
        eng.capture_graph(warmup=0)
        games = 0
        torch.cuda.synchronize()
        c0 = eng.counters()
        t0 = time.perf_counter()
        for r in range(1, rounds + 1):
            eng.step()
            if r % every == 0:
                games += len(eng.drain())
        games += len(eng.drain())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        c1 = eng.counters()
        d = {k: c1.get(k, 0) - c0.get(k, 0) for k in ("sims", "expansions", "plies", "kld_plies", "kld_sims_cut")}
        return dict(kld_gain=gain, kld_interval=interval, rounds=rounds, seconds=dt, expansions_per_s=d["expansions"] / dt,
                    plies_per_s=d["plies"] / dt, games=games, games_per_hour=games / dt * 3600.0, plies=d["plies"],
                    sims=d["sims"], sims_per_ply=d["sims"] / max(1, d["plies"]), kld_plies=d["kld_plies"],
                    kld_sims_cut=d["kld_sims_cut"], share_of_plies_cut=d["kld_plies"] / max(1, d["plies"]))
    finally:
        eng.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--gains", default="1e-5,1e-4,1e-3")
    ap.add_argument("--interval", type=int, default=100)
    ap.add_argument("--every", type=int, default=200, help="drain cadence (rounds), the worker's report_every_rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kld_gain_cost.json"))
    args = ap.parse_args()
    gains = [0.0, NEVER] + [float(x) for x in args.gains.split(",") if x]
    legs = []
    for _ in range(args.reps):
        for g in gains:
            legs.append(leg(g, args.interval, args.rounds, args.every))
            print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    by = {}
    for g in gains:
        mine = [x for x in legs if x["kld_gain"] == g]
        xs = [x["expansions_per_s"] for x in mine]
        name = "off" if g == 0.0 else ("never" if g == NEVER else f"{g:g}")
        by[name] = dict(expansions_per_s=xs, mean=sum(xs) / len(xs), spread=(max(xs) - min(xs)) / (sum(xs) / len(xs)),
                        plies_per_s=sum(x["plies_per_s"] for x in mine) / len(mine),
                        sims_per_ply=sum(x["sims_per_ply"] for x in mine) / len(mine),
                        share_of_plies_cut=sum(x["share_of_plies_cut"] for x in mine) / len(mine),
                        games_per_hour=sum(x["games_per_hour"] for x in mine) / len(mine))
    for name in by:
        by[name]["over_off"] = by[name]["mean"] / by["off"]["mean"]
        by[name]["plies_per_s_over_off"] = by[name]["plies_per_s"] / by["off"]["plies_per_s"]
    out = dict(interval=args.interval, by_gain=by, legs=legs)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
