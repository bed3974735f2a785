#!/usr/bin/env python3
"""Cost of the random leaf mirror (engine.leaf_mirror, cz_search_set_leaf_mirror) on the `normal` benchmark engine.

    python tools/leaf_mirror_cost.py [--rounds 1500] [--rates 0,0.5,1] [--reps 2]
    -> one JSON line, also written to --out (default profiles/leaf_mirror_cost.json)

Legs walk through the rates, --reps times over, in ONE process, each a fresh engine (same seed, same random network),
driven the way the self-play worker drives it: HIP graph replays, drained every report_every_rounds (200).  Reports
expansions/s per leg and, per rate, the mean and the ratio to rate 0.  What the mirror adds is on the tree kernels' side
only -- a Philox draw per expansion, the mirrored index of the board write, one table read per label on the attach side
-- and those kernels are 1-2 % of a step: the figure to compare it with is the spread between the legs of one rate.
The share of mirrored leaves is read from the per-slot flags (no counter exists for it).  With a random network the
games differ between the rates (an untrained network is not mirror-equivariant), so the legs do not run the same
trees: the rates are compared as workloads, not round by round."""
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


def leg(rate, rounds, every):
    import torch
    import bench
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.engine import SelfPlayEngine
    cfg = bench.build_config(types.SimpleNamespace(config="normal", games=None, sims_per_round=None, dtype=None,
                                                   trunk=None))
    torch.manual_seed(0)
    net = CChessNet.from_model_config(cfg.model)
    eng = SelfPlayEngine(cfg, cfg.engine.games_per_gpu, net=net, dtype=getattr(torch, cfg.engine.net_dtype), seed=20261019,
                         leaf_mirror=rate)
    try:
        if rate:
            eng.search.set_leaf_mirror(rate, flags=True)       # (the same rate again, now with the per-slot flags)
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
        share = float(eng.search.mirrored.float().mean()) if eng.search.mirrored is not None else 0.0
        return dict(leaf_mirror=rate, rounds=rounds, seconds=dt, expansions_per_s=(c1["expansions"] - c0["expansions"]) / dt,
                    games=games, plies=c1["plies"] - c0["plies"], mirrored_share_of_slots=share)
    finally:
        eng.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=1500)
    ap.add_argument("--rates", default="0,0.5,1")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--every", type=int, default=200, help="drain cadence (rounds), the worker's report_every_rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leaf_mirror_cost.json"))
    args = ap.parse_args()
    rates = [float(x) for x in args.rates.split(",")]
    if not rates or any(not 0.0 <= r <= 1.0 for r in rates):
        raise SystemExit(f"--rates {args.rates!r}: expected numbers in [0, 1]")
    legs = []
    for _ in range(args.reps):
        for r in rates:
            legs.append(leg(r, args.rounds, args.every))
            print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    by_rate = {}
    for r in rates:
        xs = [x["expansions_per_s"] for x in legs if x["leaf_mirror"] == r]
        by_rate[str(r)] = dict(expansions_per_s=xs, mean=sum(xs) / len(xs), spread=(max(xs) - min(xs)) / (sum(xs) / len(xs)))
    base = by_rate.get("0.0", {}).get("mean")
    if base:
        for v in by_rate.values():
            v["over_rate_0"] = v["mean"] / base
    out = dict(by_rate=by_rate, legs=legs)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
