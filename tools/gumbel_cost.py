#!/usr/bin/env python3
"""Cost of the Gumbel root search (engine.gumbel, cz_search_set_gumbel) on the `normal` benchmark engine.

    python tools/gumbel_cost.py [--rounds 1500] [--ms 0,16] [--reps 2]
    -> one JSON line, also written to --out (default profiles/gumbel_cost.json)
    python tools/gumbel_cost.py --full [--sims 32] [--ms 16]
    -> the full Gumbel search (engine.gumbel_full, cz_search_set_gumbel_full): every M > 0 runs with full off and on,
       alternating, at --sims simulations per move; default --out profiles/gumbel_full_cost.json

Legs walk through the candidate counts M (0 = off), --reps times over, in ONE process, each a fresh engine (same seed,
same random network) at the configuration's simulations per move, driven the way the self-play worker drives it: HIP
graph replays, drained every report_every_rounds (200).  Every leg records visits -- the option needs the visit record,
so the off leg carries it too and the legs differ in the root rule alone.  Reports expansions/s per leg and, per M, the
mean and the ratio to M = 0.  What the option adds is on the tree kernels' side only: 128 Philox draws and logarithms
per ply, and at the root a float64 logarithm per eligible edge instead of the PUCT term.  The games differ between the
legs (another root rule plays other moves), so the legs are compared as workloads, not round by round; the figure to
compare a ratio with is the spread between the legs of one M."""
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


def leg(m, rounds, every, full=False, sims=None):
    import torch
    import bench
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.engine import SelfPlayEngine
    cfg = bench.build_config(types.SimpleNamespace(config="normal", games=None, sims_per_round=None, dtype=None,
                                                   trunk=None))
    if sims:
        cfg.play.simulation_num_per_move = sims
    torch.manual_seed(0)
    net = CChessNet.from_model_config(cfg.model)
    eng = SelfPlayEngine(cfg, cfg.engine.games_per_gpu, net=net, dtype=getattr(torch, cfg.engine.net_dtype), seed=20261019,
                         record_visits=True, gumbel=m, gumbel_full=full)
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
        return dict(gumbel=m, full=bool(full), sims=cfg.play.simulation_num_per_move, rounds=rounds, seconds=dt,
                    expansions_per_s=(c1["expansions"] - c0["expansions"]) / dt, games=games, plies=c1["plies"] - c0["plies"],
                    visits_dropped=c1.get("visits_dropped", 0))
    finally:
        eng.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=1500)
    ap.add_argument("--ms", default="0,16")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--every", type=int, default=200, help="drain cadence (rounds), the worker's report_every_rounds")
    ap.add_argument("--full", action="store_true", help="the full Gumbel search: every M > 0 with full off and on")
    ap.add_argument("--sims", type=int, default=None, help="simulations per move (default: the configuration's; --full: 32)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.full and args.ms == "0,16":
        args.ms = "16"
    if args.full and args.sims is None:
        args.sims = 32
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "gumbel_full_cost.json" if args.full else "gumbel_cost.json")
    ms = [int(x) for x in args.ms.split(",")]
    if not ms or any(not 0 <= m <= 128 for m in ms):
        raise SystemExit(f"--ms {args.ms!r}: expected integers in 0 .. 128")
    legs = []
    for _ in range(args.reps):
        for m in ms:
            for full in ((False, True) if args.full and m > 0 else (False,)):
                legs.append(leg(m, args.rounds, args.every, full, args.sims))
                print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    by_m = {}
    for m in ms:
        for full in (False, True):
            xs = [x["expansions_per_s"] for x in legs if x["gumbel"] == m and x["full"] == full]
            if xs:
                by_m[f"{m}+full" if full else str(m)] = dict(expansions_per_s=xs, mean=sum(xs) / len(xs),
                                                             spread=(max(xs) - min(xs)) / (sum(xs) / len(xs)))
    base = by_m.get("0", {}).get("mean")
    if base:
        for v in by_m.values():
            v["over_off"] = v["mean"] / base
    for m in ms:                                                # the full search against the root-only search of the same M
        if f"{m}+full" in by_m:
            by_m[f"{m}+full"]["over_root_only"] = by_m[f"{m}+full"]["mean"] / by_m[str(m)]["mean"]
    out = dict(by_m=by_m, legs=legs)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
