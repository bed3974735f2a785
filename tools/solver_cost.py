#!/usr/bin/env python3
"""Cost and yield of the MCTS solver (engine.solver, cz_search_set_solver) on the `normal` benchmark engine.

    python tools/solver_cost.py [--rounds 1500] [--reps 2]
    -> one JSON line, also written to --out (default profiles/solver_cost.json)

Legs alternate solver off / on, --reps times over, in ONE process, each a fresh engine (same seed, same random network),
driven the way the self-play worker drives it: HIP graph replays, drained every report_every_rounds (200).  Reports per leg
expansions/s and, with the solver on, what it found: the share of simulations that ended on a proven node (proven_sims /
sims), the nodes proven per finished game (proofs / games) and the plies a decided root cut short (decided_plies / plies).
The off legs run the kernels that ran before the option existed; what the solver adds sits in the SOLVE instantiations of
k_sim and k_advance alone.  A random network meets few king captures in `rounds` rounds of opening play: the yield figures
say what this workload holds, not what a trained network's endgames do -- tools/solver_effect.py is the measurement of the
effect, on positions that have one."""
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


def leg(solver, rounds, every):
    import torch
    import bench
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.engine import SelfPlayEngine
    cfg = bench.build_config(types.SimpleNamespace(config="normal", games=None, sims_per_round=None, dtype=None,
                                                   trunk=None))
    torch.manual_seed(0)
    net = CChessNet.from_model_config(cfg.model)
    eng = SelfPlayEngine(cfg, cfg.engine.games_per_gpu, net=net, dtype=getattr(torch, cfg.engine.net_dtype), seed=20261019,
                         solver=solver)
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
        d = {k: c1.get(k, 0) - c0.get(k, 0) for k in ("sims", "expansions", "plies", "terminal_sims", "proven_sims", "proofs",
                                                      "decided_plies")}
        return dict(solver=bool(solver), rounds=rounds, seconds=dt, expansions_per_s=d["expansions"] / dt, games=games,
                    plies=d["plies"], sims=d["sims"], terminal_sims=d["terminal_sims"], proven_sims=d["proven_sims"],
                    proofs=d["proofs"], decided_plies=d["decided_plies"],
                    proven_share=d["proven_sims"] / max(1, d["sims"]), proofs_per_game=d["proofs"] / max(1, games),
                    decided_share_of_plies=d["decided_plies"] / max(1, d["plies"]))
    finally:
        eng.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--every", type=int, default=200, help="drain cadence (rounds), the worker's report_every_rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solver_cost.json"))
    args = ap.parse_args()
    legs = []
    for _ in range(args.reps):
        for solver in (False, True):
            legs.append(leg(solver, args.rounds, args.every))
            print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    by = {}
    for solver in (False, True):
        xs = [x["expansions_per_s"] for x in legs if x["solver"] == solver]
        by["on" if solver else "off"] = dict(expansions_per_s=xs, mean=sum(xs) / len(xs),
                                             spread=(max(xs) - min(xs)) / (sum(xs) / len(xs)))
    by["on"]["over_off"] = by["on"]["mean"] / by["off"]["mean"]
    out = dict(by_solver=by, legs=legs)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
