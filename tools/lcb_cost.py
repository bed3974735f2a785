#!/usr/bin/env python3
"""Cost of the lower-confidence-bound move choice (engine.lcb, cz_search_set_lcb) on the `normal` benchmark engine with a random
network.

    python tools/lcb_cost.py [--rounds 1500] [--reps 2] [--z 2]
    -> one JSON line, also written to --out (default profiles/lcb_cost.json)

Legs alternate option off / on, --reps times over, in ONE process, each a fresh engine (same seed, same network), driven the way
the self-play worker drives it: HIP graph replays, drained every report_every_rounds (200).  Reports per leg expansions/s and
the tree bytes per game at the end.  The off legs run the kernels that ran before the option existed (k_sim, k_advance); the on
legs run k_sim_var, k_advance_lcb and k_reserve_ml: one more 16-byte load and store per level of a backup, statistics blocks of
twice the size.  The tree kernels' round alone is tools/search_probe.py --lcb 2's.  The games of the two settings differ from the
first tau = 0 ply on which the rule picks another move.  A random network shows no playing effect: no strength claim is made
here."""
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


def leg(z, rounds, every):
    import torch
    import bench
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.engine import SelfPlayEngine
    cfg = bench.build_config(types.SimpleNamespace(config="normal", games=None, sims_per_round=None, dtype=None,
                                                   trunk=None))
    torch.manual_seed(0)
    net = CChessNet.from_model_config(cfg.model)
    eng = SelfPlayEngine(cfg, cfg.engine.games_per_gpu, net=net, dtype=getattr(torch, cfg.engine.net_dtype), seed=20261021,
                         lcb=z)
    try:
        assert eng.lcb_on == (z > 0.0)
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
        m = eng.search.memory_info()
        d = {k: c1.get(k, 0) - c0.get(k, 0) for k in ("sims", "expansions", "plies", "stat_blocks", "chunks_taken",
                                                      "tree_resets", "overflow_sims")}
        return dict(lcb=z, rounds=rounds, seconds=dt, expansions_per_s=d["expansions"] / dt, games=games,
                    plies=d["plies"], sims=d["sims"], stat_blocks=d["stat_blocks"], chunks_taken=d["chunks_taken"],
                    tree_resets=d["tree_resets"], overflow_sims=d["overflow_sims"],
                    mean_depth=(c1["sum_depth"] - c0["sum_depth"]) / max(1, d["sims"]),
                    tree_bytes_per_game=m["tree_bytes"] / eng.search.G, nodes_per_game=m["nodes"] / eng.search.G)
    finally:
        eng.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--z", type=float, default=2.0)
    ap.add_argument("--every", type=int, default=200, help="drain cadence (rounds), the worker's report_every_rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lcb_cost.json"))
    args = ap.parse_args()
    legs = []
    for _ in range(args.reps):
        for z in (0.0, args.z):
            legs.append(leg(z, args.rounds, args.every))
            print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    by = {}
    for name, sel in (("off", [x for x in legs if not x["lcb"]]), ("on", [x for x in legs if x["lcb"]])):
        xs = [x["expansions_per_s"] for x in sel]
        by[name] = dict(expansions_per_s=xs, mean=sum(xs) / len(xs), spread=(max(xs) - min(xs)) / (sum(xs) / len(xs)),
                        tree_bytes_per_game=sum(x["tree_bytes_per_game"] for x in sel) / len(sel),
                        nodes_per_game=sum(x["nodes_per_game"] for x in sel) / len(sel))
    by["on"]["over_off"] = by["on"]["mean"] / by["off"]["mean"]
    by["on"]["tree_bytes_over_off"] = by["on"]["tree_bytes_per_game"] / by["off"]["tree_bytes_per_game"]
    out = dict(z=args.z, by_setting=by, legs=legs)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
