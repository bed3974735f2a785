#!/usr/bin/env python3
"""Cost of the moves-left utility of the search (engine.moves_left_slope, cz_search_set_moves_left) on the `normal` benchmark
engine with a random network that has the moves-left output.

    python tools/moves_left_search_cost.py [--rounds 1500] [--reps 2]
    -> one JSON line, also written to --out (default profiles/moves_left_search_cost.json)

Legs alternate utility off / on, --reps times over, in ONE process, each a fresh engine (same seed, same network), driven the
way the self-play worker drives it: HIP graph replays, drained every report_every_rounds (200).  Reports per leg expansions/s
and the tree bytes per game at the end.  The off legs run the kernels that ran before the option existed (k_sim, cz_heads_tail);
the on legs run k_sim_ml, k_reserve_ml and cz_heads_tail_ml.  The two shares are measured apart: the dense tail by
tools/moves_left_tail_cost.py, the tree kernels' round by tools/search_probe.py [--moves-left-slope S].  A random network shows
no playing effect: no strength or game-length claim is made here."""
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


def leg(slope, cap, rounds, every):
    import torch
    import bench
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.engine import SelfPlayEngine
    cfg = bench.build_config(types.SimpleNamespace(config="normal", games=None, sims_per_round=None, dtype=None,
                                                   trunk=None))
    cfg.model.moves_left = True
    torch.manual_seed(0)
    net = CChessNet.from_model_config(cfg.model)
    assert net.moves_left_head
    eng = SelfPlayEngine(cfg, cfg.engine.games_per_gpu, net=net, dtype=getattr(torch, cfg.engine.net_dtype), seed=20261019,
                         moves_left_slope=slope, moves_left_cap=cap)
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
        m = eng.search.memory_info()
        d = {k: c1.get(k, 0) - c0.get(k, 0) for k in ("sims", "expansions", "plies", "stat_blocks", "chunks_taken",
                                                      "tree_resets", "overflow_sims")}
        return dict(moves_left_slope=slope, rounds=rounds, seconds=dt, expansions_per_s=d["expansions"] / dt, games=games,
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
    ap.add_argument("--slope", type=float, default=0.0027)
    ap.add_argument("--cap", type=float, default=0.0345)
    ap.add_argument("--every", type=int, default=200, help="drain cadence (rounds), the worker's report_every_rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "moves_left_search_cost.json"))
    args = ap.parse_args()
    legs = []
    for _ in range(args.reps):
        for slope in (0.0, args.slope):
            legs.append(leg(slope, args.cap, args.rounds, args.every))
            print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    by = {}
    for name, on in (("off", False), ("on", True)):
        sel = [x for x in legs if bool(x["moves_left_slope"]) == on]
        xs = [x["expansions_per_s"] for x in sel]
        by[name] = dict(expansions_per_s=xs, mean=sum(xs) / len(xs), spread=(max(xs) - min(xs)) / (sum(xs) / len(xs)),
                        tree_bytes_per_game=sum(x["tree_bytes_per_game"] for x in sel) / len(sel),
                        nodes_per_game=sum(x["nodes_per_game"] for x in sel) / len(sel))
    by["on"]["over_off"] = by["on"]["mean"] / by["off"]["mean"]
    out = dict(by_utility=by, legs=legs)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
