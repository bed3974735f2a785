#!/usr/bin/env python3
"""Cost of the root visit record (engine.record_visits) on the `normal` benchmark engine.

    python tools/visit_record_cost.py [--rounds 3000] [--legs 4]

Legs alternate recording off / on, each a fresh engine (same seed) driven the way the self-play worker drives it:
HIP graph replays, drained every report_every_rounds (200).  Prints one JSON line: expansions/s per leg, the ring's
device memory, entries and drained bytes per finished game, and the size of the finished games' play records with and
without pi."""
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


def leg(record, rounds, every):
    import torch
    import bench
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.engine import SelfPlayEngine
    from cchess_alphazero._native_search import VISIT_STRIDE
    cfg = bench.build_config(types.SimpleNamespace(config="normal", games=None, sims_per_round=None, dtype=None,
                                                   trunk=None))
    cfg.engine.record_visits = record
    G = cfg.engine.games_per_gpu
    torch.manual_seed(0)
    net = CChessNet.from_model_config(cfg.model)
    eng = SelfPlayEngine(cfg, G, net=net, dtype=getattr(torch, cfg.engine.net_dtype), seed=20260923)
    try:
        eng.start(0, 0)
        eng.prewarm()
        for _ in range(20):
            eng.step()
        eng.capture_graph(warmup=0)
        games = []
        torch.cuda.synchronize()
        c0 = eng.counters()
        t0 = time.perf_counter()
        for r in range(1, rounds + 1):
            eng.step()
            if r % every == 0:
                games += eng.drain()
        games += eng.drain()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        c1 = eng.counters()
        out = dict(record=record, rounds=rounds, seconds=dt, expansions_per_s=(c1["expansions"] - c0["expansions"]) / dt,
                   games=len(games), plies=c1["plies"] - c0["plies"])
        if record:
            full = [g for g in games if g["visits"] is not None]
            entries = sum(len(g["visits"]) for g in full)
            out.update(visits_dropped=c1["visits_dropped"], ring_entries=eng.search.visit_capacity,
                       ring_device_bytes=eng.search.visit_capacity * VISIT_STRIDE + G + 256,
                       games_with_visits=len(full), entries_per_game=entries / max(1, len(full)),
                       drained_visit_bytes_per_game=entries * VISIT_STRIDE / max(1, len(full)),
                       record_json_bytes_per_game_with_pi=sum(len(json.dumps(g["data"])) for g in full) / max(1, len(full)),
                       record_json_bytes_per_game_without_pi=sum(
                           len(json.dumps([g["data"][0]] + [it[:2] for it in g["data"][1:]])) for g in full) / max(1, len(full)))
        return out
    finally:
        eng.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3000)
    ap.add_argument("--legs", type=int, default=4)
    ap.add_argument("--every", type=int, default=200, help="drain cadence (rounds), the worker's report_every_rounds")
    args = ap.parse_args()
    legs = [leg(i % 2 == 1, args.rounds, args.every) for i in range(args.legs)]
    for x in legs:
        print(json.dumps(x), file=sys.stderr, flush=True)
    off = [x["expansions_per_s"] for x in legs if not x["record"]]
    on = [x["expansions_per_s"] for x in legs if x["record"]]
    print(json.dumps(dict(off_expansions_per_s=off, on_expansions_per_s=on,
                          on_over_off=(sum(on) / len(on)) / (sum(off) / len(off)) if on and off else None,
                          legs=legs)))


if __name__ == "__main__":
    main()
