#!/usr/bin/env python3
"""Cost of the root value record (engine.record_q) on the `normal` benchmark engine, and what it records.

    python tools/q_record_cost.py [--rounds 1500] [--legs 4] [--pattern 01] [--spread-rounds 2500]
    -> one JSON line, also written to --out (default profiles/q_record_cost.json)

Cost: legs alternate the value record off / on in ONE process, each a fresh engine (same seed, the visit record on in
both, so that the difference is the value record's own: one float64 reduction per ply in k_advance and 8 bytes per
entry in the drain), driven the way the self-play worker drives it: HIP graph replays, drained every
report_every_rounds (200).  Reports expansions/s per leg and on / off.  --pattern is the legs' order, repeated (0 = off,
1 = on): 0110 cancels a drift of the box that is linear in time, which 01 books against the value record.

Spread: one more leg at a small search (--spread-sims simulations, the same network) that runs long enough for games to
END, since z is known only then: the distribution of q - z by ply, both from the mover's view, over the stored games'
items that carry a q -- count, mean, standard deviation and mean |q - z| per bucket of ten plies.  With the random
network of this tool the numbers show the record at work, not what a trained network's values look like; the choice
of --q-ratio is the user's."""
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


def _engine(record_q, play=None, games=None):
    import torch
    import bench
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.engine import SelfPlayEngine
    cfg = bench.build_config(types.SimpleNamespace(config="normal", games=games, sims_per_round=None, dtype=None,
                                                   trunk=None))
    for k, v in (play or {}).items():
        setattr(cfg.play, k, v)
    cfg.engine.record_visits = True
    cfg.engine.record_q = record_q
    torch.manual_seed(0)
    net = CChessNet.from_model_config(cfg.model)
    return SelfPlayEngine(cfg, cfg.engine.games_per_gpu, net=net, dtype=getattr(torch, cfg.engine.net_dtype), seed=20261017)


def leg(record_q, rounds, every):
    import torch
    eng = _engine(record_q)
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
        return dict(record_q=record_q, rounds=rounds, seconds=dt, expansions_per_s=(c1["expansions"] - c0["expansions"]) / dt,
                    games=len(games), plies=c1["plies"] - c0["plies"], visits_dropped=c1["visits_dropped"],
                    value_ring_device_bytes=eng.search.visit_capacity * 8 if record_q else 0)
    finally:
        eng.close()
        torch.cuda.empty_cache()


def spread(rounds, sims, games, every):
    import numpy as np
    import torch
    eng = _engine(True, play=dict(simulation_num_per_move=sims), games=games)
    try:
        eng.start(0, 0)
        eng.prewarm()
        done = []
        for r in range(1, rounds + 1):
            eng.step()
            if r % every == 0:
                done += eng.drain()
        done += eng.drain()
        c = eng.counters()
    finally:
        eng.close()
        torch.cuda.empty_cache()
    buckets = {}
    n_none = 0
    for g in done:
        for ply, it in enumerate(g["data"][1:]):
            if len(it) < 5:
                continue
            if it[4] is None:
                n_none += 1
                continue
            buckets.setdefault(ply // 10, []).append(it[4] - it[1])
    rows = []
    for b in sorted(buckets):
        d = np.asarray(buckets[b], dtype=np.float64)
        rows.append(dict(plies=f"{10 * b}-{10 * b + 9}", n=int(d.size), mean=float(d.mean()), std=float(d.std()),
                         mean_abs=float(np.abs(d).mean())))
    every_d = np.concatenate([np.asarray(v, dtype=np.float64) for v in buckets.values()]) if buckets else np.zeros(0)
    return dict(sims=sims, games_finished=len(done), rounds=rounds, items_with_q=int(every_d.size), items_without_q=n_none,
                mean_abs_q_minus_z=float(np.abs(every_d).mean()) if every_d.size else None,
                decided_games=sum(1 for g in done if g["value"] != 0), visits_dropped=c["visits_dropped"], by_ply=rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=1500)
    ap.add_argument("--legs", type=int, default=4)
    ap.add_argument("--pattern", default="01", help="order of the legs, repeated: 0 = record off, 1 = on")
    ap.add_argument("--every", type=int, default=200, help="drain cadence (rounds), the worker's report_every_rounds")
    ap.add_argument("--spread-rounds", type=int, default=2500, help="0 = skip the q - z leg")
    ap.add_argument("--spread-sims", type=int, default=64)
    ap.add_argument("--spread-games", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q_record_cost.json"))
    args = ap.parse_args()
    if not args.pattern or set(args.pattern) - set("01"):
        raise SystemExit(f"--pattern {args.pattern!r}: expected a string of 0s and 1s")
    legs = [leg(args.pattern[i % len(args.pattern)] == "1", args.rounds, args.every) for i in range(args.legs)]
    for x in legs:
        print(json.dumps(x), file=sys.stderr, flush=True)
    off = [x["expansions_per_s"] for x in legs if not x["record_q"]]
    on = [x["expansions_per_s"] for x in legs if x["record_q"]]
    out = dict(pattern=args.pattern, off_expansions_per_s=off, on_expansions_per_s=on,
               on_over_off=(sum(on) / len(on)) / (sum(off) / len(off)) if on and off else None, legs=legs)
    if args.spread_rounds:
        out["q_minus_z"] = spread(args.spread_rounds, args.spread_sims, args.spread_games, args.every)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
