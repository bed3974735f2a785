#!/usr/bin/env python3
"""Cost of the policy surprise record (engine.record_surprise) on the `normal` benchmark engine, and what it records.

    python tools/surprise_cost.py [--rounds 1500] [--legs 4] [--pattern 0110] [--spread-rounds 2500]
    -> one JSON line, also written to --out (default profiles/surprise_cost.json)

Cost: legs alternate the surprise record off / on in ONE process, each a fresh engine (same seed, the visit record on in
both, so that the difference is the surprise record's own: three float64 reductions and one logarithm per edge per ply
in k_advance, 8 bytes per entry in the drain), driven the way the self-play worker drives it: HIP graph replays, drained
every report_every_rounds (200).  Reports expansions/s per leg and on / off.  --pattern is the legs' order, repeated (0 =
off, 1 = on): 0110 cancels a drift of the box that is linear in time.

Distribution: one more leg at a small search with a playout cap (--spread-sims simulations on a full ply,
--spread-fast-sims on a fast one, the same network) that runs long enough for games to end: the distribution of s by
ply, per bucket of ten plies, for full and for fast plies -- count, mean, median, 90th percentile, maximum -- and the
training weights --alpha would give the full plies.  With the random network of this tool the numbers show the record
at work, not what a trained network's surprise looks like."""
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


def _engine(record_surprise, play=None, games=None, **kw):
    import torch
    import bench
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.engine import SelfPlayEngine
    cfg = bench.build_config(types.SimpleNamespace(config="normal", games=games, sims_per_round=None, dtype=None,
                                                   trunk=None))
    for k, v in (play or {}).items():
        setattr(cfg.play, k, v)
    cfg.engine.record_visits = True
    cfg.engine.record_surprise = record_surprise
    torch.manual_seed(0)
    net = CChessNet.from_model_config(cfg.model)
    return SelfPlayEngine(cfg, cfg.engine.games_per_gpu, net=net, dtype=getattr(torch, cfg.engine.net_dtype), seed=20261018,
                          **kw)


def leg(record_surprise, rounds, every):
    import torch
    eng = _engine(record_surprise)
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
        return dict(record_surprise=record_surprise, rounds=rounds, seconds=dt,
                    expansions_per_s=(c1["expansions"] - c0["expansions"]) / dt, games=len(games),
                    plies=c1["plies"] - c0["plies"], visits_dropped=c1["visits_dropped"],
                    surprise_ring_device_bytes=eng.search.visit_capacity * 8 if record_surprise else 0)
    finally:
        eng.close()
        torch.cuda.empty_cache()


def _stats(x):
    import numpy as np
    d = np.asarray(x, dtype=np.float64)
    return dict(n=int(d.size), mean=float(d.mean()), median=float(np.median(d)), p90=float(np.percentile(d, 90)),
                max=float(d.max()))


def spread(rounds, sims, fast_sims, full_rate, games, every, alpha):
    import numpy as np
    import torch
    from cchess_alphazero.lib.replay_window import surprise_weights
    eng = _engine(True, play=dict(simulation_num_per_move=sims), games=games, fast_sims=fast_sims, full_rate=full_rate)
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
    buckets = {"full": {}, "fast": {}}
    n_none = 0
    s_all, tr_all, offs = [], [], [0]
    for g in done:
        for ply, it in enumerate(g["data"][1:]):
            six = len(it) >= 6
            s_all.append(it[5] if six and it[5] is not None else np.nan)
            tr_all.append(it[3] if len(it) >= 4 else 1)
            if not six:
                continue
            if it[5] is None:
                n_none += 1
                continue
            buckets["fast" if it[3] == 0 else "full"].setdefault(ply // 10, []).append(it[5])
        offs.append(len(s_all))
    by_ply = {kind: [dict(plies=f"{10 * b}-{10 * b + 9}", **_stats(v)) for b, v in sorted(d.items())]
              for kind, d in buckets.items()}
    overall = {kind: _stats([x for v in d.values() for x in v]) if d else None for kind, d in buckets.items()}
    w = surprise_weights(np.asarray(s_all, dtype=np.float32), np.asarray(tr_all, dtype=np.uint8), offs, alpha)
    tr = np.asarray(tr_all) != 0
    weights = dict(alpha=alpha, rows=int(tr.sum()), **({k: v for k, v in _stats(w[tr]).items() if k != "n"} if tr.any() else {}),
                   min=float(w[tr].min()) if tr.any() else None)
    return dict(sims=sims, fast_sims=fast_sims, full_rate=full_rate, games_finished=len(done), rounds=rounds,
                items_without_s=n_none, visits_dropped=c["visits_dropped"], overall=overall, by_ply=by_ply, weights=weights)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=1500)
    ap.add_argument("--legs", type=int, default=4)
    ap.add_argument("--pattern", default="0110", help="order of the legs, repeated: 0 = record off, 1 = on")
    ap.add_argument("--every", type=int, default=200, help="drain cadence (rounds), the worker's report_every_rounds")
    ap.add_argument("--spread-rounds", type=int, default=2500, help="0 = skip the distribution leg")
    ap.add_argument("--spread-sims", type=int, default=64)
    ap.add_argument("--spread-fast-sims", type=int, default=16)
    ap.add_argument("--spread-full-rate", type=float, default=0.25)
    ap.add_argument("--spread-games", type=int, default=1024)
    ap.add_argument("--alpha", type=float, default=0.5, help="the --surprise-weight whose weights the distribution leg reports")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surprise_cost.json"))
    args = ap.parse_args()
    if not args.pattern or set(args.pattern) - set("01"):
        raise SystemExit(f"--pattern {args.pattern!r}: expected a string of 0s and 1s")
    legs = [leg(args.pattern[i % len(args.pattern)] == "1", args.rounds, args.every) for i in range(args.legs)]
    for x in legs:
        print(json.dumps(x), file=sys.stderr, flush=True)
    off = [x["expansions_per_s"] for x in legs if not x["record_surprise"]]
    on = [x["expansions_per_s"] for x in legs if x["record_surprise"]]
    out = dict(pattern=args.pattern, off_expansions_per_s=off, on_expansions_per_s=on,
               on_over_off=(sum(on) / len(on)) / (sum(off) / len(off)) if on and off else None, legs=legs)
    if args.spread_rounds:
        out["surprise"] = spread(args.spread_rounds, args.spread_sims, args.spread_fast_sims, args.spread_full_rate,
                                 args.spread_games, args.every, args.alpha)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
