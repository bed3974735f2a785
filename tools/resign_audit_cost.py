#!/usr/bin/env python3
"""Cost of the max-q record (engine.resign_audit, cz_search_record_maxq) on the `normal` benchmark engine with
--record-visits: expansions/s with the audit off and on.

    python tools/resign_audit_cost.py [--rounds 1500] [--reps 2]
    -> one JSON line, also written to --out (default profiles/resign_audit_cost.json)

Legs alternate off / on, --reps times over, in ONE process, each a fresh engine (same seed, same random network), driven
the way the self-play worker drives it: HIP graph replays, drained every report_every_rounds (200), every drained game fed
to a ResignAudit on the `on` legs.  What the record adds is on k_advance's side only -- one more maximum over the root's
edges, one more 8-byte store per recorded ply, 8 more bytes per entry in the drain -- and that kernel is 1-2 % of a
step: the figure to compare the difference with is the spread between the legs of one setting."""
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


def leg(on, rounds, every):
    import torch
    import bench
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.engine import SelfPlayEngine
    from cchess_alphazero.lib.resign_audit import ResignAudit
    cfg = bench.build_config(types.SimpleNamespace(config="normal", games=None, sims_per_round=None, dtype=None,
                                                   trunk=None))
    torch.manual_seed(0)
    net = CChessNet.from_model_config(cfg.model)
    eng = SelfPlayEngine(cfg, cfg.engine.games_per_gpu, net=net, dtype=getattr(torch, cfg.engine.net_dtype), seed=20261019,
                         record_visits=True, resign_audit=on)
    audit = ResignAudit(cfg.play.min_resign_turn)
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
            if r % every == 0 or r == rounds:
                for g in eng.drain():
                    games += 1
                    if on:
                        audit.add_game(g["visits"], g["value"])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        c1 = eng.counters()
        return dict(resign_audit=bool(on), rounds=rounds, seconds=dt,
                    expansions_per_s=(c1["expansions"] - c0["expansions"]) / dt, games=games,
                    plies=c1["plies"] - c0["plies"], visits_dropped=c1.get("visits_dropped", 0),
                    audited=audit.games, skipped=audit.skipped)
    finally:
        eng.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--every", type=int, default=200, help="drain cadence (rounds), the worker's report_every_rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resign_audit_cost.json"))
    args = ap.parse_args()
    legs = []
    for _ in range(args.reps):
        for on in (False, True):
            legs.append(leg(on, args.rounds, args.every))
            print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    by = {}
    for on in (False, True):
        xs = [x["expansions_per_s"] for x in legs if x["resign_audit"] == on]
        by["on" if on else "off"] = dict(expansions_per_s=xs, mean=sum(xs) / len(xs),
                                         spread=(max(xs) - min(xs)) / (sum(xs) / len(xs)))
    by["on"]["over_off"] = by["on"]["mean"] / by["off"]["mean"]
    out = dict(by_setting=by, legs=legs)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
