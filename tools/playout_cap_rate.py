#!/usr/bin/env python3
"""GPU: what playout cap randomization (run.py self --fast-sims N --full-rate P) does to the rates of self-play.

Two legs of the same search configuration (bench.py's sizes: `normal` = 4096 games, 800 simulations, K = 8, the 7x128
network), each a fresh engine: the cap off, then --fast-sims / --full-rate.  A leg runs --warm rounds so that the games
have left the common opening and finish their plies in different rounds, then counts over --rounds rounds:

    expansions/s, plies/s, full plies (training rows) per hour, the mean simulations actually run per ply (subtree
    reuse included), finished games, and games/hour = plies/s / (mean plies per game) * 3600 with the game length of
    the committed complete-games run (profiles/r*_games_<config>.json, bench.py games_per_hour_estimate) -- a game is
    ~10^4 rounds, none finishes inside a leg.  That length was measured WITHOUT a cap; whether games with fast plies are
    longer or shorter is not measured here.

The budgets alone say 0.25 * 800 + 0.75 * 100 = 275 simulations per ply before reuse; the tool measures what it is.

    python tools/playout_cap_rate.py [--config normal] [--fast-sims 100] [--full-rate 0.25] [--warm 600] [--rounds 1200]
    -> one JSON line per leg and the file --out (default profiles/playout_cap_rate.json)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "chinesechess-alphazero_amd"), ROOT]
import torch  # noqa: E402


def leg(cfg, games, fast_sims, full_rate, warm, rounds, mean_plies):
    from cchess_alphazero.engine import SelfPlayEngine
    eng = SelfPlayEngine(cfg, games, dtype=getattr(torch, cfg.engine.net_dtype), seed=7, fast_sims=fast_sims,
                         full_rate=full_rate)
    eng.start()
    eng.prewarm()
    for _ in range(warm):
        eng.step()
    eng.drain(1 << 16)
    torch.cuda.synchronize()
    c0, t0 = eng.counters(), time.perf_counter()
    for _ in range(rounds):
        eng.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    c1 = eng.counters()
    eng.close()
    d = {k: c1[k] - c0[k] for k in ("expansions", "plies", "sims", "games", "root_reused_sims")}
    # no device counter tells full plies from fast ones (the counter block is bench.py's); the lottery is independent of
    # the play, so over the ~10^5 plies of a leg the full plies are full_rate of all plies to within a per cent
    frac = full_rate if fast_sims else 1.0
    plies_s = d["plies"] / dt
    return {"fast_sims": fast_sims, "full_rate": full_rate if fast_sims else None, "games": games, "warm_rounds": warm,
            "rounds": rounds, "seconds": dt, "ms_per_round": dt / rounds * 1e3,
            "expansions_per_s": d["expansions"] / dt, "plies_per_s": plies_s,
            "sims_run_per_ply": d["sims"] / max(1, d["plies"]),
            "sims_reused_per_ply": d["root_reused_sims"] / max(1, d["plies"]),
            "expansions_per_ply": d["expansions"] / max(1, d["plies"]),
            "full_plies_per_hour_expected": plies_s * frac * 3600.0,
            "games_finished": d["games"],
            "games_per_hour_steady_state": plies_s / mean_plies * 3600.0 if mean_plies else None,
            "mean_plies_per_game_assumed": mean_plies,
            "tree_resets": c1["tree_resets"], "overflow_sims": c1["overflow_sims"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="normal")
    ap.add_argument("--games", type=int, default=None)
    ap.add_argument("--fast-sims", type=int, default=100)
    ap.add_argument("--full-rate", type=float, default=0.25)
    ap.add_argument("--warm", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=1200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "playout_cap_rate.json"))
    a = ap.parse_args()
    import bench
    ns = argparse.Namespace(config=a.config, games=a.games, sims_per_round=None, dtype=None, trunk=None)
    cfg = bench.build_config(ns)
    est = bench.games_per_hour_estimate(1.0, a.config) or {}
    mean_plies = est.get("mean_plies_per_game")
    out = {"config": a.config, "sims_per_move": cfg.play.simulation_num_per_move, "K": cfg.play.search_threads,
           "mean_plies_source": est.get("source"), "legs": []}
    for fs in (0, a.fast_sims):
        r = leg(cfg, cfg.engine.games_per_gpu, fs, a.full_rate, a.warm, a.rounds, mean_plies)
        out["legs"].append(r)
        print(json.dumps(r), flush=True)
    off, on = out["legs"]
    out["ratio"] = {k: on[k] / off[k] for k in ("expansions_per_s", "plies_per_s", "sims_run_per_ply") if off[k]}
    print(json.dumps({"ratio_cap_over_off": out["ratio"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
