#!/usr/bin/env python3
"""GPU: the rate of a reanalysis (run.py reanalyse; SelfPlayEngine(script=...)) beside the self-play rate of the same build
and settings.

Two legs on bench.py's sizes (`normal` = 4096 games, 800 simulations, K = 8, the 7x128 network), the visit record on in both:

    self       self-play with games cut to --max-game-length full moves, so that they finish inside the leg; the leg runs
               until every slot has finished a game, its rates are counted from the first round, and its finished games
               become the records of the second leg;
    reanalyse  a fresh engine walks those games again as scripts, from the first round until every slot is idle.

Both legs search every ply the same way, so plies/s and expansions/s should agree; the reanalysis searches one position
more per game that the rules did not end (the position after the script's last move) and plays no second game in a slot.
What is measured is written down; nothing is asserted.

    python tools/reanalyse_rate.py [--config normal] [--games N] [--max-game-length 4] [--out profiles/reanalyse_rate.json]
    -> one JSON line per leg and the file --out
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "chinesechess-alphazero_amd"), ROOT]
import torch  # noqa: E402

KEYS = ("expansions", "plies", "sims", "games")


def rates(name, c, dt, rounds, extra=None):
    out = {"leg": name, "seconds": dt, "rounds": rounds, "ms_per_round": dt / max(rounds, 1) * 1e3,
           "plies_per_s": c["plies"] / dt, "expansions_per_s": c["expansions"] / dt,
           "sims_run_per_ply": c["sims"] / max(1, c["plies"]), "games": c["games"], "plies": c["plies"],
           "tree_resets": c["tree_resets"], "overflow_sims": c["overflow_sims"], "visits_dropped": c.get("visits_dropped", 0)}
    out.update(extra or {})
    return out


def run(eng, done, every=16, max_rounds=200000):
    """Rounds from start() until done(engine); returns (seconds, rounds, the drained games)."""
    games, r = [], 0
    eng.start(0)
    eng.prewarm()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while r < max_rounds:
        for _ in range(every):
            eng.step()
        r += every
        finished = done(eng)
        games += eng.drain(1 << 16)
        if finished:
            break
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r, games


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="normal")
    ap.add_argument("--games", type=int, default=None)
    ap.add_argument("--max-game-length", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reanalyse_rate.json"))
    a = ap.parse_args()
    import bench
    from cchess_alphazero._native_search import COUNTER_NAMES
    from cchess_alphazero.engine import SelfPlayEngine
    from cchess_alphazero.lib import reanalyse as ra
    cfg = bench.build_config(argparse.Namespace(config=a.config, games=a.games, sims_per_round=None, dtype=None, trunk=None))
    cfg.play.max_game_length = a.max_game_length
    G = cfg.engine.games_per_gpu
    kw = dict(dtype=getattr(torch, cfg.engine.net_dtype), seed=7, record_visits=True)
    out = {"config": a.config, "games_per_gpu": G, "sims_per_move": cfg.play.simulation_num_per_move,
           "K": cfg.play.search_threads, "max_game_length": a.max_game_length, "legs": []}
    i_games = COUNTER_NAMES.index("games")

    eng = SelfPlayEngine(cfg, G, **kw)
    dt, rounds, games = run(eng, lambda e: int(e.search.game_counters()[:, i_games].min()) >= 1)
    out["legs"].append(rates("self", eng.counters(), dt, rounds))
    eng.close()
    print(json.dumps(out["legs"][-1]), flush=True)

    records = [g["data"] for g in games if g["turns"] > 0][:G]
    scripts, kept, aside = ra.pack_scripts(records, 2 * a.max_game_length + 3)
    eng = SelfPlayEngine(cfg, G, script=scripts, **kw)
    dt, rounds, walked = run(eng, lambda e: e.search.pending() == 0)
    c = eng.counters()
    eng.close()
    out["legs"].append(rates("reanalyse", c, dt, rounds, dict(
        scripts=len(kept), set_aside=len(aside), script_plies=int(scripts.offsets[-1]), records=len(walked),
        mismatches=c["script_mismatch"], visits_lost=sum(1 for g in walked if g["visits"] is None))))
    print(json.dumps(out["legs"][-1]), flush=True)
    s, r = out["legs"]
    out["ratio_reanalyse_over_self"] = {k: r[k] / s[k] for k in ("plies_per_s", "expansions_per_s", "ms_per_round")}
    print(json.dumps({"ratio_reanalyse_over_self": out["ratio_reanalyse_over_self"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
