#!/usr/bin/env python3
"""GPU: what forced playouts and policy target pruning (run.py self --forced-playouts K --record-visits) do to self-play.

Two legs of the same search configuration (bench.py's sizes: `normal` = 4096 games, 800 simulations, K = 8, the 7x128
network), each a fresh engine with the visit record on: k = 0, then k = --k.  A leg runs --warm rounds so that the games
have left the common opening, then counts over --rounds rounds:

    expansions/s and plies/s; from the visit entries written in that window (resignation plies excluded, as in the
    records): the share of root visits that pruning removed, sum(raw_total - sum(pruned)) / sum(raw_total), and the mean
    entropy (nats) of the policy targets count / sum(counts) as each leg RECORDS them: raw counts in the k = 0 leg,
    pruned counts in the k leg.  The raw counts of a pruned ply are not recorded (only their total), so "raw against
    pruned" compares two legs that play different games.

Nothing here says whether a network trained on the pruned targets plays better.

    python tools/forced_playouts_rate.py [--config normal] [--k 2] [--warm 600] [--rounds 1200]
    -> one JSON line per leg and the file --out (default profiles/forced_playouts_rate.json)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "chinesechess-alphazero_amd"), ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402


def entropy(counts):
    c = counts[counts > 0].astype(np.float64)
    p = c / c.sum()
    return float(-(p * np.log(p)).sum())


def leg(cfg, games, k, warm, rounds):
    from cchess_alphazero.engine import SelfPlayEngine
    eng = SelfPlayEngine(cfg, games, dtype=getattr(torch, cfg.engine.net_dtype), seed=7, record_visits=True,
                         forced_playouts=k)
    s = eng.search
    eng.start()
    eng.prewarm()
    for _ in range(warm):
        eng.step()
    eng.drain(1 << 16)
    warm_plies = {gid: len(es) for gid, es in s.waiting_visits().items()}      # entries of the warm-up
    torch.cuda.synchronize()
    c0, t0 = eng.counters(), time.perf_counter()
    for _ in range(rounds):
        eng.step()                          # (the engine fetches the visit ring as it goes)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    c1 = eng.counters()
    entries = [e for gid, es in s.waiting_visits().items() for e in es[warm_plies.get(gid, 0):]]
    eng.close()
    entries = [e for e in entries if not e.resign and int(e.n[~e.banned].sum()) > 0]
    d = {key: c1[key] - c0[key] for key in ("expansions", "plies", "sims")}
    raw = sum(e.raw_total for e in entries if e.pruned)
    kept = sum(int(e.n[~e.banned].sum()) for e in entries if e.pruned)
    return {"k": k, "games": games, "warm_rounds": warm, "rounds": rounds, "seconds": dt,
            "ms_per_round": dt / rounds * 1e3, "expansions_per_s": d["expansions"] / dt, "plies_per_s": d["plies"] / dt,
            "sims_run_per_ply": d["sims"] / max(1, d["plies"]), "entries": len(entries),
            "pruned_entries": sum(e.pruned for e in entries), "raw_root_visits": raw, "pruned_root_visits": raw - kept,
            "pruned_share": (raw - kept) / raw if raw else 0.0,
            "mean_target_entropy_nats": float(np.mean([entropy(e.n[~e.banned]) for e in entries])) if entries else None,
            "mean_target_edges": float(np.mean([(e.n[~e.banned] > 0).sum() for e in entries])) if entries else None,
            "visits_dropped": c1.get("visits_dropped", 0), "tree_resets": c1["tree_resets"],
            "overflow_sims": c1["overflow_sims"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="normal")
    ap.add_argument("--games", type=int, default=None)
    ap.add_argument("--k", type=float, default=2.0)
    ap.add_argument("--warm", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=1200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forced_playouts_rate.json"))
    a = ap.parse_args()
    import bench
    ns = argparse.Namespace(config=a.config, games=a.games, sims_per_round=None, dtype=None, trunk=None)
    cfg = bench.build_config(ns)
    out = {"config": a.config, "sims_per_move": cfg.play.simulation_num_per_move, "K": cfg.play.search_threads,
           "noise_eps": cfg.play.noise_eps, "legs": []}
    for k in (0.0, a.k):
        r = leg(cfg, cfg.engine.games_per_gpu, k, a.warm, a.rounds)
        out["legs"].append(r)
        print(json.dumps(r), flush=True)
    off, on = out["legs"]
    out["ratio"] = {key: on[key] / off[key] for key in ("expansions_per_s", "plies_per_s") if off[key]}
    print(json.dumps({"ratio_forced_over_off": out["ratio"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
