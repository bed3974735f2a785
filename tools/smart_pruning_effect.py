#!/usr/bin/env python3
"""What the unreachable-lead stop (run.py eval --smart-pruning, cz_search_set_smart_pruning) saves in the arena, and that it
does not change a move.

    python tools/smart_pruning_effect.py [--config eval] [--games 64] [--plies 40] [--positions 256]
    -> one JSON line, also written to --out (default profiles/smart_pruning_effect.json)

1. The arena (EvaluateWorker.play_games: two random-init networks, paired games, the benchmark's `eval` configuration)
   plays --plies plies with the rule off and with it on, same seeds, in the order off, (off), on, off, on: the second leg of
   a process is slow whatever it runs (13.8 s against 10.1 s for the same 200 games, measured with the rule off; the cause
   was not looked for), so it is played and left out.  Reported per leg: seconds, plies/s, the simulations per searched
   ply and -- when the games were played to their end (--plies 0) -- games/hour.  The legs of the two settings play
   different games from the first cut on: a cut ply hands a smaller tree to the next one.  The arena advances all games
   ply by ply together, so a ply costs what its longest search costs: fewer simulations do not by themselves mean less time.
2. The moves, ply by ply from a common tree: --positions positions met by the off leg are each searched from an empty tree
   at tau = 0, once with the rule off and once with it on, same seed and K.  The rule-on search is a prefix of the other,
   batch by batch, and stops only when the leader cannot be caught: the moves must agree on every position (`disagree` is
   their number and has to be 0), and `sims_on / sims_off` is what the rule saves on a fresh tree."""
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


def arena_leg(cfg, nets, on, games, plies, K, want_trace):
    import torch
    from cchess_alphazero import _native
    from cchess_alphazero.worker.evaluator import EvaluateWorker
    cfg.engine.smart_pruning = bool(on)
    w = EvaluateWorker(cfg, evaluators=tuple(nets), dtype=_native.U8, seed=20261020)
    import numpy as np
    rng = np.random.default_rng(7)                             # the same draws in both legs
    draws = {}

    def u_fn(idx, ply):
        return draws.setdefault((int(idx), int(ply)), float(rng.random()))
    stats, trace = {}, ({} if want_trace else None)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    w.play_games(games, u_fn=u_fn, stats=stats, trace=trace, sims_per_round=K, stop_after_plies=plies or None)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    searched = sum(len(v) for v in trace.values()) if trace is not None else None
    res = dict(smart_pruning=bool(on), seconds=dt, plies=stats["plies"], plies_per_s=stats["plies"] / dt, sims=stats["sims"],
                searched_plies=searched, sims_per_searched_ply=stats["sims"] / searched if searched else None,
                games_per_hour=(games / dt * 3600.0) if not plies else None)
    return res, trace


def search_all(boards, net, on, sims, K, seed):
    import torch
    from cchess_alphazero import _native
    from cchess_alphazero._native_search import Search
    pc = types.SimpleNamespace(simulation_num_per_move=sims, search_threads=K, c_puct=1.5, noise_eps=0.0,
                               dirichlet_alpha=0.2, tau_decay_rate=0.0, virtual_loss=3, resign_threshold=-1.0,
                               min_resign_turn=1000, max_game_length=100, enable_resign_rate=0.0)
    s = Search(pc, boards.shape[0], planes_dtype=_native.U8, seed=seed)
    try:
        if on:
            s.set_smart_pruning(True)
        s.set_roots(torch.from_numpy(boards).cuda())
        with torch.no_grad():
            s.run_until_idle(lambda planes: net(planes.contiguous()))
        c = s.counters()
        return s.choose(None), c["sims"], c.get("lead_plies", 0)
    finally:
        s.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="eval", help="bench.py configuration of the arena")
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--plies", type=int, default=40, help="plies each arena leg plays (0 = the games to their end)")
    ap.add_argument("--positions", type=int, default=256)
    ap.add_argument("--threads", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smart_pruning_effect.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from cchess_alphazero.agent.model import CChessNet, guarded_inference_net
    from cchess_alphazero.environment import static_env as senv
    cfg = bench.build_config(types.SimpleNamespace(config=args.config, games=args.games, sims_per_round=None, dtype=None,
                                                   trunk=None))
    cfg.opts.evaluate = False
    dtype = getattr(torch, cfg.engine.net_dtype)
    nets = []
    for seed in (0, 1):
        torch.manual_seed(seed)
        nets.append(guarded_inference_net(CChessNet.from_model_config(cfg.model), dtype, trunk=cfg.engine.net_trunk,
                                          arith=os.environ.get("CZ_TOWER_ARITH") or cfg.engine.net_arith))
    legs, trace = [], None
    for i, rule in enumerate((False, False, True, False, True)):
        res, tr = arena_leg(cfg, nets, rule, args.games, args.plies, args.threads, True)
        print(json.dumps(res), file=sys.stderr, flush=True)
        if i == 0:
            trace = tr
        if i != 1:                                             # (the second leg of a process: left out, see above)
            legs.append(res)
    off, on = [x for x in legs if not x["smart_pruning"]], [x for x in legs if x["smart_pruning"]]
    # the positions the off leg met, without their bans (a fresh search of the position alone)
    states = []
    for rows in trace.values():
        states += [r["state"] for r in rows if not r["no_act"] and not r["inc"]]
    states = sorted(set(states))[:args.positions]
    boards = np.stack([np.asarray(senv.state_to_array(s), dtype=np.int8).reshape(90) for s in states])
    sims = cfg.play.simulation_num_per_move
    agree = dict(positions=len(states), sims_budget=sims, sims_off=0, sims_on=0, plies_cut=0, disagree=0)
    for at in range(0, len(states), 64):
        b = boards[at:at + 64]
        a0, s0, _ = search_all(b, nets[0], False, sims, args.threads, 11)
        a1, s1, cut = search_all(b, nets[0], True, sims, args.threads, 11)
        agree["sims_off"] += int(s0)
        agree["sims_on"] += int(s1)
        agree["plies_cut"] += int(cut)
        agree["disagree"] += int((np.asarray(a0) != np.asarray(a1)).sum())
    agree["sims_on_over_off"] = agree["sims_on"] / max(1, agree["sims_off"])
    out = dict(config=args.config, games=args.games, plies=args.plies, search_threads=args.threads, arena_off=off, arena_on=on,
               fresh_tree_moves=agree)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if agree["disagree"]:
        raise SystemExit(f"{agree['disagree']} moves differ between the rule off and on")


if __name__ == "__main__":
    main()
