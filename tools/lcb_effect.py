#!/usr/bin/env python3
"""How often the lower-confidence-bound move choice (run.py self / eval --lcb Z, cz_search_set_lcb) plays another move than
the most visited one, in the arena's setting with random networks.

    python tools/lcb_effect.py [--config eval] [--games 64] [--plies 24] [--positions 256] [--z 2] [--min-visits 0.15]
    -> one JSON line, also written to --out (default profiles/lcb_effect.json)

1. The arena (EvaluateWorker.play_games: two random-init networks, paired games, the benchmark's `eval` configuration) plays
   --plies plies with the option off and with it on, same seeds: seconds and plies/s of each leg.  The games differ from the
   first ply on which the rule picks another move.
2. --positions positions met by the off leg, without their bans, are each searched from an empty tree at tau = 0 with the
   option on, the configuration's simulations and lock-step batch: `differs` is the share of them on which choose() is not
   the most visited root move, `played_visit_share` the played move's mean share of the root's visits (`most_visit_share`:
   the most visited move's), `eligible_edges` the mean number of eligible edges.
A random network's values carry no information about the position, so this shows how often the rule acts, not whether it
helps: no strength claim is made here."""
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


def arena_leg(cfg, nets, z, ratio, games, plies, K, want_trace):
    import numpy as np
    import torch
    from cchess_alphazero import _native
    from cchess_alphazero.worker.evaluator import EvaluateWorker
    cfg.engine.lcb, cfg.engine.lcb_min_visits = float(z), float(ratio)
    w = EvaluateWorker(cfg, evaluators=tuple(nets), dtype=_native.U8, seed=20261021)
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
    return dict(lcb=float(z), seconds=dt, plies=stats["plies"], plies_per_s=stats["plies"] / dt, sims=stats["sims"]), trace


def search_all(boards, net, z, ratio, sims, K, seed):
    import numpy as np
    import torch
    from cchess_alphazero import _native
    from cchess_alphazero._native_search import Search
    pc = types.SimpleNamespace(simulation_num_per_move=sims, search_threads=K, c_puct=1.5, noise_eps=0.0,
                               dirichlet_alpha=0.2, tau_decay_rate=0.0, virtual_loss=3, resign_threshold=-1.0,
                               min_resign_turn=1000, max_game_length=100, enable_resign_rate=0.0)
    s = Search(pc, boards.shape[0], planes_dtype=_native.U8, seed=seed)
    try:
        s.set_lcb(z, ratio)
        s.set_roots(torch.from_numpy(boards).cuda())
        with torch.no_grad():
            s.run_until_idle(lambda planes: net(planes.contiguous()))
        st, chosen = s.root_stats(), s.choose(None)
        lcb, _ = s.root_lcb()
        out = []
        for g in range(boards.shape[0]):
            nm = int(st["counts"][g])
            n, mv = st["n"][g, :nm], st["moves"][g, :nm]
            if nm == 0 or n.sum() <= 0 or chosen[g] < 0:
                continue
            top = int(n.max())
            most = int(mv[n == top].min())                       # the most visited move, the lowest label on a tie
            j = int(np.nonzero(mv == chosen[g])[0][0])
            out.append(dict(differs=int(chosen[g]) != most, played_share=float(n[j]) / float(n.sum()),
                            most_share=float(top) / float(n.sum()), eligible=int((~np.isnan(lcb[g, :nm])).sum())))
        return out
    finally:
        s.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="eval", help="bench.py configuration of the arena")
    ap.add_argument("--games", type=int, default=64)
    ap.add_argument("--plies", type=int, default=24, help="plies each arena leg plays (0 = the games to their end)")
    ap.add_argument("--positions", type=int, default=256)
    ap.add_argument("--threads", type=int, default=32)
    ap.add_argument("--z", type=float, default=2.0)
    ap.add_argument("--min-visits", type=float, default=0.15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lcb_effect.json"))
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
    off, trace = arena_leg(cfg, nets, 0.0, args.min_visits, args.games, args.plies, args.threads, True)
    print(json.dumps(off), file=sys.stderr, flush=True)
    on, _ = arena_leg(cfg, nets, args.z, args.min_visits, args.games, args.plies, args.threads, False)
    print(json.dumps(on), file=sys.stderr, flush=True)
    states = []
    for rows in trace.values():
        states += [r["state"] for r in rows if not r["no_act"] and not r["inc"]]
    states = sorted(set(states))[:args.positions]
    boards = np.stack([np.asarray(senv.state_to_array(s), dtype=np.int8).reshape(90) for s in states])
    sims = cfg.play.simulation_num_per_move
    rows = []
    for at in range(0, len(states), 64):
        rows += search_all(boards[at:at + 64], nets[0], args.z, args.min_visits, sims, args.threads, 11)
    mean = lambda k: sum(float(r[k]) for r in rows) / max(1, len(rows))
    out = dict(config=args.config, games=args.games, plies=args.plies, search_threads=args.threads, z=args.z,
               min_visits=args.min_visits, sims=sims, arena_off=off, arena_on=on,
               fresh_tree=dict(positions=len(rows), differs=mean("differs"), played_visit_share=mean("played_share"),
                               most_visit_share=mean("most_share"), eligible_edges=mean("eligible")))
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
