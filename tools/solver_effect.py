#!/usr/bin/env python3
"""What the MCTS solver (run.py self / eval --solver) does to the move played in a position that holds a forced mate.

    python tools/solver_effect.py [--filters 32] [--blocks 2] [--threads 8] [--budgets 8,16,...,1024]
    python tools/solver_effect.py --config model_best_config.json --weights model_best_weight.h5
    -> one JSON line, also written to --out (default profiles/solver_effect.json)

For every fixture of tests/golden/solver_positions.json whose root is a forced win of at most --max-dist plies, and every
budget, a fresh search object searches the position at K = --threads without root noise, once with the solver off and once
with it on, and plays at tau = 0.  The played move MATES if the position after it is lost for its mover within d - 2 plies
-- a depth-limited minimax over the package's own rule functions, which knows nothing of the search.  Reported per
position and setting: the simulations each budget really ran, whether its move mates, the least budget whose move mates
and the least budget from which every larger one mates too (None: not within the budgets)."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "chinesechess-alphazero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def lost_within(state, depth, senv, memo):
    """+1 / -1 / 0: the mover of `state` wins / loses by force within `depth` plies (done() at the end of the line), or neither."""
    key = (state, depth)
    if key in memo:
        return memo[key]
    over, v = senv.done(state)[:2]
    if over:
        res = 1 if v > 0 else -1
    elif depth == 0:
        res = 0
    else:
        kids = [lost_within(senv.step(state, m), depth - 1, senv, memo) for m in senv.get_legal_moves(state)]
        res = 1 if any(k < 0 for k in kids) else (-1 if kids and all(k > 0 for k in kids) else 0)
    memo[key] = res
    return res


def search_all(boards, net, solver, sims, threads, seed):
    import torch
    from cchess_alphazero import _native
    from cchess_alphazero._native_search import Search
    pc = types.SimpleNamespace(simulation_num_per_move=sims, search_threads=threads, c_puct=1.5, noise_eps=0.0,
                               dirichlet_alpha=0.2, tau_decay_rate=0.0, virtual_loss=3, resign_threshold=-1.0,
                               min_resign_turn=1000, max_game_length=100, enable_resign_rate=0.0)
    s = Search(pc, boards.shape[0], planes_dtype=_native.U8, seed=seed)
    try:
        if solver:
            s.set_solver(True)
        s.set_roots(torch.from_numpy(boards).cuda())
        with torch.no_grad():
            s.run_until_idle(lambda planes: net(planes.contiguous()))
        return s.choose(None), s.root_stats()["sum_n"], s.node_proof()
    finally:
        s.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", help="model configuration JSON (default: a freshly initialised network)")
    ap.add_argument("--weights", help="model weights (the path run.py uses)")
    ap.add_argument("--filters", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--net-seed", type=int, default=0)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--budgets", default="8,16,32,64,128,256,512,1024")
    ap.add_argument("--max-dist", type=int, default=5, help="fixtures whose forced win is longer are left out (the minimax)")
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solver_effect.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from cchess_alphazero import _native
    from cchess_alphazero.agent.model import CChessModel, CChessNet, guarded_inference_net
    from cchess_alphazero.config import Config
    from cchess_alphazero.environment import static_env as senv
    from cchess_alphazero.environment.lookup_tables import ActionLabelsRed
    _native.require_gpu()
    torch.cuda.set_device(0)
    if args.config and args.weights:
        model = CChessModel(Config("mini"))
        if not model.load(args.config, args.weights):
            raise SystemExit(f"no model at {args.config} / {args.weights}")
        raw = model.model
    else:
        torch.manual_seed(args.net_seed)
        raw = CChessNet(cnn_filter_num=args.filters, res_layer_num=args.blocks)
    net = guarded_inference_net(raw.eval(), torch.float32, trunk="mfma" if raw.cfg["cnn_filter_num"] in (32, 128, 192, 256) else "library")
    with open(os.path.join(ROOT, "tests", "golden", "solver_positions.json")) as f:
        fixtures = [p for p in json.load(f)["positions"] if p["want"]["status"] == 1 and p["want"]["dist"] <= args.max_dist]
    budgets = [int(x) for x in args.budgets.split(",")]
    boards = np.stack([np.asarray(senv.state_to_array(p["state"]), dtype=np.int8).reshape(90) for p in fixtures])
    memo = {}
    out = dict(search_threads=args.threads, budgets=budgets, filters=raw.cfg["cnn_filter_num"], blocks=raw.cfg["res_layer_num"],
               net=args.weights or "fresh", positions={p["name"]: dict(dist=p["want"]["dist"]) for p in fixtures})
    for solver in (False, True):
        rows = {p["name"]: dict(ran=[], mates=[], root=[]) for p in fixtures}
        for sims in budgets:
            act, sum_n, proof = search_all(boards, net, solver, sims, args.threads, args.seed)
            for g, p in enumerate(fixtures):
                mv = ActionLabelsRed[int(act[g])]
                r = rows[p["name"]]
                r["ran"].append(int(sum_n[g]))
                r["mates"].append(lost_within(senv.step(p["state"], mv), p["want"]["dist"] - 2, senv, memo) < 0)
                r["root"].append([int(proof["status"][g]), int(proof["dist"][g])])
        for p in fixtures:
            r = rows[p["name"]]
            r["first_budget_that_mates"] = next((b for b, m in zip(budgets, r["mates"]) if m), None)
            r["mates_from_budget"] = next((b for i, b in enumerate(budgets) if all(r["mates"][i:])), None)
            out["positions"][p["name"]]["solver_on" if solver else "solver_off"] = r
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
