#!/usr/bin/env python3
"""What the Gumbel root search (run.py self --gumbel M) plays at small simulation budgets, against PUCT.

    python tools/gumbel_effect.py --fresh [--filters 128] [--blocks 7] [--positions 64] [--m 16] [--reps 4]
    -> one JSON line, also written to --out (default profiles/gumbel_effect.json)
    python tools/gumbel_effect.py --fresh --full
    -> the same with a third column, the full Gumbel search (--gumbel-full); default --out profiles/gumbel_full_effect.json

The network is the peaked-policy stand-in of a trained one: freshly initialised weights whose policy layer is scaled
until the largest probability on the positions is >= 0.85 (bench.sharpened_copy; real weights are not obtainable here).
For --positions positions of the 1k suite (tests/golden/positions_1k.json) the yardstick is the move of an 800-simulation
PUCT search without noise at temperature 0.  For N in 16 / 32 / 64 simulations it reports how often the move played
equals that move: for the Gumbel search with M candidates, and for PUCT with the `normal` configuration's root noise
and temperature (the move sampled from the visit counts as self-play's first ply does) -- over --reps seeds each, since
both draw.  The yardstick is PUCT's own large-budget answer under the same stand-in network, not the truth: the table
says how fast each root rule converges on it, nothing about playing strength."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "chinesechess-alphazero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def search_moves(boards, net, sims, threads, seed, play, gumbel=0, noisy=False, rng=None, full=False):
    """The move each root plays: label per position."""
    import torch
    from cchess_alphazero import _native
    from cchess_alphazero._native_search import Search
    pc = types.SimpleNamespace(simulation_num_per_move=sims, search_threads=threads, c_puct=play.c_puct,
                               noise_eps=play.noise_eps if noisy else 0.0, dirichlet_alpha=play.dirichlet_alpha,
                               tau_decay_rate=play.tau_decay_rate if noisy else 0.0, virtual_loss=play.virtual_loss,
                               resign_threshold=-1.0, min_resign_turn=1000, max_game_length=100, enable_resign_rate=0.0)
    s = Search(pc, boards.shape[0], planes_dtype=_native.U8, seed=seed)
    try:
        if gumbel:
            s.set_gumbel(gumbel)
        if full:
            s.set_gumbel_full(True)
        s.set_roots(torch.from_numpy(boards).cuda())
        with torch.no_grad():
            s.run_until_idle(lambda planes: net(planes.contiguous()))
        u = rng.random(boards.shape[0]) if rng is not None else None
        return s.choose(u)
    finally:
        s.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fresh", action="store_true", help="a freshly initialised network (the only kind available)")
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--net-seed", type=int, default=0)
    ap.add_argument("--positions", type=int, default=64)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--budgets", default="16,32,64")
    ap.add_argument("--reference-sims", type=int, default=800)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--full", action="store_true", help="also the full Gumbel search (set_gumbel_full)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "gumbel_full_effect.json" if args.full else "gumbel_effect.json")
    if not args.fresh:
        ap.error("--fresh: no saved weights are available here")
    import numpy as np
    import torch
    import bench
    from cchess_alphazero import _native
    from cchess_alphazero.agent.model import CChessNet, guarded_inference_net
    from cchess_alphazero.environment.static_env import done, state_to_array
    _native.require_gpu()
    torch.cuda.set_device(0)
    play = bench.build_config(types.SimpleNamespace(config="normal", games=None, sims_per_round=None, dtype=None,
                                                    trunk=None)).play     # (the benchmark's `normal`: K = 8, as gumbel_cost.py)
    with open(os.path.join(ROOT, "tests", "golden", "positions_1k.json")) as f:
        states = [p["state"] for p in json.load(f)["positions"]]
    states = [s for s in states if not done(s)[0]]
    states = states[::max(1, len(states) // args.positions)][:args.positions]
    boards = np.stack([np.asarray(state_to_array(s), dtype=np.int8).reshape(90) for s in states])
    torch.manual_seed(args.net_seed)
    raw = CChessNet(cnn_filter_num=args.filters, res_layer_num=args.blocks).eval()
    planes = _native.rules_fused(torch.from_numpy(boards).cuda(), _native.F32)["planes"]
    sharp, scale, ref = bench.sharpened_copy(raw.cuda(), planes)
    net = guarded_inference_net(sharp.cpu().eval(), torch.float32, trunk="mfma")
    K = play.search_threads
    best = np.asarray(search_moves(boards, net, args.reference_sims, K, args.seed, play))
    out = dict(positions=len(states), m=args.m, reference_sims=args.reference_sims, search_threads=K, reps=args.reps,
               filters=args.filters, blocks=args.blocks, policy_layer_scale=scale, max_policy_probability=float(ref[0].max()),
               arith=net.arith_effective, noise_eps=play.noise_eps, tau_decay_rate=play.tau_decay_rate, budgets={})
    for n in [int(x) for x in args.budgets.split(",")]:
        hit = dict(gumbel=[], puct=[], full=[])
        for rep in range(args.reps):
            seed = args.seed + 1 + rep
            g = np.asarray(search_moves(boards, net, n, K, seed, play, gumbel=args.m))
            p = np.asarray(search_moves(boards, net, n, K, seed, play, noisy=True, rng=np.random.default_rng(seed)))
            if args.full:
                f = np.asarray(search_moves(boards, net, n, K, seed, play, gumbel=args.m, full=True))
                hit["full"].append(float((f == best).mean()))
            hit["gumbel"].append(float((g == best).mean()))
            hit["puct"].append(float((p == best).mean()))
        out["budgets"][str(n)] = dict(gumbel_same_move=float(np.mean(hit["gumbel"])), puct_same_move=float(np.mean(hit["puct"])),
                                      gumbel_by_rep=hit["gumbel"], puct_by_rep=hit["puct"])
        if args.full:
            out["budgets"][str(n)].update(full_same_move=float(np.mean(hit["full"])), full_by_rep=hit["full"])
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
