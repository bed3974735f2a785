#!/usr/bin/env python3
"""What the random leaf mirror (run.py self / eval --leaf-mirror P) does to a search with a network that is NOT symmetric.

    python tools/leaf_mirror_effect.py --fresh [--filters 128] [--blocks 7] [--positions 64] [--sims 200]
    python tools/leaf_mirror_effect.py --config model_best_config.json --weights model_best_weight.h5
    -> one JSON line, also written to --out (default profiles/leaf_mirror_effect.json)

The rules are symmetric under the left-right mirror (file x <-> 8 - x), so an ideal search gives a position X and its
mirror image MX mirrored visit counts.  For --positions positions of the 1k suite (tests/golden/positions_1k.json, or
the lines of --book) this searches X and MX side by side in one search object -- no root noise, the hand-written
network path -- and reports the total-variation distance between the two roots' visit distributions, the second mapped
back through the label mirror M (cz_label_mirror): 0 = the search treats the two wings alike, 1 = disjoint moves.  Once
at rate 0, where the network's wing bias reaches the counts unchecked, and once at --rate (0.5): every leaf under a
fair coin.  tools/mirror_asymmetry.py measures the same bias on the network's raw outputs."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "chinesechess-alphazero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def visit_tv(st, M, n_pos):
    """st: root_stats of 2 * n_pos games, game n_pos + i the mirror image of game i -> the TV distance per position."""
    import numpy as np
    out = []
    for i in range(n_pos):
        d = np.zeros((2, len(M)), dtype=np.float64)
        for k, g in enumerate((i, n_pos + i)):
            c = int(st["counts"][g])
            mv = st["moves"][g, :c].astype(np.int64)
            n = st["n"][g, :c].astype(np.float64)
            if n.sum() > 0:
                d[k, M[mv] if k else mv] = n / n.sum()
        out.append(0.5 * float(np.abs(d[0] - d[1]).sum()))
    return out


def search_pairs(boards, net, rate, sims, threads, seed):
    import torch
    from cchess_alphazero import _native
    from cchess_alphazero._native_search import Search
    pc = types.SimpleNamespace(simulation_num_per_move=sims, search_threads=threads, c_puct=1.5, noise_eps=0.0,
                               dirichlet_alpha=0.2, tau_decay_rate=0.0, virtual_loss=3, resign_threshold=-1.0,
                               min_resign_turn=1000, max_game_length=100, enable_resign_rate=0.0)
    s = Search(pc, boards.shape[0], planes_dtype=_native.U8, seed=seed)
    try:
        if rate:
            s.set_leaf_mirror(rate)
        s.set_roots(torch.from_numpy(boards).cuda())
        with torch.no_grad():
            s.run_until_idle(lambda planes: net(planes.contiguous()))
        return s.root_stats(), s.counters()
    finally:
        s.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", help="model configuration JSON")
    ap.add_argument("--weights", help="model weights (the path run.py uses)")
    ap.add_argument("--fresh", action="store_true", help="a freshly initialised network instead of a saved one")
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--net-seed", type=int, default=0)
    ap.add_argument("--book", help="positions: one state string or FEN per line (lib/book.py) instead of the 1k suite")
    ap.add_argument("--positions", type=int, default=64)
    ap.add_argument("--sims", type=int, default=200)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--rate", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=20261019)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leaf_mirror_effect.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from cchess_alphazero import _native
    from cchess_alphazero.agent.model import CChessModel, CChessNet, guarded_inference_net
    from cchess_alphazero.config import Config
    from cchess_alphazero.environment.static_env import done, state_to_array
    _native.require_gpu()
    torch.cuda.set_device(0)
    if args.fresh:
        torch.manual_seed(args.net_seed)
        raw = CChessNet(cnn_filter_num=args.filters, res_layer_num=args.blocks)
    else:
        if not (args.config and args.weights):
            ap.error("--config and --weights, or --fresh")
        model = CChessModel(Config("mini"))
        if not model.load(args.config, args.weights):
            raise SystemExit(f"no model at {args.config} / {args.weights}")
        raw = model.model
    net = guarded_inference_net(raw.eval(), torch.float32, trunk="mfma" if raw.cfg["cnn_filter_num"] in (32, 128, 192, 256) else "library")
    if args.book:
        from cchess_alphazero.lib.book import load_book
        states = load_book(args.book)
    else:
        with open(os.path.join(ROOT, "tests", "golden", "positions_1k.json")) as f:
            states = [p["state"] for p in json.load(f)["positions"]]
    states = [s for s in states if not done(s)[0]]
    step = max(1, len(states) // args.positions)
    states = states[::step][:args.positions]
    x = np.stack([np.asarray(state_to_array(s), dtype=np.int8).reshape(90) for s in states])
    boards = np.concatenate([x, x.reshape(-1, 10, 9)[:, :, ::-1].reshape(-1, 90)]).copy()
    M = _native.label_mirror().astype(np.int64)
    out = dict(positions=len(states), sims=args.sims, search_threads=args.threads, filters=raw.cfg["cnn_filter_num"],
               blocks=raw.cfg["res_layer_num"], net="fresh" if args.fresh else args.weights, arith=net.arith_effective)
    for rate in (0.0, args.rate):
        st, c = search_pairs(boards, net, rate, args.sims, args.threads, args.seed)
        tv = visit_tv(st, M, len(states))
        out[f"rate_{rate:g}"] = dict(tv_mean=float(np.mean(tv)), tv_median=float(np.median(tv)), tv_max=float(np.max(tv)),
                                     same_best_move=int(sum(
                                         int(M[st["moves"][len(states) + i, np.argmax(st["n"][len(states) + i, :int(st["counts"][len(states) + i])])]])
                                         == int(st["moves"][i, np.argmax(st["n"][i, :int(st["counts"][i])])])
                                         for i in range(len(states)) if st["counts"][i] and st["counts"][len(states) + i])),
                                     expansions=c["expansions"])
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
