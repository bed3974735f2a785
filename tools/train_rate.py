#!/usr/bin/env python3
"""Trainer throughput (run.py opt, worker/optimize.py) on one device.

    python tools/train_rate.py [--games 200] [--steps 20] [--warmup 5] [--batch 512] [--mirror] [--repeats 1]
                               [--policy-mask legal]

Reports, as one JSON line:
  - the window fill rate in positions/s: ReplayWindow.add_games (cz_replay_games, sparse visit targets) and
    record_decoder.expand_records(targets="visits") (cz_step per ply, dense targets) on the same records (random legal games
    from the oracle with synthetic visit counts);
  - one training step (batch 512) on the 7x256 `normal` model and on the benchmark's 7x128 model, split into gather
    (cz_gather_planes), forward + backward (torch fp32 autograd), loss (cz_policy_value_loss) and optimiser (SGD with
    momentum), timed with device events after warm-up (median over the timed steps, milliseconds).
  - with --mirror: the same steps once more with random per-row mirror flags (run.py opt --augment mirror:
    cz_gather_planes_m / cz_policy_value_loss_m), as `step_ms_<model>_mirror` beside the unflagged figures of the same
    call; --repeats N alternates the two variants N times (`..._repeats`: every repeat's medians).
  - with --policy-mask legal: unmasked and masked steps (run.py opt --policy-mask legal: cz_policy_value_loss_l, the mask
    generated in the loss kernel) of the same build, alternated, at least two legs each: `policy_mask_<model>` holds every
    leg's loss launch time and whole step time for both, and the spread between the unmasked legs.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "chinesechess-alphazero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def random_games(seed, n_games, max_plies=100):
    from oracle import xq_oracle as xo
    rng = np.random.default_rng(seed)
    games = []
    for _ in range(n_games):
        state, data = xo.INIT_STATE, [xo.INIT_STATE]
        for ply in range(max_plies):
            if xo.done(state)[0]:
                break
            mv = xo.get_legal_moves(state)
            m = mv[int(rng.integers(len(mv)))]
            k = int(rng.integers(1, len(mv) + 1))
            pi = [[str(a), int(c)] for a, c in zip(rng.choice(mv, size=k, replace=False), rng.integers(1, 100, size=k))]
            data.append([m, 1 if ply % 2 == 0 else -1, pi])
            state = xo.step(state, m)
        games.append(data)
    return games


def fill_rates(games, repeats=3):
    import torch
    from cchess_alphazero.lib.record_decoder import expand_records
    from cchess_alphazero.lib.replay_window import ReplayWindow
    out = {}
    for name, fn in (("replay_window", lambda: ReplayWindow(10 ** 7).add_games(games)),
                     ("expand_records", lambda: expand_records(games, targets="visits"))):
        fn()
        torch.cuda.synchronize()
        best = None
        for _ in range(repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        out[name] = best
    n = sum(len(g) - 1 for g in games)
    return {"positions": n, **{f"{k}_positions_per_s": round(n / v) for k, v in out.items()}}


def step_times(window, filters, blocks, batch, warmup, steps, targets="visits", mirror=False, legal_mask=False):
    import torch
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.worker.optimize import l2_parameters
    torch.manual_seed(0)
    net = CChessNet(cnn_filter_num=filters, res_layer_num=blocks).cuda().train()
    opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9)
    l2 = l2_parameters(net)
    rng = np.random.default_rng(0)
    phases = {"gather": [], "forward_backward": [], "loss": [], "optimiser": [], "total": []}
    for s in range(warmup + steps):
        idx = torch.from_numpy(rng.integers(0, len(window), size=batch).astype(np.int32)).cuda()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        flags = torch.from_numpy(rng.integers(0, 2, size=batch, dtype=np.uint8)).cuda() if mirror else None
        ev[0].record()
        x = window.planes(idx, mirror=flags) if mirror else window.planes(idx)
        ev[1].record()
        logits, v = net(x, logits=True)
        ev[2].record()
        if legal_mask:      # what a training step of --policy-mask legal asks for: the mask and off_mask, no diagnostics
            total, _, _ = window.loss(logits, v, idx, targets, mirror=flags, legal_mask=True, mask_stats=dict(off_mask=None))
        else:
            total, _, _ = window.loss(logits, v, idx, targets, mirror=flags) if mirror else window.loss(logits, v, idx, targets)
        ev[3].record()
        opt.zero_grad(set_to_none=True)
        (total + 1e-4 * sum((w * w).sum() for w in l2)).backward()
        ev[4].record()
        opt.step()
        ev[5].record()
        torch.cuda.synchronize()
        if s < warmup:
            continue
        t = [ev[i].elapsed_time(ev[i + 1]) for i in range(5)]
        phases["gather"].append(t[0])
        phases["forward_backward"].append(t[1] + t[3])
        phases["loss"].append(t[2])
        phases["optimiser"].append(t[4])
        phases["total"].append(ev[0].elapsed_time(ev[5]))
    med = {k: round(float(np.median(v)), 4) for k, v in phases.items()}
    med["positions_per_s"] = round(batch / (med["total"] / 1e3))
    return med


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--games", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--mirror", action="store_true", help="also time the steps with random per-row mirror flags")
    ap.add_argument("--repeats", type=int, default=1, help="repeats of each variant (alternating with --mirror)")
    ap.add_argument("--policy-mask", choices=["none", "legal"], default="none",
                    help="legal: also time the steps with the loss over the legal moves, alternating with the unmasked steps")
    args = ap.parse_args()
    import torch
    from cchess_alphazero import _native
    from cchess_alphazero.lib.replay_window import ReplayWindow
    _native.require_gpu()
    torch.cuda.set_device(0)
    games = random_games(1, args.games)
    res = {"device": torch.cuda.get_device_name(0), "fill": fill_rates(games)}
    win = ReplayWindow(10 ** 7)
    win.add_games(games)
    res["window_bytes_per_position"] = round((win.n * (90 + 4 + 2 + 4 + 4) + win.nnz * 6) / win.n, 1)
    res["visited_edges_per_position"] = round(win.nnz / win.n, 1)
    for name, (f, b) in (("normal_7x256", (256, 7)), ("bench_7x128", (128, 7))):
        runs = {False: [], True: []}
        for _ in range(max(1, args.repeats)):
            for m in ((False, True) if args.mirror else (False,)):
                runs[m].append(step_times(win, f, b, args.batch, args.warmup, args.steps, mirror=m))
        res[f"step_ms_{name}"] = runs[False][0]
        if args.mirror:
            res[f"step_ms_{name}_mirror"] = runs[True][0]
        if args.repeats > 1:
            res[f"step_ms_{name}_repeats"] = {"plain": runs[False], **({"mirror": runs[True]} if args.mirror else {})}
        if args.policy_mask == "legal":
            # unmasked, masked, unmasked, masked, ... of the same build; at least two legs each, so that the spread between
            # two unmasked legs stands beside any difference
            legs = {"none": [], "legal": []}
            for _ in range(max(2, args.repeats)):
                for m in ("none", "legal"):
                    legs[m].append(step_times(win, f, b, args.batch, args.warmup, args.steps, legal_mask=m == "legal"))
            res[f"policy_mask_{name}"] = {
                **{f"{k}_ms_{m}": [leg[k] for leg in legs[m]] for k in ("loss", "total") for m in ("none", "legal")},
                "loss_ms_unmasked_spread": round(max(x["loss"] for x in legs["none"]) - min(x["loss"] for x in legs["none"]), 4),
                "total_ms_unmasked_spread": round(max(x["total"] for x in legs["none"]) - min(x["total"] for x in legs["none"]), 4)}
    res["batch"] = args.batch
    print(json.dumps(res))


if __name__ == "__main__":
    main()
