#!/usr/bin/env python3
"""GPU: how well the best model's moves-left output fits the records of a directory, evaluated THROUGH InferenceNet -- the
hand-written kernels (cz_heads_tail_ml) that would serve it -- beside the fp32 torch module the trainer optimised: the check
that what was trained is what is served.

Every position of every record file gets its target (the record items from its own to the end of its game, inclusive;
lib/replay_window.py moves_left_targets -- games cut by `run.py reanalyse --reanalyse-plies` carry targets that are too
small) and the prediction m(x) = 32 softplus(x) plies.  Printed: the mean absolute error in plies per bucket of true plies
left (1-8, 9-32, 33-128, > 128) and over all positions, for both paths, and the largest difference between the two paths'
raw outputs; with --out also one JSON line.

    python tools/moves_left_fit.py [--type mini] [--dir DIR] [--max-positions N] [--batch 1024] [--out FILE]
    (DIR defaults to the configuration's play-data directory; the best model is the configuration's)
"""
import argparse
import json
import os
import sys
from glob import glob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "chinesechess-alphazero_amd"))

BUCKETS = ((1, 8), (9, 32), (33, 128), (129, None))


def bucket_mae(pred, left):
    """{bucket name: (positions, mean |pred - left|)} for float64 numpy arrays, the buckets by true plies left."""
    import numpy as np
    out = {}
    for lo, hi in BUCKETS:
        m = (left >= lo) & ((left <= hi) if hi is not None else True)
        name = f"{lo}-{hi}" if hi is not None else f">{lo - 1}"
        out[name] = (int(m.sum()), float(np.abs(pred[m] - left[m]).mean()) if m.any() else float("nan"))
    out["all"] = (int(left.shape[0]), float(np.abs(pred - left).mean()) if left.shape[0] else float("nan"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--type", default="mini")
    ap.add_argument("--dir")
    ap.add_argument("--max-positions", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from cchess_alphazero import _native
    from cchess_alphazero.agent.model import CChessModel, guarded_inference_net, moves_left_plies
    from cchess_alphazero.config import Config
    from cchess_alphazero.lib.model_helper import load_best_model_weight
    from cchess_alphazero.lib.replay_window import ReplayWindow
    _native.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = Config(a.type)
    model = CChessModel(cfg)
    if not load_best_model_weight(model):
        raise SystemExit("no best model to evaluate")
    net = model.model
    if not net.moves_left_head:
        raise SystemExit("the best model has no moves-left output (train one with `run.py opt --moves-left W --new`)")
    d = a.dir or cfg.resource.play_data_dir
    files = sorted(glob(os.path.join(d, "*.json")))
    if not files:
        raise SystemExit(f"no record files in {d}")
    win = ReplayWindow(a.max_positions, depth=net.cfg["input_depth"], moves_left=True)
    for f in files:
        if win.full:
            break
        win.load_file(f)
    n = len(win)
    inf = guarded_inference_net(net, torch.float32, trunk="mfma", device=dev)
    net = net.to(dev).eval()
    x_k = torch.empty((n,), device=dev)
    x_m = torch.empty((n,), device=dev)
    with torch.no_grad():
        for b in range(0, n, a.batch):
            idx = torch.arange(b, min(n, b + a.batch), dtype=torch.int32, device=dev)
            planes = win.planes(idx)
            inf(planes, moves_left=x_k[b:b + idx.shape[0]])
            x_m[b:b + idx.shape[0]] = net(planes, moves_left=True)[2]
    left = win.left[:n].double().cpu().numpy()
    res = dict(files=len(win.files), positions=n, arith=inf.arith_effective,
               max_abs_x_difference=float((x_k - x_m).abs().max()),
               kernels=bucket_mae(moves_left_plies(x_k.double()).cpu().numpy(), left),
               module=bucket_mae(moves_left_plies(x_m.double()).cpu().numpy(), left))
    print(f"{n} positions of {len(win.files)} files; InferenceNet ({inf.arith_effective}) against the fp32 module: "
          f"max |x difference| {res['max_abs_x_difference']:.3g}")
    print(f"{'plies left':>12} {'positions':>10} {'MAE kernels':>12} {'MAE module':>12}")
    for name, (cnt, mae) in res["kernels"].items():
        print(f"{name:>12} {cnt:>10} {mae:>12.3f} {res['module'][name][1]:>12.3f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
