#!/usr/bin/env python3
"""How far a network is from treating the two wings of the board alike.

    python tools/mirror_asymmetry.py --config model_best_config.json --weights model_best_weight.h5
    python tools/mirror_asymmetry.py --fresh [--filters 128] [--blocks 7] [--seed 0]

Xiangqi's rules are symmetric under the left-right mirror (file x <-> 8 - x), so an ideal network gives the mirrored
position P' the mirrored policy and the same value: p(P)[l] == p(P')[M(l)] and v(P) == v(P'), M = the label mirror
(cz_label_mirror).  Over the 256 calibration positions of agent/model.py::calibration_planes (fp32 torch forward) this
prints, as one JSON line, the largest and the mean |p(P)[l] - p(P')[M(l)]| and |v(P) - v(P')|.  It is the number
`run.py opt --augment mirror` exists to push down.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "chinesechess-alphazero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def asymmetry(net, planes, chunk=64):
    """net: a CChessNet on the device, in eval mode; planes: [n, depth, 10, 9] (any dtype) -> dict of the four figures."""
    import torch
    from cchess_alphazero import _native
    M = torch.from_numpy(_native.label_mirror().astype("int64")).to(planes.device)
    dp, dv = [], []
    with torch.no_grad():
        for b in range(0, planes.shape[0], chunk):
            x = planes[b:b + chunk].float()
            p, v = net(x)
            pm, vm = net(x.flip(-1).contiguous())
            dp.append((p - pm[:, M]).abs())
            dv.append((v.reshape(-1) - vm.reshape(-1)).abs())
    dp, dv = torch.cat(dp), torch.cat(dv)
    return {"positions": int(planes.shape[0]), "policy_max": float(dp.max()), "policy_mean_row_max": float(dp.max(1).values.mean()),
            "value_max": float(dv.max()), "value_mean": float(dv.mean())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", help="model configuration JSON")
    ap.add_argument("--weights", help="model weights (the path run.py uses; the .pt beside it is read for a torch model)")
    ap.add_argument("--fresh", action="store_true", help="a freshly initialised network instead of a saved one")
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--label", default=None, help="copied into the result")
    args = ap.parse_args()
    import torch
    from cchess_alphazero import _native
    from cchess_alphazero.agent.model import CChessModel, CChessNet, calibration_planes
    from cchess_alphazero.config import Config
    _native.require_gpu()
    torch.cuda.set_device(0)
    if args.fresh:
        torch.manual_seed(args.seed)
        net = CChessNet(cnn_filter_num=args.filters, res_layer_num=args.blocks)
    else:
        if not (args.config and args.weights):
            ap.error("--config and --weights, or --fresh")
        model = CChessModel(Config("mini"))
        if not model.load(args.config, args.weights):
            raise SystemExit(f"no model at {args.config} / {args.weights}")
        net = model.model
    net = net.cuda().eval()
    planes = calibration_planes(input_depth=net.cfg["input_depth"])
    res = asymmetry(net, planes)
    if args.label:
        res["label"] = args.label
    res["filters"], res["blocks"] = net.cfg["cnn_filter_num"], net.cfg["res_layer_num"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
