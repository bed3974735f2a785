#!/usr/bin/env python3
"""GPU: what the moves-left output costs in the dense tail (cz_heads_tail_ml) beside the tail without it, for both value
heads, on the evaluation queue's full size.  The yardstick is the entry point a network without the output launches --
cz_heads_tail for the scalar head, cz_heads_tail_wdl for win / draw / loss -- on the same box in alternated legs.

All tails read the same head features ([rows, 360] policy, [rows, 180] value, O(1) data), the same packed policy and hidden
layers (2086 labels, 256 hidden units, fp16 pairs), raw logits (normalize = 0, the engine's queue) and the softmax form.  After
a warm-up the four alternate leg by leg on one stream; a leg is `launches` calls between two device events.  Printed: one JSON
line with every leg's time per call, the means and the spread (max - min) of each tail's legs, and the two differences.

    python tools/moves_left_tail_cost.py [--rows 32768] [--legs 7] [--launches 200] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "chinesechess-alphazero_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--legs", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from cchess_alphazero import _native
    _native.require_gpu()
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(1)
    n, n_lab, n_hid = a.rows, 2086, 256
    rnd = lambda *s: torch.randn(s, generator=g)
    pf, vf = (torch.relu(rnd(n, 360)) * 1.5).cuda(), (torch.relu(rnd(n, 180)) * 1.5).cuda()
    wp, w1 = _native.pack_fc_weights(rnd(n_lab, 360) * 0.08).cuda(), _native.pack_fc_weights(rnd(n_hid, 180) * 0.1).cuda()
    bp, b1 = (rnd(n_lab) * 0.5).cuda(), (rnd(n_hid) * 0.2).cuda()
    w2 = (rnd(4, n_hid) * 0.2).cuda()                                   # (win, draw, loss, moves left)
    b2 = (0.13, -0.21, 0.05, 1.85)
    w2_s, w2_w, w2_sm = w2[0].contiguous(), w2[:3].contiguous(), w2[[0, 3]].contiguous()
    pol = torch.empty((n, n_lab), device="cuda")
    val, wdl, stats = torch.empty((n,), device="cuda"), torch.empty((n, 3), device="cuda"), torch.empty((n, 2), device="cuda")
    ml = torch.empty((n,), device="cuda")
    result = dict(rows=n, launches=a.launches, legs=a.legs, device=torch.cuda.get_device_name(0))
    for normalize in (False, True):
        tails = {
            "scalar": lambda: _native.heads_tail(pf, vf, wp, bp, w1, b1, w2_s, b2[0], pol, val, stats, normalize=normalize),
            "scalar_ml": lambda: _native.heads_tail_ml(pf, vf, wp, bp, w1, b1, w2_sm, (b2[0], b2[3]), pol, val, stats, ml,
                                                       normalize=normalize),
            "wdl": lambda: _native.heads_tail_wdl(pf, vf, wp, bp, w1, b1, w2_w, b2[:3], pol, val, stats, wdl=wdl,
                                                  normalize=normalize),
            "wdl_ml": lambda: _native.heads_tail_ml(pf, vf, wp, bp, w1, b1, w2, b2, pol, val, stats, ml, wdl=wdl,
                                                    normalize=normalize),
        }

        def leg(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.launches * 1e3         # microseconds per call

        for fn in tails.values():
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in tails}
        for _ in range(a.legs):
            for k, fn in tails.items():
                us[k].append(leg(fn))
        mean = {k: sum(v) / len(v) for k, v in us.items()}
        result["normalize" if normalize else "logits"] = dict(
            us_per_call={k: [round(x, 2) for x in v] for k, v in us.items()}, mean_us={k: round(v, 2) for k, v in mean.items()},
            spread_us={k: round(max(v) - min(v), 2) for k, v in us.items()},
            scalar_ml_minus_scalar_us=round(mean["scalar_ml"] - mean["scalar"], 2),
            wdl_ml_minus_wdl_us=round(mean["wdl_ml"] - mean["wdl"], 2))
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
