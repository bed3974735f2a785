#!/usr/bin/env python3
"""Where the chained launch of the four-wave pair kernel (k_resblock_ip4_c8<128>) spends its shader cycles: a -DCZ_IP4_STAMPS
build of the library (variant, never the default) stamps the clock in one wave per board of workgroup 0 around the phases of
every block of its second (steady-state) pair.  The 7 x 128 c6 tower, 32768 boards: the stamps left behind are those of the
last chained launch of a forward (blocks 1 - 6, heads exit).  Run on the MI355X:

    python chinesechess-alphazero_amd/build.py --out variants/libczero_ip4_stamps.so -DCZ_IP4_STAMPS      (cross-compiles)
    CZ_LIB=variants/libczero_ip4_stamps.so python tools/ip4_stamps.py profiles/ip4_stamps.json
    (the plain order, nothing requested early: add -DCZ_IP4_PREFETCH=0 to the build -> profiles/ip4_stamps_parent.json;
     the epilogues as they were before their instruction diet, or single items of it: add -DCZ_IP4_EPI=<mask>, 0 = before,
     csrc/xq_conv_ip4.h above k_resblock_ip4_c8 -> profiles/ip4_stamps_epilogues_parent.json / ip4_stamps_epilogues.json)
"""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "chinesechess-alphazero_amd"))

PHASES = ["block_setup", "k1_prologue_to_first_mfma", "k1_loop", "barrier_K1", "epilogue_1", "barrier_B_and_write_bias",
          "k2_prologue_to_first_mfma", "k2_loop", "barrier_K2", "epilogue_2", "barrier_C"]
TARGETED = ["block_setup", "k1_prologue_to_first_mfma", "barrier_B_and_write_bias", "k2_prologue_to_first_mfma", "exit",
            "drain_and_fill"]


def main():
    from cchess_alphazero import _native
    from cchess_alphazero.agent.model import CChessNet, calibration_planes, guarded_inference_net
    n, nb = 32768, 6
    torch.manual_seed(0)
    net = CChessNet(cnn_filter_num=128, res_layer_num=7).eval()
    planes = calibration_planes(4096, 14, seed=1).repeat(n // 4096, 1, 1, 1).contiguous()
    g = guarded_inference_net(net, torch.float32, trunk="mfma", arith="c6", guard=False)
    for _ in range(8):                                    # warm: the clock settles under the sustained load
        g(planes)
    torch.cuda.synchronize()
    L = _native.lib()
    L.cz_debug_ip4_stamps.argtypes = [C.c_void_p]
    st = (C.c_longlong * (2 * 12 * 16))()
    assert L.cz_debug_ip4_stamps(st) == 0
    s = [[[st[(bd * 12 + b) * 16 + i] for i in range(16)] for b in range(12)] for bd in range(2)]
    boards = []
    for bd in range(2):
        rows = s[bd][:nb]
        assert all(r[0] > 0 for r in rows), "no stamps: is CZ_LIB a -DCZ_IP4_STAMPS build, and the chain six blocks long?"
        per_block = {p: [r[i + 1] - r[i] for r in rows] for i, p in enumerate(PHASES)}
        last = rows[-1]
        m = {p: sum(v) for p, v in per_block.items()}
        m["exit"] = last[12] - last[11]
        m["drain_and_fill"] = last[14] - last[12]
        pair = last[14] - rows[0][0]
        boards.append({"cycles_per_pair_by_phase": m, "per_block": per_block, "pair_cycles": pair,
                       "unstamped_cycles": pair - sum(m.values()),
                       "targeted_cycles": sum(m[p] for p in TARGETED),
                       "targeted_share": sum(m[p] for p in TARGETED) / pair})
    res = {"boards": n, "blocks_in_chain": nb, "wave_of_board": boards,
           "mfma_floor_cycles_per_kloop": 20736, "stamped": "workgroup 0, second pair, waves 0 and 2"}
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
