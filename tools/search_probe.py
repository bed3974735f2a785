#!/usr/bin/env python3
"""GPU: the tree kernels alone in a sustained state, quickly.  4096 self-play games (normal search settings) driven by
the hash-stub network (tests/stub_net.py: microseconds per round instead of 30 ms), so that a few thousand rounds --
games in every phase, trees tens of thousands of nodes deep -- take seconds; then the search round is timed with HIP
events over the next rounds (per-launch: mean / median / p99).  A/B tool for changes to the search
(csrc/xq_search.hip and the csrc/xq_search_*.h it is made of).

    python tools/search_probe.py [--rounds 3000] [--timed 200] [--compact 1] [--masks-only 1] [--leaf-mirror P]
                                 [--moves-left-slope S [--moves-left-cap C]] [--draw-average 1 [--draw-score S]]
                                 [--lcb Z [--lcb-min-visits R]]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "chinesechess-alphazero_amd"), ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3000)
    ap.add_argument("--timed", type=int, default=200)
    ap.add_argument("--compact", type=int, default=1)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--masks-only", type=int, default=0, help="1: leaves written as occupancy boards only (cz_search_leaf_planes(0))")
    ap.add_argument("--leaf-mirror", type=float, default=0.0, help="rate of the random leaf mirror (cz_search_set_leaf_mirror)")
    ap.add_argument("--moves-left-slope", type=float, default=0.0,
                    help="slope of the moves-left utility (cz_search_set_moves_left); the stub's third output feeds it")
    ap.add_argument("--moves-left-cap", type=float, default=0.0345)
    ap.add_argument("--draw-average", type=int, default=0,
                    help="1: the draw average (cz_search_set_draw); the draw stub's third output feeds it")
    ap.add_argument("--draw-score", type=float, default=0.0)
    ap.add_argument("--lcb", type=float, default=0.0,
                    help="z of the lower-confidence-bound move choice (cz_search_set_lcb): k_sim_var, k_advance_lcb")
    ap.add_argument("--lcb-min-visits", type=float, default=0.15)
    a = ap.parse_args()
    import types
    import stub_net
    from cchess_alphazero import _native
    from cchess_alphazero._native_search import Search
    pc = types.SimpleNamespace(simulation_num_per_move=800, search_threads=8, c_puct=1.5, noise_eps=0.15,
                               dirichlet_alpha=0.2, tau_decay_rate=0.9, virtual_loss=3, resign_threshold=-0.98,
                               min_resign_turn=40, max_game_length=100, enable_resign_rate=0.5)
    s = Search(pc, a.games, planes_dtype=_native.U8, seed=20260923)
    if a.masks_only:
        s.leaf_masks(True)
        s.leaf_planes(False)
    if a.leaf_mirror:
        s.set_leaf_mirror(a.leaf_mirror, flags=True)
    if a.moves_left_slope:
        import stub_moves_left
        s.set_moves_left(a.moves_left_slope, a.moves_left_cap)
    if a.draw_average:
        import stub_draw
        s.set_draw(True, a.draw_score)
    if a.lcb:
        s.set_lcb(a.lcb, a.lcb_min_visits)
    s.start_selfplay(seed=20260923)
    planes_of = (lambda: s.queue_planes()) if a.masks_only else (lambda: s.planes)   # (the same planes either way: same trees)

    def feed():
        # a near-uniform, position-dependent network: cheap, and the trees grow like the random-init net's
        p, v = stub_net.hash_stub_torch(planes_of(), 1)
        p = p * 0 + 1.0 / 2086 + p * 1e-3
        x = stub_moves_left.ml_stub_torch(planes_of(), 1)[2] if a.moves_left_slope else None
        wdl = stub_draw.draw_stub_torch(planes_of(), 1)[2] if a.draw_average else None
        if a.compact:
            rows = s.q_rows.long().clamp_(0, s.slots - 1)
            s.policy.copy_(p.index_select(0, rows))
            s.value.copy_((v * 0.05).index_select(0, rows))
            if x is not None:
                s.moves_left_x.copy_(x.index_select(0, rows))
            if wdl is not None:
                s.wdl_rows.copy_(wdl.index_select(0, rows))
        else:
            s.policy.copy_(p)
            s.value.copy_(v * 0.05)
            if x is not None:
                s.moves_left_x.copy_(x)
            if wdl is not None:
                s.wdl_rows.copy_(wdl)

    for _ in range(a.rounds):
        s.round(compact=bool(a.compact))
        feed()
    torch.cuda.synchronize()
    ev = []
    for _ in range(a.timed):
        e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        e[0].record()
        s.round(compact=bool(a.compact))
        e[1].record()
        ev.append(e)
        feed()
    torch.cuda.synchronize()
    t = sorted(x.elapsed_time(y) for x, y in ev)
    c, m = s.counters(), s.memory_info()
    out = {"rounds_before": a.rounds, "timed": a.timed, "compact": a.compact, "masks_only": a.masks_only,
           "search_round_ms": {"mean": sum(t) / len(t), "median": t[len(t) // 2], "p99": t[int(len(t) * 0.99)], "max": t[-1]},
           "mean_depth": c["sum_depth"] / max(1, c["sims"]), "plies": c["plies"], "games": c["games"],
           "tree_resets": c["tree_resets"], "overflow_sims": c["overflow_sims"], "nodes": m["nodes"],
           "tree_gb": m["tree_bytes"] / 1e9, "tree_bytes_per_game": m["tree_bytes"] / a.games,
           "moves_left_slope": a.moves_left_slope, "draw_average": a.draw_average, "draw_score": a.draw_score,
           "lcb": a.lcb, "lcb_min_visits": a.lcb_min_visits}
    if a.leaf_mirror:                      # (of the slots as they stand: every slot has held a leaf by now)
        out["leaf_mirror"] = a.leaf_mirror
        out["mirrored_share_of_slots"] = float(s.mirrored.float().mean())
    if "cyc_select" in c:                  # CZ_SIM_PROFILE build: shader-clock cycles of wave time per section, per simulation
        n = max(1, c["sims"])
        out["cycles_per_sim"] = {k: c[k] / n for k in c if k.startswith("cyc_")}
        out["levels_per_sim"] = c["sum_depth"] / n
    print(json.dumps(out))
    s.close()


if __name__ == "__main__":
    main()
