#!/usr/bin/env python3
"""What the cross-game evaluation cache (engine.eval_cache, cz_search_set_eval_cache) is worth on the `normal` engine.

    python tools/eval_cache_rate.py [--rounds 3000] [--log2 22] [--reps 2] [--sims N] [--book FILE --book-n 16]
    -> one JSON line, also written to --out (default profiles/eval_cache_rate.json)

Legs alternate cache off / on (2^--log2 entries), --reps times over, in ONE process, each a fresh engine (same seed, same
random network), driven the way the self-play worker drives it: HIP graph replays, drained every report_every_rounds
(200).  The search is the same bit for bit either way, so the legs play the same games and expansions/s compares them
round for round.  Per leg: expansions/s; with the cache on the hit rate (hits / expansions: the share of new leaves that
needed no network row) over all rounds and over the first 200, `stores`, the table's bytes.  On a sample of rounds the
share of queue rows that duplicate another row of the SAME round is taken from the occupancy boards on the host: those
the cache cannot answer (readers and writers would meet in one launch), the number a later in-round merge needs.  After
the timed rounds of a cache-on leg a few rounds run outside the graph under the profiler for the fill kernel's time per
round (None when the profiler reports no such kernel)."""
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

FIRST = 200


def duplicate_share(eng):
    """(queue rows of the last round, rows whose position another row of that round holds too) from the occupancy boards."""
    import numpy as np
    s = eng.search
    if not eng.compact or s.masks is None:
        return 0, 0
    n = int(s.q_count.item())
    if n == 0:
        return 0, 0
    boards = s.masks[s.q_rows[:n].long()].cpu().numpy()
    return n, n - len(np.unique(boards, axis=0))


def fill_kernel_us(eng, rounds=20):
    """Mean device time of k_cache_fill per round over `rounds` rounds outside the graph, in microseconds."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        graph, eng._graph = eng._graph, None
        try:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(rounds):
                    eng.step()
                torch.cuda.synchronize()
        finally:
            eng._graph = graph
        def dev_time(e):
            return getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
        rows = [e for e in prof.key_averages() if "k_cache_fill" in e.key]
        if not rows:
            return None
        return sum(dev_time(e) for e in rows) / rounds
    except Exception as e:                                       # the figure is optional; the legs are not
        print(f"fill kernel timing failed: {e}", file=sys.stderr)
        return None


def leg(log2, rounds, every, sims, book, sample):
    import torch
    import bench
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.engine import SelfPlayEngine
    cfg = bench.build_config(types.SimpleNamespace(config="normal", games=None, sims_per_round=None, dtype=None,
                                                   trunk=None))
    if sims:
        cfg.play.simulation_num_per_move = sims
    torch.manual_seed(0)
    net = CChessNet.from_model_config(cfg.model)
    eng = SelfPlayEngine(cfg, cfg.engine.games_per_gpu, net=net, dtype=getattr(torch, cfg.engine.net_dtype), seed=20261019,
                         eval_cache=log2, book=book or None)
    try:
        eng.start(0, 0)
        eng.prewarm()
        for _ in range(20):
            eng.step()
        eng.capture_graph(warmup=0)
        games = 0
        dup_rows = dup = 0
        torch.cuda.synchronize()
        c0, i0 = eng.counters(), eng.search.eval_cache_info()
        first = None
        t0 = time.perf_counter()
        for r in range(1, rounds + 1):
            eng.step()
            if r % every == 0:
                games += len(eng.drain())
            if r == FIRST:
                first = (eng.counters(), eng.search.eval_cache_info())
            if sample and r % sample == 0:
                n, d = duplicate_share(eng)
                dup_rows, dup = dup_rows + n, dup + d
        games += len(eng.drain())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        c1, i1 = eng.counters(), eng.search.eval_cache_info()
        exp = c1["expansions"] - c0["expansions"]
        out = dict(eval_cache=log2, rounds=rounds, sims=cfg.play.simulation_num_per_move, book=len(book or []), seconds=dt,
                   expansions_per_s=exp / dt, expansions=exp, games=games, plies=c1["plies"] - c0["plies"],
                   sampled_rows=dup_rows, sampled_rows_duplicating_another=dup,
                   in_round_duplicate_share=dup / dup_rows if dup_rows else None)
        if log2:
            out.update(hits=i1["hits"] - i0["hits"], probes=i1["probes"] - i0["probes"], stores=i1["stores"] - i0["stores"],
                       hit_rate=(i1["hits"] - i0["hits"]) / max(exp, 1), table_bytes=eng.search.memory_info()["eval_cache_bytes"])
            if first is not None:
                out["hit_rate_first_200"] = (first[1]["hits"] - i0["hits"]) / max(first[0]["expansions"] - c0["expansions"], 1)
            out["fill_kernel_us_per_round"] = fill_kernel_us(eng)
        return out
    finally:
        eng.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3000)
    ap.add_argument("--log2", type=int, default=22)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--sims", type=int, default=0, help="simulations per move (0: the configuration's)")
    ap.add_argument("--book", default=None, help="start-position book file (lib/book.py)")
    ap.add_argument("--book-n", type=int, default=16, help="positions of --book to use")
    ap.add_argument("--every", type=int, default=200, help="drain cadence (rounds), the worker's report_every_rounds")
    ap.add_argument("--sample", type=int, default=100, help="count in-round duplicate rows every this many rounds (0: never)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_cache_rate.json"))
    args = ap.parse_args()
    if not 10 <= args.log2 <= 24:
        raise SystemExit(f"--log2 {args.log2}: expected 10 <= LOG2 <= 24")
    book = []
    if args.book:
        from cchess_alphazero.lib.book import load_book
        book = list(load_book(args.book))[:args.book_n]
    legs = []
    for _ in range(args.reps):
        for log2 in (0, args.log2):
            legs.append(leg(log2, args.rounds, args.every, args.sims, book, args.sample))
            print(json.dumps(legs[-1]), file=sys.stderr, flush=True)
    off = [x["expansions_per_s"] for x in legs if not x["eval_cache"]]
    on = [x["expansions_per_s"] for x in legs if x["eval_cache"]]
    mean = lambda xs: sum(xs) / len(xs)  # noqa: E731
    out = dict(off=dict(expansions_per_s=off, mean=mean(off), spread=(max(off) - min(off)) / mean(off)),
               on=dict(expansions_per_s=on, mean=mean(on), spread=(max(on) - min(on)) / mean(on)),
               on_over_off=mean(on) / mean(off), legs=legs)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
