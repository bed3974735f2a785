"""Forced playouts and policy target pruning (cz_search_set_forced_playouts, run.py self --forced-playouts K) restated in
Python.  oracle/xq_mcts.c cannot force, so the yardstick is search_model.Search -- the reference's search once more, for
search_threads = 1 and noise_eps = 0 only -- which carries the forcing rule in the root branch of its selection; prune(),
the arithmetic of include/czero.h, is here, and Search.targets applies it.

The search, the positions of the tests and the walk over a case's searches are search_model's and are re-exported here:
the tests of the feature, and those of the features built on it, reach them as fo.Search, fo.cases(), fo.run_case(...)."""
import math

import numpy as np

from search_model import BANNED, SIMS, Search, ban_of, cases, play_cfg, run_case       # noqa: F401 (re-exports)
from search_model import Node as _Node                                                  # noqa: F401


def prune(labels, n, w, p, c_puct, k):
    """Policy target pruning as include/czero.h defines it.  labels: uint16 with BANNED (0x8000) on banned edges; n raw
    counts; w float64; p float32 priors without noise.  Returns (int32 pruned counts, raw_total S).  Every operation is
    one float64 operation of the definition, in its order; sqrt / floor / ceil are exact or correctly rounded."""
    labels = np.asarray(labels, dtype=np.uint16)
    n = np.asarray(n, dtype=np.int32)
    w = np.asarray(w, dtype=np.float64)
    p = np.asarray(p, dtype=np.float32)
    out = n.copy()
    live = [j for j in range(len(n)) if not labels[j] & BANNED]
    S = sum(int(n[j]) for j in live)
    if S == 0:
        return out, 0
    star = min(live, key=lambda j: (-int(n[j]), int(labels[j] & 0x7FFF)))
    c_puct, k, Sd = float(c_puct), float(k), float(S)
    sq = math.sqrt(Sd)
    e_star = float(w[star]) / float(n[star]) + ((c_puct * float(p[star])) * sq) / float(1 + int(n[star]))
    for j in live:
        if j == star or n[j] <= 0:
            continue
        nj, pj = float(n[j]), float(p[j])
        f = float(np.floor(math.sqrt((k * pj) * Sd)))
        d = e_star - float(w[j]) / nj
        need = nj
        if d > 0.0:
            with np.errstate(over="ignore", divide="ignore"):
                need = float(np.ceil(np.float64((c_puct * pj) * sq) / np.float64(d) - np.float64(1.0)))
            need = 0.0 if need < 0.0 else (nj if need > nj else need)
        keep = nj - f
        m = int(need if need > keep else keep)
        if m < n[j] and m <= 1:
            m = 0
        out[j] = m
    return out, S
