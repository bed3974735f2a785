"""The root value record (cz_search_record_values, run.py self --record-q, run.py opt --q-ratio) restated in plain Python:
the yardstick of tests/test_q_record_cpu.py and tests/test_gpu_q_record.py.

    q_root = ( sum_j m_j * (w_j / n_j) ) / ( sum_j m_j )      over non-banned edges with n_j > 0

Every quotient and product is one float64 operation; the sums are math.fsum's, exact, so the only error of this value
against the real number is the final division's and the terms' own roundings."""
import math
from collections import namedtuple

import numpy as np

BANNED = 0x8000
NAN = float("nan")
Entry = namedtuple("Entry", "moves n banned q")      # what lib/data_helper.record_item reads of a VisitEntry


def root_value(labels, m, n, w):
    """labels (bit 15 = banned), m (the recorded counts), n, w (the raw statistics) of one root's edges -> q_root, NaN when
    no non-banned edge with n > 0 has a recorded count."""
    live = [j for j in range(len(n)) if not int(labels[j]) & BANNED and int(n[j]) > 0]
    den = sum(int(m[j]) for j in live)
    if den == 0:
        return NAN
    return math.fsum(float(int(m[j])) * (float(w[j]) / float(int(n[j]))) for j in live) / float(den)


def same_value(a, b, tol=1e-13):
    """NaN where the other is NaN, otherwise within tol."""
    return (a != a and b != b) or (a == a and b == b and abs(a - b) <= tol)


def mix_f64(z, q, lam):
    """The value targets z + lam (q - z) in float64, z where q is NaN."""
    z = np.asarray(z, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    return np.where(np.isnan(q), z, z + float(lam) * (np.where(np.isnan(q), z, q) - z))


def five_element_games(games):
    """Engine records ([state, [move, value], ...]) rewritten as run.py self --record-visits --record-q --fast-sims writes
    them, by lib/data_helper.record_item: every ply but each game's last (the appended king capture / the last move keeps
    the two-element form) gets pi = its own move, every third ply is a fast one, every fifth has no value.  The moves
    and values are untouched: what the reference's expanding_data reads of an item."""
    from cchess_alphazero.environment.lookup_tables import ActionLabelsRed
    from cchess_alphazero.lib.data_helper import record_item
    label = {m: i for i, m in enumerate(ActionLabelsRed)}
    out = []
    for g in games:
        data = [g[0]]
        for i, it in enumerate(g[1:]):
            last = i == len(g) - 2
            q = None if i % 5 == 4 else 0.5 * it[1] + 0.001 * i
            e = None if last else Entry(np.array([label[it[0]]], dtype=np.uint16), np.array([7 + i], dtype=np.int32),
                                        np.array([False]), q)
            data.append(record_item(it[0], it[1], e, fast=(i % 3 == 2 and not last), record_q=True, labels=ActionLabelsRed))
        out.append(data)
    return out
