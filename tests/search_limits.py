"""Shared by tests/test_search_limits_cpu.py and tests/test_gpu_search_limits.py: the cases that drive the tree search
onto paths longer than 64 plies and into its counted cut-offs (depth_overflow, overflow_sims), and the invariants that
hold for every node of a tree once no simulation is in flight.

The invariants (v = virtual_loss; a selection from a node does sum_n += 1, n_j += v, w_j -= v; the simulation's one
backup does n_j += 1 - v, w_j += value + v on every edge of its path):
  * sum_j n_j == sum_n - 1      sum_n starts at 1 (player.py:213) and each selection ends as exactly one net visit
  * n_j >= 0
  * |w_j| <= 2 n_j              network values lie in [-1, 1], terminal values are +-2 (player.py:204-208)
A virtual loss that is never returned leaves sum_j n_j == sum_n - 1 + (v - 1) per lost one, and w_j lower by v.
"""
import numpy as np

import stub_net
from oracle import xq_oracle as xo

MID = 'r1e1s1e1r/4m4/2k1c1k2/p1p1p1p1p/9/2P6/P3P1P1P/1CK1C1K2/9/R1EMSME1R'
PEAKED = dict(kind="peaked", salt=5, squarings=8, value=0.0)

# (K, simulations, position, input planes): each reaches a path of more than 64 plies under PEAKED in the oracle
LONG_CASES = [
    (1, 400, MID, 14),
    (1, 400, xo.fliped_state(MID), 14),
    (1, 400, MID, 28),
    (8, 1600, MID, 14),
    (8, 1600, xo.fliped_state(MID), 14),
]

# the counters the engine and the oracle both keep (the engine's names)
PARITY_COUNTERS = ("sims", "expansions", "terminal_sims", "repetition_sims", "parked", "max_depth", "sum_depth",
                   "depth_overflow", "overflow_sims")


def oracle_stub(spec):
    """What xo.Player takes for a stub spec: the C stubs by spec, the peaked stub as the NumPy callable."""
    return stub_net.stub_numpy(spec) if spec["kind"] == "peaked" else spec


def node_defect(st):
    """None if the edges of one node (dict(n, w, sum_n)) satisfy the three invariants, else what is wrong."""
    n, w = np.asarray(st["n"], dtype=np.int64), np.asarray(st["w"], dtype=np.float64)
    if len(n) == 0:
        return None
    if int(n.sum()) != int(st["sum_n"]) - 1:
        return f"sum n_j = {int(n.sum())}, sum_n - 1 = {int(st['sum_n']) - 1}"
    if (n < 0).any():
        return f"negative visit count {n.min()}"
    if (np.abs(w) > 2.0 * n).any():
        return f"|w| > 2 n at edge {int(np.argmax(np.abs(w) - 2.0 * n))}"
    return None


def walk_oracle_tree(pl, root_state, limit=100000):
    """Every node of the oracle player's tree that can be reached from root_state over visited edges, breadth first:
    yields (path of labels, board, node_stats).  (node_stats spreads a node's waiting priors: harmless, the search does
    the same on its next visit.)"""
    root = xo.state_to_board(root_state) if isinstance(root_state, str) else np.asarray(root_state, dtype=np.int8)
    seen = {root.tobytes()}
    queue = [((), root)]
    while queue and limit > 0:
        nxt = []
        for path, board in queue:
            st = pl.node_stats(board)
            if st is None:
                continue
            limit -= 1
            yield path, board, st
            for j in np.nonzero(st["n"])[0]:
                child, _ = xo.step_board(board, int(st["moves"][j]))
                key = child.tobytes()
                if key not in seen and not xo.done_board(child)[0]:
                    seen.add(key)
                    nxt.append((path + (int(st["moves"][j]),), child))
        queue = nxt


def tree_defects(pl, root_state):
    """(nodes looked at, [(path, defect)]) over the whole oracle tree."""
    bad, count = [], 0
    for path, _, st in walk_oracle_tree(pl, root_state):
        count += 1
        d = node_defect(st)
        if d:
            bad.append((path, d))
    return count, bad


def zero_prior_node(pl, root_state):
    """The first node (breadth first) that was selected from and whose legal moves ALL got the prior 0 (spread_priors:
    all_p == 0 -> 1, so p_j = 0 / 1): (path, stats), or None."""
    for path, _, st in walk_oracle_tree(pl, root_state):
        if len(st["p"]) and st["sum_n"] > 1 and not st["p"].any():
            return path, st
    return None


def sims_end_one_way(c):
    """At idle every simulation has ended exactly one way: it expanded a leaf (the root's own expansion included) and
    backed up its evaluation, ended on a terminal or a repeated position, was refused tree memory at one of the three
    overflow_sims sites (each of which backs up 0 and finishes the simulation), or was cut at the depth limit."""
    return c["sims"] == (c["expansions"] + c["terminal_sims"] + c["repetition_sims"] + c["overflow_sims"]
                         + c["depth_overflow"])
