"""The full Gumbel search (cz_search_set_gumbel_full, run.py self --gumbel-full) restated in Python over gumbel_oracle: the
definitions of include/czero.h in plain float64 -- v_mix, the improved policy, the score of the selection below the root,
the full-mode policy target -- and a subclass of gumbel_oracle.Search that reads the network value every node of search_model
keeps, selects below the root by argmax pi'(a) - N(a) / (1 + sum N), and completes the target with v_mix.

The sums are Python's, in edge order; the device adds a lane's two edges first and then runs one ladder over the lanes,
and its exp is another library's.  Scores so agree to ~1e-16 and not to the bit, which is why the GPU comparison rests on
every selection's winning margin (Search.in_margins below the root, gumbel_oracle's margins at it) and allows +-1 on a
target."""
import math

import numpy as np

import gumbel_oracle as go
import search_model as sm
from oracle import xq_oracle as xo

BANNED = go.BANNED
INF = go.INF
C_VISIT, C_SCALE = go.C_VISIT, go.C_SCALE


# ---- the definitions ----------------------------------------------------------------------------------------------------
def vhat(v):
    x = (float(v) + 1.0) / 2.0
    return (1.0 if x > 1.0 else x) if x > 0.0 else 0.0


def v_mix(n, w, p, v, live=None):
    """(vhat + N (B / A)) / (1 + N) over the edges `live` (default: all), vhat where no visited edge has a prior."""
    live = range(len(n)) if live is None else live
    N = sum(int(n[j]) for j in live)
    A = sum(float(p[j]) for j in live if n[j] > 0)
    B = sum(float(p[j]) * go.q01(int(n[j]), w[j]) for j in live if n[j] > 0)
    if not A > 0.0:
        return vhat(v)
    return (vhat(v) + float(N) * (B / A)) / float(1 + N)


def improved_policy(n, w, p, v, c_visit=C_VISIT, c_scale=C_SCALE, live=None):
    """pi' over the edges `live` (default: all) as a list over all edges, 0 elsewhere; all 0 when no live edge has a
    positive prior."""
    live = list(range(len(n)) if live is None else live)
    out = [0.0] * len(n)
    if not live:
        return out
    vm = v_mix(n, w, p, v, live)
    max_n = max(int(n[j]) for j in live)
    sg = {j: go.sigma(c_visit, c_scale, max_n, go.q01(int(n[j]), w[j]) if n[j] > 0 else vm) for j in live}
    mx = max(sg.values())
    e = {j: float(p[j]) * math.exp(sg[j] - mx) for j in live}
    tot = math.fsum(e.values())
    if not tot > 0.0:
        return out
    for j in live:
        out[j] = e[j] / tot
    return out


def interior_scores(n, w, p, v, c_visit=C_VISIT, c_scale=C_SCALE):
    """score_j = pi'_j - n_j / (1 + N) for every edge of a node below the root."""
    pi = improved_policy(n, w, p, v, c_visit, c_scale)
    d = float(1 + sum(int(x) for x in n))
    return [pi[j] - float(int(n[j])) / d for j in range(len(n))]


def interior_pick(n, w, p, v, c_visit=C_VISIT, c_scale=C_SCALE):
    """(the edge of the greatest score, the later one on a tie, -1 without an edge; the scores; the winner's margin over
    the best other edge, +inf when it stands alone)."""
    sc = interior_scores(n, w, p, v, c_visit, c_scale)
    if not sc:
        return -1, sc, INF
    best = max(range(len(sc)), key=lambda j: (sc[j], j))
    rest = [sc[j] for j in range(len(sc)) if j != best]
    return best, sc, (sc[best] - max(rest) if rest else INF)


def target_v(labels, n, w, p, v, c_visit=C_VISIT, c_scale=C_SCALE):
    """The full-mode policy target of a root row with the root's network value v: (int32 m_j = floor(65536 pi'_j + 1/2),
    raw total of the non-banned edges).  gumbel_oracle.target with v_mix in the place of vbar."""
    labels = np.asarray(labels, dtype=np.uint16)
    n = np.asarray(n, dtype=np.int32)
    out = np.zeros(len(n), dtype=np.int32)
    live = [j for j in range(len(n)) if not labels[j] & BANNED]
    S = sum(int(n[j]) for j in live)
    pi = improved_policy(n, np.asarray(w, dtype=np.float64), np.asarray(p, dtype=np.float32), v, c_visit, c_scale, live)
    for j in live:
        out[j] = int(math.floor(65536.0 * pi[j] + 0.5))
    return out, S


# ---- the rows of the row tests ------------------------------------------------------------------------------------------
PAIRS = ((50.0, 1.0), (0.0, 0.1), (50.0, 0.0))      # the (c_visit, c_scale) the row tests run at


def random_rows(seed=29):
    """The 64 rows of the GPU row test, built with the _random_row recipe of tests/test_gpu_gumbel.py: edge counts 1, 2,
    63, 64, 65, 127, 128 and 57 drawn from 1 .. 128, bans as there, row 7 with nothing visited; then v uniform in [-1, 1]
    as float32.  list of dict(labels, n, w, p, v)."""
    from test_gpu_gumbel import _random_row
    rng = np.random.default_rng(seed)
    sizes = [1, 2, 63, 64, 65, 127, 128] + [int(rng.integers(1, 129)) for _ in range(57)]
    rows = [_random_row(rng, nm, ban=0.15 * (i % 3), visited=(0.0 if i == 7 else 0.7)) for i, nm in enumerate(sizes)]
    v = rng.uniform(-1.0, 1.0, len(rows)).astype(np.float32)
    for r, x in zip(rows, v):
        r["v"] = x
    return rows


def target_margin(labels, n, w, p, v, c_visit, c_scale):
    """How far the nearest 65536 pi'_j + 1/2 of a row is from an integer: a target differs between two implementations
    only where this is below their difference."""
    live = [j for j in range(len(n)) if not labels[j] & BANNED]
    pi = improved_policy(n, w, p, v, c_visit, c_scale, live)
    return min((abs((65536.0 * pi[j] + 0.5) - round(65536.0 * pi[j] + 0.5)) for j in live), default=INF)


# ---- the search ---------------------------------------------------------------------------------------------------------
class Search(go.Search):
    """gumbel_oracle.Search with, full on, the rule below the root and v_mix in the target, both over the nodes' kept
    network values.  With full off it is gumbel_oracle.Search bit for bit.  After search(): in_margins, the winner's score
    minus the best other score at every selection below the root (+inf where the node had one edge)."""

    def __init__(self, cfg, salt, k=0.0, m=0, c_visit=C_VISIT, c_scale=C_SCALE, draws=None, full=False):
        super().__init__(cfg, salt, k, m, c_visit, c_scale, draws)
        if full and not m:
            raise ValueError("the full Gumbel search needs the Gumbel root search (m > 0)")
        self.full = bool(full)
        self.in_margins = []

    def _select(self, node, is_root):
        if is_root or not (self.full and self.m > 0):
            return super()._select(node, is_root)
        if node.pending is not None:
            node.spread()
        best, _, margin = interior_pick(node.n, node.w, node.p, node.v, self.c_visit, self.c_scale)
        if best >= 0:
            self.in_margins.append(margin)
        return best, False

    def search(self, state, no_act=None, increase_temp=False):
        self.in_margins = []
        return super().search(state, no_act, increase_temp)

    def net_value(self, state):
        """The kept float32 value of `state`, None when it is not in the tree."""
        node = self.tree.get(state)
        return None if node is None else node.v

    def targets(self, state, no_act=None):
        if not (self.full and self.m > 0):
            return super().targets(state, no_act)
        st = self.node_stats(state)
        return target_v(sm.banned_labels(st["moves"], no_act), st["n"], st["w"], st["p"], self.tree[state].v,
                        self.c_visit, self.c_scale)


def run_case(case, m, sims, draws, c_visit=C_VISIT, c_scale=C_SCALE, full=True):
    """gumbel_oracle.run_case with Search above: per search its dict plus in_margins, net_value (the root's) and, for the
    position under the played move, child_state, child_stats and child_value (None where that position is terminal and so
    not in the tree).  "ban": the ban is the move an unbanned search of the same kind plays."""
    def row(s, state, no_act):
        r = go.case_row(s, state, no_act)
        child = xo.step(state, r["best"])
        r.update(in_margins=list(s.in_margins), net_value=s.net_value(state), child_state=child,
                 child_stats=s.node_stats(child), child_value=s.net_value(child))
        return r
    return sm.walk_case(case, lambda: Search(sm.play_cfg(sims), case["salt"], 0.0, m, c_visit, c_scale, draws, full), row)


def gumbel_selfplay_game(cfg, salt, seed, game_id, slot, m, c_visit=C_VISIT, c_scale=C_SCALE, init_state=None, full=True):
    """gumbel_oracle.gumbel_selfplay_game played by Search above, so the plies' targets are the full-mode ones.  The
    result gains `in_margins`, every margin below the root of the whole game, and `margins` / `best_margins`, the root's."""
    log = dict(in_margins=[], margins=[], best_margins=[])

    class Player(Search):
        def __init__(self, *a, **kw):
            super().__init__(*a, full=full, **kw)

        def search(self, state, no_act=None, increase_temp=False):
            ran = super().search(state, no_act, increase_temp)
            log["in_margins"] += self.in_margins
            log["margins"] += self.margins
            return ran

        def played(self, state, no_act=None):
            mv, margin = super().played(state, no_act)
            log["best_margins"].append(margin)
            return mv, margin

    out = go.gumbel_selfplay_game(cfg, salt, seed, game_id, slot, m, c_visit, c_scale, init_state, player=Player)
    out.update(log)
    return out
