"""The lower-confidence-bound move choice (cz_search_set_lcb, run.py self / eval --lcb) restated in Python: search_model.Search
with the V records and the rule of include/czero.h written out in the same operation order.

  * backup: on every edge of the path s2 = s2 + x * x and vn += 1, x the value the backup adds to the edge's W beyond the
    virtual loss; level by level, the product rounded and then the sum;
  * every end that is backed up counts: a network leaf, a terminal position (x = +-2), a repetition, "no edge";
  * the selection is search_model's: n, w and p are the plain search's bit for bit;
  * best_move is lcb_pick on the root's fields; without an eligible edge it is search_model's best_move.

With the option off it is search_model.Search bit for bit (tests/test_lcb_cpu.py).  Python floats and NumPy float64 are IEEE
doubles and nothing is fused, which is what the device code is compiled to as well."""
import numpy as np

import search_model as sm
from oracle import xq_oracle as xo

BANNED = sm.BANNED
Z, RATIO = 2.0, 0.15            # the parameters of the shared tests


class Node(sm.Node):
    __slots__ = ("s2", "vn")

    def __init__(self, state):
        super().__init__(state)
        self.s2 = [0.0] * len(self.moves)
        self.vn = [0] * len(self.moves)


def lcb_pick(labels, n, w, s2, vn, z, ratio):
    """The rule on one node's edges (arrays of one length; labels with BANNED): (lcb float64 array, NaN for an edge that is
    not eligible; the picked edge index, -1 without a non-banned edge).  NumPy float64, every operation on its own."""
    labels = np.asarray(labels, dtype=np.uint16)
    n = np.asarray(n, dtype=np.int32)
    w = np.asarray(w, dtype=np.float64)
    s2 = np.asarray(s2, dtype=np.float64)
    vn = np.asarray(vn, dtype=np.int32)
    z, ratio = np.float64(z), np.float64(ratio)
    lcb = np.full(len(labels), np.nan, dtype=np.float64)
    open_ = (labels & BANNED) == 0
    if not open_.any():
        return lcb, -1
    n_max = np.float64(n[open_].max())
    floor_n = ratio * n_max
    with np.errstate(all="ignore"):
        for j in np.nonzero(open_)[0]:
            if not (vn[j] >= 2 and n[j] > 0 and np.float64(n[j]) >= floor_n):
                continue
            vnj = np.float64(vn[j])
            q = w[j] / np.float64(n[j])
            qq = q * q
            var = s2[j] / vnj - qq
            if var < 0.0:
                var = np.float64(0.0)
            var = var * (vnj / np.float64(vn[j] - 1))
            lcb[j] = q - z * np.sqrt(var / vnj)
    elig = ~np.isnan(lcb)
    cand = np.nonzero(elig)[0] if elig.any() else np.nonzero(open_)[0]
    if elig.any():
        best = lcb[cand].max()
        cand = cand[lcb[cand] == best]
    key = [(-int(n[j]), int(labels[j] & 0x7FFF), int(j)) for j in cand]
    return lcb, min(key)[2]


class Search(sm.Search):
    """search_model.Search with the V records.  z, ratio as the setter's; z = 0 is off: no record is kept and best_move is
    search_model's.  below counts, since the last begin_ply, the simulations that ended below the root."""
    node_cls = Node

    def __init__(self, cfg, salt, k=0.0, z=Z, ratio=RATIO):
        super().__init__(cfg, salt, k)
        self.z, self.ratio = float(z), float(ratio)
        self.below = 0

    @property
    def on(self):
        return self.z > 0.0

    def _backup(self, path, v):
        if self.on:
            x = v
            for node, e in reversed(path):                  # level by level, with update_tree's own sign flips
                x = -x
                node.s2[e] = node.s2[e] + x * x
                node.vn[e] += 1
            self.below += bool(path)
        super()._backup(path, v)

    def begin_ply(self, state, no_act=None, increase_temp=False):
        self.below = 0
        return super().begin_ply(state, no_act, increase_temp)

    def node_values(self, state):
        """dict(s2, vn) of `state`'s node in edge order, None where it is not in the tree."""
        node = self.tree.get(state)
        if node is None:
            return None
        return dict(s2=np.array(node.s2, dtype=np.float64), vn=np.array(node.vn, dtype=np.int32))

    def root_lcb(self, state, no_act=None):
        """(lcb, pick) of `state` as a root with the bans `no_act`: what cz_search_root_lcb reports."""
        st, vr = self.node_stats(state), self.node_values(state)
        return lcb_pick(sm.banned_labels(st["moves"], no_act), st["n"], st["w"], vr["s2"], vr["vn"], self.z, self.ratio)

    def most_visited(self, state, no_act=None):
        return super().best_move(state, no_act)

    def best_move(self, state, no_act=None):
        if not self.on:
            return super().best_move(state, no_act)
        st = self.node_stats(state)
        _, pick = self.root_lcb(state, no_act)
        return xo.label_str(int(st["moves"][pick]))


def run_case(case, z=Z, ratio=RATIO, sims=sm.SIMS, k=0.0, ban=None):
    """search_model.walk_case with this Search: rows dict(state, no_act, stats, values, lcb, pick, best, most, below) plus the
    Search object.  "ban" bans what a plain search of the position plays, as search_model.run_case does."""
    def row(s, state, no_act):
        lcb, pick = s.root_lcb(state, no_act) if s.on else (None, None)
        return dict(state=state, no_act=no_act, stats=s.node_stats(state), values=s.node_values(state), lcb=lcb, pick=pick,
                    best=s.best_move(state, no_act), most=s.most_visited(state, no_act), below=s.below)
    if case["kind"] == "ban" and ban is None:
        ban = sm.ban_of(case, sims)
    return sm.walk_case(case, lambda: Search(sm.play_cfg(sims), case["salt"], k, z, ratio), row, ban)


def play_line(state, plies, sims, salt, z=Z, ratio=RATIO):
    """A tau = 0 game loop with tree reuse: list of dict(state, ran, stats, values, best) per ply, plus the Search."""
    s = Search(sm.play_cfg(sims), salt, 0.0, z, ratio)
    out = []
    for _ in range(plies):
        ran = s.search(state)
        best = s.best_move(state)
        out.append(dict(state=state, ran=ran, stats=s.node_stats(state), values=s.node_values(state), best=best,
                        most=s.most_visited(state)))
        state = xo.step(state, best)
    return out, s


# ---- the hand-made grid of the rule (tests/test_lcb_cpu.py, tests/test_gpu_lcb.py) ---------------------------------------------
def _row(name, z, ratio, edges, expect):
    """edges: list of (label, n, w, s2, vn); expect: the edge index the rule must pick (worked out by hand)."""
    return dict(name=name, z=z, ratio=ratio, edges=edges, expect=expect)


def _samples(xs):
    """(n, w, s2, vn) of an edge whose backed-up values were xs, accumulated in order."""
    w = s2 = 0.0
    for x in xs:
        w = w + x
        s2 = s2 + x * x
    return len(xs), w, s2, len(xs)


def grid():
    rows = []
    a = _samples([0.5, 0.25, 0.75, 0.5])
    rows.append(_row("identical records: the lowest label", 2.0, 0.15, [(70, *a), (30, *a), (50, *a)], 1))
    # equal lcb, different n: q = 0.5 and zero variance on both (all samples equal, binary fractions: exact)
    rows.append(_row("equal lcb: the greater n", 2.0, 0.15, [(10, *_samples([0.5] * 3)), (20, *_samples([0.5] * 5))], 1))
    rows.append(_row("every vn < 2: the most visited, lowest label", 2.0, 0.0,
                     [(40, 1, 0.9, 0.81, 1), (30, 1, 0.1, 0.01, 1), (20, 0, 0.0, 0.0, 0), (35, 1, 0.5, 0.25, 1)], 1))
    good, poor = _samples([0.9, 0.9, 0.8, 0.9]), _samples([0.1, -0.2, 0.0, 0.1, 0.2])
    rows.append(_row("the best edge banned", 2.0, 0.15, [(5 | BANNED, *good), (6, *poor), (7, *_samples([0.3, 0.2]))], 2))
    # all samples equal: s2 / vn - q * q is not 0 in floating point; seven times 0.7 gives -2.2e-16, which clamps to 0, seven
    # times 0.1 gives +1.7e-18, which does not
    rows.append(_row("all samples equal: the clamp", 2.0, 0.15, [(1, *_samples([0.7] * 7)), (2, *_samples([0.1] * 7))], 0))
    rows.append(_row("n == R * n_max exactly", 0.5, 0.25,
                     [(1, *_samples([0.1] * 8)), (2, *_samples([0.9, 0.9])), (3, 1, 0.95, 0.9025, 1)], 1))
    rows.append(_row("z = 0: the greatest q", 0.0, 0.15,
                     [(1, *_samples([0.5, -0.5, 0.6, 0.2])), (2, *_samples([0.3, 0.3, 0.31])), (3, *_samples([0.9, -0.9]))], 1))
    rows.append(_row("a terminal edge", 2.0, 0.15, [(1, *_samples([2.0, 2.0, 2.0])), (2, *_samples([0.9, 0.8, 0.9, 0.9]))], 0))
    rows.append(_row("no edge", 2.0, 0.15, [], -1))
    rng = np.random.RandomState(20261021)
    for nm, win in ((65, 64), (128, 100)):
        edges = []
        for j in range(nm):
            xs = list(np.round(rng.uniform(-0.5, 0.2, size=4 + j % 3), 3))
            edges.append((1000 - j, *_samples(xs)))
        edges[win] = (1000 - win, *_samples([0.7, 0.71, 0.69, 0.7, 0.7]))
        rows.append(_row(f"{nm} edges, the winner in the second half", 2.0, 0.15, edges, win))
    rows.append(_row("NaN in w of an ineligible edge", 2.0, 0.15,
                     [(1, 1, float("nan"), 0.5, 1), (2, *_samples([0.2, 0.3, 0.1])), (3 | BANNED, 9, float("nan"), 1.0, 9)], 1))
    return rows


def grid_arrays(rows):
    """The grid as cz_lcb_pick takes it: labels uint16, n int32, w float64, s2 float64, vn int32 [rows, 128], n_edges uint8."""
    R = len(rows)
    labels = np.zeros((R, 128), dtype=np.uint16)
    n = np.zeros((R, 128), dtype=np.int32)
    w = np.zeros((R, 128), dtype=np.float64)
    s2 = np.zeros((R, 128), dtype=np.float64)
    vn = np.zeros((R, 128), dtype=np.int32)
    ne = np.zeros((R,), dtype=np.uint8)
    for r, row in enumerate(rows):
        ne[r] = len(row["edges"])
        for j, (lab, nj, wj, sj, vj) in enumerate(row["edges"]):
            labels[r, j], n[r, j], w[r, j], s2[r, j], vn[r, j] = lab, nj, wj, sj, vj
    return labels, n, w, s2, vn, ne
