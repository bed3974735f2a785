"""The reference's search restated in Python, once: the model every feature oracle of tests/ subclasses.  oracle/xq_mcts.c
is the C restatement; this one -- for search_threads = 1 and noise_eps = 0 only -- runs over oracle.xq_oracle's rule
functions and stub_net.hash_stub_numpy and has the seams the features need: a node class, two hooks in the simulation, a
skip mask in the selection, the ply's budget as a method.

The search follows SURVEY A.6 line by line (agent/player.py; the line numbers are the reference's):
  * the tree is a dict keyed by state, so a later call on a position of the subtree reuses it (:153-158);
  * expansion sets sum_n = 1 (:213), every selection through a node adds 1 (:246), sum_n is read before that;
  * priors: float32 sum in legal-move order, float32 quotient (:272-284), spread at the node's first selection;
  * PUCT in float64; at the root (1 - eps) * p is a float32 product, elsewhere float32(c_puct) * p is (:286-320);
  * virtual loss on the way down (:245-252), 1 - vl and v + vl on the way up, the sign alternating (:340-373);
  * a terminal position is worth done.v * 2 (:206), a position repeated on the path -1 / +1 / 0 (:223-236);
  * the first edge with q > 1 - 1e-7 is taken at once (:309-311), otherwise `>=` keeps the LAST maximum (:312-314);
  * banned moves are skipped at the root (:298-300); bans, increase_temp or done == sims reset the reuse (:156-158).
With one search thread a simulation is backed up before the next starts: no parked simulations, no deferred results.

tests/test_forced_playouts_cpu.py pins Search(k = 0) to xo.Player bit for bit before anything else is trusted.  The
positions the feature tests share, and the walk over a case's searches, are at the end."""
import json
import math
import os

import numpy as np

import stub_net
from oracle import xq_oracle as xo

BANNED = 0x8000
INF = float("inf")
_LABEL = None


def _label(mv):
    global _LABEL
    if _LABEL is None:
        _LABEL = {s: i for i, s in enumerate(xo.labels())}
    return _LABEL[mv]


def banned_labels(labels, no_act):
    """A copy of node_stats' labels with BANNED (0x8000) set on the moves of `no_act`."""
    lab = labels.copy()
    for i, l in enumerate(lab):
        if xo.label_str(int(l)) in (no_act or ()):
            lab[i] |= BANNED
    return lab


class Node:
    __slots__ = ("state", "v", "moves", "labels", "n", "w", "p", "pending", "sum_n")

    def __init__(self, state):
        self.state = state
        self.v = None                   # the network's float32 value of the position, from its mover's view
        self.moves = xo.get_legal_moves(state)
        self.labels = [_label(m) for m in self.moves]
        self.n = [0] * len(self.moves)
        self.w = [0.0] * len(self.moves)
        self.p = None                   # float32 priors, set by the first selection (spread)
        self.pending = None             # the network's policy row until then
        self.sum_n = 1                  # :213

    def spread(self):                   # :272-284
        mp = [np.float32(self.pending[l]) for l in self.labels]
        all_p = None
        for x in mp:
            all_p = x if all_p is None else np.float32(all_p + x)
        if all_p is None or all_p == np.float32(0.0):
            all_p = np.float32(1.0)
        self.p = [np.float32(x / all_p) for x in mp]
        self.pending = None


class Search:
    """One CChessPlayer with search_threads = 1, noise_eps = 0 and the hash stub of `salt` as its network.
    cfg: xo.play_cfg(...).  k: forced playouts (0 = the reference's search).  forced_picks counts the selections that
    took a forced edge; sims, expansions, terminal_sims, repetition_sims count what their names say."""
    node_cls = Node

    def __init__(self, cfg, salt, k=0.0):
        if cfg.search_threads != 1 or cfg.noise_eps != 0.0:
            raise ValueError("the Python search restates search_threads = 1, noise_eps = 0 only")
        self.cfg, self.salt, self.k = cfg, salt, float(k)
        self.tree = {}
        self.root = None
        self.no_act = ()
        self.forced_picks = self.sims = self.expansions = self.terminal_sims = self.repetition_sims = 0

    def _banned(self, node, is_root):
        return [is_root and mv in self.no_act for mv in node.moves]

    def _select(self, node, is_root):
        """(edge, whether it was forced), -1 without an edge: what a feature overrides."""
        return self._puct(node, is_root, self._banned(node, is_root) if is_root and self.no_act else None)

    # ---- select_action_q_and_u, :262-320 ----
    def _puct(self, node, is_root, skip=None):
        """The reference's rule over the edges that the mask `skip` leaves; the root's bans (:298-300) are such a mask."""
        cfg = self.cfg
        xx = math.sqrt(float(node.sum_n + 1))                  # sum_n before this simulation's increment
        if node.pending is not None:
            node.spread()
        best, best_score, best_forced = -1, -99999999.0, False
        for i in range(len(node.moves)):
            if skip is not None and skip[i]:
                continue
            n = node.n[i]
            q = node.w[i] / float(n) if n else 0.0
            forced = False
            if is_root:
                a = np.float32(np.float32(1.0 - cfg.noise_eps) * node.p[i])      # float32 product (:304), eps = 0
                p_ = float(a)
                u = cfg.c_puct * p_ * xx / float(1 + n)
                if self.k > 0.0:
                    forced = n > 0 and float(n) * float(n) < self.k * p_ * float(node.sum_n)
            else:
                a = np.float32(np.float32(cfg.c_puct) * node.p[i])
                u = float(a) * xx / float(1 + n)
            score = q + u
            if q > (1.0 - 1e-7):                               # :309-311
                return i, False
            if not score >= -99999999.0:                       # rejected: never the best, never forced
                continue
            if forced:
                score = INF
            if score >= best_score:                            # :312-314
                best, best_score, best_forced = i, score, forced
        return best, best_forced

    # ---- update_tree, :340-373 ----
    def _backup(self, path, v):
        vl = self.cfg.virtual_loss
        for node, e in reversed(path):
            v = -v
            node.n[e] += 1 - vl
            node.w[e] = node.w[e] + (v + float(vl))
        self.sims += 1

    # ---- the two hooks of the simulation ----
    def _terminal(self, path, value):
        """The descent stepped onto a terminal position worth `value` (done()'s) to its mover, :204-208."""
        self._backup(path, float(value * 2))

    def _arrive(self, node, path):
        """The descent stands on an existing node that is no repetition; True ends it here (the hook has backed up)."""
        return False

    # ---- MCTS_search, :198-260 ----
    def _simulate(self):
        vl = self.cfg.virtual_loss
        state, path, seen = self.root, [], []
        while True:
            d = xo.done(state)
            if d[0]:                                           # :204-208
                self.terminal_sims += 1
                return self._terminal(path, d[1])
            node = self.tree.get(state)
            if node is None:                                   # :211-221
                node = self.tree[state] = self.node_cls(state)
                self.expansions += 1
                pol, val = stub_net.hash_stub_numpy(xo.state_to_planes(state)[None], self.salt)
                node.pending = pol[0]
                node.v = np.float32(val[0])
                return self._backup(path, float(val[0]))
            if state in seen:                                  # :223-236, state in history[:-1]
                mv = node.moves[path[seen.index(state)][1]]
                if xo.will_check_or_catch(state, mv):
                    v = -1.0
                elif xo.be_catched(state, mv):
                    v = 1.0
                else:
                    v = 0.0
                self.repetition_sims += 1
                return self._backup(path, v)
            if self._arrive(node, path):
                return
            e, forced = self._select(node, state == self.root)  # :243, :266
            if e < 0:
                return self._backup(path, 0.0)
            self.forced_picks += forced
            node.sum_n += 1                                    # :245-252
            node.n[e] += vl
            node.w[e] = node.w[e] - float(vl)
            path.append((node, e))
            seen.append(state)
            state = xo.step(state, node.moves[e])

    # ---- CChessPlayer.action up to calc_policy, :145-174 ----
    def begin_ply(self, state, no_act=None, increase_temp=False):
        """Sets root and no_act; returns the ply's budget: what the reused tree leaves of simulation_num_per_move."""
        sims = self.cfg.simulation_num_per_move
        self.root, self.no_act = state, tuple(no_act or ())
        done_n = self.tree[state].sum_n if state in self.tree else 0       # :153-155
        if self.no_act or increase_temp or done_n == sims:                 # :156-158
            done_n = 0
        return max(0, sims - done_n)

    def search(self, state, no_act=None, increase_temp=False):
        """Returns the number of simulations run."""
        budget = self.begin_ply(state, no_act, increase_temp)
        for _ in range(budget):
            self._simulate()
        return budget

    def node_stats(self, state):
        """What xo.Player.node_stats returns: dict(moves, n, w, p, sum_n), moves as labels in edge order."""
        node = self.tree.get(state)
        if node is None:
            return None
        if node.pending is not None:
            node.spread()
        p = node.p if node.p is not None else [np.float32(0.0)] * len(node.moves)
        return dict(moves=np.array(node.labels, dtype=np.uint16), n=np.array(node.n, dtype=np.int32),
                    w=np.array(node.w, dtype=np.float64), p=np.array(p, dtype=np.float32), sum_n=node.sum_n)

    def targets(self, state, no_act=None):
        """(pruned counts in edge order, raw_total) of `state` as a root with the bans `no_act`: what
        cz_search_root_targets reports and a PRUNED visit entry holds."""
        from forced_playouts_oracle import prune                # (the feature's arithmetic; that module imports this one)
        st = self.node_stats(state)
        return prune(banned_labels(st["moves"], no_act), st["n"], st["w"], st["p"], self.cfg.c_puct, self.k)

    def best_move(self, state, no_act=None):
        """The move played at tau = 0: greatest raw count among the non-banned edges, first in label order."""
        st = self.node_stats(state)
        cand = [(-int(n), int(l)) for l, n in zip(st["moves"], st["n"]) if xo.label_str(int(l)) not in (no_act or ())]
        return xo.label_str(min(cand)[1])


# ---- the positions of the CPU and GPU tests ---------------------------------------------------------------------------
SIMS = 200
_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (index into tests/golden/positions_1k.json, None = INIT_STATE, or a state -- the last case, an ADDITION to INIT_STATE and
# the seven positions of the file; stub salt; what is special).  The salts were chosen
# on the CPU so that at k = 2 most positions see forced picks and pruned visits (test_forced_playouts_cpu.py asserts it:
# a condition on these inputs, not a measurement).
_CASES = [
    (None, 1, None),
    (100, 2, None),
    (250, 3, "ban"),            # the move an unbanned search plays is banned
    (400, 4, "reuse"),          # searched, then the position after its best move is searched by the same player
    (550, 5, None),
    (700, 6, None),
    (850, 7, None),
    (625, 9, None),             # 62 moves, the widest roots of the file
    ('3s5/9/9/2K3K2/R7R/1C5C1/P1P1P1P1P/9/9/4S4', 8, None),     # more than 64 moves: both halves of the root's edges
]


def play_cfg(sims=SIMS, **kw):
    return xo.play_cfg(simulation_num_per_move=sims, search_threads=1, noise_eps=0.0, tau_decay_rate=0.0, **kw)


def cases():
    """list of dict(name, salt, state, kind): kind None, "ban" or "reuse"."""
    with open(os.path.join(_GOLD, "positions_1k.json")) as f:
        pos = json.load(f)["positions"]
    out = []
    for idx, salt, kind in _CASES:
        state = xo.INIT_STATE if idx is None else (idx if isinstance(idx, str) else pos[idx]["state"])
        name = "init" if idx is None else ("wide" if isinstance(idx, str) else f"pos{idx}")
        out.append(dict(name=name, salt=salt, state=state, kind=kind))
    return out


def walk_case(case, new, row, ban=None):
    """The searches of one case by one player new(): the list of row(search, state, no_act) -- a dict with the played
    move as `best` --, one per search, two for "reuse" (the position after the first `best`, same player), plus the
    Search object.  "ban" searches with the move `ban` banned: by default what another new() plays there unbanned."""
    no_act = []
    if case["kind"] == "ban":
        if ban is None:
            s0 = new()
            s0.search(case["state"])
            ban = row(s0, case["state"], [])["best"]
        no_act = [ban]
    s = new()
    line = [(case["state"], no_act)]
    out = []
    while line:
        state, no_act = line.pop(0)
        s.search(state, no_act)
        out.append(row(s, state, no_act))
        if case["kind"] == "reuse" and len(out) == 1:
            line.append((xo.step(state, out[0]["best"]), []))
    return out, s


def run_case(case, k, sims=SIMS, search_cls=None):
    """Searches of one case with forced playouts k: list of dict(state, no_act, stats, targets, raw_total, best) plus the
    Search object (counters).  "ban": the ban is the move a k = 0 search of the position plays, so that the ban matters."""
    def row(s, state, no_act):
        t, raw = s.targets(state, no_act)
        return dict(state=state, no_act=no_act, stats=s.node_stats(state), targets=t, raw_total=raw,
                    best=s.best_move(state, no_act))
    return walk_case(case, lambda: (search_cls or Search)(play_cfg(sims), case["salt"], k), row,
                     ban_of(case, sims) if case["kind"] == "ban" else None)


_BANS = {}


def ban_of(case, sims=SIMS):
    key = (case["name"], sims)
    if key not in _BANS:
        s = Search(play_cfg(sims), case["salt"], 0.0)
        s.search(case["state"])
        _BANS[key] = s.best_move(case["state"])
    return _BANS[key]
