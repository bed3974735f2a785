"""The MCTS solver (cz_search_set_solver, run.py self / eval --solver) restated in Python: search_model.Search
-- the reference's search for one search thread without root noise -- with the definitions of include/czero.h ("MCTS
solver") in it, and a depth-limited minimax over the oracle's rule functions as the independent yardstick of soundness.

A position has a status from its mover's view: OPEN, WIN(d) or LOSS(d), d plies to a terminal position along a line the tree
holds, saturating at 255.  A terminal child done() == (True, +1) counts as WIN(1), (True, -1) as LOSS(0).  An edge carries
the status of its child as last seen at a backup over it (terminal children by their code); it is winning if that is LOSS
and losing if it is WIN.  A simulation that ends on a terminal child or on a proven node marks the last edge of its path
when it is backed up; the node above becomes WIN(1 + min d of its winning edges) or, all of its nm > 0 edges losing,
LOSS(1 + max d); a first proof is final; a node that became proven marks the edge above it, and so on until a node stays
OPEN.  A descent that steps onto a proven node at depth >= 1 ends there, after the repetition test, worth +2 / -2 from
that node's mover.  Selection: the winning non-banned edge of least d (first in edge order) at once; else the reference's
rule over the non-banned edges that are not losing; all of them losing: over all non-banned edges.  A root that is LOSS, or
WIN with a non-banned winning edge, is decided: no simulation starts, and at such a WIN root the played move is that edge.

tests/test_solver_cpu.py pins Search(solver=False) to fo.Search bit for bit before anything else is trusted."""
import json
import os

import search_model as sm
from oracle import xq_oracle as xo

OPEN, WIN, LOSS = 0, 1, 2
DIST_MAX = 255
SALT = 3
_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def derive(marks, dists):
    """The status a node with these edges takes: marks[j] in (OPEN, WIN, LOSS) is the mark of edge j (the status of its
    child), dists[j] the child's d.  Returns (status, d).  Bans play no part."""
    win = [d for m, d in zip(marks, dists) if m == LOSS]
    if win:
        return WIN, min(DIST_MAX, 1 + min(win))
    if marks and all(m == WIN for m in marks):
        return LOSS, min(DIST_MAX, 1 + max(dists))
    return OPEN, 0


def winning_edge(marks, dists, banned):
    """Rule 1: the non-banned winning edge of least d, the first in edge order on a tie; -1 without one."""
    cand = [(dists[j], j) for j in range(len(marks)) if marks[j] == LOSS and not banned[j]]
    return min(cand)[1] if cand else -1


class _Node(sm.Node):
    __slots__ = ("term", "mark", "status", "dist")

    def __init__(self, state):
        super().__init__(state)
        self.term = [OPEN] * len(self.moves)    # WIN / LOSS: the child is terminal (CHILD_TERM_WIN / CHILD_TERM_LOSS)
        self.mark = [OPEN] * len(self.moves)    # the edge mark of a child that is a node
        self.status, self.dist = OPEN, 0


class Search(sm.Search):
    """search_model.Search(k = 0) with the solver.  solver=False: every solver rule is off, the search is that one.
    proven_sims counts the descents that ended on a proven node."""
    node_cls = _Node

    def __init__(self, cfg, salt, k=0.0, solver=True):
        if k:
            raise ValueError("the solver is not combined with forced playouts")
        super().__init__(cfg, salt, 0.0)
        self.solver = bool(solver)
        self.proven_sims = 0

    # ---- what an edge says about its child ----
    def edge_mark(self, node, e):
        return node.term[e] or node.mark[e]

    def edge_dist(self, node, e):
        if node.term[e]:
            return 1 if node.term[e] == WIN else 0
        if node.mark[e]:
            return self.tree[xo.step(node.state, node.moves[e])].dist
        return 0

    def rule1(self, node, is_root=True):
        nm = len(node.moves)
        return winning_edge([self.edge_mark(node, j) for j in range(nm)], [self.edge_dist(node, j) for j in range(nm)],
                            self._banned(node, is_root))

    # ---- select_action_q_and_u with the three rules ----
    def _select(self, node, is_root):
        if not self.solver:
            return super()._select(node, is_root)
        e = self.rule1(node, is_root)
        if e >= 0:
            return e, False
        banned = self._banned(node, is_root)
        losing = [self.edge_mark(node, j) == WIN for j in range(len(node.moves))]
        all_losing = all(l for l, b in zip(losing, banned) if not b)
        skip = [b or (l and not all_losing) for l, b in zip(losing, banned)]
        return self._puct(node, is_root, skip)

    # ---- marking and deriving, after the backup of a +-2 ----
    def _walk(self, path, status):
        """path: the simulation's (node, edge) list; status: that of the position it ended on."""
        for node, e in reversed(path):
            if not node.term[e]:
                node.mark[e] = status
            if node.status != OPEN:
                return
            nm = len(node.moves)
            st, d = derive([self.edge_mark(node, j) for j in range(nm)], [self.edge_dist(node, j) for j in range(nm)])
            if st == OPEN:
                return
            node.status, node.dist = st, d
            status = st

    # ---- the simulation's hooks: the terminal codes, the arrival and the walk ----
    def _terminal(self, path, value):
        status = WIN if value > 0 else LOSS
        if path:
            path[-1][0].term[path[-1][1]] = status
        super()._terminal(path, value)
        if self.solver and path:
            self._walk(path, status)

    def _arrive(self, node, path):
        if not (self.solver and path and node.status != OPEN):
            return False
        self.proven_sims += 1
        self._backup(path, 2.0 if node.status == WIN else -2.0)
        self._walk(path, node.status)
        return True

    # ---- the decided root ----
    def decided(self):
        node = self.tree.get(self.root)
        if not self.solver or node is None:
            return False
        return node.status == LOSS or (node.status == WIN and self.rule1(node) >= 0)

    def search(self, state, no_act=None, increase_temp=False):
        """The model's search, stopping at a decided root."""
        ran = 0
        for _ in range(self.begin_ply(state, no_act, increase_temp)):
            if self.decided():
                break
            self._simulate()
            ran += 1
        return ran

    # ---- reports ----
    def proof(self, state):
        """What cz_search_node_proof reports of `state`: dict(status, dist, mark, mark_dist), the last two per edge; None
        for a position the tree does not hold."""
        node = self.tree.get(state)
        if node is None:
            return None
        nm = len(node.moves)
        return dict(status=node.status, dist=node.dist, mark=[self.edge_mark(node, j) for j in range(nm)],
                    mark_dist=[self.edge_dist(node, j) for j in range(nm)])

    def play(self, state, no_act=None):
        """The move choice at tau = 0 without resignation: rule 1's edge at a WIN root that has one, else best_move."""
        node = self.tree.get(state)
        if self.solver and node is not None and node.status == WIN:
            self.root, self.no_act = state, tuple(no_act or ())
            e = self.rule1(node)
            if e >= 0:
                return node.moves[e]
        return self.best_move(state, no_act)

    def play_line(self, state, max_plies=64, bans=None):
        """Search and play from `state` until done(): list of dict(state, no_act, ran, move, proof, stats).  bans:
        {ply: [moves]} banned at that ply."""
        out = []
        for ply in range(max_plies):
            if xo.done(state)[0]:
                break
            no_act = list((bans or {}).get(ply, []))
            ran = self.search(state, no_act)
            mv = self.play(state, no_act)
            out.append(dict(state=state, no_act=no_act, ran=ran, move=mv, proof=self.proof(state),
                            stats=self.node_stats(state)))
            state = xo.step(state, mv)
        return out, state


# ---- the independent yardstick -------------------------------------------------------------------------------------------
def minimax(state, depth, _memo=None):
    """The game-theoretic status of `state` within `depth` plies, from its mover's view, over done / get_legal_moves / step
    alone: WIN (the mover forces a terminal win), LOSS (every line loses) or OPEN (neither within the depth)."""
    memo = {} if _memo is None else _memo
    key = (state, depth)
    if key in memo:
        return memo[key]
    d = xo.done(state)
    if d[0]:
        res = WIN if d[1] > 0 else LOSS
    elif depth == 0:
        res = OPEN
    else:
        moves = xo.get_legal_moves(state)
        kids = [minimax(xo.step(state, m), depth - 1, memo) for m in moves]
        if any(k == LOSS for k in kids):
            res = WIN
        elif kids and all(k == WIN for k in kids):
            res = LOSS
        else:
            res = OPEN
    memo[key] = res
    return res


# ---- the fixtures ------------------------------------------------------------------------------------------------------------
def positions():
    """tests/golden/solver_positions.json: list of dict(name, state, sims, ...)."""
    with open(os.path.join(_GOLD, "solver_positions.json")) as f:
        return json.load(f)["positions"]


def play_cfg(sims):
    return sm.play_cfg(sims)


def proven_nodes(search, max_dist=5):
    """(state, status, dist) of every proven node of the tree with dist <= max_dist."""
    return [(s, n.status, n.dist) for s, n in search.tree.items() if n.status != OPEN and n.dist <= max_dist]
