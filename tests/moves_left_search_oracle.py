"""The moves-left utility (cz_search_set_moves_left, run.py self / eval --moves-left-slope) restated in Python:
search_model.Search with the rule of include/czero.h written out in the same operation order.

  * a leaf's prediction: the network's raw x becomes k = min(rint(512 * softplus(x)), 16 * 1023) quanta of 1/16 ply (float32,
    stable softplus); a simulation that ends on a terminal position, on a repetition or without an edge has k = 0;
  * backup: from the leaf up with m = k, per level m += 16, the edge's ksum += m, the edge's mn += 1 (integers: exact);
  * selection: K = k_node + sum ksum_j, N = 1 + sum mn_j, Mp = (K / 16) / N; per edge with mn_j > 0 Mj = (ksum_j / 16) / mn_j,
    d = clamp(slope * (Mj - Mp), -cap, cap), a = min(|q|, 1), f = 1.6521 a + (-0.6521)(a a),
    u_m = q > 0 ? -(d f) : (q < 0 ? d f : 0), score = (q + u) + u_m; the rest is the reference's rule.

With slope = 0 it is search_model.Search bit for bit (tests/test_moves_left_search_cpu.py).  Python floats are float64 and
nothing is fused, which is what the device code is compiled to as well."""
import math

import numpy as np

import search_model as sm
import stub_moves_left as sml
from oracle import xq_oracle as xo

INF = sm.INF
QUANTA = 16
SLOPE, CAP = 0.0027, 0.0345                                  # lc0's defaults


class Node(sm.Node):
    __slots__ = ("ksum", "mn", "k")

    def __init__(self, state):
        super().__init__(state)
        self.ksum = [0] * len(self.moves)
        self.mn = [0] * len(self.moves)
        self.k = 0                      # the node's own prediction in quanta


def edge_d(slope, cap, ksum, mn, Mp):
    if mn <= 0:
        return 0.0
    Mj = (float(ksum) / 16.0) / float(mn)
    d = slope * (Mj - Mp)
    return cap if d > cap else (-cap if d < -cap else d)


def utility(d, q):
    aq = abs(q)
    a = aq if aq < 1.0 else 1.0
    f = 1.6521 * a + (-0.6521) * (a * a)
    return -(d * f) if q > 0.0 else (d * f if q < 0.0 else 0.0)


class Search(sm.Search):
    """search_model.Search with the moves-left utility.  net: planes -> (policy, value, x); default the moves-left hash stub
    of `salt`.  on: the option is on (the M records are kept, the score has its third term); slope, cap as the setter's."""
    node_cls = Node

    def __init__(self, cfg, salt, k=0.0, slope=SLOPE, cap=CAP, net=None, on=True):
        super().__init__(cfg, salt, k)
        self.slope, self.cap, self.on = float(slope), float(cap), bool(on)
        self.net = net or (lambda planes: sml.ml_stub_numpy(planes, salt))

    # ---- select_action_q_and_u with u_m ----
    def _puct(self, node, is_root, skip=None):
        cfg = self.cfg
        xx = math.sqrt(float(node.sum_n + 1))
        if node.pending is not None:
            node.spread()
        Mp = 0.0
        if self.on:
            K = node.k + sum(node.ksum)
            N = 1 + sum(node.mn)
            Mp = (float(K) / 16.0) / float(N)
        best, best_score, best_forced = -1, -99999999.0, False
        for i in range(len(node.moves)):
            if skip is not None and skip[i]:
                continue
            n = node.n[i]
            q = node.w[i] / float(n) if n else 0.0
            forced = False
            if is_root:
                a = np.float32(np.float32(1.0 - cfg.noise_eps) * node.p[i])
                p_ = float(a)
                u = cfg.c_puct * p_ * xx / float(1 + n)
                if self.k > 0.0:
                    forced = n > 0 and float(n) * float(n) < self.k * p_ * float(node.sum_n)
            else:
                a = np.float32(np.float32(cfg.c_puct) * node.p[i])
                u = float(a) * xx / float(1 + n)
            score = q + u
            if self.on:
                score = score + utility(edge_d(self.slope, self.cap, node.ksum[i], node.mn[i], Mp), q)
            if q > (1.0 - 1e-7):
                return i, False
            if not score >= -99999999.0:
                continue
            if forced:
                score = INF
            if score >= best_score:
                best, best_score, best_forced = i, score, forced
        return best, best_forced

    # ---- update_tree with m ----
    def _backup_m(self, path, k):
        m = k
        for node, e in reversed(path):
            m += QUANTA
            node.ksum[e] += m
            node.mn[e] += 1

    def _backup(self, path, v, k=0):
        if self.on:
            self._backup_m(path, k)
        super()._backup(path, v)

    # ---- MCTS_search: search_model's text with the network's third output ----
    def _simulate(self):
        vl = self.cfg.virtual_loss
        state, path, seen = self.root, [], []
        while True:
            d = xo.done(state)
            if d[0]:
                self.terminal_sims += 1
                return self._terminal(path, d[1])
            node = self.tree.get(state)
            if node is None:
                node = self.tree[state] = self.node_cls(state)
                self.expansions += 1
                pol, val, x = self.net(xo.state_to_planes(state)[None])
                node.pending = pol[0]
                node.v = np.float32(val[0])
                node.k = int(sml.quanta_of_x(np.asarray(x[:1], dtype=np.float32))[0])
                return self._backup(path, float(val[0]), node.k)
            if state in seen:
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
            e, forced = self._select(node, state == self.root)
            if e < 0:
                return self._backup(path, 0.0)
            self.forced_picks += forced
            node.sum_n += 1
            node.n[e] += vl
            node.w[e] = node.w[e] - float(vl)
            path.append((node, e))
            seen.append(state)
            state = xo.step(state, node.moves[e])

    def node_moves_left(self, state):
        """dict(ksum, mn, k_net) of `state`'s node in edge order, None where it is not in the tree."""
        node = self.tree.get(state)
        if node is None:
            return None
        return dict(ksum=np.array(node.ksum, dtype=np.int64), mn=np.array(node.mn, dtype=np.int32), k_net=node.k)


def run_case(case, slope=SLOPE, cap=CAP, sims=sm.SIMS, on=True, k=0.0, ban=None):
    """search_model.walk_case with this Search: rows dict(state, no_act, stats, ml, best) plus the Search object.  "ban"
    bans what a plain search of the position plays, as search_model.run_case does, unless `ban` names the move."""
    def row(s, state, no_act):
        return dict(state=state, no_act=no_act, stats=s.node_stats(state), ml=s.node_moves_left(state),
                    best=s.best_move(state, no_act))
    if case["kind"] == "ban" and ban is None:
        ban = sm.ban_of(case, sims)
    return sm.walk_case(case, lambda: Search(sm.play_cfg(sims), case["salt"], k, slope, cap, on=on), row, ban)
