"""The draw average (cz_search_set_draw, run.py self / eval --draw-score) restated in Python: search_model.Search with the
rule of include/czero.h written out in the same operation order.

  * a leaf's draw probability d = wdl[1] (float32) becomes dq = rint(d * 2^20) quanta; NaN or d < 0 gives 0, d >= 1 gives 2^20;
  * a repetition worth 0 is a draw, dq = 2^20; a terminal position, a repetition worth +-1 and "no edge" have dq = 0;
  * backup: on every edge of the path dsum += dq, dn += 1 (integers: exact; no sign);
  * selection at a node `depth` edges below the ply's root: sigma = -score at odd depth, score at even; per edge
    dbar = (dsum / 2^20) / dn where dn > 0, otherwise 0; edge score = (q + u) + sigma * dbar; the rest is the reference's rule.

With the option off it is search_model.Search bit for bit (tests/test_draw_search_cpu.py).  Python floats are float64 and
nothing is fused, which is what the device code is compiled to as well."""
import math

import numpy as np

import search_model as sm
import stub_draw as sd
from oracle import xq_oracle as xo

INF = sm.INF
QUANTA = sd.QUANTA


class Node(sm.Node):
    __slots__ = ("dsum", "dn", "dq")

    def __init__(self, state):
        super().__init__(state)
        self.dsum = [0] * len(self.moves)
        self.dn = [0] * len(self.moves)
        self.dq = 0                     # the node's own draw probability in quanta


def dbar(dsum, dn):
    return (float(dsum) / 1048576.0) / float(dn) if dn > 0 else 0.0


class Search(sm.Search):
    """search_model.Search with the draw average.  net: planes -> (policy, value, wdl [n, 3]); default the draw hash stub of
    `salt`.  on: the option is on (the D records are kept, the score has its third term); score as the setter's.
    rep0_sims / rep1_sims count the repetitions worth 0 / +-1; dq_below counts, since the last begin_ply, the dq of every
    simulation that ended below the root."""
    node_cls = Node

    def __init__(self, cfg, salt, k=0.0, score=0.0, net=None, on=True):
        super().__init__(cfg, salt, k)
        self.score, self.on = float(score), bool(on)
        self.net = net or (lambda planes: sd.draw_stub_numpy(planes, salt))
        self.rep0_sims = self.rep1_sims = self.dq_below = 0
        self._depth = 0

    # ---- select_action_q_and_u with sigma * dbar ----
    def _puct(self, node, is_root, skip=None):
        cfg = self.cfg
        xx = math.sqrt(float(node.sum_n + 1))
        if node.pending is not None:
            node.spread()
        sigma = -self.score if (self._depth & 1) else self.score
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
                score = score + sigma * dbar(node.dsum[i], node.dn[i])
            if q > (1.0 - 1e-7):
                return i, False
            if not score >= -99999999.0:
                continue
            if forced:
                score = INF
            if score >= best_score:
                best, best_score, best_forced = i, score, forced
        return best, best_forced

    # ---- update_tree with d ----
    def _backup(self, path, v, dq=0):
        if self.on:
            for node, e in path:
                node.dsum[e] += dq
                node.dn[e] += 1
            if path:
                self.dq_below += dq
        super()._backup(path, v)

    def begin_ply(self, state, no_act=None, increase_temp=False):
        self.dq_below = 0
        return super().begin_ply(state, no_act, increase_temp)

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
                pol, val, wdl = self.net(xo.state_to_planes(state)[None])
                node.pending = pol[0]
                node.v = np.float32(val[0])
                node.dq = int(sd.draw_quanta(np.asarray(wdl, dtype=np.float32)[:1, 1])[0])
                return self._backup(path, float(val[0]), node.dq)
            if state in seen:
                mv = node.moves[path[seen.index(state)][1]]
                if xo.will_check_or_catch(state, mv):
                    v = -1.0
                elif xo.be_catched(state, mv):
                    v = 1.0
                else:
                    v = 0.0
                self.repetition_sims += 1
                self.rep0_sims += v == 0.0
                self.rep1_sims += v != 0.0
                return self._backup(path, v, QUANTA if v == 0.0 else 0)
            if self._arrive(node, path):
                return
            self._depth = len(path)
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

    def node_draws(self, state):
        """dict(dsum, dn, dq_net) of `state`'s node in edge order, None where it is not in the tree."""
        node = self.tree.get(state)
        if node is None:
            return None
        return dict(dsum=np.array(node.dsum, dtype=np.int64), dn=np.array(node.dn, dtype=np.int32), dq_net=node.dq)


def run_case(case, score=0.0, sims=sm.SIMS, on=True, k=0.0, ban=None):
    """search_model.walk_case with this Search: rows dict(state, no_act, stats, draws, best, dq_below) plus the Search object.
    "ban" bans what a plain search of the position plays, as search_model.run_case does, unless `ban` names the move."""
    def row(s, state, no_act):
        return dict(state=state, no_act=no_act, stats=s.node_stats(state), draws=s.node_draws(state),
                    best=s.best_move(state, no_act), dq_below=s.dq_below)
    if case["kind"] == "ban" and ban is None:
        ban = sm.ban_of(case, sims)
    return sm.walk_case(case, lambda: Search(sm.play_cfg(sims), case["salt"], k, score, on=on), row, ban)
