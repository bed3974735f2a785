"""The c_puct schedule and the policy temperature (cz_search_set_cpuct_schedule, cz_search_set_policy_temperature; run.py
self / eval / reanalyse --cpuct-factor F --cpuct-base B --policy-temp T) restated in Python: search_model.Search -- the
reference's search for one search thread without root noise -- with

    c(sum_n) = c_puct + F * log((1 + sum_n + B) / B)            float64, sum_n as the selection reads it

in place of the constant of its PUCT rule (at the root c * p_ * xx / (1 + n) in that order; below it float32(c) * p is the
float32 product), and a node class whose prior spreading takes a temperature, p_j proportional to p_j ** (1 / T).

With F = 0 and T = 1 it is search_model.Search bit for bit (tests/test_puct_schedule_cpu.py).  Schedule is a mix-in, so the
solver's model composes with it: SolverSearch below.  cases() adds a tenth case to the nine shared ones: the wide position
under a salt at which F = 2, B = 50 changes its counts (under salt 8 a proven win takes every visit)."""
import math

import numpy as np

import forced_playouts_oracle as fo
import search_model as sm
import solver_oracle as so
from search_model import SIMS, ban_of, play_cfg, walk_case       # noqa: F401 (re-exports)

F, B = 2.0, 50.0                    # the schedule of the tests: strong enough to move the counts at 200 simulations
WIDE = '3s5/9/9/2K3K2/R7R/1C5C1/P1P1P1P1P/9/9/4S4'
WIDE_SALT = 14                      # chosen on the CPU: test_puct_schedule_cpu.py asserts that the schedule moves this case


def cpuct(c_puct, factor, base, sum_n):
    """c(sum_n), each operation one float64 operation in the order written."""
    return float(c_puct) + float(factor) * math.log((1.0 + float(sum_n) + float(base)) / float(base))


def _spread(self):
    """Node.spread with the temperature of the class: the row's entries to the power 1 / T (float64 log and exp, rounded to
    float32 once), then the reference's float32 sum and quotients."""
    if self.T != 1.0:
        row = np.asarray(self.pending, dtype=np.float64)
        with np.errstate(divide="ignore"):
            self.pending = np.exp(np.log(row) / self.T).astype(np.float32)
    super(type(self), self).spread()


def node_class(base, T):
    cls = type("Node", (base,), {"__slots__": (), "T": float(T)})
    cls.spread = _spread
    return cls


class Schedule:
    """Mix-in over a search_model.Search: the schedule in _puct, the temperature in the node class."""

    def set_schedule(self, factor=0.0, base=19652.0, T=1.0):
        self.factor, self.base, self.T = float(factor), float(base), float(T)
        if T != 1.0:
            self.node_cls = node_class(type(self).node_cls, T)
        return self

    def c_at(self, sum_n):
        return cpuct(self.cfg.c_puct, self.factor, self.base, sum_n)

    def _puct(self, node, is_root, skip=None):
        cfg = self.cfg
        xx = math.sqrt(float(node.sum_n + 1))                  # sum_n before this simulation's increment
        c = cfg.c_puct + self.factor * math.log((1.0 + node.sum_n + self.base) / self.base)
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
                a = np.float32(np.float32(1.0 - cfg.noise_eps) * node.p[i])
                p_ = float(a)
                u = c * p_ * xx / float(1 + n)
                if self.k > 0.0:
                    forced = n > 0 and float(n) * float(n) < self.k * p_ * float(node.sum_n)
            else:
                a = np.float32(np.float32(c) * node.p[i])
                u = float(a) * xx / float(1 + n)
            score = q + u
            if q > (1.0 - 1e-7):
                return i, False
            if not score >= -99999999.0:
                continue
            if forced:
                score = sm.INF
            if score >= best_score:
                best, best_score, best_forced = i, score, forced
        return best, best_forced

    def targets(self, state, no_act=None):
        """Search.targets with c(S), S the raw total of the non-banned edges."""
        st = self.node_stats(state)
        lab = sm.banned_labels(st["moves"], no_act)
        S = int(st["n"][(lab & sm.BANNED) == 0].sum())
        return fo.prune(lab, st["n"], st["w"], st["p"], self.c_at(S), self.k)


class Search(Schedule, sm.Search):
    def __init__(self, cfg, salt, k=0.0, factor=0.0, base=19652.0, T=1.0):
        sm.Search.__init__(self, cfg, salt, k)
        self.set_schedule(factor, base, T)


class SolverSearch(Schedule, so.Search):
    def __init__(self, cfg, salt, factor=0.0, base=19652.0, T=1.0, solver=True):
        so.Search.__init__(self, cfg, salt, 0.0, solver)
        self.set_schedule(factor, base, T)


def cases():
    """search_model.cases() and the wide position once more under WIDE_SALT."""
    return sm.cases() + [dict(name="wide_b", salt=WIDE_SALT, state=WIDE, kind=None)]


def run_case(case, factor=F, base=B, T=1.0, k=0.0, sims=SIMS, solver=None):
    """The searches of one case: list of dict(state, no_act, stats, targets, raw_total, best) plus the Search object.
    solver None: Search; True / False: SolverSearch with the solver on / off (best is then its play())."""
    def new():
        if solver is None:
            return Search(play_cfg(sims), case["salt"], k, factor, base, T)
        return SolverSearch(play_cfg(sims), case["salt"], factor, base, T, solver)

    def row(s, state, no_act):
        t, raw = s.targets(state, no_act)
        best = s.best_move(state, no_act) if solver is None else s.play(state, no_act)
        return dict(state=state, no_act=no_act, stats=s.node_stats(state), targets=t, raw_total=raw, best=best)
    return walk_case(case, new, row, ban_of(case, sims) if case["kind"] == "ban" else None)
