"""The early stop of a settled ply (cz_search_set_kld_gain, cz_search_set_smart_pruning; run.py self --kld-gain, run.py eval
--smart-pruning) restated in Python: search_model.Search -- one search thread, the hash stub as network -- with the
two rules of include/czero.h word for word at the one test point, before a simulation is started (K = 1: a batch is one
simulation, nothing is in flight between two of them).

tests/test_stop_cpu.py pins Search with both rules off to fo.Search stat for stat before anything else is trusted."""
import math

import numpy as np

import search_model as sm
from oracle import xq_oracle as xo

KLD, LEAD = "kld", "lead"


def ply_tau(cfg, turns, increase_temp=False, evaluate=False):
    """The temperature choose_action computes (player.py:453-461): 0 means the move is the arg-max of the visit counts."""
    tau = 0.0
    if turns < 30 and cfg.tau_decay_rate != 0.0:
        tau = math.pow(cfg.tau_decay_rate, float(turns + 1))
    if tau < 0.1 or (turns >= 4 and evaluate):
        tau = 0.0
    if increase_temp and not evaluate:
        tau = 0.5
    return tau


def kld_terms(m, n):
    """The float64 terms (m_j / M) * log((m_j / M) / (n_j / N)) over j with m_j > 0, in edge order; M = sum m, N = sum n."""
    M, N = float(sum(int(x) for x in m)), float(sum(int(x) for x in n))
    out = []
    for mj, nj in zip(m, n):
        if mj > 0:
            t = float(mj) / M
            out.append(t * math.log(t / (float(nj) / N)))
    return out


def kld_gain(m, n):
    """(D, g) of the snapshot m against the counts n: D = the terms summed in edge order, g = D / (N - M)."""
    D = 0.0
    for t in kld_terms(m, n):
        D = D + t
    return D, D / float(sum(int(x) for x in n) - sum(int(x) for x in m))


def gain_bound(m, n):
    """What |g_engine - g_oracle| may be: both logarithms are good to 1 ulp, each term is three more roundings and the two
    sums run in different orders: |dg| * (N - M) <= 16 * 2^-53 * n_edges * sum |term_j|."""
    terms = kld_terms(m, n)
    return 16.0 * 2.0 ** -53 * len(n) * sum(abs(t) for t in terms) / float(sum(int(x) for x in n) - sum(int(x) for x in m))


def top_two(n, banned):
    """(a, b): the largest and the second-largest count over the non-banned edges, 0 where there is no such edge."""
    live = sorted((int(x) for x, ban in zip(n, banned) if not ban), reverse=True)
    return (live + [0, 0])[0], (live + [0, 0])[1]


class Search(sm.Search):
    """search_model.Search with the stop rules.  gain G (0 = the KLD rule is off) and interval I; lead: the unreachable-lead rule is
    on; evaluate: config.opts.evaluate of the engine (tau).  measure=True takes every checkpoint and never ends a ply: the
    uncut gain sequence.  After search(): ran (simulations run), cut (None, KLD or LEAD), sims_cut (the budget not started),
    checks (checkpoints of the ply, the one that took the first snapshot included), last_gain (None: nothing measured) and
    checkpoints, a list of dict(at, M, N, D, g, m, n) -- at = simulations of the ply finished; M, D, g, m None for the first."""

    def __init__(self, cfg, salt, k=0.0, gain=0.0, interval=100, lead=False, evaluate=False, measure=False):
        super().__init__(cfg, salt, k)
        self.gain, self.interval, self.lead, self.evaluate, self.measure = float(gain), int(interval), bool(lead), evaluate, measure
        self.ran, self.cut, self.sims_cut, self.checks, self.last_gain, self.checkpoints = 0, None, 0, 0, None, []
        self.kld_plies = self.kld_sims_cut = self.lead_plies = self.lead_sims_cut = 0

    def _settled(self, tasks, finished, tau):
        node = self.tree.get(self.root)
        n = list(node.n) if node is not None else []
        N = sum(n)
        if self.gain > 0.0 or self.measure:
            if self._snap is None:
                due = finished >= self.interval
            else:
                due = N >= self._snap[1] + self.interval
            if due:
                self.checks += 1
                stop = False
                if self._snap is None:
                    self.checkpoints.append(dict(at=finished, M=None, N=N, D=None, g=None, m=None, n=n))
                else:
                    m, M = self._snap
                    D, g = kld_gain(m, n)
                    self.checkpoints.append(dict(at=finished, M=M, N=N, D=D, g=g, m=m, n=n))
                    self.last_gain = g
                    stop = g < self.gain and not self.measure
                if stop:
                    return KLD
                self._snap = (n, N)
        if self.lead and tau == 0.0 and node is not None:
            a, b = top_two(n, [mv in self.no_act for mv in node.moves])
            if a - b > tasks:
                return LEAD
        return None

    def search(self, state, no_act=None, increase_temp=False, turns=0):
        """The model's search with the test point before every simulation."""
        budget = self.begin_ply(state, no_act, increase_temp)
        tau = ply_tau(self.cfg, turns, increase_temp, self.evaluate)
        self._snap = None                                   # the snapshot is empty when the ply's search begins
        self.ran, self.cut, self.sims_cut, self.checks, self.last_gain, self.checkpoints = 0, None, 0, 0, None, []
        on = self.gain > 0.0 or self.lead or self.measure
        while self.ran < budget:
            why = self._settled(budget - self.ran, self.ran, tau) if on else None
            if why is not None:
                self.cut, self.sims_cut = why, budget - self.ran
                if why == KLD:
                    self.kld_plies += 1
                    self.kld_sims_cut += self.sims_cut
                else:
                    self.lead_plies += 1
                    self.lead_sims_cut += self.sims_cut
                break
            self._simulate()
            self.ran += 1
        return self.ran

    def play_line(self, state, plies, bans=None, first_turn=0):
        """Search and play `plies` plies from `state` with the tree carried over (or until done()): list of dict(state,
        no_act, turns, ran, cut, checks, last_gain, move, stats).  bans: {ply: [moves]} banned at that ply."""
        out = []
        for ply in range(plies):
            if xo.done(state)[0]:
                break
            no_act = list((bans or {}).get(ply, []))
            ran = self.search(state, no_act, turns=first_turn + ply)
            mv = self.best_move(state, no_act)
            out.append(dict(state=state, no_act=no_act, turns=first_turn + ply, ran=ran, cut=self.cut, checks=self.checks,
                            last_gain=self.last_gain, move=mv, stats=self.node_stats(state)))
            state = xo.step(state, mv)
        return out


# ---- the searches of the CPU and GPU tests -------------------------------------------------------------------------------
BUDGET = 256
INTERVALS = (16, 32)
SALT = 3
_MATES = ("m1", "m2", "wide_m2")


def positions():
    """(name, state, salt): the nine sm.cases() positions and three mates of tests/golden/solver_positions.json."""
    import solver_oracle as so
    mates = {p["name"]: p for p in so.positions()}
    return [("fo:" + c["name"], c["state"], c["salt"]) for c in sm.cases()] + [(n, mates[n]["state"], SALT) for n in _MATES]


_UNCUT = {}


def uncut(name, state, salt, interval, budget=BUDGET):
    """The measuring search of a position: its Search object (checkpoints = the uncut gain sequence)."""
    key = (name, interval, budget)
    if key not in _UNCUT:
        s = Search(sm.play_cfg(budget), salt, interval=interval, measure=True)
        s.search(state)
        _UNCUT[key] = s
    return _UNCUT[key]


def planned_gains():
    """One K = 1 search per position and interval: list of dict(name, state, salt, interval, gain, kind, stop_at, margin).
    gain is the geometric mean of two neighbouring values of the position's sorted uncut gain sequence, so that the stop
    is due at a known checkpoint with a margin on both sides: kind "top" takes the two largest (everything but the maximum
    is below G), "mid" the middle pair.  The sequence is extended at both ends: kind "none" is a quarter of the smallest,
    below which nothing falls -- the rule is on and the ply runs its whole budget --, kind "all" four times the largest: the
    first measured gain ends the ply, at its second checkpoint.  The kinds rotate over the list.  stop_at: the checkpoint (counted from 1, the one
    that takes the first snapshot included) at which the stop is due, None for "none"; margin: the least |g - G| over
    the sequence."""
    out = []
    for i, (name, state, salt) in enumerate(positions()):
        for k, interval in enumerate(INTERVALS):
            cps = [c for c in uncut(name, state, salt, interval).checkpoints if c["g"] is not None]
            gs = sorted(c["g"] for c in cps)
            kind = ("top", "mid", "none", "all")[(i + k) % 4]
            if len(gs) < 2 or gs[0] <= 0.0:
                kind = "none" if gs and gs[0] > 0.0 else "skip"
            if kind == "skip":
                continue
            if kind == "top":
                G = math.sqrt(gs[-1] * gs[-2])
            elif kind == "mid":
                j = (len(gs) - 2) // 2
                G = math.sqrt(gs[j] * gs[j + 1])
            elif kind == "all":
                G = gs[-1] * 4.0
            else:
                G = gs[0] / 4.0
            stop_at = next((idx + 2 for idx, c in enumerate(cps) if c["g"] < G), None)
            out.append(dict(name=name, state=state, salt=salt, interval=interval, gain=G, kind=kind, stop_at=stop_at,
                            margin=min(abs(c["g"] - G) for c in cps),
                            bound=max(gain_bound(c["m"], c["n"]) for c in cps)))
    return out


# ---- the played lines of the GPU test ------------------------------------------------------------------------------------
LINE_SIMS, LINE_I, LINE_G, LINE_PLIES = 128, 16, 2.0e-3, 12


def line_cases():
    """(name, state, salt, bans): three positions; the second line bans at ply 2 the move the unbanned line plays there."""
    pos = {n: (s, salt) for n, s, salt in positions()}
    out = []
    for name, ban_ply in (("fo:init", None), ("fo:pos550", 2), ("fo:pos850", None)):
        state, salt = pos[name]
        bans = None
        if ban_ply is not None:
            free = Search(sm.play_cfg(LINE_SIMS), salt, gain=LINE_G, interval=LINE_I).play_line(state, ban_ply + 1)
            bans = {ban_ply: [free[ban_ply]["move"]]}
        out.append((name, state, salt, bans))
    return out
