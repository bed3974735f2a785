"""Gumbel root search with sequential halving (cz_search_set_gumbel, run.py self --gumbel M) restated in Python: the
definitions of include/czero.h in plain float64 -- seq, the score, the policy target -- a subclass of
search_model.Search (one search thread, no root noise) with the root rule, `started`, the played move and the
target, and such a search as the player of selfplay_oracle.start_game.

The search takes the ply's Gumbel draws as an INPUT array (edge index -> g): a GPU test feeds it what the device drew, so
that the comparison is about the search; draws_for() restates the device's generator for the tests of the draws
themselves and for the self-play loop.  exp and log are libm's here and the device library's there: scores differ in
their last places, which is why the GPU comparison rests on every selection's winning margin (Search.margins) and allows
+-1 on a target."""
import math

import numpy as np

import search_model as sm
import selfplay_oracle
import stub_net
from oracle import xq_oracle as xo            # (the tests reach it as go.xo)

BANNED = sm.BANNED
INF = float("inf")
GUMBEL_STREAM = 4           # stream 0: the per-game lotteries, 1: the move choice, 2: the playout cap, 3: the leaf mirror
C_VISIT, C_SCALE = 50.0, 1.0


# ---- the definitions ----------------------------------------------------------------------------------------------------
def seq(m, n):
    """The visit schedule: entry t is the started count the edge taken by the t-th root selection must have."""
    if m <= 1:
        return list(range(n))
    L = int(math.ceil(math.log2(m)))
    visits = [0] * m
    k = m
    out = []
    while len(out) < n:
        e = max(1, n // (L * k))
        for _ in range(e):
            out += visits[:k]
            for i in range(k):
                visits[i] += 1
        k = max(2, k // 2)
    return out[:n]


def draws_for(seed, game_id, slot, turns, count=128):
    """g_j = -log(-log u_j), u_j = philox(seed, game_id + slot * 2654435761, stream 4, turns << 32 | j), u = 0 -> 2^-53."""
    key = (game_id + slot * 2654435761) & 0xFFFFFFFF
    out = np.empty(count, dtype=np.float64)
    for j in range(count):
        u = stub_net.philox_uniform(seed, key, GUMBEL_STREAM, (turns << 32) | j)
        if u == 0.0:
            u = 2.0 ** -53
        out[j] = -math.log(-math.log(u))
    return out


def q01(n, w):
    if n <= 0:
        return 0.0
    q = (float(w) / float(n) + 1.0) / 2.0
    return 0.0 if q < 0.0 else (1.0 if q > 1.0 else q)


def sigma(c_visit, c_scale, max_n, x):
    return ((float(c_visit) + float(max_n)) * float(c_scale)) * x


def score(g, p, n, w, max_n, c_visit, c_scale):
    lp = math.log(float(p)) if float(p) > 0.0 else -INF
    return (float(g) + lp) + sigma(c_visit, c_scale, max_n, q01(n, w))


def target(labels, n, w, p, c_visit=C_VISIT, c_scale=C_SCALE):
    """The policy target of a root row: (int32 m_j = floor(65536 pi'_j + 1/2), raw total of the non-banned edges)."""
    labels = np.asarray(labels, dtype=np.uint16)
    n = np.asarray(n, dtype=np.int32)
    w = np.asarray(w, dtype=np.float64)
    p = np.asarray(p, dtype=np.float32)
    out = np.zeros(len(n), dtype=np.int32)
    live = [j for j in range(len(n)) if not labels[j] & BANNED]
    S = sum(int(n[j]) for j in live)
    if not live:
        return out, S
    max_n = max(int(n[j]) for j in live)
    num = sum(float(p[j]) * q01(int(n[j]), w[j]) for j in live if n[j] > 0)
    den = sum(float(p[j]) for j in live if n[j] > 0)
    vbar = num / den if den > 0.0 else 0.5
    sg = {j: sigma(c_visit, c_scale, max_n, q01(int(n[j]), w[j]) if n[j] > 0 else vbar) for j in live}
    mx = max(sg.values())
    e = {j: float(p[j]) * math.exp(sg[j] - mx) for j in live}
    tot = math.fsum(e.values())
    if not tot > 0.0:
        return out, S
    for j in live:
        out[j] = int(math.floor(65536.0 * (e[j] / tot) + 0.5))
    return out, S


# ---- the search ---------------------------------------------------------------------------------------------------------
class Search(sm.Search):
    """search_model.Search with the Gumbel rule at the root.  m = 0 is that search.  draws: the ply's g array (128
    entries), or a callable(search index) -> array for searches whose plies differ in their draws.  After search():
    started (per root edge), seq_used (the schedule value of every root selection, in order), margins (winner's score
    minus the best other eligible score, +inf when it stood alone)."""

    def __init__(self, cfg, salt, k=0.0, m=0, c_visit=C_VISIT, c_scale=C_SCALE, draws=None):
        super().__init__(cfg, salt, k)
        if m and k:
            raise ValueError("the Gumbel root search excludes forced playouts")
        self.m, self.c_visit, self.c_scale, self.draws = int(m), float(c_visit), float(c_scale), draws
        self.searches = 0
        self.started, self.seq_used, self.margins, self.budget, self.g = None, [], [], 0, None

    def _live(self, node):
        return [i for i, mv in enumerate(node.moves) if mv not in self.no_act]

    def _scores(self, node, idx):
        live = self._live(node)
        max_n = max([node.n[i] for i in live], default=0)
        return {i: score(self.g[i], node.p[i], node.n[i], node.w[i], max_n, self.c_visit, self.c_scale) for i in idx}

    def _select(self, node, is_root):
        if not (is_root and self.m > 0):
            return super()._select(node, is_root)
        if node.pending is not None:
            node.spread()
        if self.started is None:
            self.started = [0] * len(node.moves)
        live = self._live(node)
        t = sum(self.started)
        v = seq(min(self.m, len(live)), self.budget)[t]             # (t < budget: a ply selects at the root at most once per simulation)
        elig = [i for i in live if self.started[i] == v]
        if not elig:
            return -1, False
        sc = self._scores(node, elig)
        best = max(elig, key=lambda i: (sc[i], i))                  # the later edge on a tie
        rest = [sc[i] for i in elig if i != best]
        self.margins.append(sc[best] - max(rest) if rest and max(rest) > -INF else INF)
        self.seq_used.append(v)
        self.started[best] += 1
        return best, False

    def begin_ply(self, state, no_act=None, increase_temp=False):
        self.budget = super().begin_ply(state, no_act, increase_temp)
        d = self.draws(self.searches) if callable(self.draws) else self.draws
        self.g = None if d is None else np.asarray(d, dtype=np.float64)
        self.started, self.seq_used, self.margins = None, [], []
        self.searches += 1
        return self.budget

    def search(self, state, no_act=None, increase_temp=False):
        ran = super().search(state, no_act, increase_temp)
        if self.started is None and state in self.tree:
            self.started = [0] * len(self.tree[state].moves)
        return ran

    def played(self, state, no_act=None):
        """(the move a Gumbel ply plays, its margin over the best other edge of greatest started)."""
        node = self.tree[state]
        if node.pending is not None:
            node.spread()
        self.no_act = tuple(no_act or ())
        live = self._live(node)
        top = max(self.started[i] for i in live)
        elig = [i for i in live if self.started[i] == top]
        sc = self._scores(node, elig)
        best = max(elig, key=lambda i: (sc[i], i))
        rest = [sc[i] for i in elig if i != best]
        return node.moves[best], (sc[best] - max(rest) if rest and max(rest) > -INF else INF)

    def best_move(self, state, no_act=None):
        if self.m > 0:
            return self.played(state, no_act)[0]
        return super().best_move(state, no_act)

    def targets(self, state, no_act=None):
        if self.m <= 0:
            return super().targets(state, no_act)
        st = self.node_stats(state)
        return target(sm.banned_labels(st["moves"], no_act), st["n"], st["w"], st["p"], self.c_visit, self.c_scale)

    def max_q(self, state, no_act=None):
        """choose_action's resign statistic: the greatest q over the non-banned edges, -100 without one."""
        node = self.tree[state]
        qs = [node.w[i] / float(node.n[i]) if node.n[i] else 0.0 for i, mv in enumerate(node.moves) if mv not in (no_act or ())]
        return max(qs, default=-100.0)


def case_row(s, state, no_act):
    """What run_case reports of one search."""
    t, raw = s.targets(state, no_act)
    best, margin = s.played(state, no_act)
    return dict(state=state, no_act=no_act, stats=s.node_stats(state), started=list(s.started),
                seq_used=list(s.seq_used), margins=list(s.margins), targets=t, raw_total=raw, best=best,
                best_margin=margin, budget=s.budget)


def run_case(case, m, sims, draws, c_visit=C_VISIT, c_scale=C_SCALE):
    """The searches of one of fo.cases() with the Gumbel rule: list of dict(state, no_act, stats, started, seq_used,
    margins, targets, raw_total, best, best_margin, budget) -- two for "reuse" -- plus the Search object.  "ban": the ban
    is the move an unbanned Gumbel search of the position plays."""
    return sm.walk_case(case, lambda: Search(sm.play_cfg(sims), case["salt"], 0.0, m, c_visit, c_scale, draws), case_row)


# ---- self-play ------------------------------------------------------------------------------------------------------------
def gumbel_selfplay_game(cfg, salt, seed, game_id, slot, m, c_visit=C_VISIT, c_scale=C_SCALE, init_state=None, player=None):
    """One self-play game of the engine with the Gumbel root search, search_threads = 1: selfplay_oracle.start_game with
    Search above (or the subclass `player`) as the player -- ONE player for the whole game, the tree carried from ply to
    ply -- and choose_action's resign test in front of the played move.  No temperature, no noise.  Returns
    selfplay_game's dict plus `plies`: per searched ply dict(state, labels, banned, targets, raw_total, started, sum_n,
    resign)."""
    enable_resign = selfplay_oracle.resign_enabled(cfg, seed, game_id)
    turns_box = [0]
    pl = (player or Search)(cfg, salt, 0.0, m, c_visit, c_scale, draws=lambda _: draws_for(seed, game_id, slot, turns_box[0]))
    plies = []

    def ply(state, turns, no_act, increase_temp):
        turns_box[0] = turns
        pl.search(state, no_act, increase_temp)
        st = pl.node_stats(state)
        t, raw = pl.targets(state, no_act)
        resign = pl.max_q(state, no_act) < cfg.resign_threshold and enable_resign and turns > cfg.min_resign_turn
        action = None if resign else pl.played(state, no_act)[0]
        plies.append(dict(state=state, labels=st["moves"], banned=np.array([mv in no_act for mv in pl.tree[state].moves]),
                          targets=t, raw_total=raw, started=list(pl.started), sum_n=st["sum_n"], resign=resign))
        return action

    out = selfplay_oracle.start_game(cfg, seed, game_id, ply, init_state)
    out["plies"] = plies
    return out
