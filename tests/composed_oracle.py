"""The search options that compose, beside each other, restated over the oracles that already carry them: the moves-left
utility (moves_left_search_oracle), the draw average (draw_search_oracle) and the lower-confidence-bound move choice
(lcb_oracle), each with forced playouts (k), the playout cap's per-ply budget and the visit entry a self-play ply must write.
The yardstick of tests/test_gpu_composed_search.py; tests/test_composed_oracle_cpu.py pins it to the oracles it is made of and
states the conditions on the inputs.

Nothing of the search is restated here.  The three Search classes select with their own third score term and carry
search_model's forcing rule beside it; this file chooses their parameters once (new_search), sets a ply's budget through
begin_ply (capped), and plays a tau = 0 line with tree reuse (play_line): lcb_oracle.play_line for any of the three.

THE FORCED PASS AND THE THIRD TERM.  include/czero.h: a forced edge is "not banned and not rejected".  The oracles reject on the
full score, (q + u) + third term; the device's forced pass (select_edge) on q + u alone.  The two agree on every input a search
can produce.  An edge that can be forced has n > 0, so q = w / n is the finite mean of backed-up values in [-2, 2] (less the
virtual losses in flight) and u is a finite non-negative product: q + u is finite and nowhere near -99999999.  The third term
is finite and bounded -- the moves-left utility by cap * f with f = 1.6521 a - 0.6521 a^2 <= 1 on a in [0, 1] and cap finite
(the setter refuses anything else), the draw term by |score| * dbar <= 1, the V records add none -- so the full score is NaN
only where q + u is, and below -99999999 only where q + u is below -99999998.  Neither happens; both sides stay as they are."""
import numpy as np

import draw_search_oracle as do
import forced_playouts_oracle as fo
import lcb_oracle as lo
import moves_left_search_oracle as mo
import playout_cap_oracle as pco
import q_record_oracle as qo
import search_model as sm
import stop_oracle as st
import surprise_oracle as su
from oracle import xq_oracle as xo

OPTIONS = ("ml", "draw", "lcb")
K = 2.0                         # forced playouts of every composed test
DRAW_SCORE = -0.5               # tests/test_draw_search_cpu.py TEST_SCORE (test_composed_oracle_cpu.py asserts it)
# the self-play line of the composed tests: chosen on the CPU (tests/test_composed_oracle_cpu.py asserts what it must show)
LINE = dict(sims=120, fast_sims=24, full_rate=0.5, seed=26, salt=21, plies=6)
_CAPPED = {}


def capped(cls):
    """`cls` with a per-ply budget: begin_ply -- search_model.Search's budget method, which every subclass and stop_oracle's
    search() go through -- reads ply_sims (None: the configuration's) as the ply's simulation_num_per_move, the reuse rule's
    `done == sims` included, as begin_search reads fast_sims on a fast ply."""
    if cls not in _CAPPED:
        class Capped(cls):
            ply_sims = None

            def begin_ply(self, state, no_act=None, increase_temp=False):
                full = self.cfg.simulation_num_per_move
                self.cfg.simulation_num_per_move = full if self.ply_sims is None else int(self.ply_sims)
                try:
                    return super().begin_ply(state, no_act, increase_temp)
                finally:
                    self.cfg.simulation_num_per_move = full
        Capped.__name__ = "Capped" + cls.__name__
        _CAPPED[cls] = Capped
    return _CAPPED[cls]


def new_search(option, sims, salt, k=0.0, on=True):
    """The oracle of `option` ("ml", "draw", "lcb", None = search_model.Search) with the parameters the composed tests use;
    on=False: the option's class with the option off."""
    cfg = sm.play_cfg(sims)
    if option == "ml":
        return capped(mo.Search)(cfg, salt, k, mo.SLOPE, mo.CAP, on=on)
    if option == "draw":
        return capped(do.Search)(cfg, salt, k, DRAW_SCORE, on=on)
    if option == "lcb":
        return capped(lo.Search)(cfg, salt, k, lo.Z if on else 0.0, lo.RATIO)
    if option is None:
        return capped(sm.Search)(cfg, salt, k)
    raise ValueError(option)


def records(search, option, state):
    """The option's records of `state`'s node (node_moves_left / node_draws / node_values), None where it is not in the tree
    or the option keeps none."""
    if option == "ml":
        return search.node_moves_left(state)
    if option == "draw":
        return search.node_draws(state)
    if option == "lcb":
        return search.node_values(state)
    return None


def same_records(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.keys() == b.keys() and all(np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes() for key in a)


def run_case(option, case, k=K, sims=sm.SIMS, on=True):
    """search_model.walk_case with new_search: rows dict(state, no_act, stats, records, child, child_stats, targets, raw_total,
    best, most) plus the Search object.  targets / raw_total: forced_playouts_oracle.prune on the root's fields -- plain
    q = W / N under every option; most: the most visited move, what `best` is without the lower-confidence-bound rule."""
    def row(s, state, no_act):
        st = s.node_stats(state)
        targets, raw = fo.prune(sm.banned_labels(st["moves"], no_act), st["n"], st["w"], st["p"], s.cfg.c_puct, s.k)
        best = s.best_move(state, no_act)
        child = xo.step(state, best)
        return dict(state=state, no_act=no_act, stats=st, records=records(s, option, state), child=child,
                    child_stats=s.node_stats(child), targets=targets, raw_total=raw, best=best,
                    most=sm.Search.best_move(s, state, no_act))
    ban = sm.ban_of(case, sims) if case["kind"] == "ban" else None
    return sm.walk_case(case, lambda: new_search(option, sims, case["salt"], k, on), row, ban)


def play_line(option, state, plies, sims, salt, k=0.0, fast_sims=0, full_rate=1.0, seed=0, game_id=0, on=True):
    """A tau = 0 game line with tree reuse over the oracle of `option`, as self-play game `game_id` of a search seeded `seed`
    plays it while no position repeats (no bans, no raised temperature) and nobody resigns.  Ply `turns` is a full search of
    `sims` simulations with forced playouts k, or -- playout_cap_oracle.ply_is_full says which -- a fast one of fast_sims
    simulations without forcing.  Returns (rows, the Search); a row is dict(state, turns, fast, ran, forced_picks (of this
    ply), stats, records, best, most, counts, pruned, raw_total, q, s, A):
      counts, pruned, raw_total: the visit entry -- on a full ply with k > 0 prune(...)'s counts, CZ_VISIT_PRUNED (set iff some
        edge has a visit) and raw_total; otherwise the raw counts, no flag and 0;
      q: q_record_oracle.root_value, s and A: surprise_oracle.surprise, both over `counts`."""
    s = new_search(option, sims, salt, 0.0, on)
    out = []
    for turns in range(plies):
        full = pco.ply_is_full(seed, game_id, turns, fast_sims, full_rate)
        s.ply_sims = sims if full else fast_sims
        s.k = float(k) if full else 0.0
        before = s.forced_picks
        ran = s.search(state)
        st = s.node_stats(state)
        counts, raw, pruned = st["n"], 0, False
        if full and k > 0.0:
            counts, raw = fo.prune(st["moves"], st["n"], st["w"], st["p"], s.cfg.c_puct, k)
            pruned = int(st["n"].sum()) > 0
        surprise, A = su.surprise(st["moves"], counts, st["p"])
        best = s.best_move(state)
        out.append(dict(state=state, turns=turns, fast=not full, ran=ran, forced_picks=s.forced_picks - before, stats=st,
                        records=records(s, option, state), best=best, most=sm.Search.best_move(s, state), counts=counts,
                        pruned=pruned, raw_total=raw, q=qo.root_value(st["moves"], counts, st["n"], st["w"]), s=surprise, A=A))
        state = xo.step(state, best)
    return out, s


# ---- the stop rules beside forced playouts -----------------------------------------------------------------------------------
def stop_search(plan, k=K):
    """One of stop_oracle.planned_gains()'s searches with forced playouts k: the Search object after the search."""
    o = st.Search(sm.play_cfg(st.BUDGET), plan["salt"], k, gain=plan["gain"], interval=plan["interval"])
    o.search(plan["state"])
    return o


def lead_search(state, salt, k=K):
    """The unreachable-lead rule (evaluate: the arena's tau) on one of stop_oracle.positions() with forced playouts k."""
    o = st.Search(sm.play_cfg(st.BUDGET), salt, k, lead=True, evaluate=True)
    o.search(state)
    return o


# ---- comparisons the option tests share --------------------------------------------------------------------------------------
def assert_targets(got, stats, no_act, c_puct, k, what=""):
    """got: root_targets() of a G = 1 search; stats: the oracle's node_stats of that root.  The pruned counts and raw_total are
    forced_playouts_oracle.prune on the oracle's n, w and p -- plain q = W / N, whatever the selection's score carries; with
    k = 0 that is the raw counts."""
    want, raw = fo.prune(sm.banned_labels(stats["moves"], no_act), stats["n"], stats["w"], stats["p"], c_puct, k)
    nm = len(want)
    assert int(got["raw_total"][0]) == raw, (what, int(got["raw_total"][0]), raw)
    assert (got["n"][0, :nm] == want).all() and not got["n"][0, nm:].any(), (what, got["n"][0, :nm], want)


def pv_first(stats, no_act):
    """The first move of cz_search_pv's line without the lower-confidence-bound move choice (include/czero.h): the most
    visited non-banned root edge, `>=` keeping the LAST maximum in edge order -- on a tie not the move choose() plays, which is
    the lowest label."""
    best, best_n = None, -1
    for label, n in zip(stats["moves"], stats["n"]):
        mv = xo.label_str(int(label))
        if mv not in (no_act or ()) and int(n) >= best_n:
            best, best_n = mv, int(n)
    return best
