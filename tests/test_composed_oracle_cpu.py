"""CPU: tests/composed_oracle.py against the oracles it is made of, and the conditions on the inputs of
tests/test_gpu_composed_search.py -- stated here as assertions, so that the GPU comparisons cannot pass on inputs where the
composition under test changes nothing."""
import numpy as np
import pytest

import composed_oracle as co
import draw_search_oracle as do
import forced_playouts_oracle as fo
import lcb_oracle as lo
import moves_left_search_oracle as mo
import playout_cap_oracle as pco
import search_model as sm
import stop_oracle as st
from oracle import xq_oracle as xo
from test_draw_search_cpu import TEST_SCORE

CASES = sm.cases()
# the cases on which the lower-confidence-bound rule plays another move than the most visited one when forcing is on (k = 2,
# z = 2; with k = 0 they are test_lcb_cpu.DIFFER_Z2).  Named, so that a change of inputs that loses one is seen as that.
LCB_DIFFER_FORCED = ("pos400", "pos700", "pos850")


def _counts(rows):
    return [r["stats"]["n"].tolist() for r in rows]


def _same_stats(a, b):
    return a["sum_n"] == b["sum_n"] and all(np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes()
                                            for key in ("moves", "n", "w", "p"))


def test_the_parameters_are_the_option_tests_own():
    assert co.DRAW_SCORE == TEST_SCORE and co.K == 2.0
    assert (mo.SLOPE, mo.CAP) == (0.0027, 0.0345) and (lo.Z, lo.RATIO) == (2.0, 0.15)


# ---- 1. option x forced playouts on the nine cases ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forced_plain():
    """The forced search with every option off: forced_playouts_oracle's own run of every case."""
    return [fo.run_case(c, co.K)[0] for c in CASES]


@pytest.mark.parametrize("option", co.OPTIONS)
def test_forcing_and_the_option_both_change_the_nine_cases(option, forced_plain):
    differs_from_off, lcb_differs = 0, []
    pruned = 0
    for c, plain in zip(CASES, forced_plain):
        rows, s = co.run_case(option, c)
        assert len(rows) == (2 if c["kind"] == "reuse" else 1)
        assert s.forced_picks > 0, c["name"]                                        # the forced pass takes an edge
        free, _ = co.run_case(option, c, k=0.0)
        assert _counts(rows) != _counts(free), c["name"]                            # ... and changes the visit counts
        if option == "lcb":                                                         # the V records leave n and w alone
            assert all(_same_stats(r["stats"], p["stats"]) for r, p in zip(rows, plain)), c["name"]
            assert any(r["records"]["vn"].sum() > 0 for r in rows)
            lcb_differs += [c["name"]] * any(r["best"] != r["most"] for r in rows)
        else:
            differs_from_off += _counts(rows) != _counts(plain)
        off, _ = co.run_case(option, c, on=False)                                   # the option's class, the option off
        assert all(_same_stats(r["stats"], p["stats"]) and r["best"] == p["best"] for r, p in zip(off, plain)), c["name"]
        for r, p in zip(off, plain):                                                # run_case's targets are Search.targets
            assert np.array_equal(r["targets"], p["targets"]) and r["raw_total"] == p["raw_total"]
        pruned += any(r["raw_total"] > int(r["targets"].sum()) for r in rows)
        for r in rows:                                                              # the child's node is in the tree
            assert r["child_stats"] is not None or xo.done(r["child"])[0], c["name"]
    if option == "lcb":
        # The issue's third condition -- the counts differ from the forced search with the option off on 8 of 9 -- cannot hold
        # for this option: its n and w ARE the forced search's, bit for bit (asserted above on all nine).  What the option
        # changes is the move, and the rule overturns the most visited move only where a runner-up has the tighter bound:
        # on these three cases, whose walks therefore pin choose(), pv() and the pick on a forced search.
        assert tuple(lcb_differs) == LCB_DIFFER_FORCED
    else:
        assert differs_from_off >= 8          # the third score term changes a forced search
    assert 2 * pruned >= len(CASES)           # root_targets is not the raw counts


def test_two_simulations_of_the_28_plane_runs_force_nothing():
    for option in co.OPTIONS:
        s = co.new_search(option, 2, CASES[0]["salt"], co.K)
        assert s.search(CASES[0]["state"]) == 2 and s.forced_picks == 0 and s.expansions == 2


# ---- 2. the stop rules x forced playouts -------------------------------------------------------------------------------------
def test_the_stop_rules_cut_forced_searches():
    plans = st.planned_gains()
    assert len(plans) == 2 * len(st.positions())
    early, changed = {}, 0
    for p in plans:
        o = co.stop_search(p, co.K)
        free = st.Search(sm.play_cfg(st.BUDGET), p["salt"], gain=p["gain"], interval=p["interval"])
        free.search(p["state"])
        assert o.forced_picks > 0, p["name"]
        changed += not _same_stats(o.node_stats(p["state"]), free.node_stats(p["state"]))
        # the decision at every checkpoint is far outside the rounding of the engine's gain
        for c in o.checkpoints:
            if c["g"] is not None:
                assert abs(c["g"] - p["gain"]) > 1e3 * st.gain_bound(c["m"], c["n"]), (p["name"], p["interval"], c["g"])
        early[p["name"]] = early.get(p["name"], False) or o.cut == st.KLD
    assert 2 * changed >= len(plans)                                    # forcing changes the searches the rule then cuts
    assert 2 * sum(early.values()) >= len(early), early                 # the planned gains end at least half the positions early
    lead = [co.lead_search(state, salt, co.K) for _, state, salt in st.positions()]
    assert all(o.forced_picks > 0 for o in lead)
    assert 2 * sum(o.cut == st.LEAD for o in lead) >= len(lead), [o.cut for o in lead]


# ---- 3. the composed self-play line ------------------------------------------------------------------------------------------
L = co.LINE


def _line(option, **kw):
    args = dict(k=co.K, fast_sims=L["fast_sims"], full_rate=L["full_rate"], seed=L["seed"])
    args.update(kw)
    return co.play_line(option, xo.INIT_STATE, L["plies"], L["sims"], L["salt"], **args)


def _same_rows(a, b, keys=("state", "ran", "best", "raw_total", "pruned", "fast"), with_records=True):
    return len(a) == len(b) and all(_same_stats(x["stats"], y["stats"])
                                    and (not with_records or co.same_records(x["records"], y["records"]))
                                    and np.array_equal(x["counts"], y["counts"]) and all(x[k] == y[k] for k in keys)
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("option", co.OPTIONS)
def test_the_line_is_the_options_own_line_without_cap_and_forcing(option):
    rows, _ = _line(option, k=0.0, fast_sims=0)
    if option == "lcb":
        want, _ = lo.play_line(xo.INIT_STATE, L["plies"], L["sims"], L["salt"])
        assert [r["best"] for r in rows] == [w["best"] for w in want]
        assert all(_same_stats(r["stats"], w["stats"]) and co.same_records(r["records"], w["values"]) and r["ran"] == w["ran"]
                   for r, w in zip(rows, want))
    else:
        o = (mo.Search(sm.play_cfg(L["sims"]), L["salt"], slope=mo.SLOPE, cap=mo.CAP) if option == "ml" else
             do.Search(sm.play_cfg(L["sims"]), L["salt"], score=TEST_SCORE))
        state = xo.INIT_STATE
        for r in rows:                                      # the walk of test_a_played_line_with_tree_reuse_matches_the_oracle
            assert r["state"] == state and o.search(state) == r["ran"]
            assert _same_stats(r["stats"], o.node_stats(state))
            assert co.same_records(r["records"], o.node_moves_left(state) if option == "ml" else o.node_draws(state))
            assert r["best"] == o.best_move(state)
            state = xo.step(state, r["best"])
    assert all(not r["fast"] and not r["pruned"] and r["raw_total"] == 0 and np.array_equal(r["counts"], r["stats"]["n"])
               for r in rows)


def test_with_every_option_off_the_line_is_the_forced_search():
    rows, _ = _line(None, fast_sims=0)
    o = sm.Search(sm.play_cfg(L["sims"]), L["salt"], co.K)
    state = xo.INIT_STATE
    for r in rows:
        assert r["state"] == state and o.search(state) == r["ran"] and _same_stats(r["stats"], o.node_stats(state))
        targets, raw = o.targets(state)
        assert np.array_equal(r["counts"], targets) and r["raw_total"] == raw and r["pruned"]
        assert r["best"] == o.best_move(state)
        state = xo.step(state, r["best"])
    for option in co.OPTIONS:
        assert _same_rows(_line(option, fast_sims=0, on=False)[0], rows, with_records=False), option


@pytest.mark.parametrize("option", co.OPTIONS)
def test_a_cap_of_rate_1_is_no_cap(option):
    assert _same_rows(_line(option, full_rate=1.0)[0], _line(option, fast_sims=0)[0])


@pytest.mark.parametrize("option", co.OPTIONS)
def test_the_line_meets_what_the_gpu_test_needs(option):
    rows, _ = _line(option)
    assert len({r["state"] for r in rows}) == len(rows)     # no position repeats: no bans, no raised temperature
    assert [r["fast"] for r in rows] == [not pco.ply_is_full(L["seed"], 0, t, L["fast_sims"], L["full_rate"])
                                         for t in range(L["plies"])]
    fast, full = [r for r in rows if r["fast"]], [r for r in rows if not r["fast"]]
    assert len(fast) >= 2 and len(full) >= 2
    assert all(r["forced_picks"] == 0 and not r["pruned"] and r["raw_total"] == 0 for r in fast)
    assert all(r["ran"] <= L["fast_sims"] for r in fast)
    assert any(r["forced_picks"] > 0 and r["raw_total"] - int(r["counts"].sum()) > 0 for r in full)
    # the idle fast ply: the reused root already holds at least fast_sims visits and nothing is searched
    assert any(r["ran"] == 0 and r["stats"]["sum_n"] > L["fast_sims"] for r in fast)
    assert any(0 < r["ran"] for r in fast)
    if option == "lcb":
        assert any(r["best"] != r["most"] for r in rows)    # the rule's move is not the most visited one
    # what the comparison would miss if it were wrong: the cap, forcing on full plies, no forcing on fast ones
    assert not _same_rows(rows, _line(option, fast_sims=0)[0])
    assert not _same_rows(rows, _line(option, k=0.0)[0])
    assert all(r["q"] == r["q"] and r["s"] == r["s"] for r in rows)
