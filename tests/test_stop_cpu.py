"""The yardstick of tests/test_gpu_stop.py, tests/stop_oracle.py, checked on the CPU: with both rules off it is
forced_playouts_oracle.Search stat for stat; its gain is the definition evaluated directly; a ply the lead rule cuts plays
the move the uncut search plays; and the inputs of the GPU tests have the properties those tests rely on."""
import math

import numpy as np
import pytest

import forced_playouts_oracle as fo
import stop_oracle as st
from oracle import xq_oracle as xo


def _same_stats(a, b):
    return (a["sum_n"] == b["sum_n"] and (a["moves"] == b["moves"]).all() and (a["n"] == b["n"]).all()
            and a["w"].tobytes() == b["w"].tobytes() and a["p"].tobytes() == b["p"].tobytes())


@pytest.mark.parametrize("case", fo.cases(), ids=[c["name"] for c in fo.cases()])
def test_with_both_rules_off_the_oracle_is_the_plain_search(case):
    want, ws = fo.run_case(case, 0.0, 96)
    got, gs = fo.run_case(case, 0.0, 96, search_cls=st.Search)
    assert len(want) == len(got)
    for a, b in zip(want, got):
        assert a["state"] == b["state"] and a["best"] == b["best"] and _same_stats(a["stats"], b["stats"])
    for key in ("sims", "expansions", "terminal_sims", "repetition_sims"):
        assert getattr(ws, key) == getattr(gs, key)
    assert gs.cut is None and gs.checks == 0 and gs.kld_plies == 0 and gs.lead_plies == 0


def test_gain_of_hand_made_counts_is_the_definition():
    rng = np.random.default_rng(5)
    cases = [([1, 0, 3], [2, 5, 3]), ([10, 10], [10, 42]), ([7], [39]), ([0, 0, 16, 0], [3, 1, 40, 4])]
    for _ in range(40):
        k = int(rng.integers(1, 100))
        m = rng.integers(0, 30, size=k)
        m[int(rng.integers(0, k))] += 1
        cases.append((m.tolist(), (m + rng.integers(0, 20, size=k) + (np.arange(k) == 0)).tolist()))
    for m, n in cases:
        ma, na = np.asarray(m, dtype=np.float64), np.asarray(n, dtype=np.float64)
        M, N = ma.sum(), na.sum()
        live = ma > 0
        with np.errstate(divide="ignore", invalid="ignore"):
            terms = (ma[live] / M) * np.log((ma[live] / M) / (na[live] / N))
        D, g = st.kld_gain(m, n)
        # NumPy's log may differ from libm's in the last place, its sum runs pairwise: the bound of the GPU test holds it
        bound = st.gain_bound(m, n)
        assert abs(g - float(terms.sum()) / (N - M)) <= bound, (m, n)
        assert g >= -bound and math.isfinite(g)
    assert st.kld_gain([5, 5], [10, 10])[0] == 0.0            # the same distribution: nothing gained
    assert st.top_two([3, 9, 9, 1], [False] * 4) == (9, 9) and st.top_two([3, 9, 7], [False, True, False]) == (7, 3)
    assert st.top_two([4], [False]) == (4, 0) and st.top_two([4], [True]) == (0, 0)


def test_tau_is_the_reference_temperature():
    cfg = fo.play_cfg(64)
    assert st.ply_tau(cfg, 0) == 0.0 and st.ply_tau(cfg, 0, increase_temp=True) == 0.5
    assert st.ply_tau(cfg, 0, increase_temp=True, evaluate=True) == 0.0
    hot = xo.play_cfg(simulation_num_per_move=64, search_threads=1, noise_eps=0.0, tau_decay_rate=0.98)
    assert st.ply_tau(hot, 5) == 0.98 ** 6 and st.ply_tau(hot, 30) == 0.0 and st.ply_tau(hot, 5, evaluate=True) == 0.0
    assert st.ply_tau(hot, 3, evaluate=True) == 0.98 ** 4


@pytest.mark.parametrize("sims", [64, 128, 200])
def test_a_ply_the_lead_rule_cuts_plays_the_uncut_move(sims):
    n_cut = 0
    for case in fo.cases():
        lines = {}
        for lead in (False, True):
            out, s = fo.run_case(case, 0.0, sims, search_cls=lambda cfg, salt, k, lead=lead: st.Search(cfg, salt, k, lead=lead))
            lines[lead] = (out, s)
        (plain, ps), (cut, cs) = lines[False], lines[True]
        # the first search starts from the same (empty) tree in both: the same move, from no more simulations
        assert cut[0]["best"] == plain[0]["best"], case["name"]
        assert cs.sims <= ps.sims
        n_cut += cs.lead_plies
        assert cs.sims + cs.lead_sims_cut == ps.sims or case["kind"] == "reuse"
        if cs.cut == st.LEAD:                                  # at the stop the lead was out of reach
            stt = cut[-1]["stats"]
            banned = [xo.label_str(int(l)) in cut[-1]["no_act"] for l in stt["moves"]]
            a, b = st.top_two(stt["n"], banned)
            assert a - b > cs.sims_cut
    assert n_cut >= 1
    # a ply with a temperature is never cut
    case = fo.cases()[0]
    s = st.Search(fo.play_cfg(sims), case["salt"], lead=True)
    assert s.search(case["state"], increase_temp=True) == sims and s.cut is None


def test_the_planned_gains_have_their_margins_and_show_every_kind_of_stop():
    plans = st.planned_gains()
    assert len(plans) == 2 * len(st.positions()) == 24
    for p in plans:
        # zero cases are left out of the GPU test: every uncut gain is further from G than the engine's gain may be from the
        # oracle's, by three orders of magnitude
        assert p["margin"] > 1e3 * p["bound"], p["name"]
        assert (p["stop_at"] is None) == (p["kind"] == "none")
        assert p["kind"] != "all" or p["stop_at"] == 2
    stops = {p["stop_at"] for p in plans}
    assert None in stops and 2 in stops and any(x is not None and x > 2 for x in stops)
    # a stopped search is the oracle's: the checkpoint it names, the budget accounted for
    p = next(p for p in plans if p["kind"] == "mid")
    o = st.Search(fo.play_cfg(st.BUDGET), p["salt"], gain=p["gain"], interval=p["interval"])
    ran = o.search(p["state"])
    assert o.cut == st.KLD and o.checks == p["stop_at"] and ran + o.sims_cut == st.BUDGET and o.last_gain < p["gain"]
    assert ran >= 2 * p["interval"]                                # two intervals at least


def test_the_played_lines_of_the_gpu_test_decide_outside_the_rounding():
    LINE_G, LINE_I, LINE_PLIES, LINE_SIMS = st.LINE_G, st.LINE_I, st.LINE_PLIES, st.LINE_SIMS
    for name, state, salt, bans in st.line_cases():
        o = st.Search(fo.play_cfg(LINE_SIMS), salt, gain=LINE_G, interval=LINE_I)
        state_now, n_cut, n_whole = state, 0, 0
        for ply in range(LINE_PLIES):
            no_act = list((bans or {}).get(ply, []))
            o.search(state_now, no_act, turns=ply)
            for c in o.checkpoints:
                if c["g"] is not None:
                    assert abs(c["g"] - LINE_G) > 1e3 * st.gain_bound(c["m"], c["n"]), (name, ply)
            n_cut += o.cut is not None
            n_whole += o.cut is None and o.ran > 0
            state_now = xo.step(state_now, o.best_move(state_now, no_act))
        assert n_cut >= 1 and n_whole >= 1, name
