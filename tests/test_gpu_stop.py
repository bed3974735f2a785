"""-m gpu: the early stop of a settled ply (cz_search_set_kld_gain, cz_search_set_smart_pruning, cz_search_root_kld; run.py
self --kld-gain, run.py eval --smart-pruning).

The yardstick is tests/stop_oracle.py, forced_playouts_oracle.Search with the two rules of include/czero.h in it;
tests/test_stop_cpu.py pins it to fo.Search with the rules off.  K = 1 searches and played lines are compared with it
exactly (the root statistics, the simulations run, the checkpoint count) and the reported gain within a bound derived from
the oracle's own terms; K = 8 is held by invariants that are recomputed from plain prefix searches -- a search the rules cut
is a prefix of the search they did not cut, batch by batch --, and a search that had a rule switched on and off again is the
search that never had it, bit for bit.  Every search has at most 8 games and 400 simulations."""
import json
import math
import os

import numpy as np
import pytest

import forced_playouts_oracle as fo
import stop_oracle as st
from oracle import xq_oracle as xo
from test_gpu_book import _engine_cfg
from test_gpu_search import (assert_root_equal, boards_tensor, gpu, no_act_tensors, play_config, stub_eval)  # noqa: F401

pytestmark = pytest.mark.gpu
ERR_ARG = -1                                                # include/czero.h CZ_ERR_ARG
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _pc(sims, K=1, **kw):
    d = dict(simulation_num_per_move=sims, search_threads=K, noise_eps=0.0, tau_decay_rate=0.0)
    d.update(kw)
    return play_config(**d)


def _ev(gpu, salt):
    return stub_eval(gpu, dict(kind="hash", salt=salt))


def _col(gpu, name):
    return gpu.S.COUNTER_NAMES.index(name)


# ---- 1. K = 1 single searches against the oracle ---------------------------------------------------------------------------
def test_single_searches_stop_where_the_oracle_stops(gpu):
    plans = st.planned_gains()
    assert len(plans) == 2 * len(st.positions())
    seen = set()
    for p in plans:
        what = f"{p['name']} I={p['interval']} {p['kind']}"
        # no case is left out: the margin of every uncut gain to G is far outside the bound on the engine's gain
        assert p["margin"] > 1e3 * p["bound"], what
        o = st.Search(fo.play_cfg(st.BUDGET), p["salt"], gain=p["gain"], interval=p["interval"])
        ran = o.search(p["state"])
        assert (o.checks if o.cut else None) == p["stop_at"], what
        s = gpu.S.Search(_pc(st.BUDGET), 1, seed=7)
        s.set_kld_gain(p["gain"], p["interval"])
        s.set_roots(boards_tensor(gpu, [p["state"]]))
        s.run_until_idle(_ev(gpu, p["salt"]))
        assert_root_equal(s.root_stats(), 0, o.node_stats(p["state"]), what)
        ctr, kld = s.counters(), s.root_kld()
        print(what, "ran", ctr["sims"], ran, "checks", int(kld["checks"][0]), o.checks, "gain", float(kld["gain"][0]), o.last_gain)
        assert ctr["sims"] == ran and ctr["overflow_sims"] == 0 and ctr["tree_resets"] == 0, what
        assert ctr["kld_plies"] == o.kld_plies == (1 if o.cut else 0) and ctr["kld_sims_cut"] == o.kld_sims_cut, what
        assert ctr["lead_plies"] == 0 and ctr["lead_sims_cut"] == 0, what
        assert ran + o.kld_sims_cut == st.BUDGET, what
        assert int(kld["checks"][0]) == o.checks, what
        last = o.checkpoints[-1]
        assert last["g"] is not None and abs(float(kld["gain"][0]) - last["g"]) <= st.gain_bound(last["m"], last["n"]), what
        seen.add("whole" if not o.cut else ("second" if o.checks == 2 else "later"))
        s.close()
    assert seen == {"whole", "second", "later"}


# ---- 2. K = 1 played lines in external mode --------------------------------------------------------------------------------
LINE_SIMS, LINE_I, LINE_G, LINE_PLIES = st.LINE_SIMS, st.LINE_I, st.LINE_G, st.LINE_PLIES
line_cases = st.line_cases


@pytest.mark.parametrize("idx", [0, 1, 2])
def test_played_lines_match_the_oracle(gpu, idx):
    name, state, salt, bans = line_cases()[idx]
    o = st.Search(fo.play_cfg(LINE_SIMS), salt, gain=LINE_G, interval=LINE_I)
    line = o.play_line(state, LINE_PLIES, bans=bans)
    assert len(line) == LINE_PLIES
    t = gpu.torch
    s = gpu.S.Search(_pc(LINE_SIMS), 1, seed=7)
    s.set_kld_gain(LINE_G, LINE_I)
    ev = _ev(gpu, salt)
    for ply, step in enumerate(line):
        na, nn = no_act_tensors(gpu, [step["no_act"]])
        before = s.counters()
        s.set_roots(boards_tensor(gpu, [step["state"]]), turns=t.tensor([ply], dtype=t.int32, device="cuda"), no_act=na, n_no_act=nn)
        s.run_until_idle(ev)
        what = f"{name} ply {ply}"
        after = s.counters()
        print(what, "ran", after["sims"] - before["sims"], step["ran"], "cut", step["cut"], "checks", step["checks"])
        assert after["sims"] - before["sims"] == step["ran"], what
        assert after["kld_plies"] - before["kld_plies"] == (1 if step["cut"] else 0), what
        assert_root_equal(s.root_stats(), 0, step["stats"], what)
        assert int(s.root_kld()["checks"][0]) == step["checks"], what
        assert xo.label_str(int(s.choose(None)[0])) == step["move"], what
    assert any(step["cut"] for step in line) and any(not step["cut"] and step["ran"] > 0 for step in line)
    if bans:
        assert line[2]["no_act"] and line[2]["move"] != bans[2][0]
    s.close()


# ---- 3. the unreachable-lead rule --------------------------------------------------------------------------------------------
def _groups():
    pos = st.positions()
    return [pos[:6], pos[6:]]


def _top_two(n_row):
    v = np.sort(n_row.astype(np.int64))[::-1]
    return int(v[0]), int(v[1])


@pytest.mark.parametrize("K,budget", [(1, 64), (1, 128), (1, 256), (8, 64), (8, 128), (8, 256)])
def test_lead_rule_stops_when_the_leader_cannot_be_caught(gpu, K, budget):
    i_sims, i_cut, i_plies = _col(gpu, "sims"), _col(gpu, "lead_sims_cut"), _col(gpu, "lead_plies")
    n_cut = 0
    for group in _groups():
        G = len(group)
        states = [p[1] for p in group]
        # every position of a group shares one stub: the salt of its first
        ev = _ev(gpu, group[0][2])
        plain = gpu.S.Search(_pc(budget, K=K), G, seed=3)
        plain.set_roots(boards_tensor(gpu, states))
        plain.run_until_idle(ev)
        want_move = plain.choose(None).tolist()
        s = gpu.S.Search(_pc(budget, K=K), G, seed=3)
        s.set_smart_pruning(True)
        s.set_roots(boards_tensor(gpu, states))
        s.run_until_idle(ev)
        gc = s.game_counters()
        ran = gc[:, i_sims].astype(np.int64)
        stats = s.root_stats()
        print(K, budget, "ran", ran.tolist(), "cut", gc[:, i_cut].tolist())
        assert s.choose(None).tolist() == want_move
        assert (ran <= budget).all() and (ran + gc[:, i_cut].astype(np.int64) == budget).all()
        assert ((ran < budget) == (gc[:, i_plies] == 1)).all()
        assert s.counters()["kld_plies"] == 0
        # the prefix property: the batches are the same, so a plain search of `ran` simulations is this search
        prefix = {}
        for r in sorted({int(x) for x in ran} | {int(x) - K for x in ran if x < budget and x - K > 0}):
            plain.reset_trees()
            plain.set_sims(r)
            plain.set_roots(boards_tensor(gpu, states))
            plain.run_until_idle(ev)
            prefix[r] = plain.root_stats()
        for g in range(G):
            r = int(ran[g])
            assert r % K == 0
            nm = int(stats["counts"][g])
            ref = prefix[r]
            assert nm == int(ref["counts"][g]) and int(stats["sum_n"][g]) == int(ref["sum_n"][g])
            assert stats["n"][g].tobytes() == ref["n"][g].tobytes() and stats["w"][g].tobytes() == ref["w"][g].tobytes()
            if r < budget:                                  # at the stop the lead is out of reach, one batch earlier it was not
                n_cut += 1
                a, b = _top_two(ref["n"][g, :nm])
                assert a - b > budget - r, (g, a, b, r)
                if r - K > 0:
                    a, b = _top_two(prefix[r - K]["n"][g, :nm])
                    assert a - b <= budget - (r - K), (g, a, b, r)
        plain.close()
        s.close()
    assert n_cut >= 1


@pytest.mark.parametrize("K", [1, 8])
def test_lead_rule_never_cuts_a_ply_with_a_temperature(gpu, K):
    group = _groups()[0]
    G, budget = len(group), 256         # (at 256 these roots are cut at K = 1 and at K = 8)
    states = [p[1] for p in group]
    ev = _ev(gpu, group[0][2])
    t = gpu.torch
    i_sims = _col(gpu, "sims")
    # the same roots at tau = 0 are cut (turns 40), so the two plies below are kept whole by their temperature alone
    for kw, cut_expected in ((dict(turns=t.full((G,), 40, dtype=t.int32, device="cuda")), True),
                             (dict(turns=t.full((G,), 5, dtype=t.int32, device="cuda")), False),          # 0.98 ** 6 > 0.1
                             (dict(turns=t.full((G,), 40, dtype=t.int32, device="cuda"),
                                   increase_temp=t.ones((G,), dtype=t.uint8, device="cuda")), False)):   # tau = 0.5
        s = gpu.S.Search(_pc(budget, K=K, tau_decay_rate=0.98), G, seed=3)
        s.set_smart_pruning(True)
        s.set_roots(boards_tensor(gpu, states), **kw)
        s.run_until_idle(ev)
        ran = s.game_counters()[:, i_sims].astype(np.int64)
        ctr = s.counters()
        print(K, "cut expected", cut_expected, ran.tolist())
        if cut_expected:
            assert ctr["lead_plies"] >= 1 and (ran < budget).any()
        else:
            assert ctr["lead_plies"] == 0 and ctr["lead_sims_cut"] == 0 and (ran == budget).all()
        s.close()


# ---- 4. K = 8 KLD by invariants ----------------------------------------------------------------------------------------------
def test_k_8_kld_stops_at_batch_boundaries_where_the_replayed_rule_stops(gpu):
    K, budget, interval, gain = 8, 256, 32, 2.0e-3
    group = st.positions()[:8]
    G = len(group)
    states = [p[1] for p in group]
    ev = _ev(gpu, group[0][2])
    s = gpu.S.Search(_pc(budget, K=K), G, seed=3)
    s.set_kld_gain(gain, interval)
    s.set_roots(boards_tensor(gpu, states))
    s.run_until_idle(ev)
    gc, kld, stats = s.game_counters(), s.root_kld(), s.root_stats()
    s.close()
    ran = gc[:, _col(gpu, "sims")].astype(np.int64)
    cut = gc[:, _col(gpu, "kld_sims_cut")].astype(np.int64)
    plies = gc[:, _col(gpu, "kld_plies")].astype(np.int64)
    assert (ran + cut == budget).all() and ((ran < budget) == (plies == 1)).all() and (ran % K == 0).all()
    # the plain prefix searches: the root's counts at every batch boundary
    plain = gpu.S.Search(_pc(budget, K=K), G, seed=3)
    counts = {}
    for r in range(K, budget + 1, K):
        plain.reset_trees()
        plain.set_sims(r)
        plain.set_roots(boards_tensor(gpu, states))
        plain.run_until_idle(ev)
        counts[r] = plain.root_stats()["n"].astype(np.int64)
    plain.close()
    n_cut = 0
    for g in range(G):
        nm = int(stats["counts"][g])
        # replay the rule over the boundaries (czero.h): the first checkpoint once `interval` simulations have finished
        snap, checks, last, stop_at = None, 0, None, None
        for r in range(K, budget, K):                       # (at r = budget nothing is left to start: no test point)
            n = counts[r][g, :nm]
            N = int(n.sum())
            if snap is None:
                if r < interval:
                    continue
            elif N < int(snap.sum()) + interval:
                continue
            checks += 1
            if snap is not None:
                assert N - int(snap.sum()) >= interval
                D, gval = st.kld_gain(snap.tolist(), n.tolist())
                bound = st.gain_bound(snap.tolist(), n.tolist())
                assert abs(gval - gain) > bound, (g, r, gval)             # the decision is outside the rounding of the gain
                last = (gval, bound)
                if gval < gain:
                    stop_at = r
                    break
            snap = n
        print("game", g, "ran", int(ran[g]), "replayed stop", stop_at, "checks", int(kld["checks"][g]), checks,
              "gain", float(kld["gain"][g]), last)
        assert int(ran[g]) == (stop_at if stop_at is not None else budget), g
        assert int(kld["checks"][g]) == checks, g
        assert last is not None and abs(float(kld["gain"][g]) - last[0]) <= last[1], g
        assert stats["n"][g, :nm].astype(np.int64).tolist() == counts[int(ran[g])][g, :nm].tolist(), g
        n_cut += stop_at is not None
    assert 1 <= n_cut


# ---- 5. on and off again -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8])
def test_rules_switched_off_again_are_a_search_that_never_had_them(gpu, K):
    group = st.positions()[:8]
    G = len(group)
    states = [p[1] for p in group]
    ev = _ev(gpu, group[0][2])
    setups = (lambda s: None,
              lambda s: (s.set_kld_gain(2.0e-3, 16), s.set_kld_gain(0.0, 16)),
              lambda s: (s.set_smart_pruning(True), s.set_smart_pruning(False)),
              lambda s: s.set_kld_gain(1e-300, 16),          # on, and nothing falls below it
              lambda s: s.set_kld_gain(2.0e-3, 16))
    out = []
    for setup in setups:
        s = gpu.S.Search(_pc(96, K=K), G, seed=3)
        setup(s)
        s.set_roots(boards_tensor(gpu, states))
        s.run_until_idle(ev)
        stt = s.root_stats()
        out.append((stt["n"].tobytes(), stt["w"].tobytes(), stt["p"].tobytes(), stt["sum_n"].tobytes(), s.counters(), s.pv()))
        s.close()
    plain, kld_back, lead_back, tiny, on = out
    assert kld_back == plain and lead_back == plain and tiny == plain
    assert plain[4]["kld_plies"] == 0 and on[4]["kld_plies"] >= 1 and on[:4] != plain[:4]      # ... and the rule does cut


# ---- 6. self-play --------------------------------------------------------------------------------------------------------------
def test_selfplay_marks_the_plies_the_rule_ended(gpu):
    from cchess_alphazero.engine import SelfPlayEngine
    from cchess_alphazero.lib.record_decoder import expand_records
    with open(os.path.join(GOLDEN, "book_games.json")) as f:
        book = json.load(f)["book"][:3]
    G, sims, interval, gain = 8, 64, 16, 2.0e-3
    pc = _pc(sims, K=8, max_game_length=40)
    i_games, i_kld = _col(gpu, "games"), _col(gpu, "kld_plies")

    def play(**kw):
        eng = SelfPlayEngine(_engine_cfg(pc), G, evaluator=_ev(gpu, 5), seed=5, book=book, book_rate=1.0, record_visits=True, **kw)
        games, n_done, at_boundary = [], np.zeros(G, dtype=np.uint64), np.zeros(G, dtype=np.uint64)
        try:
            eng.start(0, 0)
            for r in range(20000):
                eng.step()
                gc = eng.search.game_counters()
                fin = gc[:, i_games] != n_done
                at_boundary[fin] = gc[fin, i_kld]          # the slot's kld_plies when its game ended: all its entries are out
                n_done = gc[:, i_games].copy()
                if r % 16 == 15:
                    games += eng.drain()
                if n_done.min() >= 1:
                    break
            else:
                raise AssertionError(f"not finished: {len(games)} games")
            games += eng.drain()
            ctr = eng.counters()
        finally:
            eng.close()
        assert ctr["tree_resets"] == 0 and ctr["overflow_sims"] == 0 and ctr["visits_dropped"] == 0
        assert len(games) == int(n_done.sum()) >= G                 # every game finishes
        return games, int(at_boundary.sum()), ctr
    games, kld_plies, ctr = play(kld_gain=gain, kld_interval=interval)
    entries = [e for g in games for e in g["visits"]]
    early = [e for e in entries if e.early]
    whole = [e for e in entries if not e.early]
    print("entries", len(entries), "early", len(early), "kld_plies", kld_plies, "mean sum_n early",
          np.mean([e.sum_n for e in early]) if early else None)
    assert early and whole
    # a ply's budget takes the root's own count to `sims` (or beyond, where the reuse rule starts it over)
    assert all(e.sum_n < sims for e in early if not e.banned.any()) and all(e.sum_n >= sims for e in whole)
    assert kld_plies == len(early)
    assert ctr["lead_plies"] == 0
    planes, *_ = expand_records([g["data"] for g in games], targets="visits")          # the records parse unchanged
    assert planes.shape[0] == sum(len(g["data"]) - 1 for g in games)
    # with the rule off nothing is flagged and nothing is counted
    games0, kld0, ctr0 = play()
    assert kld0 == 0 and ctr0["kld_plies"] == 0 and ctr0["kld_sims_cut"] == 0
    assert not any(e.early for g in games0 for e in g["visits"])


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_argument_refusals(gpu):
    t = gpu.torch
    s = gpu.S.Search(_pc(16, K=4), 2, seed=1)
    stm, L = s._stream(), s.L
    assert L.cz_search_set_kld_gain(None, 1e-3, 16, stm) == ERR_ARG
    assert L.cz_search_set_smart_pruning(None, 1, stm) == ERR_ARG
    for bad in (-1.0, float("nan"), float("inf")):
        assert L.cz_search_set_kld_gain(s.h, bad, 16, stm) == ERR_ARG
    for bad in (0, -5):
        assert L.cz_search_set_kld_gain(s.h, 1e-3, bad, stm) == ERR_ARG
    for bad in (-1, 2):
        assert L.cz_search_set_smart_pruning(s.h, bad, stm) == ERR_ARG
    g = t.empty(2, dtype=t.float64, device="cuda")
    c = t.empty(2, dtype=t.int32, device="cuda")
    import ctypes as C
    pg, pcn = C.c_void_p(g.data_ptr()), C.c_void_p(c.data_ptr())
    assert L.cz_search_root_kld(None, pg, pcn, stm) == ERR_ARG
    assert L.cz_search_root_kld(s.h, None, pcn, stm) == ERR_ARG
    assert L.cz_search_root_kld(s.h, pg, None, stm) == ERR_ARG
    k = s.root_kld()                                           # both rules off: nothing measured
    assert np.isnan(k["gain"]).all() and (k["checks"] == 0).all()

    def on_kld():
        return L.cz_search_set_kld_gain(s.h, 1e-3, 16, stm)

    def on_lead():
        return L.cz_search_set_smart_pruning(s.h, 1, stm)
    # a rule with the Gumbel search, the solver, the evaluation cache: refused both ways round
    for switch_on, switch_off, other in ((lambda: s.set_gumbel(8), lambda: s.set_gumbel(0),
                                          lambda: L.cz_search_set_gumbel(s.h, 8, 50.0, 1.0, stm)),
                                         (lambda: s.set_solver(True), lambda: s.set_solver(False),
                                          lambda: L.cz_search_set_solver(s.h, 1, stm)),
                                         (lambda: s.set_eval_cache(10), lambda: s.set_eval_cache(0),
                                          lambda: L.cz_search_set_eval_cache(s.h, 10, stm))):
        switch_on()
        assert on_kld() == ERR_ARG and on_lead() == ERR_ARG
        assert L.cz_search_set_kld_gain(s.h, 0.0, 16, stm) == 0 and L.cz_search_set_smart_pruning(s.h, 0, stm) == 0   # off: never refused
        switch_off()
        for rule_on, rule_off in ((on_kld, lambda: s.set_kld_gain(0.0)), (on_lead, lambda: s.set_smart_pruning(False))):
            assert rule_on() == 0
            assert other() == ERR_ARG
            rule_off()
    with pytest.raises(gpu.N.NativeError):
        s.set_kld_gain(-1.0)
    assert s.kld_gain == 0.0 and not s.smart_pruning
    s.close()
    # the engine refuses the pairs before the library has to
    from cchess_alphazero.engine import SelfPlayEngine
    ev = _ev(gpu, 1)
    for kw, msg in ((dict(gumbel=8, record_visits=True), "gumbel"), (dict(solver=True), "solver"), (dict(eval_cache=10), "eval_cache")):
        with pytest.raises(ValueError, match=msg):
            SelfPlayEngine(_engine_cfg(_pc(16, K=4)), 2, evaluator=ev, kld_gain=1e-3, **kw)
