"""-m gpu: the search options that compose, run beside each other.  The moves-left utility (k_sim_ml), the draw average
(k_sim_draw) and the lower-confidence-bound move choice (k_sim_var, k_advance_lcb) -- and the two stop rules (k_sim_stop) --
are each pinned to their oracle with every other option off; include/czero.h promises that forced playouts, the playout cap,
the leaf mirror, the record columns and the per-ply reservation go on working beside them.  Here they run together.

The yardstick is tests/composed_oracle.py: the options' own oracles, which carry the forcing rule beside their score term,
with the cap's per-ply budget and the visit entry of a self-play ply; tests/test_composed_oracle_cpu.py pins it and asserts
that on the inputs used here forcing, the cap and the option each change what is compared.  K = 1 is compared exactly, K = 8
is held to the rate-0 search (the leaf mirror), to invariants and determinism (self-play) and to the device's own search on an
empty tree (the starved pool).  "ml", "draw", "lcb" name the three options; their parameters are composed_oracle.new_search's."""
import ctypes as C

import numpy as np
import pytest

import composed_oracle as co
import lcb_oracle as lo
import moves_left_search_oracle as mo
import q_record_oracle as qo
import search_model as sm
import stop_oracle as st
import stub_draw as sd
import stub_moves_left as sml
import stub_net
import surprise_oracle as su
import test_gpu_draw_search as t_draw
import test_gpu_lcb as t_lcb
import test_gpu_moves_left_search as t_ml
from oracle import xq_oracle as xo
from test_gpu_forced_playouts import _check_invariants, _entry_key
from test_gpu_leaf_mirror import G as MIRROR_G, M, WIDE_G, drive, flag_aware  # noqa: F401
from test_gpu_search import MID, assert_root_equal, boards_tensor, gpu, play_config  # noqa: F401

pytestmark = pytest.mark.gpu
OPTIONS = co.OPTIONS
CASES = sm.cases()
COUNTERS = ("sims", "expansions", "terminal_sims", "repetition_sims")


def _pc(sims, K=1, **kw):
    d = dict(simulation_num_per_move=sims, search_threads=K, noise_eps=0.0, tau_decay_rate=0.0)
    d.update(kw)
    return play_config(**d)


def _stub(option, salt):
    """The stand-in network of the option's own GPU test: planes -> (policy, value[, x or wdl])."""
    if option == "ml":
        return lambda planes: sml.ml_stub_torch(planes, salt)
    if option == "draw":
        return lambda planes: sd.draw_stub_torch(planes, salt)
    return lambda planes: stub_net.hash_stub_torch(planes, salt)


def _switch_on(s, option):
    if option == "ml":
        s.set_moves_left(mo.SLOPE, mo.CAP)
    elif option == "draw":
        s.set_draw(True, co.DRAW_SCORE)
    else:
        s.set_lcb(lo.Z, lo.RATIO)


def _records(s, option, path=None):
    """The option's records of every game's node at `path` as one dict of arrays."""
    return s.node_moves_left(path) if option == "ml" else s.node_draws(path) if option == "draw" else s.node_values(path)


def _assert_records_equal(option, got, want, what):
    """got: the records of a G = 1 search; want: the oracle's, None = not in the tree.  The option test's own comparison."""
    check = {"ml": t_ml._assert_ml_equal, "draw": t_draw._assert_draws_equal, "lcb": t_lcb._assert_values_equal}[option]
    check(got, want, what)


def _same_records(a, b):
    return a.keys() == b.keys() and all(a[key].tobytes() == b[key].tobytes() for key in a)


def _feed(s, out):
    """Write one evaluation of s.planes where the next round reads it."""
    s.policy.copy_(out[0])
    s.value.copy_(out[1])
    if len(out) > 2:
        (s.wdl_rows if s.draw_on else s.moves_left_x).copy_(out[2])


# ---- 1. single searches: option x forced playouts, K = 1, against the oracle -------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
@pytest.mark.parametrize("option", OPTIONS)
def test_single_searches_with_forced_playouts_match_the_oracle(gpu, option, case):
    """The option test's own walk -- root statistics, the option's records at the root and one level down, the counters, the
    rule's bounds and pick (lcb), choose() and pv() -- with forcing on both sides, and root_targets() against prune on the
    oracle's fields.  test_composed_oracle_cpu.py: on every case the forced pass takes edges and changes the counts."""
    if option == "ml":
        done = t_ml._walk(gpu, case, sm.SIMS, k=co.K, slope=mo.SLOPE, cap=mo.CAP)
    elif option == "draw":
        done = t_draw._walk(gpu, case, sm.SIMS, score=co.DRAW_SCORE, k=co.K)[0]
    else:
        done = len(t_lcb._walk(gpu, case, sm.SIMS, k=co.K)[0])
    assert done == (2 if case["kind"] == "reuse" else 1)


@pytest.mark.parametrize("option", OPTIONS)
def test_the_28_plane_instantiations_with_the_force_flag_set(gpu, option):
    """k_sim_ml<true>, k_sim_draw<true>, k_sim_var<true> with rc.force set: two simulations -- the root's evaluation and one
    child's, where the 28-plane stub and the oracle's 14 planes agree -- in which nothing can be forced, are still the
    oracle's search."""
    case = CASES[0]
    o = co.new_search(option, 2, case["salt"], co.K)
    assert o.search(case["state"]) == 2 and o.forced_picks == 0
    s = gpu.S.Search(_pc(2), 1, seed=7, use_history=True)
    try:
        _switch_on(s, option)
        s.set_forced_playouts(co.K)
        s.set_roots(boards_tensor(gpu, [case["state"]]))
        s.run_until_idle(_stub(option, case["salt"]))
        ref = o.node_stats(case["state"])
        assert_root_equal(s.root_stats(), 0, ref, option)
        _assert_records_equal(option, _records(s, option), co.records(o, option, case["state"]), option)
        co.assert_targets(s.root_targets(), ref, [], o.cfg.c_puct, co.K, option)
        ctr = s.counters()
        assert all(ctr[key] == getattr(o, key) for key in COUNTERS) and ctr["overflow_sims"] == 0 and ctr["tree_resets"] == 0
        assert xo.label_str(int(s.choose(None)[0])) == o.best_move(case["state"])
    finally:
        s.close()


# ---- 2. the stop rules x forced playouts, K = 1 ------------------------------------------------------------------------------
def _stop_search(gpu, state, salt, setup, evaluate=False):
    s = gpu.S.Search(_pc(st.BUDGET), 1, seed=7, evaluate=evaluate)
    try:
        setup(s)
        s.set_forced_playouts(co.K)
        s.set_roots(boards_tensor(gpu, [state]))
        s.run_until_idle(_stub("lcb", salt))
        return s.root_stats(), s.counters(), s.root_kld()
    finally:
        s.close()


def test_kld_stop_beside_forced_playouts_stops_where_the_oracle_stops(gpu):
    """stop_oracle.planned_gains() -- the searches of test_gpu_stop's K = 1 test -- with k = 2 on both sides: the root
    statistics, the simulation at which the ply ended, whether it ended early, the checkpoints.  The CPU test asserts that at
    least half the positions end early and that every decision is far outside the rounding of the engine's gain."""
    early = set()
    for p in st.planned_gains():
        what = f"{p['name']} I={p['interval']} {p['kind']}"
        o = co.stop_search(p)
        stats, ctr, kld = _stop_search(gpu, p["state"], p["salt"], lambda s: s.set_kld_gain(p["gain"], p["interval"]))
        assert_root_equal(stats, 0, o.node_stats(p["state"]), what)
        assert ctr["sims"] == o.ran and ctr["overflow_sims"] == 0 and ctr["tree_resets"] == 0, (what, ctr["sims"], o.ran)
        assert ctr["kld_plies"] == (1 if o.cut else 0) and ctr["kld_sims_cut"] == o.sims_cut == st.BUDGET - o.ran, what
        assert ctr["lead_plies"] == 0 and int(kld["checks"][0]) == o.checks, what
        last = o.checkpoints[-1]
        if last["g"] is not None:
            assert abs(float(kld["gain"][0]) - last["g"]) <= st.gain_bound(last["m"], last["n"]), what
        early |= {p["name"]} if o.cut else set()
    assert 2 * len(early) >= len(st.positions())                # at least half the positions end early


def test_lead_stop_beside_forced_playouts_stops_where_the_oracle_stops(gpu):
    """The unreachable-lead rule of the arena (evaluate, tau = 0) with k = 2 on both sides, on stop_oracle.positions()."""
    early = 0
    for name, state, salt in st.positions():
        o = co.lead_search(state, salt)
        stats, ctr, _ = _stop_search(gpu, state, salt, lambda s: s.set_smart_pruning(True), evaluate=True)
        assert_root_equal(stats, 0, o.node_stats(state), name)
        assert ctr["sims"] == o.ran and ctr["overflow_sims"] == 0 and ctr["tree_resets"] == 0, (name, ctr["sims"], o.ran)
        assert ctr["lead_plies"] == (1 if o.cut else 0) and ctr["lead_sims_cut"] == o.sims_cut and ctr["kld_plies"] == 0, name
        early += o.cut is not None
    assert 2 * early >= len(st.positions())


# ---- 3. a self-play line with everything the option composes with, K = 1 -----------------------------------------------------
@pytest.mark.parametrize("option", OPTIONS)
def test_a_self_play_line_with_cap_forcing_and_record_columns(gpu, option):
    """One self-play game at tau = 0 with the option, the playout cap, forced playouts and the q and surprise columns: the first
    six visit entries are the composed oracle's -- full plies forced and pruned, fast plies neither, one of them idle -- and,
    the positions being the oracle's, so are the moves k_advance / k_advance_lcb played.  The fast plies' sum_n pin the budget
    begin_search gives a fast ply beside the option.  (k_reserve_ml reads the same expression only when it drops a tree, and no
    test here drops one with the cap on: tree_resets is 0 below.)"""
    L = co.LINE
    want, _ = co.play_line(option, xo.INIT_STATE, L["plies"], L["sims"], L["salt"], co.K, L["fast_sims"], L["full_rate"], L["seed"])
    s = gpu.S.Search(_pc(L["sims"]), 1, seed=L["seed"])
    try:
        _switch_on(s, option)
        s.record_visits(True)
        s.set_playout_cap(L["fast_sims"], L["full_rate"])
        s.set_forced_playouts(co.K)
        s.record_values(True)
        s.record_surprise(True)
        s.start_selfplay(seed=L["seed"], first_game_id=0)
        ev = _stub(option, L["salt"])
        got = []
        for r in range(10 * L["sims"]):
            s.round()
            _feed(s, ev(s.planes))
            if r % 32 == 31:
                got = s.waiting_visits().get(0, [])
                if len(got) >= L["plies"]:
                    break
        assert len(got) >= L["plies"]
        for ply, (e, ref) in enumerate(zip(got, want)):
            what = f"{option} ply {ply}"
            assert e.ply == ply and np.array_equal(e.moves, ref["stats"]["moves"]), what        # the position: the move before it
            assert not e.banned.any() and not e.resign, what
            assert e.fast == ref["fast"] and e.pruned == ref["pruned"] and e.raw_total == ref["raw_total"], what
            assert e.sum_n == ref["stats"]["sum_n"] and np.array_equal(e.n, ref["counts"]), (what, e.n, ref["counts"])
            assert qo.same_value(qo.NAN if e.q is None else e.q, ref["q"], 1e-13), (what, e.q, ref["q"])
            assert su.same(su.NAN if e.s is None else e.s, ref["s"], ref["A"]), (what, e.s, ref["s"], ref["A"])
        ctr = s.counters()
        assert ctr["overflow_sims"] == 0 and ctr["tree_resets"] == 0 and ctr["visits_dropped"] == 0
    finally:
        s.close()


# ---- 4. the leaf mirror beside each option: the rate-0 search, bit for bit ---------------------------------------------------
@pytest.mark.parametrize("K,compact,k", [(1, False, 0.0), (8, False, 0.0), (8, True, 0.0), (8, False, co.K)])
@pytest.mark.parametrize("option", OPTIONS)
def test_leaf_mirror_beside_the_option_gives_the_rate_0_search(gpu, M, option, K, compact, k):
    """test_gpu_leaf_mirror's drive() -- 32 roots, the wide one among them, 64 simulations, the flag-aware stand-in -- with the
    option on (k: forced playouts as well).  The x / wdl rows pass the mirror as they are, like the value."""
    def setup(s):
        _switch_on(s, option)
        s.set_forced_playouts(k)

    def probe(s):
        return _records(s, option)
    ev = flag_aware(_stub(option, 3), M)
    base = drive(gpu, M, K, None, compact=compact, evaluate=ev, setup=setup, probe=probe)
    got = drive(gpu, M, K, 0.5, compact=compact, evaluate=ev, setup=setup, probe=probe)
    assert int(base["st"]["counts"][WIDE_G]) > 64 and base["ctr"]["expansions"] > MIRROR_G * 32
    for key, view in (("counts", None), ("moves", None), ("n", None), ("sum_n", None), ("w", np.uint64), ("p", np.uint32)):
        a, b = base["st"][key], got["st"][key]
        assert np.array_equal(a if view is None else a.view(view), b if view is None else b.view(view)), key
    assert all(base["ctr"][key] == got["ctr"][key] for key in COUNTERS)
    assert _same_records(base["probe"], got["probe"])
    assert any(np.asarray(v).any() for key, v in got["probe"].items() if key != "counts")
    flags = np.array([f for _, f in got["flags"]])
    assert len(flags) == got["ctr"]["expansions"] and 0 < flags.sum() < len(flags)      # some leaf was mirrored
    assert not any(f for _, f in base["flags"])


# ---- 5. K = 8 with everything on: invariants and determinism -----------------------------------------------------------------
def _selfplay_everything(gpu, M, option, pc, seed, games_wanted=32, G=32):
    s = gpu.S.Search(pc, G, seed=seed)
    try:
        _switch_on(s, option)
        s.record_visits(True)
        s.set_playout_cap(12, 0.5)
        s.set_forced_playouts(co.K)
        s.set_leaf_mirror(0.5, flags=True)
        s.record_values(True)
        s.record_surprise(True)
        s.record_maxq(True)
        s.start_selfplay(seed=seed, first_game_id=0)
        ev = flag_aware(_stub(option, 5), M)
        recs = []
        for r in range(4000):
            s.round()
            _feed(s, ev(s.planes, s.mirrored))
            if r % 16 == 15:
                recs += s.drain_records(with_visits=True)
                if len(recs) >= games_wanted:
                    break
        assert len(recs) >= games_wanted
        return sorted(recs, key=lambda g: g["game_id"]), s.counters()
    finally:
        s.close()


@pytest.mark.parametrize("option", OPTIONS)
def test_k8_self_play_with_everything_on_invariants_and_determinism(gpu, M, option):
    pc = play_config(simulation_num_per_move=48, search_threads=8, noise_eps=0.25, tau_decay_rate=0.6, max_game_length=6,
                     enable_resign_rate=0.5, resign_threshold=-0.4, min_resign_turn=4)
    recs, ctr = _selfplay_everything(gpu, M, option, pc, 17)
    assert ctr["overflow_sims"] == 0 and ctr["tree_resets"] == 0 and ctr["ring_dropped"] == 0 and ctr["visits_dropped"] == 0
    games = []
    for g in recs:                                          # the form test_gpu_forced_playouts._check_invariants reads
        assert g["visits"] is not None and g["book_index"] is None
        games.append(dict(game_id=g["game_id"], visits=g["visits"],
                          data=[xo.INIT_STATE] + [[xo.label_str(int(m))] for m in g["moves"]],
                          pruned_visits=sum(e.raw_total - int(e.n[~e.banned].sum()) for e in g["visits"] if e.pruned)))
        assert all(e.fast == f for e, f in zip(g["visits"], g["fast"]))         # (a resignation ply has an entry and no move)
        for e in g["visits"]:                                # every column is filled where the root has visits
            assert int(e.n[~e.banned].sum()) == 0 or not (e.q is None or e.s is None or e.maxq is None), g["game_id"]
    n_pruned, n_fast, removed = _check_invariants(games, pc, True, plays_most_visited=option != "lcb")
    assert n_pruned > 0 and removed > 0 and n_fast > 0
    again, ctr2 = _selfplay_everything(gpu, M, option, pc, 17)
    key = lambda g: (g["game_id"], g["turns"], g["value"], g["store"], g["resigned"], g["moves"].tolist(), g["fast"],  # noqa: E731
                     [_entry_key(e) + tuple(None if x is None else np.float64(x).tobytes() for x in (e.q, e.s, e.maxq))
                      for e in g["visits"]])
    assert [key(g) for g in again] == [key(g) for g in recs]
    assert ctr2 == ctr


# ---- 6. the starved pool under the larger statistics blocks ------------------------------------------------------------------
def _keep_with(gpu, pc, option):
    """keep_chunks of an object that has the option on: the chunks of one full search of the larger blocks."""
    probe = gpu.S.Search(pc, 1, seed=0)
    try:
        _switch_on(probe, option)
        info = (C.c_int32 * 16)()
        probe.L.cz_search_info(probe.h, info)
        return int(info[12]), probe.keep_chunks
    finally:
        probe.close()


@pytest.mark.parametrize("option", OPTIONS)
def test_the_setter_refuses_a_pool_below_the_floor_of_the_larger_blocks(gpu, option):
    """The pool is sized at creation from the plain blocks' keep_chunks and never grows.  At 800 simulations the larger blocks
    need one chunk more per game, so on a pool at the plain floor the option's setter refuses and leaves everything as it was;
    at 16 simulations both floors are 2 x 1 + 1 and the same call is accepted."""
    keep, keep_plain = _keep_with(gpu, _pc(800, K=8), option)
    s = gpu.S.Search(_pc(800, K=8), 2, seed=1, pool_chunks=1)
    try:
        assert s.pool_chunks == 2 * keep_plain + 1 < 2 * keep + 1
        before = s.memory_info()
        with pytest.raises(gpu.N.NativeError, match=rf"the pool of {s.pool_chunks} chunks is below the floor of the larger "
                                                    rf"statistics blocks, games x keep_chunks \+ 1 = {2 * keep + 1}"):
            _switch_on(s, option)
        assert (s.moves_left_slope, s.draw_on, s.lcb) == (0.0, False, 0.0)
        info = (C.c_int32 * 16)()
        s.L.cz_search_info(s.h, info)
        assert info[12] == keep_plain and s.memory_info() == before and not _records(s, option)["counts"].any()
    finally:
        s.close()
    s = gpu.S.Search(_pc(16, K=8), 2, seed=1, pool_chunks=1)
    try:
        assert s.pool_chunks == 3
        _switch_on(s, option)
        assert (s.moves_left_slope > 0.0, s.draw_on, s.lcb > 0.0) == (option == "ml", option == "draw", option == "lcb")
    finally:
        s.close()


@pytest.mark.parametrize("option", OPTIONS)
def test_exhausted_pool_under_the_larger_blocks_drops_one_tree(gpu, option):
    """test_gpu_search.test_exhausted_pool_drops_one_tree_and_returns_its_chunks with the option on: two external-mode games
    share a pool with one spare chunk above the option's floor, games x keep_chunks + 1 with the keep_chunks of the larger
    blocks.  k_reserve_ml's fallback drops a tree, counted; the dropped game's search is then a search on an empty tree.  No
    oracle searches with 8 threads and the option, so the yardstick is the device: one single-game object per game with room
    for everything -- the searches K = 1 pins to the oracle -- whose tree is reset whenever the starved game's result is not
    its own.  n, W, p, the option's records and the move are compared."""
    pc = _pc(800, K=8)
    keep, keep_plain = _keep_with(gpu, pc, option)
    assert keep > keep_plain                                # 800 simulations of the larger blocks need one more chunk
    states = [xo.INIT_STATE, MID]
    s = gpu.S.Search(pc, 2, seed=1, pool_chunks=2 * keep + 1)
    refs = [gpu.S.Search(pc, 1, seed=1) for _ in states]
    ev = _stub(option, 19)
    t = gpu.torch
    try:
        for x in [s] + refs:
            _switch_on(x, option)
        assert s.pool_chunks == 2 * keep + 1
        resets = 0
        for ply in range(16):
            s.set_roots(boards_tensor(gpu, states), turns=t.full((2,), ply, dtype=t.int32, device="cuda"))
            s.run_until_idle(ev)
            st_, rec, act = s.root_stats(), _records(s, option), s.choose(None)
            for g, ref in enumerate(refs):
                def search():
                    ref.set_roots(boards_tensor(gpu, [states[g]]), turns=t.full((1,), ply, dtype=t.int32, device="cuda"))
                    ref.run_until_idle(ev)
                    return ref.root_stats(), _records(ref, option), ref.choose(None)

                def same(want):
                    return (all(st_[key][g].tobytes() == want[0][key][0].tobytes()
                                for key in ("counts", "moves", "n", "w", "p", "sum_n"))
                            and all(rec[key][g].tobytes() == want[1][key][0].tobytes() for key in rec) and act[g] == want[2][0])
                want = search()
                if not same(want):
                    ref.reset_trees()
                    want = search()
                    resets += 1
                assert same(want), (option, ply, g)
                assert not xo.done(states[g])[0]
                states[g] = xo.step(states[g], xo.label_str(int(act[g])))
        c, m = s.counters(), s.memory_info()
        assert c["tree_resets"] == resets and resets > 0 and c["overflow_sims"] == 0, (c, resets, m)
        assert c["chunks_taken"] >= 1 and m["free_chunks"] + m["held_chunks"] == m["pool_chunks"]
        s.reset_trees()
        m = s.memory_info()                                 # every game keeps the chunks of one full search, the spare one is free
        assert m["free_chunks"] == 1 and m["held_chunks"] == 2 * keep and m["nodes"] == 0
        print(f"{option}: keep_chunks {keep} (plain {keep_plain}), tree_resets {resets}")
    finally:
        for x in [s] + refs:
            x.close()


@pytest.mark.parametrize("option", OPTIONS)
def test_starved_pool_under_the_larger_blocks_keeps_self_play_running(gpu, option):
    """test_gpu_search.test_starved_pool_keeps_self_play_running with the option on: 64 games on a pool with 16 spare chunks
    above the option's floor.  Trees are dropped, chunks circulate, nothing is lost or duplicated, no simulation is dropped."""
    pc = play_config(simulation_num_per_move=160, search_threads=8, max_game_length=40, tau_decay_rate=0.9)
    G = 64
    keep, _ = _keep_with(gpu, pc, option)
    s = gpu.S.Search(pc, G, seed=5, pool_chunks=G * keep + 16, max_nodes_per_game=12000)
    try:
        _switch_on(s, option)
        s.start_selfplay(seed=5)
        ev = _stub(option, 29)
        c = s.counters()
        for r in range(3000):
            s.round()
            _feed(s, ev(s.planes))
            if r % 100 == 99:
                m, c = s.memory_info(), s.counters()
                assert m["free_chunks"] + m["held_chunks"] == m["pool_chunks"], m
                assert m["held_chunks_max_game"] <= s.max_chunks
                in_flight = c["expansions"] + c["terminal_sims"] + c["repetition_sims"] - c["sims"]
                assert 0 <= in_flight <= G * 8, (c, in_flight)
                if c["games"] >= G and c["tree_resets"] > 0:
                    break
        assert c["games"] >= G and c["tree_resets"] > 0, c
        assert c["overflow_sims"] == 0 and c["depth_overflow"] == 0, c
        recs = s.drain_records(1 << 14)
        assert recs and all(0 < r["turns"] <= 2 * 40 + 1 for r in recs)
        print(f"{option}: keep_chunks {keep}, tree_resets {c['tree_resets']}, games {c['games']}")
    finally:
        s.close()
