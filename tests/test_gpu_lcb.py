"""-m gpu: the lower-confidence-bound move choice (cz_search_set_lcb, cz_search_node_values, cz_search_root_lcb, cz_lcb_pick;
run.py self / eval --lcb, the UCI options LCB and LCBMinVisits).

The yardstick is tests/lcb_oracle.py, search_model.Search with the V records and the rule of include/czero.h in it;
tests/test_lcb_cpu.py pins it to the plain search and pins the cases on which the rule changes the move.  K = 1 searches are
compared with it exactly: s2 is a float64 accumulated where W is and in the same order, and the rule is float64 arithmetic in a
fixed order with every operation rounded on its own.  K = 8 is held by invariants.  Every search here has at most 9 games and at
most 200 simulations."""
import ctypes as C
import io
import logging
import time
import types

import numpy as np
import pytest

import composed_oracle as co
import lcb_oracle as lo
import search_model as sm
import stub_net
from oracle import xq_oracle as xo
from test_gpu_search import (assert_root_equal, boards_tensor, gpu, no_act_tensors, play_config)  # noqa: F401
from test_lcb_cpu import DIFFER_Z2, DIFFER_Z5

pytestmark = pytest.mark.gpu
ERR_ARG = -1                                                # include/czero.h CZ_ERR_ARG
COUNTERS = ("sims", "expansions", "terminal_sims", "repetition_sims")
SEARCH_COUNTERS = COUNTERS + ("parked", "sum_depth", "max_depth", "edges_visited", "leaf_moves", "overflow_sims", "tree_resets",
                              "depth_overflow")
Z, R = lo.Z, lo.RATIO
LCB_PHRASE = "the lower-confidence-bound move choice is on (cz_search_set_lcb)"
DRAW_PHRASE = "the draw average is on (cz_search_set_draw)"
ML_PHRASE = "the moves-left utility is on (cz_search_set_moves_left)"


def _pc(sims, K=1, **kw):
    return play_config(simulation_num_per_move=sims, search_threads=K, noise_eps=0.0, tau_decay_rate=0.0, **kw)


def _err(L):
    return L.cz_last_error().decode()


def _eval(salt):
    return lambda planes: stub_net.hash_stub_torch(planes, salt)


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _assert_values_equal(got, want, what):
    """got: node_values() of a G = 1 search; want: the oracle's node_values(state), None = not in the tree."""
    if want is None:
        assert int(got["counts"][0]) == 0 and not got["s2"].any() and not got["vn"].any(), what
        return
    nm = len(want["vn"])
    assert int(got["counts"][0]) == nm, what
    assert (got["vn"][0, :nm] == want["vn"]).all(), (what, got["vn"][0, :nm], want["vn"])
    assert (_bits(got["s2"][0, :nm]) == _bits(want["s2"])).all(), (what, got["s2"][0, :nm], want["s2"])
    assert not got["s2"][0, nm:].any() and not got["vn"][0, nm:].any(), what


def _walk(gpu, case, sims, z=Z, use_history=False, k=0.0):
    """One case on the device and in the oracle, search by search: root statistics, V records at the root and one level below
    the played move, the rule's bounds and pick, the pruned counts, the played move, the line's first move.  k: forced
    playouts on both sides.  Returns (the played moves, the most visited moves)."""
    o = lo.Search(sm.play_cfg(sims), case["salt"], k, z, R)
    s = gpu.S.Search(_pc(sims), 1, seed=7, use_history=use_history)
    s.set_lcb(z, R)
    s.set_forced_playouts(k)
    line = [(case["state"], [sm.ban_of(case, sims)] if case["kind"] == "ban" else [])]
    played, most = [], []
    try:
        while line:
            state, no_act = line.pop(0)
            ran = o.search(state, no_act)
            na, nn = no_act_tensors(gpu, [no_act])
            before = s.counters()
            s.set_roots(boards_tensor(gpu, [state]), no_act=na, n_no_act=nn)
            s.run_until_idle(_eval(case["salt"]))
            what = f"{case['name']} search {len(played)} z {z}"
            ctr = s.counters()
            assert ctr["sims"] - before["sims"] == ran and ctr["overflow_sims"] == 0 and ctr["tree_resets"] == 0, what
            for key in COUNTERS:
                assert ctr[key] == getattr(o, key), (what, key, ctr[key], getattr(o, key))
            ref = o.node_stats(state)
            assert_root_equal(s.root_stats(), 0, ref, what)
            _assert_values_equal(s.node_values(), o.node_values(state), what)
            nm = len(ref["moves"])
            want_lcb, want_pick = o.root_lcb(state, no_act)
            lcb, pick = s.root_lcb()
            assert int(pick[0]) == want_pick, (what, int(pick[0]), want_pick)
            assert np.array_equal(np.isnan(lcb[0, :nm]), np.isnan(want_lcb)) and np.isnan(lcb[0, nm:]).all(), what
            ok = ~np.isnan(want_lcb)
            assert ok.any() and (_bits(lcb[0, :nm][ok]) == _bits(want_lcb[ok])).all(), (what, lcb[0, :nm], want_lcb)
            co.assert_targets(s.root_targets(), ref, no_act, o.cfg.c_puct, k, what)
            best = o.best_move(state, no_act)
            assert xo.label_str(int(s.choose(None)[0])) == best, what
            assert xo.label_str(int(s.pv()[0][0])) == best, what
            assert int(ref["moves"][want_pick]) == xo.label_of_str(best)
            # one level below the played move: the child's records
            child = xo.step(state, best)
            _assert_values_equal(s.node_values([xo.label_of_str(best)]), o.node_values(child), f"{what} child")
            if o.node_stats(child) is not None:
                st = s.node_stats([xo.label_of_str(best)])
                assert_root_equal(st, 0, o.node_stats(child), f"{what} child")
            played.append(best)
            most.append(o.most_visited(state, no_act))
            if case["kind"] == "reuse" and len(played) == 1:
                line.append((child, []))
    finally:
        s.close()
    return played, most


# ---- 1. K = 1 against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sm.cases(), ids=lambda c: c["name"])
def test_single_searches_match_the_oracle(gpu, case):
    played, most = _walk(gpu, case, sm.SIMS)
    assert len(played) == (2 if case["kind"] == "reuse" else 1)
    assert (played[0] != most[0]) == (case["name"] in DIFFER_Z2)        # the rule changes the move where the CPU test says


@pytest.mark.parametrize("name", DIFFER_Z2)
def test_z_is_read(gpu, name):
    case = [c for c in sm.cases() if c["name"] == name][0]
    played, most = _walk(gpu, case, sm.SIMS, z=5.0)
    assert (played[0] != most[0]) == (name in DIFFER_Z5)


def test_the_28_plane_instantiation_matches_the_oracle(gpu):
    """k_sim_var<true>.  An external root without a game history takes a leaf's second plane block from the search path, and the
    stub hashes all 28 planes, while the oracle hashes the position alone: the two agree where the block is empty, at depth 0
    and 1.  A search of 2 simulations stays there: the root's evaluation and one child's."""
    case = sm.cases()[0]
    o = lo.Search(sm.play_cfg(2), case["salt"], 0.0, Z, R)
    o.search(case["state"])
    s = gpu.S.Search(_pc(2), 1, seed=7, use_history=True)
    try:
        s.set_lcb(Z, R)
        s.set_roots(boards_tensor(gpu, [case["state"]]))
        s.run_until_idle(_eval(case["salt"]))
        assert_root_equal(s.root_stats(), 0, o.node_stats(case["state"]), "28 planes")
        _assert_values_equal(s.node_values(), o.node_values(case["state"]), "28 planes")
        got = s.node_values()
        assert int(got["vn"].sum()) == 1 and got["s2"].sum() > 0.0
        assert xo.label_str(int(s.choose(None)[0])) == o.best_move(case["state"])       # no eligible edge: the most visited
        assert int(s.root_lcb()[1][0]) == o.root_lcb(case["state"])[1] and np.isnan(s.root_lcb()[0]).all()
    finally:
        s.close()


def test_a_played_line_in_self_play_matches_the_oracle(gpu):
    """One self-play game, tau = 0 from the start (tau_decay_rate = 0), tree reuse: k_advance_lcb plays the oracle's moves.  The
    visit entries of the first four plies are the oracle's root counts, position by position."""
    sims, plies, salt = 120, 4, 21
    want, _ = lo.play_line(xo.INIT_STATE, plies, sims, salt)
    assert any(r["best"] != r["most"] for r in want[:3])       # (a condition on the input: the rule changes a played move)
    s = gpu.S.Search(_pc(sims), 1, seed=7)
    try:
        s.set_lcb(Z, R)
        s.record_visits(True)
        s.start_selfplay(seed=7, first_game_id=0)
        ev = _eval(salt)
        got = []
        for r in range(40 * sims):
            s.round()
            p, v = ev(s.planes)
            s.policy.copy_(p)
            s.value.copy_(v)
            if r % 32 == 31:
                got = s.waiting_visits().get(0, [])
                if len(got) >= plies:
                    break
        assert len(got) >= plies
        for ply in range(plies):
            e, ref = got[ply], want[ply]["stats"]
            assert e.ply == ply and np.array_equal(e.moves, ref["moves"]), ply      # the same position: the same move before it
            assert np.array_equal(e.n, ref["n"]) and e.sum_n == ref["sum_n"], ply
        ctr = s.counters()
        assert ctr["overflow_sims"] == 0 and ctr["tree_resets"] == 0
    finally:
        s.close()


# ---- 2. K = 8 by invariants ---------------------------------------------------------------------------------------------------------
def _search_k8(gpu, setup, sims=200, salt=5):
    states = [c["state"] for c in sm.cases() if c["name"] in ("wide", "init")]
    s = gpu.S.Search(_pc(sims, K=8), len(states), seed=7)
    try:
        setup(s)
        s.set_roots(boards_tensor(gpu, states))
        s.run_until_idle(_eval(salt))
        out = dict(stats=s.root_stats(), vr=s.node_values(), ctr=s.counters(), choose=s.choose(None), pv=s.pv(4))
        if s.lcb > 0.0:
            out["lcb"], out["pick"] = s.root_lcb()
            path = np.array([[m] for m in out["choose"]], dtype=np.uint16)
            out["child_stats"], out["child_vr"] = s.node_stats(path), s.node_values(path)
    finally:
        s.close()
    return out


def _same_stats(a, b):
    for key, view in (("moves", None), ("n", None), ("sum_n", None), ("counts", None), ("w", np.uint64), ("p", np.uint32)):
        x, y = (a[key], b[key]) if view is None else (a[key].view(view), b[key].view(view))
        assert np.array_equal(x, y), key


def test_k8_invariants(gpu):
    plain = _search_k8(gpu, lambda s: None)
    assert plain["stats"]["counts"].max() > 64                 # the wide position: both halves of the root's edges
    on = _search_k8(gpu, lambda s: s.set_lcb(Z, R))
    again = _search_k8(gpu, lambda s: s.set_lcb(Z, R))
    _same_stats(plain["stats"], on["stats"])                   # n, w, p: the plain search bit for bit
    assert {k: plain["ctr"][k] for k in SEARCH_COUNTERS} == {k: on["ctr"][k] for k in SEARCH_COUNTERS}
    assert on["ctr"]["overflow_sims"] == 0 and on["ctr"]["tree_resets"] == 0
    for st, vr in ((on["stats"], on["vr"]), (on["child_stats"], on["child_vr"])):
        n, w, s2, vn = st["n"], st["w"], vr["s2"], vr["vn"]
        assert np.array_equal(vr["counts"], st["counts"]) and vn.any()
        assert np.array_equal(vn, n)                           # idle: every visit is a completed backup
        assert (s2 >= 0.0).all() and (s2 <= 4.0 * vn).all()
        assert (s2 * vn >= w * w * (1 - 1e-12)).all()          # Cauchy-Schwarz
    assert (on["vr"]["vn"].sum(axis=1) == on["stats"]["sum_n"] - 1).all()      # the simulations that ended below the root
    for g in range(2):                                         # the rule on the device's own fields, in NumPy
        nm = int(on["stats"]["counts"][g])
        lcb, pick = lo.lcb_pick(on["stats"]["moves"][g, :nm], on["stats"]["n"][g, :nm], on["stats"]["w"][g, :nm],
                                on["vr"]["s2"][g, :nm], on["vr"]["vn"][g, :nm], Z, R)
        assert int(on["pick"][g]) == pick and int(on["choose"][g]) == int(on["stats"]["moves"][g, pick]) == on["pv"][g][0]
        ok = ~np.isnan(lcb)
        assert ok.any() and np.array_equal(np.isnan(on["lcb"][g, :nm]), ~ok) and np.isnan(on["lcb"][g, nm:]).all()
        assert np.array_equal(_bits(on["lcb"][g, :nm][ok]), _bits(lcb[ok]))
    for key in ("s2", "vn"):                                   # two runs are identical
        assert np.array_equal(on["vr"][key].view(np.uint64 if key == "s2" else np.int32),
                              again["vr"][key].view(np.uint64 if key == "s2" else np.int32)), key
    _same_stats(on["stats"], again["stats"])
    assert np.array_equal(on["choose"], again["choose"]) and np.array_equal(on["pick"], again["pick"])
    assert np.array_equal(np.isnan(on["lcb"]), np.isnan(again["lcb"]))
    assert np.array_equal(_bits(on["lcb"][~np.isnan(on["lcb"])]), _bits(again["lcb"][~np.isnan(on["lcb"])]))


# ---- 3. the rule alone ---------------------------------------------------------------------------------------------------------------
def test_lcb_pick_on_the_grid(gpu):
    t = gpu.torch
    rows = lo.grid()
    labels, n, w, s2, vn, ne = lo.grid_arrays(rows)
    dev = lambda a: t.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    lab_d = dev(labels).view(t.uint16)
    for zr in sorted({(r["z"], r["ratio"]) for r in rows}):
        lcb, pick = gpu.S.lcb_pick(lab_d, dev(n), dev(w), dev(s2), dev(vn), dev(ne), *zr)
        lcb, pick = lcb.cpu().numpy(), pick.cpu().numpy()
        for i, row in enumerate(rows):
            if (row["z"], row["ratio"]) != zr:
                continue
            k = int(ne[i])
            want_lcb, want_pick = lo.lcb_pick(labels[i, :k], n[i, :k], w[i, :k], s2[i, :k], vn[i, :k], *zr)
            assert int(pick[i]) == want_pick == row["expect"], (row["name"], int(pick[i]), want_pick)
            assert np.isnan(lcb[i, k:]).all(), row["name"]
            assert np.array_equal(np.isnan(lcb[i, :k]), np.isnan(want_lcb)), (row["name"], lcb[i, :k], want_lcb)
            ok = ~np.isnan(want_lcb)
            assert (_bits(lcb[i, :k][ok]) == _bits(want_lcb[ok])).all(), (row["name"], lcb[i, :k], want_lcb)
    L = gpu.N.lib()
    st = C.c_void_p(t.cuda.current_stream().cuda_stream)
    d = C.c_double
    p = lambda x: C.c_void_p(x.data_ptr())
    a = (lab_d, dev(n), dev(w), dev(s2), dev(vn), dev(ne))
    out, pk = t.empty((len(rows), 128), dtype=t.float64, device="cuda"), t.empty((len(rows),), dtype=t.int32, device="cuda")
    for z, r in ((-1.0, 0.15), (float("nan"), 0.15), (float("inf"), 0.15), (2.0, -0.1), (2.0, 1.5), (2.0, float("nan"))):
        assert L.cz_lcb_pick(*[p(x) for x in a], len(rows), d(z), d(r), p(out), p(pk), st) == ERR_ARG, (z, r)
    assert L.cz_lcb_pick(None, *[p(x) for x in a[1:]], len(rows), d(2.0), d(0.15), p(out), p(pk), st) == ERR_ARG


# ---- 4. off means off, switching -----------------------------------------------------------------------------------------------------
def test_off_means_off(gpu):
    """With z = 0 a search object that has heard of the option is the one that never did: counters, root statistics, the move,
    the line; node_values is all 0."""
    for case in sm.cases():
        outs = []
        for heard in (False, True):
            s = gpu.S.Search(_pc(64), 1, seed=7)
            try:
                if heard:
                    s.set_lcb(2.0, R)
                    s.set_lcb(0.0, R)
                no_act = [sm.ban_of(case, 64)] if case["kind"] == "ban" else []
                na, nn = no_act_tensors(gpu, [no_act])
                s.set_roots(boards_tensor(gpu, [case["state"]]), no_act=na, n_no_act=nn)
                s.run_until_idle(_eval(case["salt"]))
                vr = s.node_values()
                assert not vr["counts"].any() and not vr["s2"].any() and not vr["vn"].any()
                outs.append(dict(stats=s.root_stats(), ctr=s.counters(), choose=s.choose(None), pv=s.pv(8, with_visits=True),
                                 mem=s.memory_info()))
            finally:
                s.close()
        a, b = outs
        _same_stats(a["stats"], b["stats"])
        assert a["ctr"] == b["ctr"], case["name"]
        assert all(a["mem"][k] == b["mem"][k] for k in ("tree_bytes", "nodes")), case["name"]
        assert np.array_equal(a["choose"], b["choose"])
        assert np.array_equal(a["pv"][0], b["pv"][0]) and np.array_equal(a["pv"][1], b["pv"][1])


def test_switching_resets_the_trees(gpu):
    """Switching on over grown trees (their statistics blocks have no V records) and off again starts the trees over; a new z or
    ratio while on does not.  The larger blocks show in memory_info only while the option is on."""
    s = gpu.S.Search(_pc(64), 1, seed=7)
    try:
        def search():
            s.set_roots(boards_tensor(gpu, [xo.INIT_STATE]))
            s.run_until_idle(_eval(4))
            return s.memory_info()
        off = search()
        assert int(s.root_stats()["sum_n"][0]) == 64 and off["nodes"] > 1
        keep0 = s.keep_chunks
        s.set_lcb(Z, R)
        assert s.memory_info()["nodes"] == 0
        on = search()
        assert on["nodes"] == off["nodes"]
        blocks = s.counters()["stat_blocks"]
        assert on["tree_bytes"] > off["tree_bytes"]         # one more granule per edge of every statistics block
        s.set_lcb(3.0, 0.5)                                 # new parameters, still on: nothing is reset
        assert s.memory_info()["nodes"] == on["nodes"] and (s.lcb, s.lcb_min_ratio) == (3.0, 0.5)
        s.set_lcb(0.0)
        assert s.memory_info()["nodes"] == 0 and not s.node_values()["counts"].any() and s.lcb == 0.0
        back = search()
        assert back["tree_bytes"] == off["tree_bytes"] and back["nodes"] == off["nodes"] and blocks > 0
        info = (C.c_int32 * 16)()
        s.L.cz_search_info(s.h, info)
        assert info[12] == keep0
    finally:
        s.close()


# ---- 5. the setter ---------------------------------------------------------------------------------------------------------------
_ON = {"gumbel": ("cz_search_set_gumbel", lambda L, h, st: L.cz_search_set_gumbel(h, 8, 50.0, 1.0, st),
                  lambda L, h, st: L.cz_search_set_gumbel(h, 0, 50.0, 1.0, st), "the Gumbel root search is on (cz_search_set_gumbel)"),
       "solver": ("cz_search_set_solver", lambda L, h, st: L.cz_search_set_solver(h, 1, st),
                  lambda L, h, st: L.cz_search_set_solver(h, 0, st), "the MCTS solver is on (cz_search_set_solver)"),
       "kld_gain": ("cz_search_set_kld_gain", lambda L, h, st: L.cz_search_set_kld_gain(h, 1e-4, 100, st),
                    lambda L, h, st: L.cz_search_set_kld_gain(h, 0.0, 100, st), "the KLD-gain stop is on (cz_search_set_kld_gain)"),
       "smart_pruning": ("cz_search_set_smart_pruning", lambda L, h, st: L.cz_search_set_smart_pruning(h, 1, st),
                         lambda L, h, st: L.cz_search_set_smart_pruning(h, 0, st),
                         "the unreachable-lead stop is on (cz_search_set_smart_pruning)"),
       "eval_cache": ("cz_search_set_eval_cache", lambda L, h, st: L.cz_search_set_eval_cache(h, 10, st),
                      lambda L, h, st: L.cz_search_set_eval_cache(h, 0, st), "the evaluation cache is on (cz_search_set_eval_cache)")}


def test_setter_refusals_follow_the_lists(gpu):
    from cchess_alphazero import search_options as so
    assert sorted(_ON) == sorted(k for k, _ in so.LCB_EXCLUDES)
    t = gpu.torch
    s = gpu.S.Search(_pc(16), 2, seed=1)
    L, h = s.L, s.h
    st = C.c_void_p(t.cuda.current_stream().cuda_stream)
    rows = t.zeros((s.slots, 3), dtype=t.float32, device="cuda")
    x = t.zeros((s.slots,), dtype=t.float32, device="cuda")
    rp, xp = C.c_void_p(rows.data_ptr()), C.c_void_p(x.data_ptr())
    d = C.c_double
    on = lambda: L.cz_search_set_lcb(h, d(Z), d(R), st)
    off = lambda: L.cz_search_set_lcb(h, d(0.0), d(R), st)
    try:
        assert L.cz_search_set_lcb(None, d(Z), d(R), st) == ERR_ARG
        for z in (-0.5, float("nan"), float("inf")):
            assert L.cz_search_set_lcb(h, d(z), d(R), st) == ERR_ARG
            assert _err(L) == "cz_search_set_lcb: z negative or not finite"
        for r in (-0.1, 1.0001, float("nan")):
            assert L.cz_search_set_lcb(h, d(Z), d(r), st) == ERR_ARG
            assert _err(L) == "cz_search_set_lcb: min_ratio outside [0, 1] or not finite"
        assert L.cz_search_set_lcb(h, d(Z), d(0.0), st) == 0 and L.cz_search_set_lcb(h, d(Z), d(1.0), st) == 0 and off() == 0
        assert L.cz_search_root_lcb(h, None, None, st) == ERR_ARG and "is off" in _err(L)
        for key, (entry, sw_on, sw_off, phrase) in _ON.items():
            assert sw_on(L, h, st) == 0, key
            assert on() == ERR_ARG, key
            assert _err(L) == f"cz_search_set_lcb: {phrase}", key
            assert off() == 0                                                          # switching off is never refused
            assert sw_off(L, h, st) == 0, key
            assert on() == 0, key
            assert sw_on(L, h, st) == ERR_ARG, key
            assert _err(L) == f"{entry}: {LCB_PHRASE}", key
            assert sw_off(L, h, st) == 0, key                                          # nor is theirs
            assert off() == 0
        # the moves-left utility and the draw average: the same granules
        ml_on = lambda: L.cz_search_set_moves_left(h, d(0.01), d(0.1), xp, st)
        ml_off = lambda: L.cz_search_set_moves_left(h, d(0.0), d(0.1), None, st)
        dr_on = lambda: L.cz_search_set_draw(h, 1, d(0.25), rp, st)
        dr_off = lambda: L.cz_search_set_draw(h, 0, d(0.0), None, st)
        for name, o_on, o_off, phrase in (("cz_search_set_moves_left", ml_on, ml_off, ML_PHRASE),
                                          ("cz_search_set_draw", dr_on, dr_off, DRAW_PHRASE)):
            assert o_on() == 0
            assert on() == ERR_ARG and _err(L) == f"cz_search_set_lcb: {phrase}"
            assert off() == 0 and o_off() == 0 and on() == 0
            assert o_on() == ERR_ARG and _err(L) == f"{name}: {LCB_PHRASE}"
            assert o_off() == 0 and off() == 0
        # a script: refused beside the option, and the option beside it
        s.record_visits(True)
        script = (np.stack([xo.state_to_board(xo.INIT_STATE)]).astype(np.int8), np.array([0], dtype=np.uint16),
                  np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int8))
        assert on() == 0
        with pytest.raises(gpu.N.NativeError, match="cz_search_set_script: " + LCB_PHRASE.replace("(", r"\(").replace(")", r"\)")):
            s.set_script(*script)
        assert off() == 0
        s.set_script(*script)
        assert on() == ERR_ARG and _err(L) == "cz_search_set_lcb: a script is set (cz_search_set_script)"
        s.set_script()
        # what it composes with
        s.set_playout_cap(8, 0.5)
        s.set_forced_playouts(2.0)
        s.set_leaf_mirror(0.5)
        s.record_values(True)
        s.record_surprise(True)
        assert on() == 0
    finally:
        s.close()


# ---- 6. the wrapper -------------------------------------------------------------------------------------------------------------
def test_search_wrapper(gpu):
    s = gpu.S.Search(_pc(16), 2, seed=1)
    try:
        assert (s.lcb, s.lcb_min_ratio) == (0.0, 0.15)
        got = s.node_values()
        assert not got["counts"].any() and got["s2"].shape == (2, 128) and got["vn"].shape == (2, 128)
        assert got["s2"].dtype == np.float64 and got["vn"].dtype == np.int32
        with pytest.raises(gpu.N.NativeError, match="is off"):
            s.root_lcb()
        s.set_lcb(2.0)
        assert (s.lcb, s.lcb_min_ratio) == (2.0, 0.15)
        lcb, pick = s.root_lcb()
        assert lcb.shape == (2, 128) and pick.shape == (2,) and (pick == -1).all() and np.isnan(lcb).all()   # no roots yet
        with pytest.raises(gpu.N.NativeError, match="z negative"):
            s.set_lcb(-1.0)
        with pytest.raises(gpu.N.NativeError, match="min_ratio outside"):
            s.set_lcb(2.0, 1.5)
        s.set_solver(False)
        with pytest.raises(gpu.N.NativeError, match="cz_search_set_solver: "):
            s.set_solver(True)
        assert (s.lcb, s.lcb_min_ratio) == (2.0, 0.15)         # a refusal leaves the attributes as they were
        s.set_lcb()
        assert (s.lcb, s.lcb_min_ratio) == (0.0, 0.15)
        s.set_solver(True)
        with pytest.raises(gpu.N.NativeError, match="cz_search_set_lcb: the MCTS solver is on"):
            s.set_lcb(2.0, 0.3)
        assert (s.lcb, s.lcb_min_ratio) == (0.0, 0.15)
    finally:
        s.close()


# ---- 7. the front ends -----------------------------------------------------------------------------------------------------------
def _net(seed, value_outputs=1):
    import torch
    from cchess_alphazero.agent.model import CChessNet
    torch.manual_seed(seed)
    return CChessNet(cnn_filter_num=128, res_layer_num=2, value_outputs=value_outputs).eval()


def _cfg(**engine):
    from cchess_alphazero.config import Config
    cfg = Config("mini")
    cfg.model.cnn_filter_num, cfg.model.res_layer_num = 128, 2
    cfg.play.simulation_num_per_move, cfg.play.search_threads, cfg.play.noise_eps = 16, 8, 0.0
    cfg.play.max_game_length = 8
    for k, v in engine.items():
        setattr(cfg.engine, k, v)
    return cfg


def test_selfplay_engine_runs_and_logs_the_line(gpu, tmp_path, monkeypatch, caplog):
    import torch as t
    from cchess_alphazero import search_options as so
    from cchess_alphazero.engine import SelfPlayEngine
    from cchess_alphazero.worker.self_play import SelfPlayWorker
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    with pytest.raises(ValueError, match="lcb excludes solver"):
        SelfPlayEngine(_cfg(lcb=2.0, solver=True), 2, net=_net(1), dtype=t.float32, seed=13)
    with pytest.raises(ValueError, match="lcb_min_visits 2"):
        SelfPlayEngine(_cfg(lcb=2.0, lcb_min_visits=2.0), 2, net=_net(1), dtype=t.float32, seed=13)
    cfg = _cfg(lcb=2.0, games_per_gpu=2, use_hip_graph=False, net_dtype="float32")
    w = SelfPlayWorker(cfg, model=types.SimpleNamespace(model=_net(2)))
    try:
        with caplog.at_level(logging.INFO, logger="cchess_alphazero.worker.self_play"):
            w._make_engine()
        line = so.LCB_LOG.format(lcb=2.0, lcb_min_visits=0.15)
        assert sum(line in r.getMessage() for r in caplog.records) == 1
        eng = w.engine
        assert eng.lcb_on and (eng.search.lcb, eng.search.lcb_min_ratio) == (2.0, 0.15) and eng.search.G == 2
        for _ in range(3):
            eng.step()
        t.cuda.synchronize()
        vr, st = eng.search.node_values(), eng.search.root_stats()
        assert (vr["counts"] == st["counts"]).all() and ((vr["vn"] >= 0) & (vr["vn"] <= st["n"])).all()   # (virtual loss in flight)
        c = eng.counters()
        assert c["overflow_sims"] == 0 and c["tree_resets"] == 0
    finally:
        if w.engine is not None:
            w.engine.close()
    off = SelfPlayEngine(_cfg(), 2, net=_net(2), dtype=t.float32, seed=13)
    try:
        assert not off.lcb_on and off.search.lcb == 0.0
    finally:
        off.close()


def test_the_arena_accepts_it(gpu):
    import torch as t
    from cchess_alphazero.agent.model import InferenceNet
    from cchess_alphazero.worker.evaluator import EvaluateWorker
    dev = t.device("cuda", t.cuda.current_device())
    cfg = _cfg(lcb=2.0, lcb_min_visits=0.25)
    cfg.eval.game_num = 2
    a, b = (InferenceNet(_net(k), t.float32, trunk="mfma").to(dev) for k in (7, 8))
    w = EvaluateWorker(cfg, evaluators=(a, b), dtype=gpu.N.U8)
    assert w.lcb_on and (w.lcb, w.lcb_min_visits) == (2.0, 0.25)
    stats = {}
    res = w.play_games(2, u_fn=lambda i, ply: 0.5, stats=stats)
    assert len(res) == 2 and stats["expansions"] > 0 and stats["overflow_sims"] == 0
    with pytest.raises(ValueError, match="lcb excludes smart_pruning"):
        EvaluateWorker(_cfg(lcb=2.0, smart_pruning=True), evaluators=(a, b), dtype=gpu.N.U8)


def _player_cfg(tmp_path, monkeypatch):
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    from cchess_alphazero.config import Config
    cfg = Config("mini")
    for k, v in dict(simulation_num_per_move=sm.SIMS, search_threads=1, noise_eps=0, tau_decay_rate=0, c_puct=1.5).items():
        setattr(cfg.play, k, v)                             # (sm.play_cfg's search: the rest of `mini` is its defaults)
    cfg.model.cnn_filter_num, cfg.model.res_layer_num = 128, 2
    cfg.resource.model_best_config_path = "/nonexistent/config.json"      # `uci` builds a random network: replaced by the stub
    return cfg


def _go(u, out, cmd):
    n = out.getvalue().count("bestmove")
    u.handle(cmd)
    t0 = time.time()
    while out.getvalue().count("bestmove") <= n:
        assert time.time() - t0 < 120, out.getvalue()
        time.sleep(0.02)


def test_player_and_uci_play_the_lcb_move(gpu, tmp_path, monkeypatch):
    """One of the cases on which the rule changes the move: CChessPlayer.action and a UCI `go depth 2` (depth N is N * 100
    simulations: the oracle's 200) with `setoption name LCB value 2` answer the oracle's move, and the last info line's pv
    starts with it.  A malformed value yields an info string and leaves the option as it was."""
    from cchess_alphazero.agent.player import CChessPlayer
    from cchess_alphazero.environment import static_env as senv
    from cchess_alphazero.uci import UCI
    case = [c for c in sm.cases() if c["name"] == DIFFER_Z2[0]][0]
    rows, _ = lo.run_case(case, z=2.0)
    want, most = rows[0]["best"], rows[0]["most"]
    assert want != most
    pipe = lambda: stub_net.StubPipe(lambda p: stub_net.hash_stub_numpy(p, case["salt"]))
    cfg = _player_cfg(tmp_path, monkeypatch)
    plain = CChessPlayer(cfg, search_tree={}, pipes=pipe(), enable_resign=False)
    try:
        assert not plain.lcb_on and plain.action(case["state"], 0)[0] == most           # without the option: the most visited
    finally:
        plain.close()
    cfg.engine.lcb = 2.0
    pl = CChessPlayer(cfg, search_tree={}, pipes=pipe(), enable_resign=False, debugging=True, uci=True, side=0)
    try:
        pl.out = io.StringIO()
        assert pl.lcb_on and (pl._search.lcb, pl._search.lcb_min_ratio) == (2.0, 0.15)
        action, _ = pl.action(case["state"], 0, depth=sm.SIMS)
        assert action == want and pl.done_tasks == sm.SIMS, (action, want, most)
        assert pl.principal_variation(case["state"])[0] == want
        last = [l for l in pl.out.getvalue().splitlines() if l.startswith("info depth") and " pv " in l][-1].split()
        assert last[last.index("pv") + 1] == senv.to_uci_move(want)
    finally:
        pl.close()
    out = io.StringIO()
    u = UCI(_player_cfg(tmp_path, monkeypatch), out=out)
    u.handle("uci")
    assert "option name LCB type string default 0" in out.getvalue()
    assert "option name LCBMinVisits type string default 0.15" in out.getvalue()
    u.pipe = pipe()
    for line in ("setoption name LCB value 2", "setoption name LCB value minus", "setoption name LCBMinVisits value 7", "isready",
                 "position fen " + senv.state_to_fen(case["state"], 0).rsplit(" ", 1)[0] + " 1"):
        u.handle(line)
    assert "info string LCB minus: expected a finite value >= 0" in out.getvalue()
    assert "info string LCBMinVisits 7: expected a value in [0, 1]" in out.getvalue()
    assert (u.config.engine.lcb, u.config.engine.lcb_min_visits) == (2.0, 0.15)
    assert u.state == case["state"] and u.turns == 0
    _go(u, out, "go depth 2")
    text = out.getvalue().splitlines()
    best = [l for l in text if l.startswith("bestmove")][-1].split()[1]
    assert best == senv.to_uci_move(want), (best, want, most)
    info = [l for l in text if l.startswith("info depth") and " pv " in l][-1].split()
    assert info[info.index("pv") + 1] == best
    assert u.handle("quit") is False
