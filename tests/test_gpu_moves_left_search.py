"""-m gpu: the moves-left utility of the search (cz_search_set_moves_left, cz_search_node_moves_left, cz_moves_left_quanta;
run.py self / eval --moves-left-slope).

The yardstick is tests/moves_left_search_oracle.py, search_model.Search with the rule of include/czero.h in it;
tests/test_moves_left_search_cpu.py pins it to the plain search with the utility off.  K = 1 searches are compared with it
exactly: the M records are integers, the utility is float64 arithmetic in a fixed order, and the stub's x rounds back to its
quanta with four orders of magnitude to spare (stub_moves_left.py), so no ulp of the device's exp or log1p reaches the tree.
K = 8 is held by invariants.  Every search here has at most 8 games and at most 400 simulations."""
import ctypes as C

import numpy as np
import pytest

import composed_oracle as co
import moves_left_search_oracle as mo
import search_model as sm
import stub_moves_left as sml
from oracle import xq_oracle as xo
from test_gpu_search import (assert_root_equal, boards_tensor, gpu, no_act_tensors, play_config)  # noqa: F401
from test_moves_left_search_cpu import TEST_CAP, TEST_SLOPE

pytestmark = pytest.mark.gpu
ERR_ARG = -1                                                # include/czero.h CZ_ERR_ARG
COUNTERS = ("sims", "expansions", "terminal_sims", "repetition_sims")
K_MAX = 16 * 1023


def _pc(sims, K=1, **kw):
    return play_config(simulation_num_per_move=sims, search_threads=K, noise_eps=0.0, tau_decay_rate=0.0, **kw)


def _err(L):
    return L.cz_last_error().decode()


# what a search does, as opposed to what its memory costs (chunks_taken, stat_blocks: the larger statistics blocks)
SEARCH_COUNTERS = COUNTERS + ("parked", "sum_depth", "max_depth", "edges_visited", "leaf_moves", "overflow_sims", "tree_resets",
                              "depth_overflow")


def _search_ctr(ctr):
    return {k: ctr[k] for k in SEARCH_COUNTERS}


def _eval(salt, variant="hash"):
    return lambda planes: sml.ml_stub_torch(planes, salt, variant)


def _assert_ml_equal(got, want, what):
    """got: node_moves_left() of a G = 1 search; want: the oracle's node_moves_left(state), None = not in the tree."""
    if want is None:
        assert int(got["counts"][0]) == 0 and not got["ksum"].any() and not got["mn"].any(), what
        return
    nm = len(want["ksum"])
    assert int(got["counts"][0]) == nm, what
    assert int(got["k_net"][0]) == want["k_net"], (what, int(got["k_net"][0]), want["k_net"])
    assert (got["ksum"][0, :nm] == want["ksum"]).all(), (what, got["ksum"][0, :nm], want["ksum"])
    assert (got["mn"][0, :nm] == want["mn"]).all(), (what, got["mn"][0, :nm], want["mn"])
    assert not got["ksum"][0, nm:].any() and not got["mn"][0, nm:].any(), what


def _walk(gpu, case, sims, use_history=False, variant="hash", k=0.0, slope=TEST_SLOPE, cap=TEST_CAP):
    """One case on the device and in the oracle, search by search: root statistics, M records at the root and one level down,
    counters, the pruned counts, the played move.  k: forced playouts on both sides.  Returns how many searches ran."""
    o = mo.Search(sm.play_cfg(sims), case["salt"], k, slope=slope, cap=cap,
                  net=lambda planes: sml.ml_stub_numpy(planes, case["salt"], variant))
    s = gpu.S.Search(_pc(sims), 1, seed=7, use_history=use_history)
    s.set_moves_left(slope, cap)
    s.set_forced_playouts(k)
    ev = _eval(case["salt"], variant)
    line = [(case["state"], [sm.ban_of(case, sims)] if case["kind"] == "ban" else [])]
    done = 0
    try:
        while line:
            state, no_act = line.pop(0)
            ran = o.search(state, no_act)
            na, nn = no_act_tensors(gpu, [no_act])
            before = s.counters()
            s.set_roots(boards_tensor(gpu, [state]), no_act=na, n_no_act=nn)
            s.run_until_idle(ev)
            what = f"{case['name']} search {done}"
            ctr = s.counters()
            assert ctr["sims"] - before["sims"] == ran and ctr["overflow_sims"] == 0 and ctr["tree_resets"] == 0, what
            for key in COUNTERS:
                assert ctr[key] == getattr(o, key), (what, key, ctr[key], getattr(o, key))
            assert_root_equal(s.root_stats(), 0, o.node_stats(state), what)
            _assert_ml_equal(s.node_moves_left(), o.node_moves_left(state), what)
            root = o.tree[state]
            linked = 0
            for j, mv in enumerate(root.moves):             # one level down: a linked child's records, or nothing
                child = xo.step(state, mv)
                is_node = root.n[j] > 0 and not xo.done(child)[0]
                linked += is_node
                _assert_ml_equal(s.node_moves_left([root.labels[j]]), o.node_moves_left(child) if is_node else None,
                                 f"{what} child {j}")
            assert linked >= 1, what
            co.assert_targets(s.root_targets(), o.node_stats(state), no_act, o.cfg.c_puct, k, what)
            best = o.best_move(state, no_act)
            assert xo.label_str(int(s.choose(None)[0])) == best, what
            assert xo.label_str(int(s.pv()[0][0])) == co.pv_first(o.node_stats(state), no_act), what
            done += 1
            if case["kind"] == "reuse" and done == 1:
                line.append((xo.step(state, best), []))
    finally:
        s.close()
    return done


# ---- 1. K = 1 against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sm.cases(), ids=lambda c: c["name"])
def test_single_searches_match_the_oracle(gpu, case):
    assert _walk(gpu, case, sm.SIMS) == (2 if case["kind"] == "reuse" else 1)


def test_the_28_plane_instantiation_matches_the_oracle(gpu):
    """k_sim_ml<true>.  An external root without a game history takes a leaf's second plane block from the search path, and
    the stub hashes all 28 planes, while the oracle hashes the position alone: the two agree where the block is empty, at
    depth 0 and 1.  With the flat stub (equal priors, a value of -1e-3) every root edge is visited once before any is visited
    twice, so a search of 1 + nm simulations stays there."""
    case = sm.cases()[0]
    nm = len(xo.get_legal_moves(case["state"]))
    assert _walk(gpu, case, 1 + nm, use_history=True, variant=("flat", -1e-3)) == 1


def test_a_played_line_with_tree_reuse_matches_the_oracle(gpu):
    sims, plies, salt = 120, 4, 21
    o = mo.Search(sm.play_cfg(sims), salt, slope=TEST_SLOPE, cap=TEST_CAP)
    s = gpu.S.Search(_pc(sims), 1, seed=7)
    s.set_moves_left(TEST_SLOPE, TEST_CAP)
    t = gpu.torch
    state, reused = xo.INIT_STATE, 0
    try:
        for ply in range(plies):
            ran = o.search(state)
            before = s.counters()["sims"]
            s.set_roots(boards_tensor(gpu, [state]), turns=t.tensor([ply], dtype=t.int32, device="cuda"))
            s.run_until_idle(_eval(salt))
            assert s.counters()["sims"] - before == ran, ply
            reused += ran < sims
            assert_root_equal(s.root_stats(), 0, o.node_stats(state), f"ply {ply}")
            _assert_ml_equal(s.node_moves_left(), o.node_moves_left(state), f"ply {ply}")
            best = o.best_move(state)
            assert xo.label_str(int(s.choose(None)[0])) == best, ply
            state = xo.step(state, best)
    finally:
        s.close()
    assert reused >= plies - 1                              # every later ply starts from a subtree it searched before


# ---- 2. K = 8 by invariants ---------------------------------------------------------------------------------------------------------
def _search_k8(gpu, setup, sims=200, salt=5, after=None):
    states = [c["state"] for c in sm.cases()][:8]
    s = gpu.S.Search(_pc(sims, K=8), len(states), seed=7)
    try:
        setup(s)
        s.set_roots(boards_tensor(gpu, states))
        s.run_until_idle(_eval(salt))
        out = dict(stats=s.root_stats(), ml=s.node_moves_left(), ctr=s.counters())
        if after:
            after(s, out)
    finally:
        s.close()
    return out


def _same_stats(a, b):
    for key, view in (("moves", None), ("n", None), ("sum_n", None), ("counts", None), ("w", np.uint64), ("p", np.uint32)):
        x, y = (a[key], b[key]) if view is None else (a[key].view(view), b[key].view(view))
        assert np.array_equal(x, y), key


def test_k8_invariants(gpu):
    plain = _search_k8(gpu, lambda s: None)
    assert not plain["ml"]["counts"].any() and not plain["ml"]["ksum"].any() and not plain["ml"]["k_net"].any()   # off: all 0
    # the utility on with a cap of 0: u_m is +-0 on every edge, so the search is the plain one bit for bit, and keeps records
    flat = _search_k8(gpu, lambda s: s.set_moves_left(TEST_SLOPE, 0.0))
    _same_stats(plain["stats"], flat["stats"])
    assert _search_ctr(plain["ctr"]) == _search_ctr(flat["ctr"])
    on = _search_k8(gpu, lambda s: s.set_moves_left(TEST_SLOPE, TEST_CAP))
    changed = 0
    for run in (flat, on):
        st, ml = run["stats"], run["ml"]
        assert run["ctr"]["overflow_sims"] == 0 and run["ctr"]["tree_resets"] == 0
        assert np.array_equal(ml["counts"], st["counts"])
        # mn counts the completed backups over the edge: with every simulation backed up that is the edge's visit count, and
        # their sum the simulations that went through the root
        assert np.array_equal(ml["mn"], st["n"])
        assert (ml["mn"].sum(axis=1) == st["sum_n"] - 1).all()
        assert (ml["ksum"] >= 16 * ml["mn"].astype(np.int64)).all()          # whole quanta (integers), at least one ply per level
        assert (ml["ksum"] <= (K_MAX + 16 * 128) * ml["mn"].astype(np.int64)).all()
        assert ((ml["k_net"] >= 1) & (ml["k_net"] <= sml.KQ_MAX)).all()      # the stub's range
    changed = sum(not np.array_equal(on["stats"]["n"][g], plain["stats"]["n"][g]) for g in range(8))
    assert changed >= 4
    # on, then off, then searching: the search that never had it
    back = _search_k8(gpu, lambda s: (s.set_moves_left(TEST_SLOPE, TEST_CAP), s.set_moves_left(0.0)))
    _same_stats(plain["stats"], back["stats"])
    assert _search_ctr(plain["ctr"]) == _search_ctr(back["ctr"]) and not back["ml"]["counts"].any()


def test_switching_resets_the_trees(gpu):
    """Switching on over grown trees (their statistics blocks have no M records) and off again starts the trees over."""
    s = gpu.S.Search(_pc(64), 1, seed=7)
    try:
        s.set_roots(boards_tensor(gpu, [xo.INIT_STATE]))
        s.run_until_idle(_eval(4))
        assert int(s.root_stats()["sum_n"][0]) == 64 and s.memory_info()["nodes"] > 1
        keep0 = s.keep_chunks
        s.set_moves_left(TEST_SLOPE, TEST_CAP)
        assert s.memory_info()["nodes"] == 0
        s.set_moves_left(TEST_SLOPE / 2, TEST_CAP)          # new values, still on: nothing is reset
        s.set_roots(boards_tensor(gpu, [xo.INIT_STATE]))
        s.run_until_idle(_eval(4))
        nodes = s.memory_info()["nodes"]
        assert nodes > 1
        s.set_moves_left(TEST_SLOPE, TEST_CAP)
        assert s.memory_info()["nodes"] == nodes
        s.set_moves_left(0.0)
        assert s.memory_info()["nodes"] == 0 and not s.node_moves_left()["counts"].any()
        info = (C.c_int32 * 16)()
        s.L.cz_search_info(s.h, info)
        assert info[12] == keep0
    finally:
        s.close()


# ---- 3. the conversion ---------------------------------------------------------------------------------------------------------------
def test_quanta_of_the_grid(gpu):
    """k against 512 * softplus in float64.  The device computes t = 512 * (max(x, 0) + log1p(exp(-|x|))) in float32 and rounds
    to nearest: exp and log1p are each within 1 ulp (the ROCm device library's stated bounds), the error of e = exp(-|x|) reaches
    log1p(e) multiplied by e / (1 + e) <= log1p(e), the sum is rounded once (half an ulp) and the product with 512 is exact.
    With ulp = 2^-23 relative that is |t - 512 softplus(x)| <= (1 + 1 + 0.5) 2^-23 * 512 softplus(x); a device that flushes a
    subnormal exp(-|x|) to zero adds at most 512 * 2^-126.  Rounding adds 0.5, and min(., cap) moves nothing apart."""
    t = gpu.torch
    grid = np.array([-104.0, -20.0, -6.2, -1e-3, 0.0, 5.0, 17.0, 40.0, 100.0, np.inf, -np.inf, np.nan, 1e-40], dtype=np.float32)
    assert 0.0 < abs(float(grid[-1])) < np.finfo(np.float32).tiny                # a subnormal
    x = t.from_numpy(grid).cuda()
    k = t.full((len(grid),), -7, dtype=t.int32, device="cuda")
    L = gpu.N.lib()
    st = C.c_void_p(t.cuda.current_stream().cuda_stream)
    assert L.cz_moves_left_quanta(C.c_void_p(x.data_ptr()), C.c_void_p(k.data_ptr()), len(grid), st) == 0
    k = k.cpu().numpy()
    x64 = grid.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        exact = 512.0 * (np.maximum(x64, 0.0) + np.log1p(np.exp(-np.abs(x64))))
    for i, xi in enumerate(grid):
        if np.isnan(xi) or xi == -np.inf:
            assert k[i] == 0, (xi, k[i])
        elif xi == np.inf:
            assert k[i] == K_MAX, (xi, k[i])
        else:
            bound = 0.5 + 2.5 * 2.0 ** -23 * exact[i] + 512.0 * 2.0 ** -126
            print(f"x = {xi:g}: k = {k[i]}, 512 softplus = {exact[i]:.6f}, bound {bound:.6f}")
            assert abs(k[i] - min(exact[i], K_MAX)) <= bound, (xi, k[i], exact[i])
    assert 0 <= k.min() and k.max() == K_MAX and k[list(grid).index(0.0)] == 355        # 512 ln 2 = 354.89
    assert (sml.quanta_of_x(grid) == k).all()                                            # the oracle's restatement
    assert L.cz_moves_left_quanta(None, C.c_void_p(k.ctypes.data), 1, st) == ERR_ARG


# ---- 4. the setter ---------------------------------------------------------------------------------------------------------------
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
ML_PHRASE = "the moves-left utility is on (cz_search_set_moves_left)"


def test_setter_refusals_follow_the_table(gpu):
    from cchess_alphazero import search_options as so
    assert sorted(_ON) == sorted(k for k, _ in so.MOVES_LEFT_EXCLUDES)
    t = gpu.torch
    s = gpu.S.Search(_pc(16), 2, seed=1)
    L, h = s.L, s.h
    st = C.c_void_p(t.cuda.current_stream().cuda_stream)
    x = t.zeros((s.slots,), dtype=t.float32, device="cuda")
    xp = C.c_void_p(x.data_ptr())
    d = C.c_double
    on = lambda: L.cz_search_set_moves_left(h, d(TEST_SLOPE), d(TEST_CAP), xp, st)
    off = lambda: L.cz_search_set_moves_left(h, d(0.0), d(TEST_CAP), None, st)
    try:
        assert L.cz_search_set_moves_left(None, d(0.1), d(0.1), xp, st) == ERR_ARG
        for slope, cap in ((-1.0, 0.1), (float("nan"), 0.1), (float("inf"), 0.1), (0.1, -1.0), (0.1, float("inf"))):
            assert L.cz_search_set_moves_left(h, d(slope), d(cap), xp, st) == ERR_ARG
            assert "slope or cap negative or not finite" in _err(L)
        assert L.cz_search_set_moves_left(h, d(0.1), d(0.1), None, st) == ERR_ARG      # NULL rows with slope > 0
        assert _err(L) == "cz_search_set_moves_left: x_rows is NULL"
        assert off() == 0                                                              # off needs no rows
        for key, (entry, sw_on, sw_off, phrase) in _ON.items():
            assert sw_on(L, h, st) == 0, key
            assert on() == ERR_ARG, key
            assert _err(L) == f"cz_search_set_moves_left: {phrase}", key
            assert off() == 0                                                          # switching off is never refused
            assert sw_off(L, h, st) == 0, key
            assert on() == 0, key
            assert sw_on(L, h, st) == ERR_ARG, key
            assert _err(L) == f"{entry}: {ML_PHRASE}", key
            assert sw_off(L, h, st) == 0, key                                          # nor is theirs
            assert off() == 0
        # a script: refused beside the utility, and the utility beside it
        s.record_visits(True)
        script = (np.stack([xo.state_to_board(xo.INIT_STATE)]).astype(np.int8), np.array([0], dtype=np.uint16),
                  np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int8))
        assert on() == 0
        with pytest.raises(gpu.N.NativeError, match="cz_search_set_script: " + ML_PHRASE.replace("(", r"\(").replace(")", r"\)")):
            s.set_script(*script)
        assert off() == 0
        s.set_script(*script)
        assert on() == ERR_ARG and _err(L) == "cz_search_set_moves_left: a script is set (cz_search_set_script)"
        s.set_script()
        # what it composes with
        s.set_playout_cap(8, 0.5)
        s.set_forced_playouts(2.0)
        s.set_leaf_mirror(0.5)
        assert on() == 0
    finally:
        s.close()


def test_search_wrapper(gpu):
    s = gpu.S.Search(_pc(16), 2, seed=1)
    try:
        assert s.moves_left_x is None and s.moves_left_slope == 0.0
        got = s.node_moves_left()
        assert not got["counts"].any() and got["ksum"].shape == (2, 128) and got["mn"].shape == (2, 128) and got["k_net"].shape == (2,)
        s.set_moves_left(0.0027)
        assert s.moves_left_x.shape == (s.slots,) and s.moves_left_x.dtype == gpu.torch.float32
        assert (s.moves_left_slope, s.moves_left_cap) == (0.0027, 0.0345)
        ptr = s.moves_left_x.data_ptr()
        s.set_moves_left(0.0)
        s.set_moves_left(0.01, 0.1)
        assert s.moves_left_x.data_ptr() == ptr                                         # the owned buffer stays where it is
        with pytest.raises(gpu.N.NativeError, match="slope or cap"):
            s.set_moves_left(-1.0)
    finally:
        s.close()


# ---- 5. the engine ---------------------------------------------------------------------------------------------------------------
def _net(seed, moves_left=True):
    import torch
    from cchess_alphazero.agent.model import CChessNet
    torch.manual_seed(seed)
    return CChessNet(cnn_filter_num=128, res_layer_num=2, moves_left=moves_left).eval()


def _cfg(**engine):
    from cchess_alphazero.config import Config
    cfg = Config("mini")
    cfg.model.cnn_filter_num, cfg.model.res_layer_num = 128, 2
    cfg.play.simulation_num_per_move, cfg.play.search_threads, cfg.play.noise_eps = 16, 8, 0.0
    cfg.play.max_game_length = 8
    for k, v in engine.items():
        setattr(cfg.engine, k, v)
    return cfg


def test_selfplay_engine_runs_with_the_utility_and_refuses_a_net_without_the_output(gpu):
    import torch as t
    from cchess_alphazero.engine import SelfPlayEngine
    G = 4
    with pytest.raises(ValueError, match="opt --moves-left"):
        SelfPlayEngine(_cfg(moves_left_slope=0.0027), G, net=_net(1, moves_left=False), dtype=t.float32, seed=13)
    with pytest.raises(ValueError, match="moves_left_slope excludes solver"):
        SelfPlayEngine(_cfg(moves_left_slope=0.0027, solver=True), G, net=_net(1), dtype=t.float32, seed=13)
    eng = SelfPlayEngine(_cfg(moves_left_slope=0.0027), G, net=_net(2), dtype=t.float32, seed=13)
    games = []
    try:
        assert eng.moves_left and eng.search.moves_left_slope == 0.0027 and eng.search.moves_left_cap == 0.0345
        assert eng.net.calibration is None or "moves_left_max_abs" in eng.net.calibration["chosen"]
        eng.start()
        eng.search.moves_left_x.fill_(float("nan"))
        for _ in range(48):
            eng.step()
        games += eng.drain()
        n = int(eng.search.q_count.item()) if eng.compact else eng.search.slots
        assert n > 0 and t.isfinite(eng.search.moves_left_x[:n]).all()                 # the forward writes the rows the search reads
        ml = eng.search.node_moves_left()
        st = eng.search.root_stats()
        assert (ml["counts"] == st["counts"]).all() and (ml["k_net"] > 0).any()
        # a hot reload to a model without the output is refused, and the games stay on the old network
        old = eng.net
        with pytest.raises(ValueError, match="opt --moves-left"):
            eng.set_network(_net(3, moves_left=False))
        assert eng.net is old
        eng.set_network(_net(4))
        for _ in range(16):
            eng.step()
        games += eng.drain()
        c = eng.counters()
        assert c["overflow_sims"] == 0 and c["tree_resets"] == 0 and c["ring_dropped"] == 0
        # the guard and the live audit measure x only while the utility is on
        m = eng.audit_network(16)
        assert m is not None and "moves_left_max_abs" in m and m["moves_left_max_abs"] <= 2e-4 and m["ok"]
    finally:
        eng.close()
    assert len(games) >= G
    for g in games:
        state = g["data"][0]
        for item in g["data"][1:]:
            assert item[0] in xo.get_legal_moves(state), g["game_id"]
            state = xo.step(state, item[0])
    off = SelfPlayEngine(_cfg(), G, net=_net(2), dtype=t.float32, seed=13)
    try:
        assert not off.moves_left and off.search.moves_left_x is None
        off.start()
        for _ in range(8):
            off.step()
        m = off.audit_network(16)
        assert m is not None and "moves_left_max_abs" not in m
        assert off.net.calibration is None or "moves_left_max_abs" not in off.net.calibration["chosen"]
    finally:
        off.close()


def test_guard_reports_x_only_when_asked(gpu):
    import torch as t
    from cchess_alphazero.agent.model import (calibration_planes, guarded_inference_net, measure_against_reference,
                                              reference_forward_f64, within_guard)
    dev = t.device("cuda", t.cuda.current_device())
    raw = _net(5)
    inf = guarded_inference_net(raw, t.float32, trunk="mfma", device=dev, moves_left=True)
    assert inf.calibration is not None and all("moves_left_max_abs" in m for m in inf.calibration["candidates"])
    planes = calibration_planes(32, 14, dev, seed=9)
    ref = reference_forward_f64(raw, planes, with_moves_left=True)
    m = measure_against_reference(inf, ref, planes, moves_left_ref=ref[-1])
    print(f"\nguard with the moves-left output ({inf.arith_effective}): {m}")
    assert within_guard(m) and m["moves_left_max_abs"] <= 2e-4
    assert not within_guard(dict(m, moves_left_max_abs=3e-4))
    plain = measure_against_reference(inf, ref, planes)
    assert "moves_left_max_abs" not in plain and {k: v for k, v in m.items() if k != "moves_left_max_abs"} == plain
    with pytest.raises(RuntimeError, match="no moves-left output"):
        guarded_inference_net(_net(6, moves_left=False), t.float32, trunk="mfma", device=dev, moves_left=True)


def test_arena_needs_the_output_in_both_networks(gpu):
    import torch as t
    from cchess_alphazero.agent.model import InferenceNet
    from cchess_alphazero.worker.evaluator import EvaluateWorker
    dev = t.device("cuda", t.cuda.current_device())
    cfg = _cfg(moves_left_slope=0.0027)
    cfg.eval.game_num = 2
    with_x = InferenceNet(_net(7), t.float32, trunk="mfma").to(dev)
    without = InferenceNet(_net(8, moves_left=False), t.float32, trunk="mfma").to(dev)
    with pytest.raises(ValueError, match="opt --moves-left"):
        EvaluateWorker(cfg, evaluators=(with_x, without), dtype=gpu.N.U8)
    w = EvaluateWorker(cfg, evaluators=(with_x, with_x), dtype=gpu.N.U8)
    stats = {}
    res = w.play_games(2, u_fn=lambda i, ply: 0.5, stats=stats)
    assert len(res) == 2 and stats["expansions"] > 0 and stats["overflow_sims"] == 0
