"""-m gpu: the draw average of the search (cz_search_set_draw, cz_search_node_draws, cz_draw_quanta; run.py self / eval
--draw-score, the UCI options UCI_ShowWDL and DrawScore).

The yardstick is tests/draw_search_oracle.py, search_model.Search with the rule of include/czero.h in it;
tests/test_draw_search_cpu.py pins it to the plain search with the option off and with a score of 0.  K = 1 searches are
compared with it exactly: the D records are integers, the stub's d is an exact multiple of 2^-20 (stub_draw.py), and the
score's third term is float64 arithmetic in a fixed order.  K = 8 is held by invariants.  Every search here has at most 8
games and at most 400 simulations."""
import ctypes as C
import io
import time

import numpy as np
import pytest

import composed_oracle as co
import draw_search_oracle as do
import search_limits as sl
import search_model as sm
import stub_draw as sd
from oracle import xq_oracle as xo
from test_draw_search_cpu import MID_SCORE, MID_SIMS, TEST_SCORE
from test_gpu_search import (assert_root_equal, boards_tensor, gpu, no_act_tensors, play_config)  # noqa: F401

pytestmark = pytest.mark.gpu
ERR_ARG = -1                                                # include/czero.h CZ_ERR_ARG
COUNTERS = ("sims", "expansions", "terminal_sims", "repetition_sims")
Q = sd.QUANTA
# what a search does, as opposed to what its memory costs (chunks_taken, stat_blocks: the larger statistics blocks)
SEARCH_COUNTERS = COUNTERS + ("parked", "sum_depth", "max_depth", "edges_visited", "leaf_moves", "overflow_sims", "tree_resets",
                              "depth_overflow")


def _pc(sims, K=1, **kw):
    return play_config(simulation_num_per_move=sims, search_threads=K, noise_eps=0.0, tau_decay_rate=0.0, **kw)


def _err(L):
    return L.cz_last_error().decode()


def _search_ctr(ctr):
    return {k: ctr[k] for k in SEARCH_COUNTERS}


def _eval(salt, variant="hash"):
    return lambda planes: sd.draw_stub_torch(planes, salt, variant)


def _assert_draws_equal(got, want, what):
    """got: node_draws() of a G = 1 search; want: the oracle's node_draws(state), None = not in the tree."""
    if want is None:
        assert int(got["counts"][0]) == 0 and not got["dsum"].any() and not got["dn"].any(), what
        return
    nm = len(want["dsum"])
    assert int(got["counts"][0]) == nm, what
    assert int(got["dq_net"][0]) == want["dq_net"], (what, int(got["dq_net"][0]), want["dq_net"])
    assert (got["dsum"][0, :nm] == want["dsum"]).all(), (what, got["dsum"][0, :nm], want["dsum"])
    assert (got["dn"][0, :nm] == want["dn"]).all(), (what, got["dn"][0, :nm], want["dn"])
    assert not got["dsum"][0, nm:].any() and not got["dn"][0, nm:].any(), what


def _walk(gpu, case, sims, use_history=False, variant="hash", score=TEST_SCORE, k=0.0):
    """One case on the device and in the oracle, search by search: root statistics, D records at the root and one level down,
    counters, the pruned counts, the played move.  k: forced playouts on both sides.  Returns (how many searches ran, the
    oracle)."""
    o = do.Search(sm.play_cfg(sims), case["salt"], k, score=score,
                  net=lambda planes: sd.draw_stub_numpy(planes, case["salt"], variant))
    s = gpu.S.Search(_pc(sims), 1, seed=7, use_history=use_history)
    s.set_draw(True, score)
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
            _assert_draws_equal(s.node_draws(), o.node_draws(state), what)
            root = o.tree[state]
            linked = 0
            for j, mv in enumerate(root.moves):             # one level down: a linked child's records, or nothing
                child = xo.step(state, mv)
                is_node = root.n[j] > 0 and not xo.done(child)[0]
                linked += is_node
                _assert_draws_equal(s.node_draws([root.labels[j]]), o.node_draws(child) if is_node else None,
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
    return done, o


# ---- 1. K = 1 against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sm.cases(), ids=lambda c: c["name"])
def test_single_searches_match_the_oracle(gpu, case):
    assert _walk(gpu, case, sm.SIMS)[0] == (2 if case["kind"] == "reuse" else 1)


def test_the_28_plane_instantiation_matches_the_oracle(gpu):
    """k_sim_draw<true>.  An external root without a game history takes a leaf's second plane block from the search path, and
    the stub hashes all 28 planes, while the oracle hashes the position alone: the two agree where the block is empty, at
    depth 0 and 1.  With the flat stub (equal priors, a value of 0) and a score of -0.02 every root edge is visited once before
    any is visited twice (test_draw_search_cpu.test_the_sign_follows_the_depth says why), so a search of 1 + nm simulations
    stays there."""
    case = sm.cases()[0]
    nm = len(xo.get_legal_moves(case["state"]))
    assert _walk(gpu, case, 1 + nm, use_history=True, variant=("flat", 0.0), score=-0.02)[0] == 1


def test_a_played_line_with_tree_reuse_matches_the_oracle(gpu):
    sims, plies, salt = 120, 4, 21
    o = do.Search(sm.play_cfg(sims), salt, score=TEST_SCORE)
    s = gpu.S.Search(_pc(sims), 1, seed=7)
    s.set_draw(True, TEST_SCORE)
    t = gpu.torch
    state, reused = xo.INIT_STATE, 0
    try:
        for ply in range(plies):                            # (the parity of sigma is the current root's at every ply)
            ran = o.search(state)
            before = s.counters()["sims"]
            s.set_roots(boards_tensor(gpu, [state]), turns=t.tensor([ply], dtype=t.int32, device="cuda"))
            s.run_until_idle(_eval(salt))
            assert s.counters()["sims"] - before == ran, ply
            reused += ran < sims
            assert_root_equal(s.root_stats(), 0, o.node_stats(state), f"ply {ply}")
            _assert_draws_equal(s.node_draws(), o.node_draws(state), f"ply {ply}")
            best = o.best_move(state)
            assert xo.label_str(int(s.choose(None)[0])) == best, ply
            state = xo.step(state, best)
    finally:
        s.close()
    assert reused >= plies - 1                              # every later ply starts from a subtree it searched before


@pytest.mark.parametrize("score", [MID_SCORE, TEST_SCORE])
def test_the_deferred_ends_match_the_oracle(gpu, score):
    """flush_deferred<..., DRAW> through all of its values: the MID position under the peaked policy.  At MID_SCORE the oracle
    sees repetitions worth 0 (dq = 2^20), repetitions worth +-1 and terminal ends (dq = 0); at TEST_SCORE the draws by
    repetition are avoided (tests/test_draw_search_cpu.py says why) and the other two remain."""
    case = dict(name="mid", salt=sl.PEAKED["salt"], state=sl.MID, kind=None)
    done, o = _walk(gpu, case, MID_SIMS, variant="peaked", score=score)
    assert done == 1
    if score == MID_SCORE:
        assert o.rep0_sims >= 10 and o.rep1_sims >= 1 and o.terminal_sims >= 1
    else:
        assert o.rep1_sims >= 1 and o.terminal_sims >= 1


# ---- 2. K = 8 by invariants ---------------------------------------------------------------------------------------------------------
def _search_k8(gpu, setup, sims=200, salt=5):
    states = [c["state"] for c in sm.cases()][:8]
    s = gpu.S.Search(_pc(sims, K=8), len(states), seed=7)
    try:
        setup(s)
        s.set_roots(boards_tensor(gpu, states))
        s.run_until_idle(_eval(salt))
        out = dict(stats=s.root_stats(), dr=s.node_draws(), ctr=s.counters())
    finally:
        s.close()
    return out


def _same_stats(a, b):
    for key, view in (("moves", None), ("n", None), ("sum_n", None), ("counts", None), ("w", np.uint64), ("p", np.uint32)):
        x, y = (a[key], b[key]) if view is None else (a[key].view(view), b[key].view(view))
        assert np.array_equal(x, y), key


def test_k8_invariants(gpu):
    plain = _search_k8(gpu, lambda s: None)
    assert not plain["dr"]["counts"].any() and not plain["dr"]["dsum"].any() and not plain["dr"]["dn"].any()    # off: all 0
    assert not plain["dr"]["dq_net"].any()
    # on with a score of 0: every comparison is the plain search's, bit for bit, and the records are kept
    zero = _search_k8(gpu, lambda s: s.set_draw(True, 0.0))
    _same_stats(plain["stats"], zero["stats"])
    assert _search_ctr(plain["ctr"]) == _search_ctr(zero["ctr"])
    on = _search_k8(gpu, lambda s: s.set_draw(True, TEST_SCORE))
    for run in (zero, on):
        st, dr = run["stats"], run["dr"]
        assert run["ctr"]["overflow_sims"] == 0 and run["ctr"]["tree_resets"] == 0
        assert np.array_equal(dr["counts"], st["counts"])
        # dn counts the completed backups over the edge: with every simulation backed up that is the edge's visit count, and
        # their sum the simulations that went through the root
        assert np.array_equal(dr["dn"], st["n"])
        assert (dr["dn"].sum(axis=1) == st["sum_n"] - 1).all()
        assert (dr["dsum"] >= 0).all() and (dr["dsum"] <= Q * dr["dn"].astype(np.int64)).all()
        assert ((dr["dq_net"] >= 0) & (dr["dq_net"] <= Q)).all() and dr["dsum"].any()
    changed = sum(not np.array_equal(on["stats"]["n"][g], plain["stats"]["n"][g]) for g in range(8))
    assert changed >= 4
    # on, then off, then searching: the search that never had it
    back = _search_k8(gpu, lambda s: (s.set_draw(True, TEST_SCORE), s.set_draw(False)))
    _same_stats(plain["stats"], back["stats"])
    assert _search_ctr(plain["ctr"]) == _search_ctr(back["ctr"]) and not back["dr"]["counts"].any()


# ---- 3. switching ---------------------------------------------------------------------------------------------------------------------
def test_switching_resets_the_trees(gpu):
    """Switching on over grown trees (their statistics blocks have no D records) and off again starts the trees over; a new
    score while on does not."""
    s = gpu.S.Search(_pc(64), 1, seed=7)
    try:
        s.set_roots(boards_tensor(gpu, [xo.INIT_STATE]))
        s.run_until_idle(_eval(4))
        assert int(s.root_stats()["sum_n"][0]) == 64 and s.memory_info()["nodes"] > 1
        keep0 = s.keep_chunks
        s.set_draw(True, TEST_SCORE)
        assert s.memory_info()["nodes"] == 0
        s.set_roots(boards_tensor(gpu, [xo.INIT_STATE]))
        s.run_until_idle(_eval(4))
        nodes = s.memory_info()["nodes"]
        assert nodes > 1
        s.set_draw(True, 0.25)                              # a new score, still on: nothing is reset
        assert s.memory_info()["nodes"] == nodes and (s.draw_on, s.draw_score) == (True, 0.25)
        s.set_draw(False)
        assert s.memory_info()["nodes"] == 0 and not s.node_draws()["counts"].any() and not s.draw_on
        info = (C.c_int32 * 16)()
        s.L.cz_search_info(s.h, info)
        assert info[12] == keep0
    finally:
        s.close()


# ---- 4. the conversion ---------------------------------------------------------------------------------------------------------------
def test_quanta_of_the_grid(gpu):
    """Equality with the NumPy restatement is exact: the product with 2^20 is exact in float32 and rint has no ulp."""
    t = gpu.torch
    L = gpu.N.lib()
    st = C.c_void_p(t.cuda.current_stream().cuda_stream)
    grid = sd.GRID
    assert 0.0 < abs(float(grid[-1])) < np.finfo(np.float32).tiny                # a subnormal
    n = len(grid)
    for stride in (3, 1):
        host = np.full((n, stride), np.float32(0.75), dtype=np.float32)          # (the other columns must not be read)
        host[:, 0] = grid
        d = t.from_numpy(host).cuda()
        dq = t.full((n + 1,), -7, dtype=t.int32, device="cuda")
        assert L.cz_draw_quanta(C.c_void_p(d.data_ptr()), stride, C.c_void_p(dq.data_ptr()), n, st) == 0
        got = dq.cpu().numpy()
        assert got[n] == -7                                                      # nothing past n
        assert got[:n].tolist() == sd.draw_quanta(grid).tolist() == sd.GRID_DQ, (stride, got)
    # the draw column of rows [n, 3], as the attach reads it: offset 1, stride 3
    rows = np.zeros((n, 3), dtype=np.float32)
    rows[:, 1] = grid
    d = t.from_numpy(rows).cuda()
    dq = t.zeros((n,), dtype=t.int32, device="cuda")
    assert L.cz_draw_quanta(C.c_void_p(d.data_ptr() + 4), 3, C.c_void_p(dq.data_ptr()), n, st) == 0
    assert dq.cpu().numpy().tolist() == sd.GRID_DQ
    assert L.cz_draw_quanta(None, 1, C.c_void_p(dq.data_ptr()), 1, st) == ERR_ARG
    assert L.cz_draw_quanta(C.c_void_p(d.data_ptr()), 0, C.c_void_p(dq.data_ptr()), 1, st) == ERR_ARG


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
DRAW_PHRASE = "the draw average is on (cz_search_set_draw)"
ML_PHRASE = "the moves-left utility is on (cz_search_set_moves_left)"


def test_setter_refusals_follow_the_table(gpu):
    from cchess_alphazero import search_options as so
    assert sorted(_ON) == sorted(k for k, _ in so.DRAW_EXCLUDES)
    t = gpu.torch
    s = gpu.S.Search(_pc(16), 2, seed=1)
    L, h = s.L, s.h
    st = C.c_void_p(t.cuda.current_stream().cuda_stream)
    rows = t.zeros((s.slots, 3), dtype=t.float32, device="cuda")
    rp = C.c_void_p(rows.data_ptr())
    x = t.zeros((s.slots,), dtype=t.float32, device="cuda")
    xp = C.c_void_p(x.data_ptr())
    d = C.c_double
    on = lambda: L.cz_search_set_draw(h, 1, d(TEST_SCORE), rp, st)
    off = lambda: L.cz_search_set_draw(h, 0, d(0.0), None, st)
    try:
        assert L.cz_search_set_draw(None, 1, d(0.1), rp, st) == ERR_ARG
        for score in (1.5, -1.0001, float("nan"), float("inf"), float("-inf")):
            assert L.cz_search_set_draw(h, 1, d(score), rp, st) == ERR_ARG
            assert "score outside [-1, 1] or not finite" in _err(L)
        assert L.cz_search_set_draw(h, 1, d(0.1), None, st) == ERR_ARG                 # NULL rows with on
        assert _err(L) == "cz_search_set_draw: wdl_rows is NULL"
        assert off() == 0                                                              # off needs no rows
        assert L.cz_search_set_draw(h, 1, d(1.0), rp, st) == 0 and L.cz_search_set_draw(h, 1, d(-1.0), rp, st) == 0
        assert off() == 0
        for key, (entry, sw_on, sw_off, phrase) in _ON.items():
            assert sw_on(L, h, st) == 0, key
            assert on() == ERR_ARG, key
            assert _err(L) == f"cz_search_set_draw: {phrase}", key
            assert off() == 0                                                          # switching off is never refused
            assert sw_off(L, h, st) == 0, key
            assert on() == 0, key
            assert sw_on(L, h, st) == ERR_ARG, key
            assert _err(L) == f"{entry}: {DRAW_PHRASE}", key
            assert sw_off(L, h, st) == 0, key                                          # nor is theirs
            assert off() == 0
        # the moves-left utility: the same granules
        ml_on = lambda: L.cz_search_set_moves_left(h, d(0.01), d(0.1), xp, st)
        ml_off = lambda: L.cz_search_set_moves_left(h, d(0.0), d(0.1), None, st)
        assert ml_on() == 0
        assert on() == ERR_ARG and _err(L) == f"cz_search_set_draw: {ML_PHRASE}"
        assert off() == 0 and ml_off() == 0 and on() == 0
        assert ml_on() == ERR_ARG and _err(L) == f"cz_search_set_moves_left: {DRAW_PHRASE}"
        assert ml_off() == 0 and off() == 0
        # a script: refused beside the average, and the average beside it
        s.record_visits(True)
        script = (np.stack([xo.state_to_board(xo.INIT_STATE)]).astype(np.int8), np.array([0], dtype=np.uint16),
                  np.array([0, 1], dtype=np.int32), np.array([0], dtype=np.int8))
        assert on() == 0
        with pytest.raises(gpu.N.NativeError, match="cz_search_set_script: " + DRAW_PHRASE.replace("(", r"\(").replace(")", r"\)")):
            s.set_script(*script)
        assert off() == 0
        s.set_script(*script)
        assert on() == ERR_ARG and _err(L) == "cz_search_set_draw: a script is set (cz_search_set_script)"
        s.set_script()
        # what it composes with
        s.set_playout_cap(8, 0.5)
        s.set_forced_playouts(2.0)
        s.set_leaf_mirror(0.5)
        assert on() == 0
    finally:
        s.close()


# ---- 6. the wrapper -------------------------------------------------------------------------------------------------------------
def test_search_wrapper(gpu):
    s = gpu.S.Search(_pc(16), 2, seed=1)
    try:
        assert s.wdl_rows is None and s.draw_on is False and s.draw_score == 0.0
        got = s.node_draws()
        assert not got["counts"].any() and got["dsum"].shape == (2, 128) and got["dn"].shape == (2, 128)
        assert got["dq_net"].shape == (2,) and got["dsum"].dtype == np.int64 and got["dn"].dtype == np.int32
        s.set_draw(True, -0.25)
        assert s.wdl_rows.shape == (s.slots, 3) and s.wdl_rows.dtype == gpu.torch.float32
        assert (s.draw_on, s.draw_score) == (True, -0.25)
        ptr = s.wdl_rows.data_ptr()
        s.set_draw(False)
        assert (s.draw_on, s.draw_score) == (False, 0.0)
        s.set_draw(True)
        assert s.wdl_rows.data_ptr() == ptr and (s.draw_on, s.draw_score) == (True, 0.0)   # the owned buffer stays where it is
        with pytest.raises(gpu.N.NativeError, match="score outside"):
            s.set_draw(True, 2.0)
        assert (s.draw_on, s.draw_score) == (True, 0.0)
    finally:
        s.close()


# ---- 7. the engine ---------------------------------------------------------------------------------------------------------------
def _net(seed, value_outputs=3, moves_left=False):
    import torch
    from cchess_alphazero.agent.model import CChessNet
    torch.manual_seed(seed)
    return CChessNet(cnn_filter_num=128, res_layer_num=2, value_outputs=value_outputs, moves_left=moves_left).eval()


def _cfg(**engine):
    from cchess_alphazero.config import Config
    cfg = Config("mini")
    cfg.model.cnn_filter_num, cfg.model.res_layer_num = 128, 2
    cfg.play.simulation_num_per_move, cfg.play.search_threads, cfg.play.noise_eps = 16, 8, 0.0
    cfg.play.max_game_length = 8
    for k, v in engine.items():
        setattr(cfg.engine, k, v)
    return cfg


@pytest.mark.parametrize("moves_left", [False, True], ids=["wdl", "wdl+moves_left"])
def test_selfplay_engine_runs_with_the_average_and_refuses_a_scalar_net(gpu, moves_left):
    import torch as t
    from cchess_alphazero.engine import SelfPlayEngine
    G = 4
    with pytest.raises(ValueError, match="opt --value-head wdl"):
        SelfPlayEngine(_cfg(draw_score=TEST_SCORE), G, net=_net(1, value_outputs=1), dtype=t.float32, seed=13)
    with pytest.raises(ValueError, match="draw_score excludes solver"):
        SelfPlayEngine(_cfg(draw_score=TEST_SCORE, solver=True), G, net=_net(1), dtype=t.float32, seed=13)
    eng = SelfPlayEngine(_cfg(draw_score=TEST_SCORE), G, net=_net(2, moves_left=moves_left), dtype=t.float32, seed=13)
    games = []
    try:
        assert eng.draw and eng.search.draw_on and eng.search.draw_score == TEST_SCORE and not eng.moves_left
        assert eng.net.calibration is None or "draw_max_abs" in eng.net.calibration["chosen"]
        eng.start()
        eng.search.wdl_rows.fill_(float("nan"))
        for _ in range(48):
            eng.step()
        games += eng.drain()
        n = int(eng.search.q_count.item()) if eng.compact else eng.search.slots
        assert n > 0 and t.isfinite(eng.search.wdl_rows[:n]).all()                     # the forward writes the rows the search reads
        dr = eng.search.node_draws()
        st = eng.search.root_stats()
        assert (dr["counts"] == st["counts"]).all() and (dr["dq_net"] > 0).any()
        assert ((dr["dn"] >= 0) & (dr["dn"] <= st["n"])).all()                        # (simulations in flight hold virtual loss)
        # a hot reload to a scalar model is refused, and the games stay on the old network
        old = eng.net
        with pytest.raises(ValueError, match="opt --value-head wdl"):
            eng.set_network(_net(3, value_outputs=1))
        assert eng.net is old
        eng.set_network(_net(4, moves_left=moves_left))
        for _ in range(16):
            eng.step()
        games += eng.drain()
        c = eng.counters()
        assert c["overflow_sims"] == 0 and c["tree_resets"] == 0 and c["ring_dropped"] == 0
        # the guard and the live audit measure d only while the average is on
        m = eng.audit_network(16)
        print(f"\naudit with the draw average ({eng.net_arith_effective}): {m}")
        assert m is not None and "draw_max_abs" in m and m["draw_max_abs"] <= 5e-5 and m["ok"]
    finally:
        eng.close()
    assert len(games) >= G
    for g in games:
        state = g["data"][0]
        for item in g["data"][1:]:
            assert item[0] in xo.get_legal_moves(state), g["game_id"]
            state = xo.step(state, item[0])
    if moves_left:
        return
    off = SelfPlayEngine(_cfg(), G, net=_net(2), dtype=t.float32, seed=13)
    try:
        assert not off.draw and off.search.wdl_rows is None
        off.start()
        for _ in range(8):
            off.step()
        m = off.audit_network(16)
        assert m is not None and "draw_max_abs" not in m
        assert off.net.calibration is None or "draw_max_abs" not in off.net.calibration["chosen"]
    finally:
        off.close()
    shown = SelfPlayEngine(_cfg(show_wdl=True), G, net=_net(2), dtype=t.float32, seed=13)       # on by show_wdl alone
    try:
        assert shown.draw and shown.search.draw_on and shown.search.draw_score == 0.0
    finally:
        shown.close()


def test_guard_reports_d_only_when_asked(gpu):
    import torch as t
    from cchess_alphazero.agent.model import (calibration_planes, guarded_inference_net, measure_against_reference,
                                              reference_forward_f64, within_guard)
    dev = t.device("cuda", t.cuda.current_device())
    raw = _net(5)
    inf = guarded_inference_net(raw, t.float32, trunk="mfma", device=dev, draw=True)
    assert inf.calibration is not None and all("draw_max_abs" in m for m in inf.calibration["candidates"])
    planes = calibration_planes(32, 14, dev, seed=9)
    ref = reference_forward_f64(raw, planes, with_wdl=True)
    m = measure_against_reference(inf, ref, planes, draw_ref=ref[-1][:, 1])
    print(f"\nguard with the draw probability ({inf.arith_effective}): {m}")
    assert within_guard(m) and m["draw_max_abs"] <= 5e-5
    assert not within_guard(dict(m, draw_max_abs=6e-5))
    plain = measure_against_reference(inf, ref, planes)
    assert "draw_max_abs" not in plain and {k: v for k, v in m.items() if k != "draw_max_abs"} == plain
    with pytest.raises(RuntimeError, match="scalar value head"):
        guarded_inference_net(_net(6, value_outputs=1), t.float32, trunk="mfma", device=dev, draw=True)


# ---- 8. the arena ------------------------------------------------------------------------------------------------------------------
def test_arena_needs_the_head_in_both_networks(gpu):
    import torch as t
    from cchess_alphazero.agent.model import InferenceNet
    from cchess_alphazero.worker.evaluator import EvaluateWorker
    dev = t.device("cuda", t.cuda.current_device())
    cfg = _cfg(draw_score=TEST_SCORE)
    cfg.eval.game_num = 2
    with_wdl = InferenceNet(_net(7), t.float32, trunk="mfma").to(dev)
    scalar = InferenceNet(_net(8, value_outputs=1), t.float32, trunk="mfma").to(dev)
    for pair in ((with_wdl, scalar), (scalar, with_wdl)):
        with pytest.raises(ValueError, match="opt --value-head wdl"):
            EvaluateWorker(cfg, evaluators=pair, dtype=gpu.N.U8)
    w = EvaluateWorker(cfg, evaluators=(with_wdl, with_wdl), dtype=gpu.N.U8)
    stats = {}
    res = w.play_games(2, u_fn=lambda i, ply: 0.5, stats=stats)
    assert len(res) == 2 and stats["expansions"] > 0 and stats["overflow_sims"] == 0


# ---- 9. CChessPlayer and the UCI front-end -----------------------------------------------------------------------------------------
def _uci_cfg(value_outputs):
    from cchess_alphazero.config import Config, PlayWithHumanConfig
    cfg = Config(config_type="mini")
    PlayWithHumanConfig().update_play_config(cfg.play)
    cfg.model.cnn_filter_num, cfg.model.res_layer_num, cfg.model.value_outputs = 128, 2, value_outputs
    cfg.play.search_threads = 8
    cfg.resource.model_best_config_path = "/nonexistent/config.json"      # random-init network
    return cfg


def _wdl_of(line):
    tok = line.split()
    i = tok.index("wdl")
    assert tok[i - 2] == "score"                            # directly behind the score
    return [int(x) for x in tok[i + 1:i + 4]]


def _go(u, out, cmd):
    n = out.getvalue().count("bestmove")
    u.handle(cmd)
    t0 = time.time()
    while out.getvalue().count("bestmove") <= n:
        assert time.time() - t0 < 120, out.getvalue()
        time.sleep(0.02)


def test_player_and_uci_show_wdl(gpu):
    from cchess_alphazero.agent.player import CChessPlayer, DrawUnavailable
    from cchess_alphazero.uci import UCI
    out = io.StringIO()
    u = UCI(_uci_cfg(3), out=out)
    for line in ("uci", "setoption name UCI_ShowWDL value true", "setoption name DrawScore value -0.25", "isready",
                 "position startpos moves h2e2"):
        u.handle(line)
    assert "option name UCI_ShowWDL type check default false" in out.getvalue()
    # one search of 64 simulations by the player the front-end builds: the chosen move's W / D / L
    p = CChessPlayer(u.config, search_tree={}, pipes=u.pipe, uci=True, debugging=True, side=1)
    try:
        assert p.draw and p.show_wdl and p._search.draw_on and p._search.draw_score == -0.25
        action, _ = p.action(u.state, u.turns, depth=64)
        assert action is not None and p.done_tasks == 64
        assert p.last_wdl is not None and sum(p.last_wdl) == 1000 and min(p.last_wdl) >= 0
        dr, st = p._search.node_draws(), p._search.root_stats()
        assert np.array_equal(dr["dn"], st["n"]) and dr["dsum"].any()
    finally:
        p.close()
    # `go depth 1`: 100 simulations, the fewest a `go` can ask for; the per-depth line and the last line carry the triple
    _go(u, out, "go depth 1")
    info = [l for l in out.getvalue().splitlines() if l.startswith("info depth")]
    assert len(info) >= 2 and all(" wdl " in l for l in info), info
    for l in info:
        w = _wdl_of(l)
        assert sum(w) == 1000 and min(w) >= 0, l
    assert " pv " in info[0]
    u.handle("setoption name UCI_ShowWDL value false")      # the draw score alone: the average is on, nothing is shown
    _go(u, out, "go depth 1")
    later = [l for l in out.getvalue().splitlines() if l.startswith("info depth")][len(info):]
    assert later and not any(" wdl " in l for l in later)
    assert u.handle("quit") is False
    # a scalar model: an info string, and the search goes on without the option
    out = io.StringIO()
    u = UCI(_uci_cfg(1), out=out)
    for line in ("uci", "setoption name UCI_ShowWDL value true", "isready", "position startpos"):
        u.handle(line)
    with pytest.raises(DrawUnavailable, match="opt --value-head wdl"):
        CChessPlayer(u.config, search_tree={}, pipes=u.pipe, uci=True)
    _go(u, out, "go depth 1")
    text = out.getvalue()
    assert "info string the draw average" in text and "opt --value-head wdl" in text and " wdl " not in text.replace("head wdl", "")
    assert [l for l in text.splitlines() if l.startswith("bestmove")][-1].split()[1] != "none"
    assert u.handle("quit") is False
