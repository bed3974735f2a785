"""-m gpu: the schedule of c_puct and the policy temperature (cz_search_set_cpuct_schedule, cz_search_set_policy_temperature,
cz_debug_cpuct; run.py self / eval / reanalyse --cpuct-factor F --cpuct-base B --policy-temp T; the UCI options CPuctFactor,
CPuctBase, PolicyTemperature).

The yardstick of the schedule is tests/puct_schedule_oracle.py, search_model.Search with c(sum_n) in its PUCT rule;
tests/test_puct_schedule_cpu.py pins it to the plain search at F = 0 and asserts that F = 2, B = 50 moves the counts of the
cases.  K = 1 searches on probability rows are compared with it exactly.  The temperature is held by an exact identity -- a
search at T fed l against a search at T = 1 fed l / T, T a power of two -- and by the float64 softmax of l / T.  Every search
here is one game, K = 1, at most 200 simulations.  With K > 1 there is no Python model: only determinism is checked."""
import ctypes as C
import io
import logging
import math

import numpy as np
import pytest

import puct_schedule_oracle as po
import stub_net
from oracle import xq_oracle as xo
from test_gpu_search import assert_root_equal, boards_tensor, gpu, no_act_tensors, play_config, stub_eval  # noqa: F401

pytestmark = pytest.mark.gpu
ERR_ARG = -1                                                # include/czero.h CZ_ERR_ARG
F, B = po.F, po.B
C_PUCT = 1.5


def _pc(sims=po.SIMS, K=1):
    return play_config(simulation_num_per_move=sims, search_threads=K, noise_eps=0.0, tau_decay_rate=0.0)


# ---- 1. the device function alone ----------------------------------------------------------------------------------------------
SUMS = [0, 1, 2, 63, 64, 199, 800, 10 ** 6, 2 ** 31 - 2]
PARAMS = [(0.0, 19652.0), (2.0, 50.0), (1.0, 19652.0), (3.894, 38739.0)]


def test_debug_cpuct(gpu):
    t = gpu.torch
    sums = t.tensor(SUMS, dtype=t.int32, device="cuda")
    worst = 0.0
    for f, b in PARAMS:
        c, c32 = gpu.S.debug_cpuct(sums, C_PUCT, f, b)
        c, c32 = c.cpu().numpy(), c32.cpu().numpy()
        want = np.array([po.cpuct(C_PUCT, f, b, n) for n in SUMS], dtype=np.float64)
        d = float(np.abs(c - want).max())
        worst = max(worst, d)
        print(f"F = {f}, B = {b}: worst |c - oracle| = {d:.3e}")
        assert d <= 1e-12, (f, b, c, want)
        assert (c32.view(np.uint32) == c.astype(np.float32).view(np.uint32)).all()
        if f == 0.0:
            assert (c.view(np.uint64) == np.float64(C_PUCT).view(np.uint64)).all()
            assert (c32.view(np.uint32) == np.float32(C_PUCT).view(np.uint32)).all()
    print(f"worst difference seen: {worst:.3e}")
    L = gpu.N.lib()
    out = t.empty(len(SUMS), dtype=t.float64, device="cuda")
    out32 = t.empty(len(SUMS), dtype=t.float32, device="cuda")
    st = C.c_void_p(t.cuda.current_stream().cuda_stream)
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    nan, inf = float("nan"), float("inf")
    for f, b in ((-1.0, 50.0), (nan, 50.0), (inf, 50.0), (2.0, -50.0), (2.0, nan), (2.0, inf), (2.0, 0.5), (2.0, 0.0)):
        assert L.cz_debug_cpuct(ptr(sums), len(SUMS), C_PUCT, f, b, ptr(out), ptr(out32), st) == ERR_ARG, (f, b)
    assert L.cz_debug_cpuct(ptr(sums), 0, C_PUCT, 2.0, 50.0, ptr(out), ptr(out32), st) == 0
    assert L.cz_debug_cpuct(None, 1, C_PUCT, 2.0, 50.0, ptr(out), ptr(out32), st) == ERR_ARG


# ---- 2. whole searches against the oracle --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_runs():
    """The oracle's searches of the ten cases at F = 2, B = 50, computed once."""
    return [(c, po.run_case(c)) for c in po.cases()]


def _walk(gpu, c, res, setup, targets=False):
    """The searches `res` of one case on one search object; returns the kinds of search seen."""
    s = gpu.S.Search(_pc(), 1, seed=7)
    try:
        s.policy_logits(False)                              # probability rows: the priors are the oracle's bits
        setup(s)
        ev = stub_eval(gpu, dict(kind="hash", salt=c["salt"]))
        for r in res:
            na, nn = no_act_tensors(gpu, [r["no_act"]])
            s.set_roots(boards_tensor(gpu, [r["state"]]), no_act=na, n_no_act=nn)
            s.run_until_idle(ev)
            what = f"{c['name']} {r['state']}"
            assert_root_equal(s.root_stats(), 0, r["stats"], what)
            assert xo.label_str(int(s.choose([0.5])[0])) == r["best"], what
            if targets:
                t = s.root_targets()
                nm = len(r["targets"])
                assert int(t["raw_total"][0]) == r["raw_total"], what
                assert (t["n"][0, :nm] == r["targets"]).all(), (what, t["n"][0, :nm], r["targets"])
                assert (t["n"][0, nm:] == 0).all(), what
        return s.counters()
    finally:
        s.close()


def test_searches_under_the_schedule_match_the_oracle(gpu, oracle_runs):
    kinds = set()
    for c, (res, osearch) in oracle_runs:
        ctr = _walk(gpu, c, res, lambda s: s.set_cpuct_schedule(F, B))
        for key in ("sims", "expansions", "terminal_sims", "repetition_sims"):
            assert ctr[key] == getattr(osearch, key), (c["name"], key)
        kinds.add(c["kind"])
        kinds.add("wide" if len(res[0]["stats"]["n"]) > 64 else None)
    assert kinds >= {"ban", "reuse", "wide"}
    # the second half of a root's edges is searched under the schedule (the tenth case)
    n = oracle_runs[9][1][0][0]["stats"]["n"]
    assert len(n) > 64 and (n[64:] > 0).any()


def test_solver_searches_under_the_schedule_match_the_oracle(gpu, oracle_runs):
    """solver_oracle's model composes with the schedule by subclassing (po.SolverSearch): every case is compared with it,
    and where it proves nothing the counts are those of the search without the solver."""
    open_cases = 0
    for c, (plain, _) in oracle_runs:
        res, osearch = po.run_case(c, solver=True)

        def setup(s):
            s.set_solver(True)
            s.set_cpuct_schedule(F, B)
        _walk(gpu, c, res, setup)
        if not any(n.status != po.so.OPEN for n in osearch.tree.values()):
            open_cases += 1
            assert [r["stats"]["n"].tolist() for r in res] == [r["stats"]["n"].tolist() for r in plain], c["name"]
    assert open_cases > 0


# ---- 3. forced playouts under the schedule -------------------------------------------------------------------------------------
def test_forced_playouts_prune_with_the_schedule(gpu):
    pruned = differ = 0
    for c in po.cases():
        res, osearch = po.run_case(c, k=2.0)

        def setup(s):
            s.set_forced_playouts(2.0)
            s.set_cpuct_schedule(F, B)
        _walk(gpu, c, res, setup, targets=True)
        for r in res:
            pruned += int(r["raw_total"] > int(r["targets"][(po.sm.banned_labels(r["stats"]["moves"], r["no_act"])
                                                              & po.sm.BANNED) == 0].sum()))
            st = r["stats"]
            lab = po.sm.banned_labels(st["moves"], r["no_act"])
            flat, _ = po.fo.prune(lab, st["n"], st["w"], st["p"], C_PUCT, 2.0)
            differ += int((flat != r["targets"]).any())
    assert pruned > 0
    assert differ > 0                                       # c(S) is not c_puct: the pruning reads the schedule


# ---- 4. / 5. the policy temperature -------------------------------------------------------------------------------------------
def _logit_search(gpu, c, sims, T, scale=1.0, setup=None, state=None):
    """One K = 1 search fed l = log p + per-row offset, times `scale`, with the temperature T.  Returns (root_stats, chosen
    label, the first evaluated row's logits as fed -- the root's --, the search's eval_cache_info)."""
    t = gpu.torch
    s = gpu.S.Search(_pc(sims), 1, seed=7)
    try:
        s.policy_logits(True)
        if setup:
            setup(s)
        s.set_policy_temperature(T)
        ev = stub_eval(gpu, dict(kind="hash", salt=c["salt"]))
        s.set_roots(boards_tensor(gpu, [state or c["state"]]))
        first, i = None, 0
        for _ in range(10000):
            s.round()
            pending, rows = s.leaf_rows()
            if pending == 0:
                break
            if not rows.numel():
                continue
            p, v = ev(s.planes.index_select(0, rows))
            off = float((i % 13) - 6) * 3.5                 # -21 .. +21, another one per evaluation
            l = (t.log(p.double()).float() + off) * np.float32(scale)
            i += 1
            if first is None:
                first = l[0].cpu().numpy().copy()
            s.policy.index_copy_(0, rows, l)
            s.value.index_copy_(0, rows, v.float())
        else:
            raise AssertionError("the search did not finish")
        return s.root_stats(), int(s.choose([0.5])[0]), first, s.eval_cache_info()
    finally:
        s.close()


@pytest.mark.parametrize("T", [2.0, 0.5])
def test_temperature_is_the_scaled_logits_search_bit_for_bit(gpu, T):
    """Scaling by a power of two commutes with the float32 subtraction of the maximum: a search at T fed l is a search at
    T = 1 fed l / T, in p, n, w and the chosen move."""
    cases = po.cases()
    moved = 0
    for c in (cases[0], cases[4], cases[9]):
        a, move_a, _, _ = _logit_search(gpu, c, po.SIMS, T)
        b, move_b, _, _ = _logit_search(gpu, c, po.SIMS, 1.0, scale=1.0 / T)
        one, _, _, _ = _logit_search(gpu, c, po.SIMS, 1.0)
        nm = int(a["counts"][0])
        ref = dict(moves=b["moves"][0, :nm], n=b["n"][0, :nm], w=b["w"][0, :nm], p=b["p"][0, :nm], sum_n=int(b["sum_n"][0]))
        assert_root_equal(a, 0, ref, f"{c['name']} T = {T}")
        assert move_a == move_b
        moved += int((a["p"][0, :nm] != one["p"][0, :nm]).any() and (a["n"][0, :nm] != one["n"][0, :nm]).any())
    assert moved > 0                                        # (the equality is not the plain search's)


def test_temperature_priors_are_the_softmax_of_the_scaled_logits(gpu):
    T = 1.4
    cases = po.cases()
    wide = 0
    for c in (cases[0], cases[7], cases[9]):
        st, _, row, _ = _logit_search(gpu, c, 8, T)
        nm = int(st["counts"][0])
        l = row[st["moves"][0, :nm].astype(np.int64)].astype(np.float64) / T
        want = np.exp(l - l.max())
        want /= want.sum()
        got = st["p"][0, :nm].astype(np.float64)
        d = np.abs(got - want)
        print(f"{c['name']}: {nm} moves, worst |dp| = {d.max():.3e} at max p = {want.max():.3e}, sum = {got.sum():.9f}")
        assert d.max() <= 4e-6 * want.max() and np.all(d <= 2e-5 * want + 1e-12), (c["name"], got, want)
        assert abs(got.sum() - 1.0) <= 64 * 2.0 ** -24
        wide += int(nm > 64)
    assert wide > 0


# ---- 6. the setters ------------------------------------------------------------------------------------------------------------
def _err(s):
    return s.L.cz_last_error().decode()


def test_setters(gpu):
    t = gpu.torch
    c = po.cases()[0]
    s = gpu.S.Search(_pc(32), 1, seed=3)
    try:
        st = s._stream()
        # arguments
        nan, inf = float("nan"), float("inf")
        for f, b in ((-1.0, 50.0), (nan, 50.0), (inf, 50.0), (2.0, 0.5), (2.0, nan), (2.0, inf), (2.0, -1.0)):
            assert s.L.cz_search_set_cpuct_schedule(s.h, f, b, st) == ERR_ARG, (f, b)
        assert s.L.cz_search_set_cpuct_schedule(None, 2.0, 50.0, st) == ERR_ARG
        for bad in (0.0, 0.0999, 10.5, -1.0, nan, inf):
            assert s.L.cz_search_set_policy_temperature(s.h, bad, st) == ERR_ARG, bad
        assert s.L.cz_search_set_policy_temperature(None, 2.0, st) == ERR_ARG
        # a temperature needs logit rows, and keeps them
        s.policy_logits(False)
        assert s.L.cz_search_set_policy_temperature(s.h, 2.0, st) == ERR_ARG and "probabilities" in _err(s)
        with pytest.raises(gpu.N.NativeError):
            s.set_policy_temperature(2.0)
        assert s.policy_temp == 1.0
        s.set_policy_temperature(1.0)                       # T = 1 is never refused
        s.policy_logits(True)
        s.set_policy_temperature(2.0)
        assert s.policy_temp == 2.0
        assert s.L.cz_search_policy_logits(s.h, 0) == ERR_ARG and "cz_search_set_policy_temperature" in _err(s)
        s.policy_logits(True)
        s.set_policy_temperature(1.0)
        s.policy_logits(False)
        # a change of T drops the trees
        s.policy_logits(True)
        ev = stub_eval(gpu, dict(kind="hash", salt=c["salt"]))
        logit_ev = lambda planes: (t.log(ev(planes)[0].double()).float(), ev(planes)[1])  # noqa: E731
        s.set_roots(boards_tensor(gpu, [c["state"]]))
        s.run_until_idle(logit_ev)
        assert s.memory_info()["nodes"] > 0 and int(s.root_stats()["counts"][0]) > 0
        s.set_policy_temperature(1.0)                       # no change: nothing is reset
        assert s.memory_info()["nodes"] > 0
        s.set_cpuct_schedule(F, B)                          # the schedule resets nothing either
        assert s.memory_info()["nodes"] > 0 and (s.cpuct_factor, s.cpuct_base) == (F, B)
        s.set_policy_temperature(2.0)
        assert s.memory_info()["nodes"] == 0 and int(s.root_stats()["counts"][0]) == 0
        assert math.isnan(float(s.node_net_value()[0]))     # the root is not in the tree
    finally:
        s.close()


def test_a_change_of_temperature_empties_the_evaluation_cache(gpu):
    t = gpu.torch
    c = po.cases()[0]
    ev = stub_eval(gpu, dict(kind="hash", salt=c["salt"]))
    logit_ev = lambda planes: (t.log(ev(planes)[0].double()).float(), ev(planes)[1])  # noqa: E731

    def search(s):
        s.set_roots(boards_tensor(gpu, [c["state"]]))
        s.run_until_idle(logit_ev)
        return s.root_stats()

    s = gpu.S.Search(_pc(64), 1, seed=3)
    fresh = gpu.S.Search(_pc(64), 1, seed=3)
    try:
        for x in (s, fresh):
            x.policy_logits(True)
        s.set_eval_cache(12)
        search(s)
        assert s.eval_cache_info()["stores"] > 0
        s.reset_trees()
        search(s)                                           # the repeated position is answered by the table
        assert s.eval_cache_info()["hits"] > 0
        s.set_policy_temperature(2.0)                       # the entries hold priors formed at T = 1
        assert s.eval_cache_info() == dict(entries=1 << 12, probes=0, hits=0, stores=0)
        a = search(s)
        info = s.eval_cache_info()
        assert info["hits"] == 0 and info["stores"] > 0
        fresh.set_policy_temperature(2.0)
        b = search(fresh)
        nm = int(b["counts"][0])
        ref = dict(moves=b["moves"][0, :nm], n=b["n"][0, :nm], w=b["w"][0, :nm], p=b["p"][0, :nm], sum_n=int(b["sum_n"][0]))
        assert_root_equal(a, 0, ref, "after the change of T")
    finally:
        s.close()
        fresh.close()


def test_both_setters_succeed_beside_every_other_option(gpu):
    from cchess_alphazero.lib import reanalyse as ra
    from test_gpu_reanalyse import _record, stored_games
    others = {
        "gumbel": lambda s: s.set_gumbel(8),
        "gumbel_full": lambda s: (s.set_gumbel(8), s.set_gumbel_full(True)),
        "solver": lambda s: s.set_solver(True),
        "kld_gain": lambda s: s.set_kld_gain(1e-3, 16),
        "smart_pruning": lambda s: s.set_smart_pruning(True),
        "forced_playouts": lambda s: s.set_forced_playouts(2.0),
        "playout_cap": lambda s: s.set_playout_cap(8, 0.25),
        "eval_cache": lambda s: s.set_eval_cache(10),
        "moves_left": lambda s: s.set_moves_left(0.0027, 0.0345),
        "draw": lambda s: s.set_draw(True, -0.25),
        "lcb": lambda s: s.set_lcb(2.0, 0.15),
        "script": lambda s: (s.record_visits(True), s.set_script(*ra.pack_scripts([_record(*stored_games()[0])], 19)[0])),
    }
    for name, on in others.items():
        for first in (True, False):                         # the other option first, or the two setters first
            s = gpu.S.Search(play_config(simulation_num_per_move=16, search_threads=4), 2, seed=1)
            try:
                s.policy_logits(True)
                if first:
                    on(s)
                s.set_cpuct_schedule(3.894, 38739.0)
                s.set_policy_temperature(1.4)
                if not first:
                    on(s)
                assert (s.cpuct_factor, s.cpuct_base, s.policy_temp) == (3.894, 38739.0, 1.4), name
            finally:
                s.close()


# ---- K > 1: no Python model, determinism alone ---------------------------------------------------------------------------------
def test_two_runs_at_k_8_are_identical(gpu):
    t = gpu.torch
    c = po.cases()[1]
    ev = stub_eval(gpu, dict(kind="hash", salt=c["salt"]))
    logit_ev = lambda planes: (t.log(ev(planes)[0].double()).float(), ev(planes)[1])  # noqa: E731

    def run(factor):
        s = gpu.S.Search(_pc(po.SIMS, K=8), 1, seed=5)
        try:
            s.policy_logits(True)
            s.set_cpuct_schedule(factor, B)
            s.set_policy_temperature(1.4)
            s.set_roots(boards_tensor(gpu, [c["state"]]))
            s.run_until_idle(logit_ev)
            st = s.root_stats()
            return [st[k].tobytes() for k in ("moves", "n", "w", "p", "sum_n")]
        finally:
            s.close()
    a = run(F)
    assert a == run(F)
    assert a != run(0.0)


# ---- 7. engine, UCI ------------------------------------------------------------------------------------------------------------
def _cfg(**engine):
    from cchess_alphazero.config import Config
    cfg = Config("mini")
    cfg.model.cnn_filter_num, cfg.model.res_layer_num = 128, 2
    cfg.play.simulation_num_per_move, cfg.play.search_threads, cfg.play.noise_eps = 16, 8, 0.0
    cfg.play.max_game_length = 8
    for k, v in engine.items():
        setattr(cfg.engine, k, v)
    return cfg


def _net(seed):
    import torch
    from cchess_alphazero.agent.model import CChessNet
    torch.manual_seed(seed)
    return CChessNet(cnn_filter_num=128, res_layer_num=2).eval()


def test_selfplay_engine_runs_logs_and_reports(gpu, tmp_path, monkeypatch, caplog):
    import torch as t
    from cchess_alphazero import search_options as so
    from cchess_alphazero.engine import SelfPlayEngine
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    with caplog.at_level(logging.INFO, logger="cchess_alphazero.engine"):
        eng = SelfPlayEngine(_cfg(cpuct_factor=3.894, cpuct_base=38739.0, policy_temp=1.4), 4, net=_net(2), dtype=t.float32,
                             seed=13)
    try:
        for line in (so.CPUCT_LOG.format(cpuct_factor=3.894, cpuct_base=38739.0), so.POLICY_TEMP_LOG.format(policy_temp=1.4)):
            assert sum(line in r.getMessage() for r in caplog.records) == 1, line
        assert eng.policy_logits and eng.cpuct_on and eng.policy_temp_on
        assert (eng.cpuct_factor, eng.cpuct_base, eng.policy_temp) == (3.894, 38739.0, 1.4)
        assert (eng.search.cpuct_factor, eng.search.cpuct_base, eng.search.policy_temp) == (3.894, 38739.0, 1.4)
        eng.start(0, 0)
        for _ in range(6):
            eng.step()
        t.cuda.synchronize()
        ctr = eng.counters()
        assert ctr["expansions"] > 0 and ctr["overflow_sims"] == 0 and ctr["tree_resets"] == 0
    finally:
        eng.close()
    # the keyword arguments override the configuration; the defaults switch nothing on
    off = SelfPlayEngine(_cfg(), 4, net=_net(2), dtype=t.float32, seed=13, cpuct_factor=2.0, cpuct_base=50.0)
    try:
        assert off.cpuct_on and not off.policy_temp_on and (off.search.cpuct_factor, off.search.policy_temp) == (2.0, 1.0)
    finally:
        off.close()
    # probabilities cannot take a temperature: an evaluator callable, a network asked for probability rows
    ev = stub_eval(gpu, dict(kind="hash", salt=1))
    with pytest.raises(ValueError, match="the policy temperature .policy_temp 1.4. is applied to the legal moves' logits, and an "
                                         "evaluator callable hands the search probabilities"):
        SelfPlayEngine(_cfg(policy_temp=1.4), 4, evaluator=ev, seed=13)
    with pytest.raises(ValueError, match="engine.policy_logits = False hands the search probabilities"):
        SelfPlayEngine(_cfg(policy_temp=1.4, policy_logits=False), 4, net=_net(2), dtype=t.float32, seed=13)
    with pytest.raises(ValueError, match="policy_temp 11"):
        SelfPlayEngine(_cfg(policy_temp=11.0), 4, net=_net(2), dtype=t.float32, seed=13)
    eng = SelfPlayEngine(_cfg(cpuct_factor=2.0), 4, evaluator=ev, seed=13)      # the schedule needs nothing of the rows
    try:
        assert eng.search.cpuct_factor == 2.0
    finally:
        eng.close()


def test_uci_lists_and_accepts_the_options(gpu, tmp_path, monkeypatch):
    from cchess_alphazero.uci import UCI
    from test_gpu_lcb import _go, _player_cfg
    out = io.StringIO()
    u = UCI(_player_cfg(tmp_path, monkeypatch), out=out)
    u.handle("uci")
    for line in ("option name CPuctFactor type string default 0", "option name CPuctBase type string default 19652",
                 "option name PolicyTemperature type string default 1"):
        assert line in out.getvalue()
    u.pipe = stub_net.StubPipe(lambda p: stub_net.hash_stub_numpy(p, 1))
    for line in ("setoption name CPuctFactor value 2", "setoption name CPuctBase value 50",
                 "setoption name PolicyTemperature value 1.4", "setoption name CPuctBase value 0.5", "isready", "position startpos"):
        u.handle(line)
    assert "info string CPuctBase 0.5: expected a finite value >= 1" in out.getvalue()
    e = u.config.engine
    assert (e.cpuct_factor, e.cpuct_base, e.policy_temp) == (2.0, 50.0, 1.4)
    _go(u, out, "go depth 1")
    # the player's pipe hands over probabilities: the temperature is refused in one sentence, the schedule is searched with
    assert "info string the policy temperature (policy_temp 1.4) is applied to the legal moves' logits" in out.getvalue()
    assert out.getvalue().count("bestmove") == 1
    assert u.handle("quit") is False
    from cchess_alphazero.agent.player import CChessPlayer, PolicyTempUnavailable
    cfg = _player_cfg(tmp_path, monkeypatch)
    cfg.engine.cpuct_factor, cfg.engine.cpuct_base, cfg.engine.policy_temp = 2.0, 50.0, 1.4
    pipe = stub_net.StubPipe(lambda p: stub_net.hash_stub_numpy(p, 1))
    with pytest.raises(PolicyTempUnavailable, match="the player's pipe hands the search probabilities"):
        CChessPlayer(cfg, search_tree={}, pipes=pipe, enable_resign=False)
    pl = CChessPlayer(cfg, search_tree={}, pipes=pipe, enable_resign=False, policy_temp=1.0)
    try:
        assert pl.cpuct_on and (pl._search.cpuct_factor, pl._search.cpuct_base, pl._search.policy_temp) == (2.0, 50.0, 1.0)
    finally:
        pl.close()
