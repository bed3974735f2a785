"""The draw average of the search on the CPU: the stub, the Python oracle against search_model.Search, the conversion, the
W / D / L line of the UCI front-end, the option checks of the host layers, and what the rule does to a search.

TEST_SCORE is what tests/test_gpu_draw_search.py searches with: a draw is worth -0.5 to the side to move at the root, large
enough that at 200 simulations of the hash stub it decides visits (test_the_cases_show_the_draw_score asserts it: a
condition on these inputs, not a measurement)."""
import io

import numpy as np
import pytest

import draw_search_oracle as do
import search_limits as sl
import search_model as sm
import stub_draw as sd
from oracle import xq_oracle as xo

TEST_SCORE = -0.5
Q = sd.QUANTA
MID_SIMS = 400


# ---- the stub ----------------------------------------------------------------------------------------------------------------
def test_stub_numpy_and_torch_agree_bit_for_bit():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(5)
    planes = (rng.random((64, 14, 10, 9)) < 0.1).astype(np.uint8)
    for variant in ("hash", ("flat", 0.25), "peaked"):
        a = sd.draw_stub_numpy(planes, 11, variant)
        b = sd.draw_stub_torch(torch.from_numpy(planes), 11, variant)
        for u, v in zip(a, b):
            assert np.array_equal(u.view(np.uint32), v.numpy().view(np.uint32)), variant
        p, v, wdl = a
        dq = sd.dq_numpy(planes, 11, variant)
        assert dq.min() >= 0 and dq.max() <= Q and len(set(dq.tolist())) > 16
        d = wdl[:, 1]
        assert np.array_equal(d.astype(np.float64) * Q, dq.astype(np.float64))      # exact multiples of 2^-20
        assert (d.astype(np.float64) <= 1.0 - np.abs(v.astype(np.float64))).all()   # d <= 1 - |v|
        assert np.array_equal(sd.draw_quanta(d), dq)                                 # and the search reads dq back


# ---- (e) the conversion ------------------------------------------------------------------------------------------------------
def test_draw_quanta_of_the_grid():
    assert 0.0 < abs(float(sd.GRID[-1])) < np.finfo(np.float32).tiny                # a subnormal
    assert sd.draw_quanta(sd.GRID).tolist() == sd.GRID_DQ
    assert sd.draw_quanta(sd.GRID[::3]).tolist() == sd.GRID_DQ[::3]


# ---- (a) off is the plain search, bit for bit ----------------------------------------------------------------------------------
def _same_rows(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["best"] == y["best"] and x["stats"]["sum_n"] == y["stats"]["sum_n"]
        for key in ("moves", "n", "p"):
            assert np.array_equal(x["stats"][key], y["stats"][key]), key
        assert np.array_equal(x["stats"]["w"].view(np.uint64), y["stats"]["w"].view(np.uint64))


_COUNTERS = ("sims", "expansions", "terminal_sims", "repetition_sims")


@pytest.mark.parametrize("case", sm.cases(), ids=lambda c: c["name"])
def test_off_and_score_zero_are_the_plain_search(case):
    base, s0 = sm.run_case(case, 0.0)
    off, s = do.run_case(case, TEST_SCORE, on=False)
    _same_rows(base, off)
    assert [getattr(s, k) for k in _COUNTERS] == [getattr(s0, k) for k in _COUNTERS]
    for r in off:
        assert not r["draws"]["dsum"].any() and not r["draws"]["dn"].any()
    # (b) on with score 0: the plain search, and the records are kept
    rows, s = do.run_case(case, 0.0)
    _same_rows(base, rows)
    assert [getattr(s, k) for k in _COUNTERS] == [getattr(s0, k) for k in _COUNTERS]
    for i, r in enumerate(rows):
        dr, st = r["draws"], r["stats"]
        assert np.array_equal(dr["dn"], st["n"])
        assert (dr["dsum"] >= 0).all() and (dr["dsum"] <= Q * dr["dn"].astype(np.int64)).all()
        if i == 0:      # a search on an empty tree: the root's records hold every simulation that ended below it
            assert int(dr["dsum"].sum()) == r["dq_below"] and r["dq_below"] > 0
            assert int(dr["dn"].sum()) == st["sum_n"] - 1


# ---- (c) the inputs show the draw score ------------------------------------------------------------------------------------------
def test_the_cases_show_the_draw_score():
    differ = 0
    cases = sm.cases()
    for case in cases:
        base, _ = sm.run_case(case, 0.0)
        rows, _ = do.run_case(case, TEST_SCORE)
        differ += any(not np.array_equal(a["stats"]["n"], b["stats"]["n"]) for a, b in zip(base, rows))
    assert 2 * differ >= len(cases), differ


def test_the_sign_follows_the_depth():
    """Uniform policy, value 0: every root move has the same prior and q stays 0, while one more visit costs an edge a third of
    its exploration term (0.04 here) and the draw term spans at most |score| = 0.02: the edges are visited once each before any
    is visited twice, and which ones get the second visit is decided by sigma * dbar alone.  After one visit an edge's mean is
    its child's own d.  With score < 0 the root's second visits go to the children with the smallest d, with score > 0 to the
    largest."""
    salt = 3
    nm = len(xo.get_legal_moves(xo.INIT_STATE))
    extra = nm // 2
    net = lambda planes: sd.draw_stub_numpy(planes, salt, ("flat", 0.0))
    for score in (-0.02, 0.02):
        s = do.Search(sm.play_cfg(1 + nm + extra), salt, score=score, net=net)
        s.search(xo.INIT_STATE)
        root = s.tree[xo.INIT_STATE]
        dq = np.array([s.tree[xo.step(xo.INIT_STATE, mv)].dq for mv in root.moves])
        n = np.array(root.n)
        assert sorted(set(n.tolist())) == [1, 2] and int((n == 2).sum()) == extra and len(set(dq.tolist())) > nm // 4
        pairs = [(i, j) for i in range(nm) for j in range(nm) if dq[i] < dq[j]]
        if score < 0:
            assert all(n[i] >= n[j] for i, j in pairs), (dq, n)
        else:
            assert all(n[i] <= n[j] for i, j in pairs), (dq, n)


# ---- (d) the deferred ends ---------------------------------------------------------------------------------------------------
MID_SCORE = 0.0


def mid_search(score=MID_SCORE):
    """The MID position under the peaked policy, K = 1, 400 simulations, option on: what drives every deferred value.
    The score is 0 here.  The peaked stub's value is 0 everywhere, so q is 0 and a repetition worth 0 needs both sides to walk
    back into it; with any other score sigma is negative for one of the two, whose edges into the repetition (dbar = 1) then
    lose every tie, and the draws by repetition vanish: 0 of them at scores +-0.02 .. +-1 and, at TEST_SCORE, at every stub
    salt from 1 to 40 (checked on the CPU).  That is the rule at work, not a defect of the case; the records and the deferred
    values are what this case is for, and they are the same code at any score."""
    salt = sl.PEAKED["salt"]
    s = do.Search(sm.play_cfg(MID_SIMS), salt, score=score, net=lambda planes: sd.draw_stub_numpy(planes, salt, "peaked"))
    s.search(sl.MID)
    return s


def test_the_mid_case_has_every_deferred_end():
    s = mid_search()
    print(f"rep0 {s.rep0_sims}, rep1 {s.rep1_sims}, terminal {s.terminal_sims}")
    assert s.rep0_sims >= 10 and s.rep1_sims >= 1 and s.terminal_sims >= 1
    root = s.node_draws(sl.MID)
    assert int(root["dsum"].sum()) == s.dq_below >= Q * s.rep0_sims                 # each draw by repetition is a whole 2^20
    avoid = mid_search(TEST_SCORE)                                                   # and a score makes them go away
    assert avoid.rep0_sims == 0 and avoid.rep1_sims >= 1 and avoid.terminal_sims >= 1


# ---- (f) the W / D / L line ----------------------------------------------------------------------------------------------------
def test_wdl_permille():
    from cchess_alphazero.uci import wdl_permille
    assert wdl_permille(0.0, 0, 0, 0) is None and wdl_permille(1.0, 0, Q, 1) is None
    assert wdl_permille(0.0, 4, 4 * Q, 4) == (0, 1000, 0)
    assert wdl_permille(4.0, 4, 0, 4) == (1000, 0, 0) and wdl_permille(-8.0, 4, 0, 4) == (0, 0, 1000)   # |w / n| up to 2
    assert wdl_permille(8.0, 4, 4 * Q, 4) == (1000, 0, 0)                            # d is cut to 1 - |a|
    assert wdl_permille(1.0, 4, 0, 0) == (625, 0, 375)                               # no backup through the draw record yet
    assert wdl_permille(1.0, 4, 2 * Q, 4) == (375, 500, 125)
    rng = np.random.default_rng(1)
    for _ in range(2000):
        n = int(rng.integers(1, 50))
        w = float(rng.uniform(-2.0, 2.0)) * n
        dn = int(rng.integers(0, n + 1))
        dsum = int(rng.integers(0, Q * dn + 1))
        a = wdl_permille(w, n, dsum, dn)
        b = wdl_permille(-w, n, dsum, dn)
        assert sum(a) == 1000 and min(a) >= 0, (w, n, dsum, dn, a)
        assert (a[0], a[2]) == (b[2], b[0]) and a[1] == b[1], (w, n, dsum, dn, a, b)


# ---- (g) the option checks -----------------------------------------------------------------------------------------------------
_ROOT = "each defines its own root rule"
_CACHE = "the cache has a kernel instantiation of its own"
_SCRIPT = "each defines its own root rule, start position or game end"
_KERNEL = "each has a kernel instantiation of its own"
PARENT_EXCLUDES = (("gumbel", "fast_sims", _ROOT), ("gumbel", "forced_playouts", _ROOT), ("solver", "gumbel", _ROOT),
                   ("solver", "forced_playouts", _ROOT), ("solver", "eval_cache", _CACHE), ("kld_gain", "gumbel", _ROOT),
                   ("kld_gain", "solver", _ROOT), ("kld_gain", "eval_cache", _CACHE), ("smart_pruning", "gumbel", _ROOT),
                   ("smart_pruning", "solver", _ROOT), ("smart_pruning", "eval_cache", _CACHE))
PARENT_SCRIPT_EXCLUDES = (("gumbel", _SCRIPT), ("solver", _SCRIPT), ("kld_gain", _SCRIPT), ("smart_pruning", _SCRIPT))
PARENT_MOVES_LEFT_EXCLUDES = (
    ("gumbel", "the Gumbel search keeps the network value in the node header word that holds the moves-left prediction"),
    ("solver", _KERNEL), ("kld_gain", _KERNEL), ("smart_pruning", _KERNEL),
    ("eval_cache", _KERNEL + ", and a cache entry holds no moves-left output"))
PARENT_OPTIONS = [("record_visits", ["record_visits"], None), ("fast_sims", ["fast_sims", "full_rate"], "set_playout_cap"),
                  ("forced_playouts", ["forced_playouts"], "set_forced_playouts"), ("record_q", ["record_q"], "record_values"),
                  ("record_surprise", ["record_surprise"], "record_surprise"), ("leaf_mirror", ["leaf_mirror"], "set_leaf_mirror"),
                  ("gumbel", ["gumbel", "gumbel_visit", "gumbel_scale"], "set_gumbel"),
                  ("gumbel_full", ["gumbel_full"], "set_gumbel_full"), ("eval_cache", ["eval_cache"], "set_eval_cache"),
                  ("solver", ["solver"], "set_solver"), ("kld_gain", ["kld_gain", "kld_interval"], "set_kld_gain"),
                  ("smart_pruning", ["smart_pruning"], "set_smart_pruning")]
PARENT_DEFAULTS = {"record_visits": False, "fast_sims": 0, "full_rate": 0.25, "forced_playouts": 0.0, "record_q": False,
                   "record_surprise": False, "leaf_mirror": 0.0, "gumbel": 0, "gumbel_visit": 50.0, "gumbel_scale": 1.0,
                   "gumbel_full": False, "eval_cache": 0, "solver": False, "kld_gain": 0.0, "kld_interval": 100,
                   "smart_pruning": False}


def test_search_options_table():
    from cchess_alphazero import search_options as so
    # the tables this one stands beside are what they were
    assert so.EXCLUDES == PARENT_EXCLUDES and so.SCRIPT_EXCLUDES == PARENT_SCRIPT_EXCLUDES
    assert so.MOVES_LEFT_EXCLUDES == PARENT_MOVES_LEFT_EXCLUDES and so.DEFAULTS == PARENT_DEFAULTS
    assert [(o.values[0].key, [v.key for v in o.values], o.setter) for o in so.OPTIONS] == PARENT_OPTIONS
    assert [k for k, _ in so.DRAW_EXCLUDES] == ["gumbel", "solver", "kld_gain", "smart_pruning", "eval_cache"]
    ok = dict(record_visits=True, fast_sims=8, forced_playouts=2.0, leaf_mirror=0.5, record_q=True, record_surprise=True)
    so.check(ok, sims=64, draw=True)                            # what it composes with
    for key, why in so.DRAW_EXCLUDES:
        v = dict(record_visits=True)
        v[key] = {"gumbel": 8, "kld_gain": 1e-4, "eval_cache": 12}.get(key, True)
        so.check(v, sims=64)                                    # fine without the average
        with pytest.raises(so.SearchOptionError, match=f"draw_score excludes {key}: ") as e:
            so.check(v, sims=64, draw=True)
        assert why in str(e.value)
        with pytest.raises(so.SearchOptionError, match=f"--draw-score excludes {so.VALUES[key].flag}"):
            so.check(v, flags=True, sims=64, draw=True)
    with pytest.raises(so.SearchOptionError, match="draw_score excludes a script"):
        so.check(dict(record_visits=True), script=True, draw=True)
    with pytest.raises(so.SearchOptionError, match="draw_score excludes moves_left_slope: an edge's draw record lies"):
        so.check({}, moves_left=True, draw=True)
    with pytest.raises(so.SearchOptionError, match="moves_left_slope excludes solver"):     # consulted after moves-left
        so.check(dict(solver=True), moves_left=True, draw=True)
    assert so.check_draw(0.0) is False and so.check_draw(0.0, True) is True and so.check_draw(-0.5) is True
    assert so.check_draw(1.0) is True and so.check_draw(-1.0, False) is True
    for bad in (1.5, -1.0001, float("nan"), float("inf")):
        with pytest.raises(so.SearchOptionError, match=r"draw_score .*: expected a finite value in \[-1, 1\]"):
            so.check_draw(bad)
    with pytest.raises(so.SearchOptionError, match="--draw-score 2"):
        so.check_draw(2.0, flags=True)
    assert "opt --value-head wdl" in so.DRAW_REFUSAL
    assert so.DRAW_DEFAULTS == dict(draw_score=0.0, show_wdl=False)


# ---- (h) the flags ---------------------------------------------------------------------------------------------------------------
def test_manager_flags():
    from cchess_alphazero import manager
    p = manager.create_parser()
    cfg = manager.build_config(p.parse_args(["self"]))
    assert (cfg.engine.draw_score, cfg.engine.show_wdl) == (0.0, False)
    cfg = manager.build_config(p.parse_args(["eval", "--draw-score", "-0.25"]))
    assert cfg.engine.draw_score == -0.25
    cfg = manager.build_config(p.parse_args(["self", "--draw-score", "0.5", "--fast-sims", "8", "--leaf-mirror", "0.5"]))
    assert cfg.engine.draw_score == 0.5
    for argv, msg in ((["self", "--draw-score", "-1.5"], "expected a finite value in [-1, 1]"),
                      (["self", "--draw-score", "nan"], "expected a finite value in [-1, 1]"),
                      (["opt", "--draw-score", "0.1"], "is an option of `run.py self` and `run.py eval`"),
                      (["reanalyse", "--draw-score", "0.1"], "--draw-score excludes a script"),
                      (["self", "--draw-score", "0.1", "--solver"], "--draw-score excludes --solver"),
                      (["self", "--draw-score", "0.1", "--kld-gain", "1e-4"], "--draw-score excludes --kld-gain"),
                      (["self", "--draw-score", "0.1", "--eval-cache", "12"], "--draw-score excludes --eval-cache"),
                      (["self", "--draw-score", "0.1", "--record-visits", "--gumbel", "8"], "--draw-score excludes --gumbel"),
                      (["eval", "--draw-score", "0.1", "--smart-pruning"], "--draw-score excludes --smart-pruning"),
                      (["self", "--draw-score", "0.1", "--moves-left-slope", "0.01"],
                       "--draw-score excludes --moves-left-slope")):
        with pytest.raises(SystemExit) as e:
            manager.build_config(p.parse_args(argv))
        assert msg in str(e.value), (argv, str(e.value))
    manager.build_config(p.parse_args(["self", "--solver"]))               # switched off it refuses nothing


def test_uci_option_lines():
    from cchess_alphazero import manager, uci
    assert "option name UCI_ShowWDL type check default false" in uci.ENGINE_ID
    assert "option name DrawScore type string default 0" in uci.ENGINE_ID
    out = io.StringIO()
    u = uci.UCI(manager.build_config(manager.create_parser().parse_args(["self"])), out=out)
    u.handle("setoption name UCI_ShowWDL value true")
    u.handle("setoption name DrawScore value -0.25")
    assert (u.config.engine.show_wdl, u.config.engine.draw_score) == (True, -0.25)
    u.handle("setoption name DrawScore value 3")
    assert u.config.engine.draw_score == -0.25 and "info string DrawScore 3" in out.getvalue()
    u.handle("setoption name UCI_ShowWDL value false")
    assert u.config.engine.show_wdl is False
