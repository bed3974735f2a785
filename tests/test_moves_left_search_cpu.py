"""The moves-left utility of the search on the CPU: the stub's table, the Python oracle against search_model.Search, the
option checks of the host layers, and what the rule does to a search.

TEST_SLOPE / TEST_CAP are what tests/test_gpu_moves_left_search.py searches with: larger than lc0's 0.0027 / 0.0345 so that,
at 200 simulations of the hash stub, the utility decides moves (test_the_cases_show_the_utility asserts it: a condition on
these inputs, not a measurement)."""
import io

import numpy as np
import pytest

import moves_left_search_oracle as mo
import search_model as sm
import stub_moves_left as sml
from oracle import xq_oracle as xo

TEST_SLOPE, TEST_CAP = 0.01, 0.1


# ---- the stub ----------------------------------------------------------------------------------------------------------------
def test_stub_table_rounds_back_with_four_orders_of_margin():
    kq = np.arange(1, sml.KQ_MAX + 1)
    x = sml.X_TABLE[kq]
    assert x.dtype == np.float32 and np.isfinite(x).all()
    stable = 512.0 * sml.softplus_f32(x).astype(np.float64)
    with np.errstate(over="ignore"):
        naive = 512.0 * np.log(np.float32(1.0) + np.exp(x)).astype(np.float32).astype(np.float64)
    f64 = 512.0 * (np.maximum(x.astype(np.float64), 0.0) + np.log1p(np.exp(-np.abs(x.astype(np.float64)))))
    for name, got in (("stable float32", stable), ("naive float32", naive), ("float64", f64)):
        err = np.abs(got - kq).max()
        assert err < 1.3e-4, (name, err)
    assert (sml.quanta_of_x(x) == kq).all()


def test_stub_numpy_and_torch_agree_bit_for_bit():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(5)
    planes = (rng.random((64, 14, 10, 9)) < 0.1).astype(np.uint8)
    for variant in ("hash", ("flat", 0.25)):
        a = sml.ml_stub_numpy(planes, 11, variant)
        b = sml.ml_stub_torch(torch.from_numpy(planes), 11, variant)
        for u, v in zip(a, b):
            assert np.array_equal(u.view(np.uint32), v.numpy().view(np.uint32))
    kq = sml.kq_numpy(planes, 11)
    assert kq.min() >= 1 and kq.max() <= 2048 and len(set(kq.tolist())) > 32


def test_quanta_of_x_edges():
    x = np.array([np.inf, -np.inf, np.nan, 100.0, -104.0, 0.0], dtype=np.float32)
    assert sml.quanta_of_x(x).tolist() == [16 * 1023, 0, 0, 16 * 1023, 0, int(np.rint(np.float32(512.0) * np.float32(np.log1p(np.float32(1.0)))))]


# ---- (a) slope 0 is the plain search, bit for bit ---------------------------------------------------------------------------------
def _same_rows(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["best"] == y["best"] and x["stats"]["sum_n"] == y["stats"]["sum_n"]
        for key in ("moves", "n", "p"):
            assert np.array_equal(x["stats"][key], y["stats"][key]), key
        assert np.array_equal(x["stats"]["w"].view(np.uint64), y["stats"]["w"].view(np.uint64))


@pytest.mark.parametrize("case", sm.cases(), ids=lambda c: c["name"])
def test_slope_zero_is_the_plain_search(case):
    base, s0 = sm.run_case(case, 0.0)
    for kw in (dict(slope=0.0), dict(slope=TEST_SLOPE, cap=0.0), dict(on=False)):
        rows, s = mo.run_case(case, **kw)
        _same_rows(base, rows)
        assert (s.sims, s.expansions, s.terminal_sims, s.repetition_sims) == (s0.sims, s0.expansions, s0.terminal_sims, s0.repetition_sims)


def test_backup_invariants():
    """sum_j mn_j = the backups through the node; every ksum is at least 16 * mn; a leaf's k is the stub's quanta."""
    case = sm.cases()[1]
    rows, s = mo.run_case(case, TEST_SLOPE, TEST_CAP)
    ml, st = rows[0]["ml"], rows[0]["stats"]
    assert int(ml["mn"].sum()) == s.sims - 1 == int(st["n"].sum())      # (the first simulation made the root: no edge)
    assert (ml["ksum"] >= 16 * ml["mn"]).all() and (ml["mn"] == st["n"]).all()
    for state, node in s.tree.items():
        assert node.k == int(sml.kq_numpy(xo.state_to_planes(state)[None], case["salt"])[0])


# ---- (b) the option checks -----------------------------------------------------------------------------------------------------
def test_search_options_table():
    from cchess_alphazero import search_options as so
    assert [k for k, _ in so.MOVES_LEFT_EXCLUDES] == ["gumbel", "solver", "kld_gain", "smart_pruning", "eval_cache"]
    ok = dict(record_visits=True, fast_sims=8, forced_playouts=2.0, leaf_mirror=0.5, record_q=True, record_surprise=True)
    so.check(ok, sims=64, moves_left=True)                      # what it composes with
    for key, why in so.MOVES_LEFT_EXCLUDES:
        v = dict(record_visits=True)
        v[key] = {"gumbel": 8, "kld_gain": 1e-4, "eval_cache": 12}.get(key, True)
        so.check(v, sims=64)                                    # fine without the utility
        with pytest.raises(so.SearchOptionError, match=f"moves_left_slope excludes {key}: ") as e:
            so.check(v, sims=64, moves_left=True)
        assert why in str(e.value)
        with pytest.raises(so.SearchOptionError, match=f"--moves-left-slope excludes {so.VALUES[key].flag}"):
            so.check(v, flags=True, sims=64, moves_left=True)
    with pytest.raises(so.SearchOptionError, match="moves_left_slope excludes a script"):
        so.check(dict(record_visits=True), script=True, moves_left=True)
    assert so.check_moves_left(0.0, 0.0345) is False and so.check_moves_left(0.0027, 0.0) is True
    for bad in ((-1.0, 0.1), (float("nan"), 0.1), (0.1, float("inf")), (0.1, -0.5)):
        with pytest.raises(so.SearchOptionError, match="expected a finite value >= 0"):
            so.check_moves_left(*bad)
    assert "opt --moves-left" in so.MOVES_LEFT_REFUSAL
    assert len(so.EXCLUDES) == 11 and len(so.SCRIPT_EXCLUDES) == 4          # the tables this one stands beside are untouched


def test_manager_flags():
    from cchess_alphazero import manager
    p = manager.create_parser()
    cfg = manager.build_config(p.parse_args(["self"]))
    assert (cfg.engine.moves_left_slope, cfg.engine.moves_left_cap) == (0.0, 0.0345)
    cfg = manager.build_config(p.parse_args(["eval", "--moves-left-slope", "0.0027", "--moves-left-cap", "0.05"]))
    assert (cfg.engine.moves_left_slope, cfg.engine.moves_left_cap) == (0.0027, 0.05)
    cfg = manager.build_config(p.parse_args(["self", "--moves-left-slope", "0.0027", "--fast-sims", "8", "--leaf-mirror", "0.5"]))
    assert cfg.engine.moves_left_slope == 0.0027
    for argv, msg in ((["self", "--moves-left-slope", "-1"], "expected a finite value >= 0"),
                      (["self", "--moves-left-slope", "nan"], "expected a finite value >= 0"),
                      (["self", "--moves-left-slope", "0.01", "--moves-left-cap", "inf"], "expected a finite value >= 0"),
                      (["opt", "--moves-left-slope", "0.01"], "is an option of `run.py self` and `run.py eval`"),
                      (["reanalyse", "--moves-left-slope", "0.01"], "--moves-left-slope excludes a script"),
                      (["self", "--moves-left-slope", "0.01", "--solver"], "--moves-left-slope excludes --solver"),
                      (["self", "--moves-left-slope", "0.01", "--kld-gain", "1e-4"], "--moves-left-slope excludes --kld-gain"),
                      (["self", "--moves-left-slope", "0.01", "--eval-cache", "12"], "--moves-left-slope excludes --eval-cache"),
                      (["self", "--moves-left-slope", "0.01", "--record-visits", "--gumbel", "8"],
                       "--moves-left-slope excludes --gumbel"),
                      (["eval", "--moves-left-slope", "0.01", "--smart-pruning"], "--moves-left-slope excludes --smart-pruning")):
        with pytest.raises(SystemExit) as e:
            manager.build_config(p.parse_args(argv))
        assert msg in str(e.value), (argv, str(e.value))
    manager.build_config(p.parse_args(["self", "--solver"]))               # switched off it refuses nothing


def test_uci_option_lines():
    from cchess_alphazero import manager, uci
    assert "option name MovesLeftSlope type string default 0" in uci.ENGINE_ID
    assert "option name MovesLeftCap type string default 0.0345" in uci.ENGINE_ID
    out = io.StringIO()
    u = uci.UCI(manager.build_config(manager.create_parser().parse_args(["self"])), out=out)
    u.handle("setoption name MovesLeftSlope value 0.0027")
    u.handle("setoption name MovesLeftCap value 0.05")
    assert (u.config.engine.moves_left_slope, u.config.engine.moves_left_cap) == (0.0027, 0.05)
    u.handle("setoption name MovesLeftSlope value minus")
    assert u.config.engine.moves_left_slope == 0.0027 and "info string MovesLeftSlope minus" in out.getvalue()


# ---- (c) the inputs show the utility ------------------------------------------------------------------------------------------
def test_the_cases_show_the_utility():
    differ = moved = 0
    for case in sm.cases():
        base, _ = sm.run_case(case, 0.0)
        rows, _ = mo.run_case(case, TEST_SLOPE, TEST_CAP)
        differ += any(not np.array_equal(a["stats"]["n"], b["stats"]["n"]) for a, b in zip(base, rows))
        moved += any(a["best"] != b["best"] for a, b in zip(base, rows))
    assert differ >= 6 and moved >= 1, (differ, moved)


# ---- (d) the property: shorter wins, longer losses -------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf_value", [-1e-3, 1e-3])
def test_visits_are_monotone_in_m(leaf_value):
    """Uniform policy and a constant, tiny value: every root move has the same prior, and q stays within 2e-3 of 0 while one
    more visit costs an edge a third of its exploration term (0.04 here), so the edges are visited once each before any is
    visited twice, and which ones get the second visit is decided by u_m alone.  After one visit an edge's mean is its child's
    own m, (k + 16) / 16 plies; Mp is common to all edges and nothing is clamped (slope 0.001, cap 1).  With the leaves worth
    -1e-3 to their movers the root is winning (q > 0) and the second visits go to the children with the smallest k; with +1e-3
    it is losing and they go to the largest.  Ties in k aside, the visit counts are monotone against k."""
    salt = 3
    nm = len(xo.get_legal_moves(xo.INIT_STATE))
    extra = nm // 2
    net = lambda planes: sml.ml_stub_numpy(planes, salt, ("flat", leaf_value))
    s = mo.Search(sm.play_cfg(1 + nm + extra), salt, slope=0.001, cap=1.0, net=net)
    s.search(xo.INIT_STATE)
    root = s.tree[xo.INIT_STATE]
    k = np.array([s.tree[xo.step(xo.INIT_STATE, mv)].k for mv in root.moves])
    n = np.array(root.n)
    assert sorted(set(n.tolist())) == [1, 2] and int((n == 2).sum()) == extra and len(set(k.tolist())) > nm // 2
    pairs = [(i, j) for i in range(nm) for j in range(nm) if k[i] < k[j]]
    if leaf_value < 0:      # the root is winning: the shorter game gets the visits
        assert all(n[i] >= n[j] for i, j in pairs), (k, n)
    else:                   # the root is losing: the longer one does
        assert all(n[i] <= n[j] for i, j in pairs), (k, n)
    # and without the utility the second visits are the plain rule's: the last edges in order
    p = mo.Search(sm.play_cfg(1 + nm + extra), salt, on=False, net=net)
    p.search(xo.INIT_STATE)
    assert not np.array_equal(np.array(p.tree[xo.INIT_STATE].n), n)
