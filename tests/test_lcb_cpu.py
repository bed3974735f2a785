"""The lower-confidence-bound move choice without a device: tests/lcb_oracle.py against search_model.Search, the rule on a
hand-made grid, and the Python front ends (search_options, manager, uci).

The conditions on the shared inputs below are conditions, not measurements: the nine cases at 200 simulations must be
positions where the rule matters, or the GPU tests that compare moves would compare nothing."""
import io

import numpy as np
import pytest

import lcb_oracle as lo
import search_model as sm

# the cases of sm.cases() whose LCB move (the first search of the case) is not the most visited move, at 200 simulations, K = 1,
# R = 0.15; worked out with the oracle below and pinned here so that tests/test_gpu_lcb.py can name them
DIFFER_Z2 = ("pos100", "pos850", "pos625")
DIFFER_Z5 = ("pos850",)

_RUNS = {}


def runs(z, sims=sm.SIMS):
    """{case name: rows} of lo.run_case over sm.cases(), computed once per (z, sims)."""
    if (z, sims) not in _RUNS:
        _RUNS[(z, sims)] = {c["name"]: lo.run_case(c, z=z, sims=sims)[0] for c in sm.cases()}
    return _RUNS[(z, sims)]


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def test_off_is_the_plain_search_bit_for_bit():
    for case in sm.cases()[:4]:                             # init, a plain position, the ban, the reuse
        plain, ps = sm.run_case(case, 0.0, 64)
        off, s = lo.run_case(case, z=0.0, sims=64)
        assert len(plain) == len(off)
        for a, b in zip(plain, off):
            assert a["best"] == b["best"] == b["most"]
            for key in ("moves", "n", "p"):
                assert np.array_equal(a["stats"][key], b["stats"][key]), (case["name"], key)
            assert np.array_equal(_bits(a["stats"]["w"]), _bits(b["stats"]["w"])), case["name"]
            assert not b["values"]["s2"].any() and not b["values"]["vn"].any()        # off: no record is kept
        assert (ps.sims, ps.expansions, ps.terminal_sims, ps.repetition_sims) == \
               (s.sims, s.expansions, s.terminal_sims, s.repetition_sims)


def test_on_keeps_n_w_p_and_the_records_are_consistent():
    on = runs(lo.Z)
    for case in sm.cases():
        plain, _ = sm.run_case(case, 0.0)
        rows = on[case["name"]]
        assert len(plain) == len(rows)
        for i, (a, b) in enumerate(zip(plain, rows)):
            if i == 0:                                      # (a reuse case's second search starts from the move played)
                assert a["state"] == b["state"]
            if a["state"] != b["state"]:
                continue
            for key in ("moves", "n", "p"):
                assert np.array_equal(a["stats"][key], b["stats"][key]), (case["name"], key)
            assert np.array_equal(_bits(a["stats"]["w"]), _bits(b["stats"]["w"])), case["name"]
            assert b["most"] == a["best"]
        for i, b in enumerate(rows):
            st, vr = b["stats"], b["values"]
            assert np.array_equal(vr["vn"], st["n"])        # nothing in flight: every visit is a completed backup
            assert (vr["s2"] >= 0).all() and (vr["s2"] <= 4.0 * vr["vn"]).all()
            assert (vr["s2"] * vr["vn"] >= st["w"] * st["w"] * (1 - 1e-12)).all()     # Cauchy-Schwarz
            # the root's vn add up to the simulations that ended below it (a reused root carries the earlier search's too)
            assert int(vr["vn"].sum()) == b["below"] if i == 0 else int(vr["vn"].sum()) >= b["below"]


def test_the_rule_matters_on_the_shared_cases():
    """At z = 2 the LCB move differs from the most visited move on at least three of the nine cases, at z = 5 on at least one
    and on fewer: the inputs exercise the rule and z is read.  The names are pinned for the GPU tests."""
    d2 = tuple(name for name, rows in runs(2.0).items() if rows[0]["best"] != rows[0]["most"])
    d5 = tuple(name for name, rows in runs(5.0).items() if rows[0]["best"] != rows[0]["most"])
    print(f"\nLCB move != most visited move: z = 2 on {d2}, z = 5 on {d5}")
    assert len(d2) >= 3 and 1 <= len(d5) < len(d2)
    assert d2 == DIFFER_Z2 and d5 == DIFFER_Z5
    for name in d2:                                         # the played move has fewer visits and the better bound
        r = runs(2.0)[name][0]
        lab = [sm.xo.label_str(int(l)) for l in r["stats"]["moves"]]
        jb, jm = lab.index(r["best"]), lab.index(r["most"])
        assert r["stats"]["n"][jb] < r["stats"]["n"][jm] and r["lcb"][jb] > r["lcb"][jm]
        assert r["pick"] == jb


def test_the_grid():
    rows = lo.grid()
    assert len(rows) == 12
    for row in rows:
        e = row["edges"]
        lcb, pick = lo.lcb_pick([x[0] for x in e], [x[1] for x in e], [x[2] for x in e], [x[3] for x in e],
                                [x[4] for x in e], row["z"], row["ratio"])
        assert pick == row["expect"], (row["name"], pick, lcb)
        assert len(lcb) == len(e)
        for j, x in enumerate(e):                           # NaN exactly where the edge is not eligible
            open_ = not (x[0] & lo.BANNED)
            n_max = max([y[1] for y in e if not (y[0] & lo.BANNED)], default=0)
            elig = open_ and x[4] >= 2 and x[1] > 0 and float(x[1]) >= row["ratio"] * float(n_max)
            assert np.isnan(lcb[j]) != elig, (row["name"], j)
    by = {r["name"]: r for r in rows}
    # the clamp row: the raw variance of at least one edge is negative by rounding
    raw = [s2 / vn - (w / n) * (w / n) for _, n, w, s2, vn in by["all samples equal: the clamp"]["edges"]]
    assert raw[0] < 0.0 < raw[1], raw
    # the boundary row: n = R * n_max exactly
    r = by["n == R * n_max exactly"]
    assert float(r["edges"][1][1]) == r["ratio"] * float(r["edges"][0][1])
    # the tie rows: the bounds are equal bit for bit
    e = by["equal lcb: the greater n"]["edges"]
    lcb, _ = lo.lcb_pick(*[[x[i] for x in e] for i in range(5)], 2.0, 0.15)
    assert lcb[0] == lcb[1] and e[0][1] != e[1][1]
    # a terminal edge: x = +-2, x * x = 4
    assert by["a terminal edge"]["edges"][0][3] == 12.0


def test_a_played_line_reuses_its_tree():
    line, s = lo.play_line(sm.xo.INIT_STATE, 3, 120, 21)
    assert [r["ran"] for r in line][0] == 120 and all(r["ran"] < 120 for r in line[1:])
    for r in line:
        assert np.array_equal(r["values"]["vn"], r["stats"]["n"])


def test_check_lcb_and_the_exclusions():
    from cchess_alphazero import search_options as so
    assert so.LCB_DEFAULTS == dict(lcb=0.0, lcb_min_visits=0.15)
    assert so.check_lcb(0.0, 0.15) is False and so.check_lcb(2.0, 0.0) is True and so.check_lcb(1e-9, 1.0) is True
    for z in (-0.1, float("nan"), float("inf")):
        with pytest.raises(so.SearchOptionError, match="lcb .*: expected a finite value >= 0"):
            so.check_lcb(z, 0.15)
    for r in (-0.01, 1.01, float("nan")):
        with pytest.raises(so.SearchOptionError, match=r"lcb_min_visits .*: expected a value in \[0, 1\]"):
            so.check_lcb(2.0, r)
    with pytest.raises(so.SearchOptionError, match="^--lcb -1"):
        so.check_lcb(-1.0, 0.15, flags=True)
    with pytest.raises(so.SearchOptionError, match="^--lcb-min-visits 2"):
        so.check_lcb(1.0, 2.0, flags=True)
    assert [k for k, _ in so.LCB_EXCLUDES] == ["gumbel", "solver", "kld_gain", "smart_pruning", "eval_cache"]
    on = dict(gumbel=dict(gumbel=8, record_visits=True), solver=dict(solver=True), kld_gain=dict(kld_gain=1e-4),
              smart_pruning=dict(smart_pruning=True), eval_cache=dict(eval_cache=10))
    for key, why in so.LCB_EXCLUDES:
        so.check(on[key])                                   # fine without the option
        so.check(on[key], lcb=False)
        with pytest.raises(so.SearchOptionError) as e:
            so.check(on[key], lcb=True)
        assert str(e.value) == f"lcb excludes {key}: {why}"
        with pytest.raises(so.SearchOptionError) as e:
            so.check(on[key], flags=True, lcb=True)
        assert str(e.value) == f"--lcb excludes {so.VALUES[key].flag}: {why}"
    with pytest.raises(so.SearchOptionError) as e:
        so.check(dict(record_visits=True), script=True, lcb=True)
    assert str(e.value) == f"lcb excludes a script: {so.LCB_SCRIPT}"
    with pytest.raises(so.SearchOptionError) as e:
        so.check({}, moves_left=True, lcb=True)
    assert str(e.value) == f"lcb excludes moves_left_slope: {so.LCB_MOVES_LEFT}"
    with pytest.raises(so.SearchOptionError) as e:
        so.check({}, draw=True, lcb=True)
    assert str(e.value) == f"lcb excludes draw_score: {so.LCB_DRAW}"
    # the order: the table, a script, the moves-left utility, the draw average, then this option
    with pytest.raises(so.SearchOptionError, match="^draw_score excludes solver"):
        so.check(dict(solver=True), draw=True, lcb=True)
    with pytest.raises(so.SearchOptionError, match="^lcb excludes gumbel"):
        so.check(dict(gumbel=8, record_visits=True, eval_cache=10), lcb=True)
    # what it composes with
    so.check(dict(fast_sims=8, forced_playouts=2.0, record_visits=True, record_q=True, record_surprise=True, leaf_mirror=0.5),
             sims=16, lcb=True)
    so.check({}, history=True, lcb=True)
    assert "{lcb" in so.LCB_LOG and "2" in so.LCB_LOG.format(lcb=2.0, lcb_min_visits=0.15)
    # the table itself is what it was
    assert len(so.OPTIONS) == 12 and len(so.EXCLUDES) == 11


def test_manager_flags():
    from cchess_alphazero import manager
    p = manager.create_parser()
    cfg = manager.build_config(p.parse_args(["self"]))
    assert (cfg.engine.lcb, cfg.engine.lcb_min_visits) == (0.0, 0.15)
    cfg = manager.build_config(p.parse_args(["eval", "--lcb", "2"]))
    assert (cfg.engine.lcb, cfg.engine.lcb_min_visits) == (2.0, 0.15)
    cfg = manager.build_config(p.parse_args(["self", "--lcb", "1.5", "--lcb-min-visits", "0.3", "--fast-sims", "8",
                                             "--leaf-mirror", "0.5", "--record-visits", "--forced-playouts", "2"]))
    assert (cfg.engine.lcb, cfg.engine.lcb_min_visits) == (1.5, 0.3)
    for argv, msg in ((["self", "--lcb", "-1"], "--lcb -1.0: expected a finite value >= 0"),
                      (["self", "--lcb", "nan"], "expected a finite value >= 0"),
                      (["self", "--lcb", "2", "--lcb-min-visits", "1.5"], "--lcb-min-visits 1.5: expected a value in [0, 1]"),
                      (["opt", "--lcb", "2"], "--lcb is an option of `run.py self` and `run.py eval`"),
                      (["opt", "--lcb-min-visits", "0.3"], "--lcb-min-visits is an option of `run.py self` and `run.py eval`"),
                      (["reanalyse", "--lcb", "2"], "--lcb excludes a script"),
                      (["reanalyse", "--lcb-min-visits", "0.3"], "--lcb-min-visits is an option of"),
                      (["self", "--lcb", "2", "--solver"], "--lcb excludes --solver"),
                      (["self", "--lcb", "2", "--kld-gain", "1e-4"], "--lcb excludes --kld-gain"),
                      (["eval", "--lcb", "2", "--smart-pruning"], "--lcb excludes --smart-pruning"),
                      (["self", "--lcb", "2", "--eval-cache", "10"], "--lcb excludes --eval-cache"),
                      (["self", "--lcb", "2", "--gumbel", "8", "--record-visits"], "--lcb excludes --gumbel"),
                      (["self", "--lcb", "2", "--moves-left-slope", "0.01"], "--lcb excludes --moves-left-slope"),
                      (["self", "--lcb", "2", "--draw-score", "0.5"], "--lcb excludes --draw-score")):
        with pytest.raises(SystemExit) as e:
            manager.build_config(p.parse_args(argv))
        assert msg in str(e.value), (argv, str(e.value))
    manager.build_config(p.parse_args(["self", "--solver"]))               # switched off it refuses nothing
    text = p.format_help()
    assert "--lcb Z" in text and "--lcb-min-visits R" in text


def test_uci_option_lines():
    from cchess_alphazero import manager, uci
    assert "option name LCB type string default 0" in uci.ENGINE_ID
    assert "option name LCBMinVisits type string default 0.15" in uci.ENGINE_ID
    out = io.StringIO()
    u = uci.UCI(manager.build_config(manager.create_parser().parse_args(["self"])), out=out)
    u.handle("setoption name LCB value 2")
    u.handle("setoption name LCBMinVisits value 0.25")
    assert (u.config.engine.lcb, u.config.engine.lcb_min_visits) == (2.0, 0.25)
    for line, msg in (("setoption name LCB value -1", "info string LCB -1: expected a finite value >= 0"),
                      ("setoption name LCB value two", "info string LCB two: expected a finite value >= 0"),
                      ("setoption name LCB value inf", "info string LCB inf: expected a finite value >= 0"),
                      ("setoption name LCBMinVisits value 1.5", "info string LCBMinVisits 1.5: expected a value in [0, 1]"),
                      ("setoption name LCBMinVisits value nan", "info string LCBMinVisits nan: expected a value in [0, 1]")):
        u.handle(line)
        assert msg in out.getvalue(), line
        assert (u.config.engine.lcb, u.config.engine.lcb_min_visits) == (2.0, 0.25)       # the option stays as it was
