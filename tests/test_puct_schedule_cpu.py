"""The c_puct schedule and the policy temperature on the CPU: the Python model of tests/puct_schedule_oracle.py against
search_model.Search, the option checks of search_options.py and the command line's flags.  No device."""
import math

import numpy as np
import pytest

import puct_schedule_oracle as po
import search_model as sm
import solver_oracle as so


def _key(rows):
    return [tuple(r["stats"][k].tobytes() for k in ("n", "w", "p")) + (r["stats"]["sum_n"], r["best"]) for r in rows]


def _dn(a, b):
    return sum(int(np.abs(x["stats"]["n"] - y["stats"]["n"]).sum()) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def plain_runs():
    """search_model.Search on the ten cases, computed once."""
    return [(c, sm.run_case(c, 0.0)[0]) for c in po.cases()]


def test_off_is_the_plain_search_bit_for_bit(plain_runs):
    for c, plain in plain_runs[:9]:
        got, _ = po.run_case(c, 0.0, 19652.0, 1.0)
        assert _key(got) == _key(plain), c["name"]


def test_the_schedule_moves_the_counts_of_these_cases(plain_runs):
    """A condition on the inputs, not a measurement: F = 2, B = 50 at 200 simulations has to matter."""
    moved = []
    for c, plain in plain_runs:
        got, _ = po.run_case(c)
        moved.append(_dn(got, plain))
    print("sum |dn| per case under F = 2, B = 50:", moved)
    assert sum(d > 0 for d in moved[:9]) >= 7
    assert moved[9] > 0                                     # the tenth case: the wide position under its second salt
    wide, _ = po.run_case(po.cases()[9])
    n = wide[0]["stats"]["n"]
    assert len(n) > 64 and (n[64:] > 0).any()               # the second half of the edges is visited under the schedule


def test_the_temperature_moves_the_counts_of_these_cases(plain_runs):
    moved = [_dn(po.run_case(c, 0.0, 19652.0, 2.0)[0], plain) for c, plain in plain_runs[:9]]
    print("sum |dn| per case under T = 2:", moved)
    assert all(d > 0 for d in moved)


def test_cpuct_values():
    assert po.cpuct(1.5, 0.0, 19652.0, 10 ** 6) == 1.5
    assert po.cpuct(1.5, 2.0, 50.0, 0) == 1.5 + 2.0 * math.log(51.0 / 50.0)
    # AlphaZero's constants: 1.25 at the start, + 1 near N = 33 000
    assert abs(po.cpuct(1.25, 1.0, 19652.0, 33767) - 2.25) < 1e-3
    assert all(po.cpuct(1.5, 2.0, 50.0, n + 1) > po.cpuct(1.5, 2.0, 50.0, n) for n in (0, 1, 63, 199, 10 ** 6))


def test_the_solver_model_composes_with_the_schedule():
    c = sm.cases()[1]
    plain, _ = po.run_case(c)
    off, _ = po.run_case(c, solver=False)
    assert _key(off) == _key(plain)
    s = po.SolverSearch(sm.play_cfg(), c["salt"], 0.0, 19652.0, 1.0, True)
    t = so.Search(sm.play_cfg(), c["salt"])
    s.search(c["state"])
    t.search(c["state"])
    assert s.node_stats(c["state"])["n"].tolist() == t.node_stats(c["state"])["n"].tolist()


def test_check_cpuct_and_check_policy_temp():
    from cchess_alphazero import search_options as opt
    assert opt.CPUCT_DEFAULTS == dict(cpuct_factor=0.0, cpuct_base=19652.0)
    assert opt.POLICY_TEMP_DEFAULTS == dict(policy_temp=1.0)
    assert opt.check_cpuct(0.0, 19652.0) is False and opt.check_cpuct(3.894, 38739.0) is True
    assert opt.check_cpuct(2, 1) is True
    nan, inf = float("nan"), float("inf")
    inf_ = inf
    for bad in (-1.0, nan, inf, -inf_, "2", None):
        with pytest.raises(opt.SearchOptionError, match=r"^cpuct_factor .*: expected a finite value >= 0$"):
            opt.check_cpuct(bad, 50.0)
        with pytest.raises(opt.SearchOptionError, match=r"^--cpuct-factor .*: expected a finite value >= 0$"):
            opt.check_cpuct(bad, 50.0, flags=True)
    for bad in (0.0, 0.99, -5.0, nan, inf, "50"):
        with pytest.raises(opt.SearchOptionError, match=r"^cpuct_base .*: expected a finite value >= 1$"):
            opt.check_cpuct(2.0, bad)
        with pytest.raises(opt.SearchOptionError, match=r"^--cpuct-base .*: expected a finite value >= 1$"):
            opt.check_cpuct(2.0, bad, flags=True)
    assert opt.check_policy_temp(1.0) is False and opt.check_policy_temp(1) is False
    assert opt.check_policy_temp(1.4) is True and opt.check_policy_temp(0.1) is True and opt.check_policy_temp(10.0) is True
    for bad in (0.0, 0.0999, 10.001, -1.0, nan, inf, "1.4", None):
        with pytest.raises(opt.SearchOptionError, match=r"^policy_temp .*: expected a value in \[0\.1, 10\]$"):
            opt.check_policy_temp(bad)
        with pytest.raises(opt.SearchOptionError, match=r"^--policy-temp .*: expected a value in \[0\.1, 10\]$"):
            opt.check_policy_temp(bad, flags=True)
    assert "2.5" in opt.CPUCT_LOG.format(cpuct_factor=2.5, cpuct_base=50.0)
    assert "1.4" in opt.POLICY_TEMP_LOG.format(policy_temp=1.4)
    # beside the table: the table and its defaults are what they were
    assert not {"cpuct_factor", "cpuct_base", "policy_temp"} & set(opt.DEFAULTS)


def test_manager_flags(tmp_path, monkeypatch):
    from cchess_alphazero import manager
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    parse = manager.create_parser().parse_args
    flags = ["--cpuct-factor", "3.894", "--cpuct-base", "38739", "--policy-temp", "1.4"]
    for cmd in ("self", "eval", "reanalyse"):
        cfg = manager.build_config(parse([cmd, "--type", "mini"] + flags))
        assert (cfg.engine.cpuct_factor, cfg.engine.cpuct_base, cfg.engine.policy_temp) == (3.894, 38739.0, 1.4)
    cfg = manager.build_config(parse(["self", "--type", "mini"]))
    assert (cfg.engine.cpuct_factor, cfg.engine.cpuct_base, cfg.engine.policy_temp) == (0.0, 19652.0, 1.0)
    for one, name in ((["--cpuct-factor", "2"], "--cpuct-factor"), (["--cpuct-base", "50"], "--cpuct-base"),
                      (["--policy-temp", "1.4"], "--policy-temp")):
        with pytest.raises(SystemExit, match=f"^{name} is an option of `run.py self`, `run.py eval` and `run.py reanalyse`$"):
            manager.build_config(parse(["opt", "--type", "mini"] + one))
    manager.build_config(parse(["opt", "--type", "mini"]))      # the defaults are no use of the options
    for bad, msg in ((["--cpuct-factor", "-1"], "--cpuct-factor -1.0: expected a finite value >= 0"),
                     (["--cpuct-factor", "nan"], "--cpuct-factor nan: expected a finite value >= 0"),
                     (["--cpuct-base", "0.5"], "--cpuct-base 0.5: expected a finite value >= 1"),
                     (["--policy-temp", "0"], r"--policy-temp 0.0: expected a value in \[0.1, 10\]"),
                     (["--policy-temp", "11"], r"--policy-temp 11.0: expected a value in \[0.1, 10\]")):
        with pytest.raises(SystemExit, match=msg):
            manager.build_config(parse(["self", "--type", "mini"] + bad))
    # beside every other option: nothing excludes them
    for other in (["--solver"], ["--record-visits", "--gumbel", "16"], ["--eval-cache", "12"], ["--kld-gain", "1e-4"],
                  ["--lcb", "2"], ["--record-visits", "--forced-playouts", "2"]):
        manager.build_config(parse(["self", "--type", "mini"] + flags + other))


def test_uci_options():
    import io
    import types
    from cchess_alphazero import uci
    for line in ("option name CPuctFactor type string default 0", "option name CPuctBase type string default 19652",
                 "option name PolicyTemperature type string default 1"):
        assert line in uci.ENGINE_ID
    cfg = types.SimpleNamespace(engine=types.SimpleNamespace(cpuct_factor=0.0, cpuct_base=19652.0, policy_temp=1.0),
                                opts=types.SimpleNamespace(), play=types.SimpleNamespace())
    out = io.StringIO()
    u = uci.UCI(cfg, out=out)
    u.handle("setoption name CPuctFactor value 3.894")
    u.handle("setoption name CPuctBase value 38739")
    u.handle("setoption name PolicyTemperature value 1.4")
    assert (cfg.engine.cpuct_factor, cfg.engine.cpuct_base, cfg.engine.policy_temp) == (3.894, 38739.0, 1.4)
    assert out.getvalue() == ""
    for line, msg in (("setoption name CPuctFactor value -1", "info string CPuctFactor -1: expected a finite value >= 0"),
                      ("setoption name CPuctFactor value inf", "info string CPuctFactor inf: expected a finite value >= 0"),
                      ("setoption name CPuctBase value 0", "info string CPuctBase 0: expected a finite value >= 1"),
                      ("setoption name CPuctBase value nan", "info string CPuctBase nan: expected a finite value >= 1"),
                      ("setoption name PolicyTemperature value 0.05",
                       "info string PolicyTemperature 0.05: expected a value in [0.1, 10]"),
                      ("setoption name PolicyTemperature value hot",
                       "info string PolicyTemperature hot: expected a value in [0.1, 10]")):
        out.seek(0)
        out.truncate()
        u.handle(line)
        assert out.getvalue().strip() == msg
    assert (cfg.engine.cpuct_factor, cfg.engine.cpuct_base, cfg.engine.policy_temp) == (3.894, 38739.0, 1.4)
