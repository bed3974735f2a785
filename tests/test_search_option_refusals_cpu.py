"""The command line and search_options.check() against a recording made before the side options (moves-left utility, draw
average, lower-confidence-bound move choice, c_puct schedule, policy temperature) got their table, search_options.SIDE: every
option group alone and every pair of groups, for run.py self / eval / reanalyse / opt, answers what it answered then, byte for
byte (tests/golden/make_golden_search_option_refusals.py has the enumeration and wrote the recording).  And the side table's
defaults are the five *_DEFAULTS, through resolve_side() and in every configuration."""
import os
import sys
import types

from cchess_alphazero import search_options as so
from cchess_alphazero.config import Config
from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import make_golden_search_option_refusals as gen  # noqa: E402

SIDE_DEFAULTS = {**so.MOVES_LEFT_DEFAULTS, **so.DRAW_DEFAULTS, **so.LCB_DEFAULTS, **so.CPUCT_DEFAULTS, **so.POLICY_TEMP_DEFAULTS}
ON_FLAGS = ("moves_left", "draw", "lcb_on", "cpuct_on", "policy_temp_on")


def test_every_group_and_pair_answers_what_it_answered_before_the_side_table():
    want = load_golden("search_option_refusals.json")
    n = len(gen.GROUPS)
    assert n == 19 and os.path.getsize(os.path.join(GOLDEN, "search_option_refusals.json")) < 1 << 20
    got = gen.record()
    assert set(got) == set(want) == {"build_config", "check"}
    assert set(got["build_config"]) == set(want["build_config"]) == set(gen.COMMANDS)
    for cmd in gen.COMMANDS:
        assert len(want["build_config"][cmd]) == n + n * (n - 1) // 2
        for case, answer in want["build_config"][cmd].items():
            assert got["build_config"][cmd][case] == answer, (cmd, case)
        assert got["build_config"][cmd] == want["build_config"][cmd]
    assert len(want["check"]) == n + n * (n - 1) // 2
    for case, answers in want["check"].items():
        assert got["check"][case] == answers, case
    assert got == want
    # the recording is not vacuous: every command refuses something and accepts something, check() under every spelling too
    for cmd in gen.COMMANDS:
        answers = list(want["build_config"][cmd].values())
        assert 0 < sum(a == "ok" for a in answers) < len(answers)
    for spelling in ("key", "flag", "key+script", "flag+script"):
        answers = [a[spelling] for a in want["check"].values()]
        assert 0 < sum(a == "ok" for a in answers) < len(answers)


def test_the_side_tables_defaults_are_the_five_defaults_and_the_configurations():
    assert len(SIDE_DEFAULTS) == 9
    side = so.resolve_side(types.SimpleNamespace())
    values = {k: v for k, v in side.items() if k not in ON_FLAGS}
    assert values == SIDE_DEFAULTS and all(type(values[k]) is type(v) for k, v in SIDE_DEFAULTS.items())
    assert list(values) == list(SIDE_DEFAULTS)                             # (in the order the options were added)
    assert {k: side[k] for k in ON_FLAGS} == dict.fromkeys(ON_FLAGS, False) and len(side) == 9 + 5
    assert [r.on for r in so.SIDE] == list(ON_FLAGS)
    assert {k: d for r in so.SIDE for k, d in r.values.items()} == SIDE_DEFAULTS
    for kind in ("mini", "normal", "distribute"):
        engine = Config(kind).engine
        for k, v in SIDE_DEFAULTS.items():
            assert getattr(engine, k) == v and type(getattr(engine, k)) is type(v), (kind, k)
        assert so.resolve_side(Config(kind)) == side
    # an override wins over the configuration's value, which wins over the default; each in the default's type
    cfg = Config("mini")
    cfg.engine.lcb, cfg.engine.cpuct_base = 2, 1000
    side = so.resolve_side(cfg, draw_score=None, show_wdl=1, cpuct_base=500)
    assert (side["lcb"], side["lcb_on"], side["show_wdl"], side["draw"], side["cpuct_base"]) == (2.0, True, True, True, 500.0)
    assert type(side["lcb"]) is float and side["show_wdl"] is True and not side["cpuct_on"]
