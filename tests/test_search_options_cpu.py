"""The search options' table (cchess_alphazero/search_options.py) against the layers that use it, without a device: every
pair of the seven features that take part in exclusions is refused iff the table lists it, by check() under both spellings
and by the command line; every option alone reaches config.engine; the defaults are the configuration's; the engine
refuses before it asks for a device.  The library's half of the matrix is tests/test_gpu_search_options.py."""
import itertools
import types

import pytest

from cchess_alphazero import manager, search_options as so
from cchess_alphazero.config import Config

# one legal "on" setting per feature of the exclusion matrix: config.engine values, command-line words
FEATURES = {
    "fast_sims": (dict(fast_sims=8), ["--fast-sims", "8"]),
    "forced_playouts": (dict(forced_playouts=2.0, record_visits=True), ["--forced-playouts", "2", "--record-visits"]),
    "gumbel": (dict(gumbel=8, record_visits=True), ["--gumbel", "8", "--record-visits"]),
    "eval_cache": (dict(eval_cache=10), ["--eval-cache", "10"]),
    "solver": (dict(solver=True), ["--solver"]),
    "kld_gain": (dict(kld_gain=1e-3), ["--kld-gain", "1e-3"]),
    "smart_pruning": (dict(smart_pruning=True), ["--smart-pruning"]),
}
# every other option alone at a legal value that is not its default
SINGLES = dict(FEATURES, record_visits=(dict(record_visits=True), ["--record-visits"]),
               full_rate=(dict(fast_sims=8, full_rate=0.5), ["--fast-sims", "8", "--full-rate", "0.5"]),
               record_q=(dict(record_q=True, record_visits=True), ["--record-q", "--record-visits"]),
               record_surprise=(dict(record_surprise=True, record_visits=True), ["--record-surprise", "--record-visits"]),
               leaf_mirror=(dict(leaf_mirror=0.5), ["--leaf-mirror", "0.5"]),
               gumbel_visit_scale=(dict(gumbel=16, gumbel_visit=20.0, gumbel_scale=0.5, record_visits=True),
                                   ["--gumbel", "16", "--gumbel-visit", "20", "--gumbel-scale", "0.5", "--record-visits"]),
               gumbel_full=(dict(gumbel=16, gumbel_full=True, record_visits=True),
                            ["--gumbel", "16", "--gumbel-full", "--record-visits"]),
               kld_interval=(dict(kld_gain=1e-3, kld_interval=50), ["--kld-gain", "1e-3", "--kld-interval", "50"]))
PAIRS = {frozenset(p[:2]) for p in so.EXCLUDES}


def _config(cmd, words):
    return manager.build_config(manager.create_parser().parse_args([cmd] + words))


def _commands(*keys):
    """The run.py commands that accept all of these options."""
    by_key = {o.values[0].key: o.commands for o in so.OPTIONS}
    return [c for c in ("self", "eval") if all(by_key[k] is None or c in by_key[k] for k in keys)]


def test_the_matrix_is_the_issues_eleven_pairs():
    assert len(so.EXCLUDES) == len(PAIRS) == 11 and all(len(p) == 2 and p <= set(FEATURES) for p in PAIRS)
    order = [o.values[0].key for o in so.OPTIONS]
    assert all(order.index(later) > order.index(earlier) for later, earlier, _ in so.EXCLUDES)
    excluded_by = {k: {next(iter(p - {k})) for p in PAIRS if k in p} for k in FEATURES}
    assert excluded_by["gumbel"] == {"fast_sims", "forced_playouts", "solver", "kld_gain", "smart_pruning"}
    assert excluded_by["solver"] == {"gumbel", "forced_playouts", "eval_cache", "kld_gain", "smart_pruning"}
    assert excluded_by["eval_cache"] == {"solver", "kld_gain", "smart_pruning"}
    assert {w for _, _, w in so.EXCLUDES} == {"each defines its own root rule", "the cache has a kernel instantiation of its own"}


@pytest.mark.parametrize("a, b", list(itertools.combinations(FEATURES, 2)))
def test_a_pair_is_refused_iff_the_table_lists_it(a, b):
    values = {**FEATURES[a][0], **FEATURES[b][0]}
    words = FEATURES[a][1] + [w for w in FEATURES[b][1] if w != "--record-visits" or w not in FEATURES[a][1]]
    cmds = _commands(a, b)
    if frozenset((a, b)) not in PAIRS:
        so.check(values)
        so.check(values, flags=True)
        for cmd in cmds:
            engine = _config(cmd, words).engine
            assert all(getattr(engine, k) == v for k, v in values.items())
        return
    for flags in (False, True):
        with pytest.raises(so.SearchOptionError) as e:
            so.check(values, flags=flags)
        first, _, rest = str(e.value).partition(" excludes ")
        named = {first, rest.split(":")[0]}
        assert named == {so.VALUES[k].flag if flags else k for k in (a, b)}, str(e.value)
        assert isinstance(e.value, ValueError)
    for cmd in cmds:
        with pytest.raises(SystemExit) as x:
            _config(cmd, words)
        assert str(x.value) == str(e.value)                 # (the command line says what check() says, in flags)


@pytest.mark.parametrize("name", list(SINGLES))
def test_every_option_alone_is_accepted_and_reaches_the_engine_section(name):
    values, words = SINGLES[name]
    assert any(values[k] != so.DEFAULTS[k] for k in values)
    so.check(values)
    cmds = _commands(*[o.values[0].key for o in so.OPTIONS if any(v.key in values for v in o.values)])
    assert cmds
    for cmd in cmds:
        engine = _config(cmd, words).engine
        assert all(getattr(engine, k) == v and type(getattr(engine, k)) is type(v) for k, v in values.items())
        rest = set(so.DEFAULTS) - set(values)
        assert all(getattr(engine, k) == so.DEFAULTS[k] for k in rest)


def test_the_tables_defaults_are_the_configurations():
    assert len(so.DEFAULTS) == 16
    assert so.DEFAULTS == dict(record_visits=False, fast_sims=0, full_rate=0.25, forced_playouts=0.0, record_q=False,
                               record_surprise=False, leaf_mirror=0.0, gumbel=0, gumbel_visit=50.0, gumbel_scale=1.0,
                               gumbel_full=False, eval_cache=0, solver=False, kld_gain=0.0, kld_interval=100,
                               smart_pruning=False)
    for kind in ("mini", "normal", "distribute"):
        engine = Config(kind).engine
        for k, v in so.DEFAULTS.items():
            assert getattr(engine, k) == v and type(getattr(engine, k)) is type(v), (kind, k)
    engine = _config("self", []).engine
    assert all(getattr(engine, k) == v for k, v in so.DEFAULTS.items())
    # a configuration without an engine section resolves to the defaults, an override wins over the section
    assert so.resolve(types.SimpleNamespace(), **dict.fromkeys(so.DEFAULTS)) == so.DEFAULTS
    cfg = Config("mini")
    cfg.engine.kld_gain = 1e-3
    assert so.resolve(cfg, kld_gain=None, solver=1, gumbel=None) == dict(kld_gain=1e-3, solver=True, gumbel=0)


def test_the_order_of_the_report_is_range_command_needs_exclusions():
    bad = dict(kld_gain=-1.0, gumbel=8, solver=True)
    with pytest.raises(so.SearchOptionError, match="gumbel 8 needs record_visits"):       # (table order across options)
        so.check(bad)
    with pytest.raises(so.SearchOptionError, match="solver excludes gumbel"):
        so.check(dict(bad, record_visits=True))
    with pytest.raises(so.SearchOptionError, match="kld_gain -1.0: expected a finite G >= 0"):
        so.check(dict(kld_gain=-1.0, solver=True), cmd="eval")
    with pytest.raises(so.SearchOptionError, match="--kld-gain is an option of `run.py self`"):
        so.check(dict(kld_gain=1e-3, solver=True), cmd="eval", flags=True)
    with pytest.raises(so.SearchOptionError, match="kld_gain excludes solver"):
        so.check(dict(kld_gain=1e-3, solver=True), cmd="self")


def test_apply_and_describe_follow_the_table():
    calls = []

    class Recorder:
        def __getattr__(self, name):
            return lambda *a: calls.append((name,) + a)
    values = so.resolve(types.SimpleNamespace(), **dict.fromkeys(so.DEFAULTS))
    so.apply(Recorder(), values)
    assert calls == [] and so.describe(values, 800) == []
    values.update(record_visits=True, fast_sims=8, record_q=True, leaf_mirror=0.5, eval_cache=10, kld_gain=1e-3)
    so.apply(Recorder(), values, skip=("eval_cache",))
    assert calls == [("set_playout_cap", 8, 0.25), ("record_values", True), ("set_leaf_mirror", 0.5),
                     ("set_kld_gain", 1e-3, 100)]
    del calls[:]
    so.apply(Recorder(), dict(solver=True, smart_pruning=False))
    assert calls == [("set_solver", True)]
    lines = so.describe(values, 800)
    assert len(lines) == 5 and lines[0].startswith("playout cap: a ply is a full search (800 simulations) with probability 0.25")
    assert lines[3] == "evaluation cache: 2^10 entries, 0 MiB, kept across games" and "less than 0.001 per" in lines[4]


def test_the_engine_player_and_arena_refuse_without_a_device(monkeypatch):
    from cchess_alphazero import _native
    from cchess_alphazero.agent.player import CChessPlayer
    from cchess_alphazero.engine import SelfPlayEngine
    from cchess_alphazero.worker.evaluator import EvaluateWorker

    def no_device():
        raise AssertionError("the options are checked before a device is asked for")
    monkeypatch.setattr(_native, "require_gpu", no_device)
    cfg = Config("mini")
    for later, earlier, _ in so.EXCLUDES:
        if "smart_pruning" in (later, earlier):
            continue                                        # (not an option of the self-play engine)
        with pytest.raises(ValueError, match=f"{later} excludes {earlier}"):
            SelfPlayEngine(cfg, 2, **{**FEATURES[later][0], **FEATURES[earlier][0]})
    with pytest.raises(ValueError, match="gumbel 8 needs record_visits"):
        SelfPlayEngine(cfg, 2, gumbel=8)
    with pytest.raises(ValueError, match="leaf_mirror 1.5: expected 0 <= P <= 1"):
        SelfPlayEngine(cfg, 2, leaf_mirror=1.5)
    cfg.engine.solver = True                                # the configuration's value against a keyword
    with pytest.raises(ValueError, match="kld_gain excludes solver"):
        SelfPlayEngine(cfg, 2, kld_gain=1e-3)
    # the player refuses before it creates its search object, the arena worker when it is made
    monkeypatch.setattr("cchess_alphazero.agent.player.Search", lambda *a, **k: no_device())
    with pytest.raises(ValueError, match="smart_pruning excludes solver"):
        CChessPlayer(cfg, pipes=object(), smart_pruning=True)
    cfg.engine.smart_pruning = True
    with pytest.raises(ValueError, match="smart_pruning excludes solver"):
        EvaluateWorker(cfg, evaluators=(None, None))
    w = EvaluateWorker(types.SimpleNamespace(), evaluators=(None, None))
    assert (w.leaf_mirror, w.solver, w.smart_pruning) == (0.0, False, False)
