"""run.py opt --augment mirror without a GPU: the label mirror M (cz_label_mirror) against the string rule, the rules'
equivariance under the left-right mirror through the oracle on every golden position (what licenses calling a mirrored
row a real position), the command line, and the worker's flag generator."""
import numpy as np
import pytest


def test_label_mirror_table():
    from cchess_alphazero import _native
    from cchess_alphazero.environment.lookup_tables import ActionLabelsRed, MirrorLabels, mirror_move, mirror_policy
    M = _native.label_mirror()
    assert M.dtype == np.uint16 and M.shape == (2086,)
    index = {m: i for i, m in enumerate(ActionLabelsRed)}
    rule = [index[f"{8 - int(m[0])}{m[1]}{8 - int(m[2])}{m[3]}"] for m in ActionLabelsRed]     # every label maps to a label
    assert M.tolist() == rule == list(MirrorLabels)
    assert [mirror_move(m) for m in ActionLabelsRed] == [ActionLabelsRed[i] for i in rule]
    assert (M[M] == np.arange(2086)).all()                                  # an involution
    assert sorted(M.tolist()) == list(range(2086))                          # onto: all 2086 labels
    fixed = np.flatnonzero(M == np.arange(2086))
    assert len(fixed) == 90 and all(ActionLabelsRed[i][0] == "4" == ActionLabelsRed[i][2] for i in fixed)
    pol = np.arange(2086, dtype=np.float32)
    assert (mirror_policy(pol)[M] == pol).all()


def test_rules_are_equivariant_on_all_golden_positions(positions_1k):
    """Legal-move set, done (both need_check settings, final move through M) and planes of mirror_state(s) are the mirror
    images of those of s -- on all positions, none left out.  (The ORDER of the move lists differs: sets are compared.)"""
    from oracle import xq_oracle as xo
    from cchess_alphazero.environment.lookup_tables import mirror_move
    from cchess_alphazero.environment.static_env import mirror_state
    assert len(positions_1k) == 1032
    for pos in positions_1k:
        s = pos["state"]
        m = mirror_state(s)
        assert mirror_state(m) == s
        assert np.array_equal(xo.state_to_board(m).reshape(10, 9), xo.state_to_board(s).reshape(10, 9)[:, ::-1]), s
        assert set(xo.get_legal_moves(m)) == {mirror_move(a) for a in xo.get_legal_moves(s)}, s
        for need_check in (False, True):
            a, b = xo.done(s, need_check), xo.done(m, need_check)
            a = a[:2] + (None if a[2] is None else mirror_move(a[2]),) + a[3:]
            assert a == b, (s, need_check)
        assert np.array_equal(xo.state_to_planes(m), xo.state_to_planes(s)[:, :, ::-1]), s


def test_augment_option_reaches_the_config(monkeypatch, tmp_path):
    from cchess_alphazero import manager
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    parse = manager.create_parser().parse_args
    assert manager.build_config(parse(["opt", "--augment", "mirror"])).trainer.augment == "mirror"
    assert manager.build_config(parse(["opt", "--augment", "none"])).trainer.augment == "none"
    assert manager.build_config(parse(["opt"])).trainer.augment == "none"
    with pytest.raises(SystemExit):
        parse(["opt", "--augment", "flip"])


def _worker(monkeypatch, tmp_path, **trainer):
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    from cchess_alphazero.config import Config
    from cchess_alphazero.worker.optimize import OptimizeWorker
    cfg = Config("mini")
    for k, v in trainer.items():
        setattr(cfg.trainer, k, v)
    return cfg, OptimizeWorker(cfg)


def test_flag_generator(monkeypatch, tmp_path):
    # none (set, or the attribute missing as in a Config built without the command line): no flags, and self.rng is the
    # parent's generator, draw for draw
    for kw in (dict(), dict(augment="none")):
        cfg, w = _worker(monkeypatch, tmp_path, **kw)
        assert w.augment == "none" and w.mirror_flags(1000) is None
        ref = np.random.default_rng(cfg.engine.base_seed)
        for n in (980, 17, 980):
            assert w.mirror_flags(n) is None
            assert (w.rng.permutation(np.arange(n)) == ref.permutation(np.arange(n))).all()
    # mirror: the flags do not touch self.rng, two workers with one seed agree, and the coin is fair
    cfg, a = _worker(monkeypatch, tmp_path, augment="mirror")
    _, b = _worker(monkeypatch, tmp_path, augment="mirror")
    ref = np.random.default_rng(cfg.engine.base_seed)
    n = 100000
    fa, fb = a.mirror_flags(n), b.mirror_flags(n)
    assert fa.dtype == np.uint8 and fa.shape == (n,) and set(np.unique(fa)) == {0, 1}
    assert (fa == fb).all() and (a.mirror_flags(333) == b.mirror_flags(333)).all()
    assert abs(int(fa.sum()) - n / 2) <= 5 * np.sqrt(n) / 2                  # five sigma of Binomial(n, 1/2)
    assert (a.rng.permutation(np.arange(980)) == ref.permutation(np.arange(980))).all()
    with pytest.raises(ValueError):
        _worker(monkeypatch, tmp_path, augment="flip")
