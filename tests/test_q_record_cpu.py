"""The root value record and the z/q value mix (cz_search_record_values, run.py self --record-q, run.py opt --q-ratio), the
parts that need no GPU: the arithmetic's restatement (tests/q_record_oracle.py) on hand-made rows, the command-line
flags, the record item builder and the float32 value target."""
import math

import numpy as np
import pytest

import q_record_oracle as qo

B = qo.BANNED


def test_root_value_formula_on_hand_made_rows():
    # no bans, m = n: sum w / sum n
    assert qo.root_value([1, 2], [2, 2], [2, 2], [1.0, -0.5]) == 0.125
    assert qo.root_value([1, 2, 3], [10, 30, 60], [10, 30, 60], [5.0, -15.0, 30.0]) == (5.0 - 15.0 + 30.0) / 100
    # a banned edge counts for nothing, whatever it holds
    assert qo.root_value([1, 2 | B, 3], [4, 1000, 4], [4, 1000, 4], [2.0, 1000.0, -1.0]) == (2.0 - 1.0) / 8
    # pruned m: the weights are the recorded counts, the q's the raw ones
    got = qo.root_value([1, 2, 3], [90, 0, 2], [90, 6, 4], [45.0, -6.0, 1.0])
    assert got == (90 * 0.5 + 0 * -1.0 + 2 * 0.25) / 92
    assert got > qo.root_value([1, 2, 3], [90, 6, 4], [90, 6, 4], [45.0, -6.0, 1.0])       # forcing's visits dragged it down
    # an edge with n = 0 has no q: skipped, even with a (malformed) recorded count
    assert qo.root_value([1, 2], [3, 0], [3, 0], [1.5, 0.0]) == 0.5
    assert qo.root_value([1, 2], [3, 5], [3, 0], [1.5, 9.0]) == 0.5
    # nothing left: NaN
    for row in (([1 | B, 2 | B], [3, 4], [3, 4], [1.0, 1.0]), ([], [], [], []), ([1, 2], [0, 0], [0, 0], [0.0, 0.0]),
                ([1, 2], [0, 0], [5, 5], [1.0, 1.0])):
        assert math.isnan(qo.root_value(*row))
    # one edge: its own q, whatever its weight
    assert qo.root_value([7], [1], [3], [-2.0]) == -2.0 / 3
    assert qo.root_value([7], [3], [3], [6.0]) == 2.0                                        # a proven win: done.v * 2
    assert qo.same_value(qo.NAN, qo.NAN) and not qo.same_value(qo.NAN, 0.0) and not qo.same_value(0.0, 2e-13)
    # the sums are exact: many terms that cancel leave the small one
    n = [1] * 101
    w = [1e16, -1e16] * 50 + [1.0]
    assert qo.root_value(list(range(101)), n, n, w) == 1.0 / 101


def test_command_line_flags():
    from cchess_alphazero import manager
    from cchess_alphazero.config import Config
    assert Config("mini").engine.record_q is False
    p = manager.create_parser()
    cfg = manager.build_config(p.parse_args(["self"]))
    assert cfg.engine.record_q is False and cfg.trainer.q_ratio == 0.0 and cfg.engine.record_visits is False
    cfg = manager.build_config(p.parse_args(["self", "--record-visits"]))
    assert cfg.engine.record_q is False
    cfg = manager.build_config(p.parse_args(["self", "--record-visits", "--record-q"]))
    assert cfg.engine.record_q is True and cfg.engine.record_visits is True
    with pytest.raises(SystemExit) as e:
        manager.build_config(p.parse_args(["self", "--record-q"]))
    assert "--record-q needs --record-visits" in str(e.value)
    for ok in ("0", "0.3", "1"):
        assert manager.build_config(p.parse_args(["opt", "--q-ratio", ok])).trainer.q_ratio == float(ok)
    for bad in ("-0.1", "1.5", "nan", "inf"):
        with pytest.raises(SystemExit) as e:
            manager.build_config(p.parse_args(["opt", "--q-ratio", bad]))
        assert f"--q-ratio {bad}" in str(e.value), bad


def test_record_item_forms():
    from cchess_alphazero.environment.lookup_tables import ActionLabelsRed as L
    from cchess_alphazero.lib.data_helper import mean_abs_q_minus_z, record_item
    e = qo.Entry(np.array([5, 9, 11], dtype=np.uint16), np.array([4, 0, 6], dtype=np.int32), np.array([False, False, True]),
                 0.12345678)
    pi = [[L[5], 4]]
    mv = L[5]
    # as before the option: with record_q off nothing changes
    assert record_item(mv, 1, None, labels=L) == [mv, 1]
    assert record_item(mv, 1, e, labels=L) == [mv, 1, pi]
    assert record_item(mv, -1, e, fast=True, labels=L) == [mv, -1, pi, 0]
    assert record_item(mv, -1, None, fast=True, labels=L) == [mv, -1, None, 0]
    # record_q on: five elements where the ply has an entry
    assert record_item(mv, 1, e, record_q=True, labels=L) == [mv, 1, pi, 1, 0.123457]
    assert record_item(mv, 1, e, fast=True, record_q=True, labels=L) == [mv, 1, pi, 0, 0.123457]
    assert record_item(mv, 1, e._replace(q=None), record_q=True, labels=L) == [mv, 1, pi, 1, None]
    # ... and the shorter forms where it has none: the appended king capture, games without a complete visit record
    assert record_item(mv, 1, None, record_q=True, labels=L) == [mv, 1]
    assert record_item(mv, 1, None, fast=True, record_q=True, labels=L) == [mv, 1, None, 0]
    assert record_item(mv, 1, e._replace(q=-2.0), record_q=True, labels=L)[4] == -2.0
    data = ["state", [mv, 1, pi, 1, 0.5], [mv, -1, pi, 0, None], [mv, 1, pi, 0, -0.25], [mv, -1]]
    assert mean_abs_q_minus_z(data) == (0.5 + 1.25, 2)
    assert mean_abs_q_minus_z(["state", [mv, 1], [mv, -1, pi]]) == (0, 0)


def test_float32_value_target_against_float64():
    from cchess_alphazero.lib.replay_window import Q_BOUND, mix_targets
    rng = np.random.default_rng(2026)
    n = 1000
    z = rng.choice(np.array([-1.0, 0.0, 1.0], dtype=np.float32), size=n)
    q = rng.uniform(-Q_BOUND, Q_BOUND, size=n).astype(np.float32)
    q[rng.random(n) < 0.2] = np.nan
    u = 2.0 ** -24                                  # unit roundoff of float32
    for lam in (0.0, 0.3, 0.5, 1.0):
        t = mix_targets(z, q, lam)
        assert t.dtype == np.float32 and t.shape == (n,)
        lam32 = float(np.float32(lam))              # the kernel takes L as a float32: that rounding is not the mix's
        ref = qo.mix_f64(z, q, lam32)
        # three float32 operations, each within u of its exact result: the difference d = q - z, the product L d (it
        # inherits L u |d| from d), the sum t (it inherits the product's error): 2 L u |d| + u |t|, to first order
        d = np.abs(np.where(np.isnan(q), z, q).astype(np.float64) - z)
        bound = (2 * lam32 * d + np.abs(ref)) * u * (1 + 2.0 ** -20)
        assert (np.abs(t.astype(np.float64) - ref) <= bound).all(), lam
        nan = np.isnan(q)
        assert (t[nan] == z[nan]).all() and not np.isnan(t).any()
        if lam == 0.0:
            assert t.tobytes() == z.tobytes()
        if lam == 1.0:                              # z + (q - z): q itself up to the two roundings
            assert (np.abs(t[~nan] - q[~nan]) <= 3 * u * 3).all()
    # the same bits step by step
    lam = np.float32(0.3)
    step = z + (lam * (q - z).astype(np.float32)).astype(np.float32)
    assert mix_targets(z, q, 0.3)[~nan].tobytes() == step.astype(np.float32)[~nan].tobytes()
