"""The policy surprise record and the surprise weighting (cz_search_record_surprise, run.py self --record-surprise, run.py
opt --surprise-weight), the parts that need no GPU: the arithmetic's restatement (tests/surprise_oracle.py), the per-game
training weights, the record item builder, the command-line flags and the six-element record format."""
import json
import math
import os

import numpy as np
import pytest

import surprise_oracle as so

B = so.BANNED
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _f32(x):
    return np.asarray(x, dtype=np.float32)


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def test_oracle_on_hand_made_rows():
    # t = (1/2, 1/2), r = (1/4, 3/4): (ln 2 + ln(2/3)) / 2
    s, A = so.surprise([1, 2], [5, 5], _f32([0.25, 0.75]))
    assert abs(s - 0.14384103622589045) < 1e-15 and abs(s - 0.5 * math.log(4.0 / 3.0)) < 1e-15
    assert abs(A - 0.5 * (math.log(2.0) + math.log(1.5))) < 1e-15
    # the priors need not be normalised: P divides them
    assert so.surprise([1, 2], [5, 5], _f32([0.125, 0.375]))[0] == s
    # t = r: exactly 0
    assert so.surprise([1, 2, 3], [1, 2, 1], _f32([0.25, 0.5, 0.25])) == (0.0, 0.0)
    assert so.surprise([7], [9], _f32([0.125])) == (0.0, 0.0)
    # an unvisited edge adds nothing but still counts in P
    s2, _ = so.surprise([1, 2, 3], [4, 0, 4], _f32([0.25, 0.5, 0.25]))
    assert abs(s2 - math.log(2.0)) < 1e-15
    # the floor: a visited edge with a prior of 0 is finite and below the bound
    s3, A3 = so.surprise([1, 2], [1, 1], _f32([0.0, 1.0]))
    assert math.isfinite(s3) and 0.0 < s3 < so.S_BOUND
    assert abs(s3 - 0.5 * (math.log(0.5 / 1e-30) + math.log(0.5))) < 1e-13
    worst, _ = so.surprise([1, 2], [1000000, 0], _f32([0.0, 1.0]))          # every visit on a prior of 0: the supremum
    assert abs(worst - math.log(1e30)) < 1e-13 and worst < so.S_BOUND
    # banned edges are excluded from M and from P, whatever they hold
    a = so.surprise([1, 2 | B, 3], [5, 1000, 5], _f32([0.25, 100.0, 0.75]))
    assert a == so.surprise([1, 3], [5, 5], _f32([0.25, 0.75]))
    # nothing to measure: NaN
    for row in (([], [], _f32([])), ([1 | B, 2 | B], [3, 4], _f32([0.5, 0.5])), ([1, 2], [0, 0], _f32([0.5, 0.5])),
                ([1, 2], [3, 4], _f32([0.0, 0.0])), ([1 | B, 2], [3, 0], _f32([0.5, 0.5]))):
        got = so.surprise(*row)
        assert math.isnan(got[0]) and got[1] == 0.0, row
    assert so.same(so.NAN, so.NAN, 0.0) and not so.same(so.NAN, 0.0, 1.0) and not so.same(0.0, 1e-14, 1.0)
    assert so.same(1.0, 1.0 + 2.0 ** -50, 1.0) and so.bound(0.0) == 1e-300


def test_oracle_is_never_negative_on_seeded_rows():
    rng = np.random.default_rng(2026)
    lo = 1.0
    for i in range(1000):
        nm = int(rng.integers(1, 129))
        p = rng.dirichlet(np.full(nm, 0.3)).astype(np.float32)
        m = (rng.integers(0, 50, nm) * (rng.random(nm) < 0.6)).astype(np.int32)
        if i % 4 == 0:                                      # counts close to the priors: s close to 0
            m = np.round(p.astype(np.float64) * 4000).astype(np.int32)
        lab = rng.permutation(2086)[:nm].astype(np.uint16)
        lab[rng.random(nm) < 0.1 * (i % 3)] |= B
        s, A = so.surprise(lab, m, p)
        assert s != s or (0.0 <= s <= A + 1e-300 and s < so.S_BOUND), (i, s, A)
        if s == s:
            lo = min(lo, s)
    assert lo < 1e-3


# ---- the weights -----------------------------------------------------------------------------------------------------------------
def test_surprise_weights():
    from cchess_alphazero.lib.replay_window import surprise_weights
    nan = np.nan
    rng = np.random.default_rng(7)
    lens = [1, 5, 40, 1, 17, 3]
    offs = np.concatenate([[0], np.cumsum(lens)])
    n = int(offs[-1])
    s = rng.gamma(0.5, 0.4, n).astype(np.float32)
    s[rng.random(n) < 0.2] = nan
    tr = (rng.random(n) < 0.7).astype(np.uint8)
    tr[0] = 1
    s[0] = 0.3                                              # a game of a single row, with an s
    tr[offs[3]] = 1
    s[offs[3]] = nan                                        # ... and one without
    for a in (0.0, 0.25, 0.5, 1.0):
        w = surprise_weights(s, tr, offs, a)
        assert w.dtype == np.float32 and w.shape == (n,)
        assert (w[tr == 0] == 0).all()                      # weight-0 rows stay 0
        no_s = (tr == 1) & np.isnan(s)
        assert (w[no_s] == 1).all()                         # rows without s get 1
        for lo, hi in zip(offs[:-1], offs[1:]):
            f = (tr[lo:hi] == 1) & np.isfinite(s[lo:hi])
            k = int(f.sum())
            if k:                                           # float32 rounding of k weights of about 1: half an ulp each
                tot = float(w[lo:hi][f].astype(np.float64).sum())
                assert abs(tot - k) <= k * 2.0 ** -24 * max(1.0, float(w[lo:hi][f].max())), (a, lo, tot, k)
                want = (1 - a) + a * k * s[lo:hi][f].astype(np.float64) / s[lo:hi][f].astype(np.float64).sum()
                assert (w[lo:hi][f] == want.astype(np.float32)).all()
        assert w[0] == 1.0 and w[offs[3]] == 1.0            # the single-row games
        if a == 0.0:
            assert (w == tr).all()                          # alpha = 0: all ones
    # alpha = 1 with one surprising row: the whole of |F| on that row
    w = surprise_weights([0.0, 0.0, 2.5, 0.0, nan], [1, 1, 1, 1, 1], [0, 5], 1.0)
    assert w.tolist() == [0.0, 0.0, 4.0, 0.0, 1.0]
    w = surprise_weights([0.0, 0.0, 2.5, 0.0, nan], [1, 1, 1, 1, 1], [0, 5], 0.5)
    assert w.tolist() == [0.5, 0.5, 2.5, 0.5, 1.0]
    # S = 0: ones
    assert surprise_weights([0.0, 0.0, nan], [1, 1, 0], [0, 3], 1.0).tolist() == [1.0, 1.0, 0.0]
    # games do not mix; an empty game and no game at all are handled
    w = surprise_weights([1.0, 3.0, 5.0, 5.0], [1, 1, 1, 1], [0, 2, 2, 4], 1.0)
    assert w.tolist() == [0.5, 1.5, 1.0, 1.0]
    assert surprise_weights([], [], [0], 0.5).shape == (0,)
    # a fast ply's s takes no part: it is not in F
    w = surprise_weights([1.0, 9.0, 3.0], [1, 0, 1], [0, 3], 1.0)
    assert w.tolist() == [0.5, 0.0, 1.5]


# ---- the record items ------------------------------------------------------------------------------------------------------------
def test_record_item_forms():
    from cchess_alphazero.environment.lookup_tables import ActionLabelsRed as L
    from cchess_alphazero.lib.data_helper import record_item, surprise_sums
    e = so.Entry(np.array([5, 9, 11], dtype=np.uint16), np.array([4, 0, 6], dtype=np.int32), np.array([False, False, True]),
                 0.12345678, 0.98765432)
    pi = [[L[5], 4]]
    mv = L[5]
    # the option off: every form is what it was
    assert record_item(mv, 1, None, labels=L) == [mv, 1]
    assert record_item(mv, 1, e, labels=L) == [mv, 1, pi]
    assert record_item(mv, -1, e, fast=True, labels=L) == [mv, -1, pi, 0]
    assert record_item(mv, -1, None, fast=True, labels=L) == [mv, -1, None, 0]
    assert record_item(mv, 1, e, record_q=True, labels=L) == [mv, 1, pi, 1, 0.123457]
    assert record_item(mv, 1, e, fast=True, record_q=True, labels=L) == [mv, 1, pi, 0, 0.123457]
    assert record_item(mv, 1, None, record_q=True, labels=L) == [mv, 1]
    for q in (False, True):
        assert record_item(mv, 1, e, fast=True, record_q=q, labels=L, record_surprise=False) == \
               record_item(mv, 1, e, fast=True, record_q=q, labels=L)
    # the option on: six elements where the ply has an entry, an explicit weight, q None with record_q off
    assert record_item(mv, 1, e, labels=L, record_surprise=True) == [mv, 1, pi, 1, None, 0.987654]
    assert record_item(mv, 1, e, fast=True, labels=L, record_surprise=True) == [mv, 1, pi, 0, None, 0.987654]
    assert record_item(mv, 1, e, record_q=True, labels=L, record_surprise=True) == [mv, 1, pi, 1, 0.123457, 0.987654]
    assert record_item(mv, 1, e, fast=True, record_q=True, labels=L, record_surprise=True) == \
           [mv, 1, pi, 0, 0.123457, 0.987654]
    assert record_item(mv, 1, e._replace(s=None), record_q=True, labels=L, record_surprise=True) == \
           [mv, 1, pi, 1, 0.123457, None]
    assert record_item(mv, 1, e._replace(q=None, s=0.0), record_q=True, labels=L, record_surprise=True) == \
           [mv, 1, pi, 1, None, 0.0]
    assert record_item(mv, 1, e._replace(s=69.0775527898), labels=L, record_surprise=True)[5] == 69.077553
    # ... and the shorter forms where it has none
    assert record_item(mv, 1, None, record_q=True, labels=L, record_surprise=True) == [mv, 1]
    assert record_item(mv, 1, None, fast=True, labels=L, record_surprise=True) == [mv, 1, None, 0]
    data = ["state", [mv, 1, pi, 1, 0.5, 0.25], [mv, -1, pi, 0, None, 1.5], [mv, 1, pi, 1, None, None], [mv, 1, pi, 1, 0.1, 0.5],
            [mv, -1, pi, 0, 0.2, 0.5], [mv, -1, pi, 1, 0.2], [mv, -1]]
    assert surprise_sums(data) == (0.75, 2, 2.0, 2)
    assert surprise_sums(["state", [mv, 1], [mv, -1, pi]]) == (0, 0, 0, 0)


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_command_line_flags():
    from cchess_alphazero import manager
    from cchess_alphazero.config import Config
    assert Config("mini").engine.record_surprise is False
    p = manager.create_parser()
    cfg = manager.build_config(p.parse_args(["self"]))
    assert cfg.engine.record_surprise is False and cfg.trainer.surprise_weight == 0.0
    cfg = manager.build_config(p.parse_args(["self", "--record-visits"]))
    assert cfg.engine.record_surprise is False
    cfg = manager.build_config(p.parse_args(["self", "--record-visits", "--record-surprise"]))
    assert cfg.engine.record_surprise is True and cfg.engine.record_visits is True and cfg.engine.record_q is False
    with pytest.raises(SystemExit) as e:
        manager.build_config(p.parse_args(["self", "--record-surprise"]))
    assert "--record-surprise needs --record-visits" in str(e.value)
    for ok in ("0", "0.5", "1"):
        assert manager.build_config(p.parse_args(["opt", "--surprise-weight", ok])).trainer.surprise_weight == float(ok)
    for bad in ("-0.1", "1.5", "nan", "inf"):
        with pytest.raises(SystemExit) as e:
            manager.build_config(p.parse_args(["opt", "--surprise-weight", bad]))
        assert f"--surprise-weight {bad}" in str(e.value), bad


# ---- the record format -----------------------------------------------------------------------------------------------------------
def six_element_games(games):
    """Engine records rewritten as run.py self --record-visits --record-q --record-surprise --fast-sims writes them, by
    lib/data_helper.record_item: every ply but each game's last gets pi = its own move, every third ply is a fast one,
    every fifth has no q, every seventh no s.  The moves and values are untouched."""
    from cchess_alphazero.environment.lookup_tables import ActionLabelsRed
    from cchess_alphazero.lib.data_helper import record_item
    label = {m: i for i, m in enumerate(ActionLabelsRed)}
    out = []
    for g in games:
        data = [g[0]]
        for i, it in enumerate(g[1:]):
            last = i == len(g) - 2
            q = None if i % 5 == 4 else 0.5 * it[1] + 0.001 * i
            s = None if i % 7 == 6 else 0.01 * (i % 11) ** 2
            e = None if last else so.Entry(np.array([label[it[0]]], dtype=np.uint16), np.array([7 + i], dtype=np.int32),
                                           np.array([False]), q, s)
            data.append(record_item(it[0], it[1], e, fast=(i % 3 == 2 and not last), record_q=True, labels=ActionLabelsRed,
                                    record_surprise=True))
        out.append(data)
    return out


def test_six_element_records_split_like_the_shorter_ones():
    from cchess_alphazero.lib.record_decoder import split_games
    with open(os.path.join(GOLDEN, "engine_records.json")) as f:
        games = [g["data"] for g in json.load(f)["games"]]
    six = six_element_games(games)
    items = [it for g in six for it in g[1:]]
    assert {len(it) for it in items} == {2, 6}
    assert {it[3] for it in items if len(it) == 6} == {0, 1}
    for col in (4, 5):
        assert any(it[col] is None for it in items if len(it) == 6) and any(it[col] is not None for it in items if len(it) == 6)
    assert all(it[5] is None or 0.0 <= it[5] <= so.S_BOUND for it in items if len(it) == 6)
    assert json.loads(json.dumps(six)) == six
    flat = [x for g in six for x in g]                      # several games in one file, as nb_game_in_file > 1 writes them
    assert split_games(json.loads(json.dumps(flat))) == six
    for g, d in zip(games, six):
        assert [it[:2] for it in d[1:]] == [list(it[:2]) for it in g[1:]] and d[0] == g[0]
