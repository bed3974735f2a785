"""Gumbel root search with sequential halving without a GPU: tests/gumbel_oracle.py -- the yardstick of
test_gpu_gumbel.py -- is held to hand-written schedules, to forced_playouts_oracle.Search where the two must agree
(M = 0), to the invariants of the halving and of the policy target, and to the condition the GPU comparison rests on: on
the inputs of that comparison no selection is decided by less than 1e-9, far above what two libraries' exp and log
differ by.  The command line is checked against config.engine and config.play."""
import numpy as np
import pytest

import forced_playouts_oracle as fo
import gumbel_oracle as go

SIMS, M, SEED = 64, 16, 7


def test_seq_against_hand_written_cases():
    assert go.seq(1, 5) == [0, 1, 2, 3, 4]
    assert go.seq(2, 3) == [0, 0, 1]
    assert go.seq(4, 8) == [0, 0, 0, 0, 1, 1, 2, 2]
    assert go.seq(16, 32) == [0] * 16 + [1] * 8 + [2] * 4 + [3] * 4
    # L = 4: 12 rounds of 16, 25 of 8, 50 of 4, 100 of 2, then the last pair goes on
    want = [v for v in range(12) for _ in range(16)] + [v for v in range(12, 37) for _ in range(8)]
    want += [v for v in range(37, 87) for _ in range(4)] + [v for v in range(87, 187) for _ in range(2)]
    want += [187, 187, 188, 188, 189, 189, 190, 190]
    assert len(want) == 800 and go.seq(16, 800) == want
    assert go.seq(5, 7) == [0, 0, 0, 0, 0, 1, 1]


@pytest.fixture(scope="module")
def draws():
    return go.draws_for(SEED, 0, 0, 0)


@pytest.fixture(scope="module")
def runs(draws):
    return [(c, go.run_case(c, M, SIMS, draws)) for c in fo.cases()]


def test_m_0_is_the_plain_search_bit_for_bit(draws):
    for c in fo.cases():
        want, _ = fo.run_case(c, 0.0, sims=SIMS)
        got, _ = fo.run_case(c, 0.0, sims=SIMS, search_cls=lambda cfg, salt, k: go.Search(cfg, salt, k, 0, draws=draws))
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a["state"] == b["state"] and a["no_act"] == b["no_act"] and a["best"] == b["best"]
            assert a["stats"]["sum_n"] == b["stats"]["sum_n"]
            for k in ("moves", "n", "w", "p"):
                assert a["stats"][k].tobytes() == b["stats"][k].tobytes(), (c["name"], k)
            assert (a["targets"] == b["targets"]).all() and a["raw_total"] == b["raw_total"]


def test_started_is_the_schedule_as_a_multiset(runs):
    kinds = set()
    for c, (res, _) in runs:
        kinds.add(c["kind"])
        for r in res:
            started, used = np.array(r["started"]), r["seq_used"]
            live = [i for i, l in enumerate(r["stats"]["moves"]) if go.xo.label_str(int(l)) not in r["no_act"]]
            assert sum(r["started"]) == len(used) > 0 and len(used) <= r["budget"]
            assert used == go.seq(min(M, len(live)), r["budget"])[:len(used)]
            for v in range(max(used) + 2):
                assert int((started > v).sum()) == used.count(v), (c["name"], v)
            assert all(started[i] == 0 for i in range(len(started)) if i not in live)
            # the played move is one of the most-started edges, and exactly min(M, edges) edges were ever started
            top = [i for i in live if started[i] == started[live].max()]
            assert go.xo.label_of_str(r["best"]) in [int(r["stats"]["moves"][i]) for i in top]
            assert int((started > 0).sum()) == min(M, len(live), len(used))
    assert kinds >= {"ban", "reuse"}
    assert any(len(r["started"]) > 64 for _, (res, _) in runs for r in res)


def test_ban_case_bans_what_an_unbanned_run_plays(runs, draws):
    c, (res, _) = next(x for x in runs if x[0]["kind"] == "ban")
    free = go.Search(fo.play_cfg(SIMS), c["salt"], 0.0, M, draws=draws)
    free.search(c["state"])
    assert res[0]["no_act"] == [free.played(c["state"])[0]] and res[0]["best"] != res[0]["no_act"][0]


def test_target_properties(runs):
    for c, (res, _) in runs:
        for r in res:
            st = r["stats"]
            lab = st["moves"].copy()
            banned = np.array([go.xo.label_str(int(l)) in r["no_act"] for l in lab])
            lab[banned] |= go.BANNED
            t, raw = go.target(lab, st["n"], st["w"], st["p"])
            assert (t == r["targets"]).all() and raw == r["raw_total"] == int(st["n"][~banned].sum())
            assert abs(int(t.sum()) - 65536) <= int((~banned).sum()), c["name"]
            assert (t[banned] == 0).all()
            # c_scale = 0: sigma vanishes, the target is the prior renormalised over the live edges
            t0, _ = go.target(lab, st["n"], st["w"], st["p"], 50.0, 0.0)
            p = st["p"].astype(np.float64) * ~banned
            assert (t0 == np.floor(65536.0 * (p / p.sum()) + 0.5).astype(np.int32)).all(), c["name"]
    # nothing visited: the completed q is one half everywhere, the target is the prior again
    p = np.array([0.5, 0.25, 0.25, 0.0], dtype=np.float32)
    t, raw = go.target(np.arange(4, dtype=np.uint16), np.zeros(4, np.int32), np.zeros(4), p)
    assert t.tolist() == [32768, 16384, 16384, 0] and raw == 0
    # a visited edge with a good value gains, an edge with prior 0 stays 0
    t, _ = go.target(np.arange(4, dtype=np.uint16), np.array([3, 2, 0, 0], np.int32), np.array([3.0, -2.0, 0, 0]), p,
                     c_visit=0.0, c_scale=0.1)
    assert t[0] > 32768 and t[1] < t[2] and t[3] == 0 and abs(int(t.sum()) - 65536) <= 4


def test_margins_carry_the_gpu_comparison(runs):
    """Every root selection and every final choice of the GPU test's searches is decided by more than 1e-9: a score is a
    sum of a few terms of magnitude <= 1e2, two float64 libraries agree on it to ~1e-13."""
    for c, (res, _) in runs:
        for r in res:
            assert min(r["margins"]) > 1e-9, (c["name"], min(r["margins"]))
            assert r["best_margin"] > 1e-9, (c["name"], r["best_margin"])


def test_command_line(monkeypatch, tmp_path):
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    from cchess_alphazero import manager
    p = manager.create_parser()
    cfg = manager.build_config(p.parse_args(["self"]))
    default_sims = cfg.play.simulation_num_per_move
    assert cfg.engine.gumbel == 0 and cfg.engine.gumbel_visit == 50.0 and cfg.engine.gumbel_scale == 1.0
    cfg = manager.build_config(p.parse_args(["self", "--record-visits", "--gumbel", "16", "--sims", "16"]))
    assert cfg.engine.gumbel == 16 and cfg.play.simulation_num_per_move == 16 != default_sims
    cfg = manager.build_config(p.parse_args(["self", "--record-visits", "--gumbel", "8", "--gumbel-visit", "20",
                                             "--gumbel-scale", "0.5", "--leaf-mirror", "0.5", "--record-q",
                                             "--record-surprise", "--book", "b.txt"]))
    assert (cfg.engine.gumbel, cfg.engine.gumbel_visit, cfg.engine.gumbel_scale) == (8, 20.0, 0.5)
    assert cfg.play.simulation_num_per_move == default_sims
    cfg = manager.build_config(p.parse_args(["self", "--sims", "32", "--fast-sims", "32"]))     # (the bound follows --sims)
    assert cfg.play.simulation_num_per_move == 32 and cfg.engine.fast_sims == 32
    for bad, word in ((["--gumbel", "16"], "needs --record-visits"),
                      (["--record-visits", "--gumbel", "16", "--fast-sims", "8"], "--fast-sims"),
                      (["--record-visits", "--gumbel", "16", "--forced-playouts", "2"], "--forced-playouts"),
                      (["--record-visits", "--gumbel", "129"], "--gumbel 129"),
                      (["--record-visits", "--gumbel", "-1"], "--gumbel -1"),
                      (["--record-visits", "--gumbel", "4", "--gumbel-visit", "-1"], "--gumbel-visit"),
                      (["--record-visits", "--gumbel", "4", "--gumbel-scale", "nan"], "--gumbel-scale"),
                      (["--sims", "0"], "--sims 0"),
                      (["--sims", "32", "--fast-sims", "33"], "--fast-sims")):
        with pytest.raises(SystemExit) as e:
            manager.build_config(p.parse_args(["self"] + bad))
        assert word in str(e.value), (bad, str(e.value))
    with pytest.raises(SystemExit) as e:
        manager.build_config(p.parse_args(["eval", "--sims", "32"]))
    assert "--sims" in str(e.value)
