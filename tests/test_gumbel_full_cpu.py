"""The full Gumbel search without a GPU: tests/gumbel_full_oracle.py -- the yardstick of test_gpu_gumbel_full.py -- is held
to hand-computed rows, to gumbel_oracle.Search where the two must agree (full off), and to the condition the GPU
comparison rests on: on the inputs of that comparison every selection at the root, every selection below it and every
played move is decided by at least 1e-9, far above what two libraries' exp and two orders of summation differ by.  The
command line is checked against config.engine."""
import math

import numpy as np
import pytest

import forced_playouts_oracle as fo
import gumbel_full_oracle as gf
import gumbel_oracle as go
from oracle import xq_oracle as xo

SIMS, M, SEED = 64, 16, 7               # test_gpu_gumbel_full.py's single searches
F32 = np.float32


# ---- the definitions against hand-computed rows ---------------------------------------------------------------------------
def test_one_edge():
    for n, w, v in ((0, 0.0, 0.3), (5, -2.5, -1.0), (1, 2.0, 1.0)):
        pick, sc, margin = gf.interior_pick([n], [w], [F32(1.0)], F32(v))
        assert pick == 0 and margin == gf.INF
        assert sc == [1.0 - n / (1.0 + n)]                      # pi' = 1
    assert gf.interior_pick([], [], [], F32(0.0))[0] == -1
    # a single edge of prior 0: pi' = 0, the score is -n / (1 + N)
    assert gf.interior_pick([3], [0.0], [F32(0.0)], F32(0.0))[1] == [-0.75]


def test_nothing_visited_is_the_normalised_prior():
    p = [F32(0.5), F32(0.25), F32(0.125), F32(0.125)]
    for v in (-1.0, 0.0, 0.7):
        for cv, cs in gf.PAIRS:
            assert gf.v_mix([0] * 4, [0.0] * 4, p, F32(v)) == (float(F32(v)) + 1.0) / 2.0
            pick, sc, margin = gf.interior_pick([0] * 4, [0.0] * 4, p, F32(v), cv, cs)
            assert sc == [0.5, 0.25, 0.125, 0.125] and pick == 0 and margin == 0.25
    # priors that do not sum to one are normalised; the greatest prior wins, the LATER edge on a tie
    pick, sc, margin = gf.interior_pick([0] * 3, [0.0] * 3, [F32(0.25), F32(0.5), F32(0.5)], F32(0.2))
    assert sc == [0.2, 0.4, 0.4] and pick == 2 and margin == 0.0
    t, raw = gf.target_v(np.arange(4, dtype=np.uint16), np.zeros(4, np.int32), np.zeros(4), np.array(p), F32(-0.4))
    assert t.tolist() == [32768, 16384, 8192, 8192] and raw == 0


def test_all_priors_zero_picks_the_least_n():
    n = [2, 1, 3, 1]
    pick, sc, margin = gf.interior_pick(n, [0.5, 0.1, -1.0, 0.3], [F32(0.0)] * 4, F32(0.5))
    assert sc == [-2 / 8.0, -1 / 8.0, -3 / 8.0, -1 / 8.0] and pick == 3 and margin == 0.0      # later on the tie
    t, raw = gf.target_v(np.arange(4, dtype=np.uint16), np.array(n, np.int32), np.zeros(4), np.zeros(4, F32), F32(0.5))
    assert t.tolist() == [0, 0, 0, 0] and raw == 7


def test_one_visited_edge_with_a_clamped_value():
    """Two edges of prior 1/2, edge 0 visited twice with q = +-2 (a terminal value), v = 0, c_visit = 0, c_scale = 1:
    max n = 2, sigma(x) = 2 x.  q = +2: q01 = 1, v_mix = (1/2 + 2 * 1) / 3 = 5/6, s = (2, 5/3), pi' = (1, e^(-1/3)) / T.
    q = -2: q01 = 0, v_mix = (1/2 + 0) / 3 = 1/6, s = (0, 1/3), pi' = (e^(-1/3), 1) / T."""
    p = [F32(0.5), F32(0.5)]
    a = math.exp(-1.0 / 3.0)
    for w, q01, vm, pi in ((4.0, 1.0, 5.0 / 6.0, (1.0 / (1.0 + a), a / (1.0 + a))),
                           (-4.0, 0.0, 1.0 / 6.0, (a / (1.0 + a), 1.0 / (1.0 + a)))):
        assert go.q01(2, w) == q01
        assert abs(gf.v_mix([2, 0], [w, 0.0], p, F32(0.0)) - vm) < 1e-15
        got = gf.improved_policy([2, 0], [w, 0.0], p, F32(0.0), 0.0, 1.0)
        assert max(abs(x - y) for x, y in zip(got, pi)) < 1e-15
        pick, sc, _ = gf.interior_pick([2, 0], [w, 0.0], p, F32(0.0), 0.0, 1.0)
        assert abs(sc[0] - (pi[0] - 2.0 / 3.0)) < 1e-15 and abs(sc[1] - pi[1]) < 1e-15 and pick == 1
    # the node's value is clamped as well: v = -3 reads as vhat = 0, v = 3 as 1
    assert gf.vhat(F32(-3.0)) == 0.0 and gf.vhat(F32(3.0)) == 1.0 and gf.vhat(F32(0.5)) == 0.75
    # a banned edge takes no part in the root's v_mix
    lab = np.array([1, 2 | gf.BANNED, 3], dtype=np.uint16)
    t, raw = gf.target_v(lab, np.array([2, 50, 0], np.int32), np.array([4.0, -50.0, 0.0]),
                         np.array([0.5, 0.25, 0.25], F32), F32(0.0), 0.0, 1.0)
    want = [x / (0.5 + 0.25 * a) for x in (0.5, 0.25 * a)]     # (sigma = max n over the live edges = 2)
    assert raw == 2 and t.tolist() == [int(math.floor(65536 * want[0] + 0.5)), 0, int(math.floor(65536 * want[1] + 0.5))]


# ---- full off is gumbel_oracle.Search ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def draws():
    return go.draws_for(SEED, 0, 0, 0)


@pytest.fixture(scope="module")
def runs(draws):
    return [(c, gf.run_case(c, M, SIMS, draws)) for c in fo.cases()]


@pytest.fixture(scope="module")
def root_only(draws):
    return [(c, go.run_case(c, M, SIMS, draws)) for c in fo.cases()]


def test_full_off_is_the_root_only_search_bit_for_bit(draws, root_only):
    n_searches = 0
    for c, (want, osearch) in root_only:
        got, s = gf.run_case(c, M, SIMS, draws, full=False)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            n_searches += 1
            assert a["state"] == b["state"] and a["no_act"] == b["no_act"] and a["best"] == b["best"]
            assert a["stats"]["sum_n"] == b["stats"]["sum_n"] and a["started"] == b["started"]
            assert a["seq_used"] == b["seq_used"] and a["margins"] == b["margins"] and a["in_margins"] == []
            for k in ("moves", "n", "w", "p"):
                assert a["stats"][k].tobytes() == b["stats"][k].tobytes(), (c["name"], k)
            assert (a["targets"] == b["targets"]).all() and a["raw_total"] == b["raw_total"]
        for key in ("sims", "expansions", "terminal_sims", "repetition_sims"):
            assert getattr(s, key) == getattr(osearch, key), (c["name"], key)
    assert n_searches == 10


def test_kept_values_are_the_stubs(runs):
    import stub_net
    for c, (res, _) in runs:
        for r in res:
            for state, v in ((r["state"], r["net_value"]), (r["child_state"], r["child_value"])):
                if v is None:
                    assert xo.done(state)[0]
                    continue
                want = stub_net.hash_stub_numpy(xo.state_to_planes(state)[None], c["salt"])[1][0]
                assert v.dtype == np.float32 and v == F32(want)


# ---- the condition the GPU comparison rests on -----------------------------------------------------------------------------
def test_margins_of_the_searches_carry_the_gpu_comparison(runs):
    """Every selection of the ten searches -- at the root, below it, the played move -- is decided by at least 1e-9: a
    score is a sum of a few terms of magnitude <= 1e2 (root) or <= 1 (below it), on which two float64 libraries and two
    orders of summation agree to ~1e-13.  A condition on the inputs, not a measurement."""
    least_in = least_root = gf.INF
    n = 0
    for c, (res, _) in runs:
        for r in res:
            n += 1
            assert len(r["in_margins"]) > 0, c["name"]
            assert min(r["in_margins"]) >= 1e-9, (c["name"], min(r["in_margins"]))
            assert min(r["margins"]) >= 1e-9 and r["best_margin"] >= 1e-9, (c["name"], min(r["margins"]), r["best_margin"])
            least_in = min(least_in, min(r["in_margins"]))
            least_root = min(least_root, min(r["margins"]), r["best_margin"])
    assert n == 10
    print(f"ten searches: least margin below the root {least_in:.3e}, at the root {least_root:.3e}")


def test_margins_of_the_games_carry_the_gpu_comparison():
    """The four self-play games of the GPU test (seed 13, salt 5, m = 8, 32 simulations, max_game_length = 3)."""
    from test_gpu_search import oracle_cfg, play_config
    pc = play_config(simulation_num_per_move=32, search_threads=1, noise_eps=0.0, tau_decay_rate=0.0, max_game_length=3,
                     enable_resign_rate=0.5, resign_threshold=-0.3, min_resign_turn=1)
    least_in = least_root = gf.INF
    for gid in range(4):
        g = gf.gumbel_selfplay_game(oracle_cfg(pc), 5, 13, gid, gid, 8)
        assert len(g["plies"]) > 0 and len(g["in_margins"]) > 0
        assert min(g["in_margins"]) >= 1e-9, (gid, min(g["in_margins"]))
        assert min(g["margins"]) >= 1e-9 and min(g["best_margins"], default=gf.INF) >= 1e-9, gid
        least_in = min(least_in, min(g["in_margins"]))
        least_root = min([least_root] + g["margins"] + g["best_margins"])
        # the full game differs from nothing it should not: the loop's bookkeeping is gumbel_oracle's
        assert g["searched"] == len(g["plies"]) or g["resigned"]
    print(f"four games: least margin below the root {least_in:.3e}, at the root {least_root:.3e}")


def test_margins_of_the_random_rows_carry_the_gpu_comparison():
    rows = gf.random_rows()
    assert len(rows) == 64 and [len(r["n"]) for r in rows[:7]] == [1, 2, 63, 64, 65, 127, 128]
    assert int(rows[7]["n"].sum()) == 0 and sum(len(r["n"]) > 64 for r in rows) > 8
    assert all(r["v"].dtype == np.float32 and -1.0 <= r["v"] <= 1.0 for r in rows)
    for cv, cs in gf.PAIRS:
        least = gf.INF
        for i, r in enumerate(rows):
            pick, sc, margin = gf.interior_pick(r["n"], r["w"], r["p"], r["v"], cv, cs)
            assert margin >= 1e-9, (i, cv, cs, margin)
            least = min(least, margin)
        print(f"64 rows at ({cv}, {cs}): least margin {least:.3e}")


def test_the_rule_is_exercised(runs, root_only):
    """In at least five of the ten searches the full search's root counts differ from the root-only Gumbel search's."""
    differ = 0
    for (_, (a, _)), (_, (b, _)) in zip(runs, root_only):
        for x, y in zip(a, b):
            if x["state"] == y["state"] and x["no_act"] == y["no_act"]:
                differ += x["stats"]["n"].tobytes() != y["stats"]["n"].tobytes()
            else:
                differ += 1                                     # (a ban or a reused line that already went another way)
    print(f"{differ} of 10 searches differ at the root")
    assert differ >= 5


def test_full_targets_follow_their_definition(runs):
    for c, (res, _) in runs:
        for r in res:
            st = r["stats"]
            lab = st["moves"].copy()
            banned = np.array([xo.label_str(int(l)) in r["no_act"] for l in lab])
            lab[banned] |= gf.BANNED
            t, raw = gf.target_v(lab, st["n"], st["w"], st["p"], r["net_value"])
            assert (t == r["targets"]).all() and raw == r["raw_total"] == int(st["n"][~banned].sum())
            assert abs(int(t.sum()) - 65536) <= int((~banned).sum()) and (t[banned] == 0).all(), c["name"]
            # c_scale = 0: sigma vanishes and with it v_mix: the target is the prior renormalised over the live edges
            t0, _ = gf.target_v(lab, st["n"], st["w"], st["p"], r["net_value"], 50.0, 0.0)
            assert (t0 == go.target(lab, st["n"], st["w"], st["p"], 50.0, 0.0)[0]).all()


# ---- run.py ----------------------------------------------------------------------------------------------------------------
def test_command_line(monkeypatch, tmp_path):
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    from cchess_alphazero import manager
    p = manager.create_parser()
    cfg = manager.build_config(p.parse_args(["self"]))
    assert cfg.engine.gumbel_full is False
    cfg = manager.build_config(p.parse_args(["self", "--record-visits", "--gumbel", "16", "--sims", "32"]))
    assert cfg.engine.gumbel == 16 and cfg.engine.gumbel_full is False
    cfg = manager.build_config(p.parse_args(["self", "--record-visits", "--gumbel", "16", "--gumbel-full", "--sims", "32"]))
    assert cfg.engine.gumbel == 16 and cfg.engine.gumbel_full is True and cfg.play.simulation_num_per_move == 32
    for bad in (["--gumbel-full"], ["--record-visits", "--gumbel-full"], ["--record-visits", "--gumbel", "0", "--gumbel-full"]):
        with pytest.raises(SystemExit) as e:
            manager.build_config(p.parse_args(["self"] + bad))
        assert "--gumbel-full needs --gumbel" in str(e.value), (bad, str(e.value))
