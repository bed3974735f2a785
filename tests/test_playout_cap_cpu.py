"""Playout cap randomization without a GPU: tests/playout_cap_oracle.py -- the yardstick of test_gpu_playout_cap.py --
is pinned to tests/selfplay_oracle.py where the two must agree, the per-ply lottery to the generator, the command line
to config.engine.

record_decoder.expand_records on four-element items is checked in tests/test_gpu_playout_cap.py, not here: the function
runs the package's rule kernels and returns device tensors, so it needs a GPU like every other test of it."""
import json
import os

import pytest

import playout_cap_oracle as pco
import selfplay_oracle as so
from oracle import xq_oracle as xo

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("init_state", "moves", "value", "turns", "store", "searched", "resigned", "final_state")


def _games():
    with open(os.path.join(GOLD, "games_k1.json")) as f:
        return json.load(f)["games"]


def _cfg_of_game(gm, K=1, sims=None):
    return xo.play_cfg(simulation_num_per_move=gm["sims"] if sims is None else sims, search_threads=K,
                       c_puct=gm.get("c_puct", 1.5), tau_decay_rate=gm["tau"], max_game_length=gm["max_game_length"],
                       enable_resign_rate=gm.get("enable_resign_rate", 1.0),
                       resign_threshold=gm.get("resign_threshold", -0.92), min_resign_turn=gm.get("min_resign_turn", 20))


def _fast_sims(gm):
    return max(2, gm["sims"] // 5)      # (a search of ONE simulation only expands its root: no visit, no move to choose)


@pytest.mark.parametrize("K", [1, 8])
def test_capped_oracle_identities(K):
    """Cap off and rate 1 are selfplay_game; rate 0 is selfplay_game of a configuration with simulation_num_per_move =
    fast_sims; a mixed schedule ends full plies at the full budget and fast plies at fast_sims, or above it where the
    reused root already had more."""
    games = _games()
    assert len(games) >= 15
    mixed_differs = above = 0
    for gm in games:
        if K > 1 and gm["sims"] >= 800:
            continue                    # (as in test_selfplay_oracle_cpu.py: the loop, not the search, is on trial)
        cfg, n = _cfg_of_game(gm, K), _fast_sims(gm)
        stub = {"kind": "hash", "salt": gm["salt"]}
        for game_id in (0, 3):
            base = so.selfplay_game(cfg, stub, gm["seed"], game_id)
            off = pco.capped_selfplay_game(cfg, stub, gm["seed"], game_id, 0, 0.25)
            one = pco.capped_selfplay_game(cfg, stub, gm["seed"], game_id, n, 1.0)
            for got in (off, one):
                assert {k: got[k] for k in KEYS} == base, (gm["name"], K, game_id)
                assert not any(got["fast"]) and got["idle_fast"] == 0
            small = so.selfplay_game(_cfg_of_game(gm, K, sims=n), stub, gm["seed"], game_id)
            zero = pco.capped_selfplay_game(cfg, stub, gm["seed"], game_id, n, 0.0)
            assert {k: zero[k] for k in KEYS} == small, (gm["name"], K, game_id)
            assert all(zero["fast"]) and len(zero["fast"]) == zero["searched"] + zero["resigned"]
            assert pco.move_flags(zero) == [True] * zero["searched"] + [False] * (zero["turns"] - zero["searched"])
            if gm["sims"] >= 800:
                continue
            trace = []
            mix = pco.capped_selfplay_game(cfg, stub, gm["seed"], game_id, n, 0.25, trace=trace)
            assert len(trace) == len(mix["fast"]) == mix["searched"] + mix["resigned"]
            assert mix["fast"] == [not pco.ply_is_full(gm["seed"], game_id, t, n, 0.25) for t in range(len(mix["fast"]))]
            for t, ply in enumerate(trace):
                if ply["no_act"] or ply["inc"]:
                    continue            # (bans / increase_temp restart the count: the root ends at carried + budget)
                if ply["fast"]:
                    assert ply["sum_n"] >= n, (gm["name"], K, game_id, t)
                    above += ply["sum_n"] > n
                else:
                    assert ply["sum_n"] == gm["sims"], (gm["name"], K, game_id, t)
            mixed_differs += mix["moves"] != base["moves"]
    assert mixed_differs > 0
    if K == 1:
        assert above > 0                # a fast ply whose reused root exceeded the budget


def test_capped_oracle_meets_the_idle_fast_ply():
    """The configuration test_gpu_playout_cap.py leans on: 200 / 40 simulations, hash stub, seed 11, K = 1 -- game ids 1
    and 2 hold fast plies that search nothing because the reused root already has more than 40 visits."""
    cfg = xo.play_cfg(simulation_num_per_move=200, search_threads=1, tau_decay_rate=0.98, max_game_length=12)
    idle, sums = 0, set()
    for gid in (1, 2):
        trace = []
        g = pco.capped_selfplay_game(cfg, dict(kind="hash", salt=5), 11, gid, 40, 0.25, trace=trace)
        idle += g["idle_fast"]
        sums |= {p["sum_n"] for p in trace if p["fast"]}
        assert all(p["sum_n"] == 200 for p in trace if not p["fast"] and not p["no_act"] and not p["inc"])
        assert any(g["fast"]) and not all(g["fast"])
    assert idle >= 1 and 40 in sums and max(sums) > 40


def test_capped_oracle_refuses_a_wrong_layout_and_bad_arguments():
    cfg = xo.play_cfg(simulation_num_per_move=8, search_threads=1, max_game_length=4)
    pl = xo.Player(cfg, dict(kind="hash", salt=1), seed=3, game_id=0)
    other = xo.play_cfg(simulation_num_per_move=9, search_threads=1, max_game_length=4)
    assert pco._player_cfg(pl, cfg).simulation_num_per_move == 8
    with pytest.raises(AssertionError):
        pco._player_cfg(pl, other)
    pl.close()
    with pytest.raises(ValueError):
        pco.capped_selfplay_game(cfg, dict(kind="hash", salt=1), 3, 0, 9, 0.5)
    noisy = xo.play_cfg(simulation_num_per_move=8, search_threads=1, max_game_length=4, noise_eps=0.25)
    with pytest.raises(ValueError):
        pco.capped_selfplay_game(noisy, dict(kind="hash", salt=1), 3, 0, 4, 0.5)


def test_lottery():
    def never(*a):
        raise AssertionError("rates 0 and 1, and a cap that is off, draw nothing")
    for t in range(50):
        assert pco.ply_is_full(7, 3, t, 40, 1.0, uniform=never)
        assert not pco.ply_is_full(7, 3, t, 40, 0.0, uniform=never)
        assert pco.ply_is_full(7, 3, t, 0, 0.25, uniform=never)
    pairs = [(g, t) for g in range(40) for t in range(100)]
    full = [p for p in pairs if pco.ply_is_full(7, p[0], p[1], 40, 0.25)]
    assert full == [p for p in pairs if xo.philox_uniform(7, p[0], 2, p[1]) < 0.25]
    assert 890 <= len(full) <= 1110          # 4000 * 0.25 = 1000, +- 4 standard deviations of sqrt(4000 * 3 / 16) = 27
    # stream 2 is a stream of its own: not the move choice's draws (stream 1), not the per-game lotteries' (stream 0)
    assert full != [p for p in pairs if xo.philox_uniform(7, p[0], 1, p[1]) < 0.25]


def test_command_line_flags():
    from cchess_alphazero import manager
    p = manager.create_parser()
    cfg = manager.build_config(p.parse_args(["self", "--fast-sims", "8", "--full-rate", "0.5"]))
    assert (cfg.engine.fast_sims, cfg.engine.full_rate) == (8, 0.5)
    cfg = manager.build_config(p.parse_args(["self", "--fast-sims", "8"]))
    assert (cfg.engine.fast_sims, cfg.engine.full_rate) == (8, 0.25)
    cfg = manager.build_config(p.parse_args(["self"]))
    assert (cfg.engine.fast_sims, cfg.engine.full_rate) == (0, 0.25)
    sims = cfg.play.simulation_num_per_move
    cfg = manager.build_config(p.parse_args(["self", "--fast-sims", str(sims), "--full-rate", "0"]))
    assert (cfg.engine.fast_sims, cfg.engine.full_rate) == (sims, 0.0)
    for bad, needle in ((["--fast-sims", "-1"], "--fast-sims"), (["--fast-sims", str(sims + 1)], "--fast-sims"),
                        (["--fast-sims", "8", "--full-rate", "1.5"], "--full-rate"),
                        (["--fast-sims", "8", "--full-rate", "-0.1"], "--full-rate")):
        with pytest.raises(SystemExit) as e:
            manager.build_config(p.parse_args(["self"] + bad))
        assert needle in str(e.value), bad


def test_config_defaults():
    from cchess_alphazero.config import Config
    for kind in ("mini", "normal"):
        ec = Config(kind).engine
        assert ec.fast_sims == 0 and ec.full_rate == 0.25
