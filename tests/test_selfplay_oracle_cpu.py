"""tests/selfplay_oracle.py -- the yardstick of the book tests -- proved before the GPU is compared with it:
from INIT_STATE it equals the oracle's C restatement of SelfPlayWorker.start_game (itself pinned to the reference's
recorded games, test_oracle_mcts.py), from other start positions it equals games recorded from the reference's own
start_game with senv.INIT_STATE set to them (tests/golden/book_games.json, make_golden_book.py)."""
import json
import os

import pytest

import selfplay_oracle as so
from oracle import xq_oracle as xo

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _golden(name):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)


def _cfg_of_game(gm, K=1):
    return xo.play_cfg(simulation_num_per_move=gm["sims"], search_threads=K, c_puct=gm.get("c_puct", 1.5),
                       tau_decay_rate=gm["tau"], max_game_length=gm["max_game_length"],
                       enable_resign_rate=gm.get("enable_resign_rate", 1.0),
                       resign_threshold=gm.get("resign_threshold", -0.92), min_resign_turn=gm.get("min_resign_turn", 20))


@pytest.mark.parametrize("K", [1, 8])
def test_restated_loop_equals_the_c_oracle_from_init_state(K):
    games = _golden("games_k1.json")["games"]
    assert len(games) >= 15
    for gm in games:
        if K > 1 and gm["sims"] >= 800:
            continue                    # (K = 8 needs no second 800-simulation game: the loop, not the search, is on trial)
        cfg = _cfg_of_game(gm, K)
        stub = {"kind": "hash", "salt": gm["salt"]}
        for game_id in (0, 3):
            a = xo.selfplay_game(cfg, stub, gm["seed"], game_id)
            b = so.selfplay_game(cfg, stub, gm["seed"], game_id)
            assert b["init_state"] == xo.INIT_STATE
            assert b["moves"] == a["moves"], (gm["name"], K, game_id)
            assert b["value"] == a["value"] and b["store"] == a["store"] and b["turns"] == a["turns"], (gm["name"], K)
        if K == 1:                      # ... and, at K = 1, the reference's own record
            r = so.selfplay_game(cfg, stub, gm["seed"], 0)
            assert (r["turns"], r["value"], r["store"]) == (gm["turns"], gm["value"], gm["store"]), gm["name"]
            if gm["record"] is not None:
                assert r["moves"] == [m for m, _ in gm["record"][1:]], gm["name"]


def test_restated_loop_equals_the_reference_from_book_positions():
    data = _golden("book_games.json")
    book = data["book"]
    assert len(book) >= 6
    assert '3s5/4m4/9/9/4p4/2R6/9/4C4/4M4/3MS4' in book and 'r1e1s1e1r/4m4/2k1c1k2/p1p1p1p1p/9/2P6/P3P1P1P/1CK1C1K2/9/R1EMSME1R' in book
    assert len(data["configs"]) == 2
    assert {c["stub"]["kind"] for c in data["configs"]} == {"hash", "uniform"}
    assert len({c["tau"] for c in data["configs"]}) == 2
    short = lottery_both = 0
    for c in data["configs"]:
        cfg = _cfg_of_game(c)
        stores = set()
        for gm in c["games"]:
            gid = gm["game_id"]
            assert gm["position"] == book[gid % len(book)]
            r = so.selfplay_game(cfg, c["stub"], c["seed"], gid, init_state=gm["position"])
            assert r["init_state"] == gm["position"]
            assert r["moves"] == gm["moves"], (c["name"], gid)
            assert (r["turns"], r["value"], r["store"]) == (gm["turns"], gm["value"], gm["store"]), (c["name"], gid)
            assert r["searched"] == gm["searched"] and r["final_state"] == gm["final_state"], (c["name"], gid)
            if gm["turns"] < 10:
                short += 1
                stores.add(gm["store"])
        lottery_both += stores == {True, False}
    assert short >= 4 and lottery_both >= 1        # the < 10 plies store lottery fell both ways


def test_book_lottery_draws_nothing_at_rates_0_and_1():
    assert not so.book_lottery(7, 3, 0.0) and so.book_lottery(7, 3, 1.0)
    hits = [g for g in range(400) if so.book_lottery(7, g, 0.5)]
    assert hits == [g for g in range(400) if xo.philox_uniform(7, g, 0, 2) < 0.5]
    assert 150 < len(hits) < 250
