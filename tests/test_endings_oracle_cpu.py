"""The yardsticks of tests/test_gpu_endings.py, proved before the GPU is compared with them.

tests/golden/endings_games.json holds games recorded from the reference's own SelfPlayWorker.start_game and
EvaluateWorker.start_game (K = 1) from the sparse endgame positions of tests/golden/endgame_book.txt, at
max_game_length = 100 -- long enough for the 120-plies-without-capture draw to come before the length cap, and for the
repetition checks to look back over more than 64 plies.  tests/selfplay_oracle.py and tests/arena_oracle.py must
reproduce every one of them; the classifier tests/game_endings.py must agree with the reference's record and with the
oracles' traces on every ply; and the recorded games must reach the endings they were recorded for (the coverage
condition, asserted)."""
import json
import os

import pytest

import game_endings as ge
from game_endings import arena_moves, arena_pc, arena_u_fn, assert_trace_agrees, selfplay_cfg
import selfplay_oracle as so
from arena_oracle import arena_game, visit_crc
from oracle import xq_oracle as xo

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _golden(name="endings_games.json"):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)


def test_endgame_book_is_the_book_of_the_golden_games():
    from cchess_alphazero.lib.book import load_book
    gold = _golden()
    book = load_book(os.path.join(GOLD, "endgame_book.txt"), rules=xo)
    assert book == gold["book"] and len(book) == 4
    assert book[2] in _golden("book_games.json")["book"]


def test_selfplay_oracle_reproduces_the_recorded_games_and_the_classifier_agrees():
    """Recorded with salt 8 (seed 4242, sims 10, K = 1); the classifier's counts over the 13 recorded games:
    no_eat120 3, free3 2, no_attack 2, length 2, mate 2, king_capture 2; block0_late 2, block1 7, both 1; 4 plies with a
    ban, 58 plies with increase_temp handed to a search that moved.  (Salt 2 of the same run has one no_attack game only.)"""
    gold = _golden()
    book = gold["book"]
    (c,) = gold["configs"]
    assert c["max_game_length"] == 100 and c["tau"] == 0.9
    assert 12 <= len(c["games"]) <= 16
    cfg = selfplay_cfg(c)
    results = []
    for gm in c["games"]:
        gid = gm["game_id"]
        assert gm["position"] == book[gid % len(book)]
        trace = []
        r = so.selfplay_game(cfg, c["stub"], c["seed"], gid, init_state=gm["position"], trace=trace)
        assert r["moves"] == gm["moves"], gid
        assert (r["turns"], r["value"], r["store"]) == (gm["turns"], gm["value"], gm["store"]), gid
        assert r["searched"] == gm["searched"] and r["final_state"] == gm["final_state"], gid
        assert not r["resigned"]
        # ... and what the reference's loop handed to every search, with the visit counts that search left behind
        assert len(trace) == len(gm["plies"]), gid
        for t, (e, p) in enumerate(zip(trace, gm["plies"])):
            assert (e["action"], e["no_act"], e["inc"], e["sum_n"]) == (p["action"], p["no_act"], p["inc"], p["sum_n"]), (gid, t)
            assert visit_crc(e["moves"], e["n"]) == p["crc"], (gid, t)
        k = ge.classify(gm["position"], gm["moves"], c["max_game_length"])
        assert (k["turns"], k["value"], k["searched"], k["final_state"]) == \
            (gm["turns"], gm["value"], gm["searched"], gm["final_state"]), (gid, k["ending"])
        assert [(b, i) for b, i in zip(k["bans"], k["inc"])] == [(p["no_act"], p["inc"]) for p in gm["plies"]], gid
        assert_trace_agrees(k, trace, gid)
        assert (k["value"] == 0) == (k["ending"] in ge.DRAWS), gid
        results.append(k)
    n = ge.assert_coverage(results)
    assert n == dict(no_eat120=3, free3=2, no_attack=2, length=2, mate=2, king_capture=2, resign=0, block0_late=2,
                     block1=7, both=1, ban_plies=4, inc_sampled=58), n


def test_arena_oracle_reproduces_the_recorded_games_and_the_classifier_agrees():
    """Recorded with salts (36, 136), seed 5036, sims 10, evaluate = True, K = 1; the classifier's counts over the 8
    recorded games: no_eat120 2, free3 2, no_attack 2, length 1, mate 1; block0_late 2, block1 6; 2 plies with a ban, 69
    plies with increase_temp handed to a search that moved.  With config.opts.evaluate such a ply restarts the search from
    zero visits (sum_n, the visit fingerprint) and still plays the argmax: the flag is pinned through the visit counts,
    not through temperature sampling (tests/golden/arena_k1.json has the sampled kind, end_inc)."""
    gold = _golden()
    book, a = gold["book"], gold["arena"]
    assert a["max_game_length"] == 100 and a["evaluate"] is True
    assert 6 <= len(a["games"]) <= 8
    specs = tuple(dict(kind="hash", salt=x) for x in a["salts"])
    results = []
    for gm in a["games"]:
        idx = gm["idx"]
        assert gm["init_state"] == book[(idx // 2) % len(book)]
        trace = []
        value, turns, evals = arena_game(idx, arena_pc(a), specs, arena_u_fn(a["seed"]), init_state=gm["init_state"],
                                         evaluate=True, trace=trace)
        assert (value, turns) == (gm["value"], gm["turns"]), idx
        assert len(trace) == len(gm["plies"]), idx
        for t, (e, p) in enumerate(zip(trace, gm["plies"])):
            assert (e["state"], e["action"], e["crc"], e["sum_n"]) == (p["state"], p["action"], p["crc"], p["sum_n"]), (idx, t)
            assert e["no_act"] == p["no_act"] and e["inc"] == p["inc"], (idx, t)
        assert evals == gm["nn_positions"], idx
        assert arena_moves(gm["init_state"], trace, turns) == gm["moves"], idx
        k = ge.classify(gm["init_state"], gm["moves"], a["max_game_length"], arena=True)
        assert (k["turns"], k["value"], k["searched"]) == (gm["turns"], gm["value"], gm["searched"]), (idx, k["ending"])
        assert_trace_agrees(k, gm["plies"], idx)
        assert_trace_agrees(k, trace, idx)
        results.append(k)
    n = ge.assert_coverage(results, both=False)
    assert n == dict(no_eat120=2, free3=2, no_attack=2, length=1, mate=1, king_capture=0, resign=0, block0_late=2,
                     block1=6, ban_plies=2, inc_sampled=69), n


# ---- the runs of tests/test_gpu_endings.py at K > 1 (game_endings.SELFPLAY_CASES, ARENA_K8) ------------------------------
@pytest.mark.parametrize("K,salt,c_puct,hist,ids", ge.SELFPLAY_CASES)
def test_selfplay_runs_of_the_gpu_test_meet_the_coverage_condition(K, salt, c_puct, hist, ids):
    """The classifier over the game ids of each run (no_eat120 / free3 / no_attack / length / mate / king_capture;
    block0_late / block1 / both; ban plies; increase_temp plies):
        K=8 salt 43:          2 / 2 / 2 / 1 / 1 / 1;  2 / 3 / 1;  2;  28
        K=3 salt 25:          2 / 2 / 2 / 1 / 1 / 1;  2 / 5 / 2;  2;  50
        K=8 salt 17, history: 2 / 2 / 2 / 1 / 1 / 1;  2 / 5 / 1;  2;  40"""
    gold = _golden()
    book, (c,) = gold["book"], gold["configs"]
    cfg = selfplay_cfg(dict(c, sims=ge.SELFPLAY_SIMS, c_puct=c_puct), K, hist)
    results = []
    for gid in ids:
        trace = []
        r = so.selfplay_game(cfg, dict(kind="hash", salt=salt), c["seed"], gid, init_state=book[gid % len(book)], trace=trace)
        k = ge.classify(book[gid % len(book)], r["moves"], c["max_game_length"])
        assert (k["turns"], k["value"], k["searched"], k["final_state"]) == \
            (r["turns"], r["value"], r["searched"], r["final_state"]), (gid, k["ending"])
        assert_trace_agrees(k, trace, gid)
        assert max(len(b) for b in k["bans"]) <= 1          # (a ban list of two moves: not reached, see the issue)
        results.append(k)
    n = ge.assert_coverage(results)
    expect = {(8, 43): (2, 2, 2, 1, 1, 1, 2, 3, 1, 2, 28), (3, 25): (2, 2, 2, 1, 1, 1, 2, 5, 2, 2, 50),
              (8, 17): (2, 2, 2, 1, 1, 1, 2, 5, 1, 2, 40)}[(K, salt)]
    assert tuple(n[x] for x in ("no_eat120", "free3", "no_attack", "length", "mate", "king_capture", "block0_late",
                                "block1", "both", "ban_plies", "inc_sampled")) == expect, n


def test_arena_run_of_the_gpu_test_meets_the_coverage_condition():
    """Salts (42, 142), seed 5042, c_puct 0.5, 16 simulations, K = 8; the classifier over the games: no_eat120 2, free3 2, no_attack 2,
    length 1, mate 1, king_capture 1; block0_late 2, block1 3; 2 ban plies, 43 increase_temp plies.
    With config.opts.evaluate an increase_temp ply restarts the search (sum_n) and still plays the argmax: these games pin
    the flag through the visit counts, not through temperature sampling."""
    gold = _golden()
    book, a = gold["book"], dict(gold["arena"], **ge.ARENA_K8)
    specs = tuple(dict(kind="hash", salt=x) for x in a["salts"])
    results = []
    for i in ge.ARENA_K8_INDICES:
        init = book[(i // 2) % len(book)]
        trace = []
        value, turns, _ = arena_game(i, arena_pc(a, 8), specs, arena_u_fn(a["seed"]), init_state=init, evaluate=True,
                                     trace=trace)
        k = ge.classify(init, arena_moves(init, trace, turns), a["max_game_length"], arena=True)
        assert (k["value"], k["turns"]) == (value, turns), (i, k["ending"])
        assert_trace_agrees(k, trace, i)
        results.append(k)
    n = ge.assert_coverage(results, both=False)
    assert n == dict(no_eat120=2, free3=2, no_attack=2, length=1, mate=1, king_capture=1, resign=0, block0_late=2,
                     block1=3, ban_plies=2, inc_sampled=43), n


def test_c_restatement_stays_pinned_from_the_opening_position():
    """xo.selfplay_game takes no start state: it stays pinned where it is pinned today (games_k1.json, from INIT_STATE),
    and the classifier reads the same endings out of the moves it returns."""
    games = _golden("games_k1.json")["games"]
    seen = set()
    for gm in games:
        if gm["sims"] >= 800:
            continue
        cfg = xo.play_cfg(simulation_num_per_move=gm["sims"], search_threads=1, c_puct=gm.get("c_puct", 1.5),
                          tau_decay_rate=gm["tau"], max_game_length=gm["max_game_length"],
                          enable_resign_rate=gm.get("enable_resign_rate", 1.0),
                          resign_threshold=gm.get("resign_threshold", -0.92), min_resign_turn=gm.get("min_resign_turn", 20))
        stub = {"kind": "hash", "salt": gm["salt"]}
        a = xo.selfplay_game(cfg, stub, gm["seed"], 0)
        assert (a["turns"], a["value"], a["store"]) == (gm["turns"], gm["value"], gm["store"]), gm["name"]
        k = ge.classify(xo.INIT_STATE, a["moves"], gm["max_game_length"])
        assert (k["turns"], k["value"]) == (gm["turns"], gm["value"]), (gm["name"], k["ending"])
        assert [(b, i) for b, i in zip(k["bans"], k["inc"])] == [(p["no_act"], p["inc"]) for p in gm["plies"]], gm["name"]
        seen.add(k["ending"])
        assert not (k["block0_late"] or k["block1"])            # (what these games never reach)
    assert {"length", "king_capture", "resign"} <= seen and not seen & {"no_eat120", "no_attack"}


def test_classifier_flags_and_rejections():
    s = [dict(ply=64, matches=[60]), dict(ply=65, matches=[3]), dict(ply=70, matches=[66]), dict(ply=90, matches=[10, 64])]
    assert ge.scan_flags(s[:1]) == dict(block0_late=False, block1=False, both=False)     # 64 plies: one trip still
    assert ge.scan_flags(s[1:2]) == dict(block0_late=True, block1=False, both=False)
    assert ge.scan_flags(s[2:3]) == dict(block0_late=False, block1=True, both=False)
    assert ge.scan_flags(s[1:3]) == dict(block0_late=True, block1=True, both=False)      # two scans, not one
    assert ge.scan_flags(s[3:]) == dict(block0_late=True, block1=True, both=True)
    gm = _golden()["configs"][0]["games"][0]
    with pytest.raises(ValueError):                          # a finished game goes on
        ge.classify(gm["position"], gm["moves"] + gm["moves"][-1:], 100)
    with pytest.raises(ValueError):                          # the king capture is missing
        ge.classify(gm["position"], gm["moves"][:-1], 100)
    short = ge.classify(gm["position"], gm["moves"][:10], 100)
    assert short["ending"] == "resign" and short["value"] == -1 and len(short["states"]) == 11
