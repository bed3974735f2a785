"""-m gpu: the game loops on their rare endings -- advance_game (csrc/xq_search_selfplay.h, self-play) and the arena's host loop
(worker/evaluator.py, on the rule kernels) at max_game_length = 100, from the sparse endgame positions of
tests/golden/endgame_book.txt: the 120-plies-without-capture draw BEFORE the length cap, the "no attacking piece" draw,
three free repetitions, perpetual-check bans, the temperature bump, the length cap, and games of more than 64 plies, where
the device's repetition scan takes a second trip over the history (a match in block 0 after ply 64, a match at ply >= 64,
both in one scan).

Every comparison is exact.  K = 1 against games recorded from the reference's own workers (tests/golden/
endings_games.json), K > 1 against tests/selfplay_oracle.py / tests/arena_oracle.py, which
tests/test_endings_oracle_cpu.py pins to that record.  What the games of each run reach is asserted with the classifier
tests/game_endings.py (the coverage condition), so a changed salt cannot hollow a case out.  The network is the exact
stub of tests/stub_net.py."""
import json
import os

import numpy as np
import pytest

import game_endings as ge
import selfplay_oracle as so
import stub_net
from arena_oracle import arena_game, visit_crc
from game_endings import arena_moves, arena_pc, arena_u_fn, assert_trace_agrees
from oracle import xq_oracle as xo
from test_gpu_book import _assert_game, _moves, _pc_of, _play
from test_gpu_search import gpu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = 32                      # slots: slot g's first game is game id g


def _gold():
    with open(os.path.join(GOLDEN, "endings_games.json")) as f:
        return json.load(f)


def _drained(ids):
    return lambda games: set(ids) <= {g["game_id"] for g in games}


def _assert_counters(ctr, games, results):
    """The counters over a run whose every finished game was drained, against the classifier's reading of those games."""
    assert ctr["games"] == len(games)
    assert ctr["games"] == ctr["red_wins"] + ctr["black_wins"] + ctr["draws"]
    assert ctr["draws"] == sum(1 for k in results if k["ending"] in ge.DRAWS)
    assert ctr["red_wins"] == sum(1 for k in results if k["value"] > 0)
    assert ctr["black_wins"] == sum(1 for k in results if k["value"] < 0)
    assert ctr["resigns"] == sum(1 for k in results if k["ending"] == "resign")
    assert ctr["no_act_truncated"] == 0 and ctr["tree_resets"] == 0 and ctr["overflow_sims"] == 0


def _classified(games, book, pc):
    """classify() of every drained game from the engine's own record; value and turns must be what the record says."""
    out = {}
    for g in games:
        k = ge.classify(book[g["book_index"]], _moves(g), pc.max_game_length)
        assert (k["turns"], k["value"], k["ending"] == "resign") == (g["turns"], g["value"], g["resigned"]), g["game_id"]
        out[g["game_id"]] = k
    return out


def test_endgame_book_loads_on_the_rule_kernels(gpu, tmp_path):
    from cchess_alphazero.lib.book import load_book
    assert load_book(os.path.join(GOLDEN, "endgame_book.txt")) == _gold()["book"]
    # an elephant where no elephant stands is refused by the parser: the rule kernels never see the position
    p = tmp_path / "bad.txt"
    p.write_text("3s1e3/4m4/4e4/9/r8/6K2/9/4E3R/4M4/2E1S4\n")
    with pytest.raises(ValueError, match="elephant 'e' in row 1, file 6"):
        load_book(str(p))


# ---- self-play, K = 1: the reference's record ----------------------------------------------------------------------------
def test_selfplay_reproduces_the_reference_games_at_K_1(gpu):
    gold = _gold()
    book, (c,) = gold["book"], gold["configs"]
    ref = {g["game_id"]: g for g in c["games"]}
    assert set(ref) <= set(range(G))
    pc = _pc_of(c)
    games, ctr = _play(gpu, pc, c["stub"], G, c["seed"], book, stop=_drained(ref), record_visits=True)
    assert ctr["visits_dropped"] == 0
    got = {g["game_id"]: g for g in games}
    for gid, r in ref.items():
        g = got[gid]
        assert r["position"] == book[gid % len(book)]
        _assert_game(g, r, book[gid % len(book)], gid % len(book), gid)
        assert g["resigned"] is False
        # what the reference's loop handed to each search, and the visit counts that search left (one entry per action())
        vis = g["visits"]
        assert vis is not None and len(vis) == len(r["plies"]), gid
        for t, (e, p) in enumerate(zip(vis, r["plies"])):
            assert (e.ply, e.sum_n, visit_crc(e.moves, e.n)) == (t, p["sum_n"], p["crc"]), (gid, t)
            assert sorted(xo.label_str(int(m)) for m in e.moves[e.banned]) == sorted(set(p["no_act"])), (gid, t)
    klass = _classified(games, book, pc)
    ge.assert_coverage([klass[gid] for gid in ref])
    _assert_counters(ctr, games, list(klass.values()))


# ---- self-play, K > 1: the restated loop, ply by ply -----------------------------------------------------------------------
@pytest.mark.parametrize("K,salt,c_puct,hist,ids", ge.SELFPLAY_CASES)
def test_selfplay_matches_the_oracle_ply_by_ply(gpu, K, salt, c_puct, hist, ids):
    """The runs, their game ids and what those games reach: tests/game_endings.py SELFPLAY_CASES (the device plays all 32
    slots; the oracle replays the ids that carry the coverage condition, the classifier reads every drained game)."""
    gold = _gold()
    book, (c,) = gold["book"], gold["configs"]
    stub, seed = dict(kind="hash", salt=salt), c["seed"]
    pc = _pc_of(c, K=K, simulation_num_per_move=ge.SELFPLAY_SIMS, c_puct=c_puct)
    games, ctr = _play(gpu, pc, stub, G, seed, book, stop=_drained(ids), record_visits=True, use_history=hist)
    assert ctr["visits_dropped"] == 0
    cfg = so.oracle_cfg(pc, use_history=hist)
    klass = _classified(games, book, pc)
    oracle_klass = {}
    got = {g["game_id"]: g for g in games}
    for gid in ids:
        g = got[gid]
        init = book[gid % len(book)]
        trace = []
        ref = so.selfplay_game(cfg, stub, seed, gid, init_state=init, trace=trace)
        _assert_game(g, ref, init, gid % len(book), (K, gid))
        assert g["resigned"] == ref["resigned"], gid
        # every search of the game: the root's moves, visit counts and banned edges, as the move was chosen
        vis = g["visits"]
        assert vis is not None and len(vis) == len(trace), (gid, None if vis is None else len(vis), len(trace))
        for t, (e, r) in enumerate(zip(vis, trace)):
            assert e.ply == t and e.sum_n == r["sum_n"], (gid, t, e.sum_n, r["sum_n"])
            assert np.array_equal(e.moves, r["moves"]) and np.array_equal(e.n, r["n"]), (gid, t)
            assert sorted(xo.label_str(int(m)) for m in e.moves[e.banned]) == sorted(set(r["no_act"])), (gid, t)
        k = ge.classify(init, ref["moves"], pc.max_game_length)
        assert_trace_agrees(k, trace, gid)
        assert k["ending"] == klass[gid]["ending"], gid
        oracle_klass[gid] = k
    ge.assert_coverage([oracle_klass[gid] for gid in ids])
    _assert_counters(ctr, games, list(klass.values()))


# ---- arena -----------------------------------------------------------------------------------------------------------------
def _arena(gpu, a, K, indices, starts, tmp_path, monkeypatch):
    from cchess_alphazero.config import Config
    from cchess_alphazero.worker.evaluator import EvaluateWorker
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    cfg = Config("mini")
    for k, v in vars(arena_pc(a, K)).items():
        setattr(cfg.play, k, v)
    cfg.opts.evaluate = True
    evs = tuple((lambda planes, s=s: stub_net.hash_stub_torch(planes, s)) for s in a["salts"])
    trace = {}
    got = EvaluateWorker(cfg, evaluators=evs, seed=5).play_games(len(indices), u_fn=arena_u_fn(a["seed"]),
                                                                 indices=indices, init_state=starts, trace=trace)
    return got, trace


def _assert_arena_trace(got, ref, what):
    """One game's device trace against the reference's / the oracle's: state, action, visit fingerprint, bans, inc."""
    assert len(got) == len(ref), (what, len(got), len(ref))
    for t, (e, r) in enumerate(zip(got, ref)):
        assert (e["state"], e["action"], e["sum_n"]) == (r["state"], r["action"], r["sum_n"]), (what, t)
        assert visit_crc(e["moves"], e["n"]) == r["crc"], (what, t)
        assert e["no_act"] == r["no_act"] and e["inc"] == r["inc"], (what, t, e["no_act"], r["no_act"])


def test_arena_reproduces_the_reference_games_at_K_1(gpu, tmp_path, monkeypatch):
    """With config.opts.evaluate an increase_temp ply restarts the search from zero visits and still plays the argmax:
    the flag is pinned here through sum_n and the visit fingerprint, not through temperature sampling."""
    gold = _gold()
    a = gold["arena"]
    indices = [g["idx"] for g in a["games"]]
    got, trace = _arena(gpu, a, 1, indices, [g["init_state"] for g in a["games"]], tmp_path, monkeypatch)
    assert got == [(g["value"], g["turns"]) for g in a["games"]]
    results = []
    for g in a["games"]:
        _assert_arena_trace(trace[g["idx"]], g["plies"], g["idx"])
        results.append(ge.classify(g["init_state"], g["moves"], a["max_game_length"], arena=True))
    ge.assert_coverage(results, both=False)


def test_arena_matches_the_oracle_at_K_8(gpu, tmp_path, monkeypatch):
    """The run, its game indices and what those games reach: tests/game_endings.py ARENA_K8, ARENA_K8_INDICES."""
    from cchess_alphazero.worker.evaluator import book_states
    gold = _gold()
    book = gold["book"]
    a = dict(gold["arena"], **ge.ARENA_K8)
    indices = list(ge.ARENA_K8_INDICES)
    starts = dict(zip(indices, book_states(book, indices)))
    got, trace = _arena(gpu, a, 8, indices, [starts[i] for i in indices], tmp_path, monkeypatch)
    got = dict(zip(indices, got))
    specs = tuple(dict(kind="hash", salt=x) for x in a["salts"])
    results = []
    for i in indices:
        ref = []
        value, turns, _ = arena_game(i, arena_pc(a, 8), specs, arena_u_fn(a["seed"]), init_state=starts[i], evaluate=True,
                                     trace=ref)
        assert got[i] == (value, turns), i
        _assert_arena_trace(trace[i], ref, i)
        k = ge.classify(starts[i], arena_moves(starts[i], ref, turns), a["max_game_length"], arena=True)
        assert (k["value"], k["turns"]) == (value, turns), (i, k["ending"])
        assert_trace_agrees(k, ref, i)
        results.append(k)
    ge.assert_coverage(results, both=False)
