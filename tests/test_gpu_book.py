"""-m gpu: self-play and arena games from a start-position book (cz_search_set_book, run.py self / eval --book).

The device game loop is compared, game by game and with no tolerance, with games recorded from the reference's own
SelfPlayWorker.start_game whose senv.INIT_STATE was set to the book positions (tests/golden/book_games.json, K = 1) and
with tests/selfplay_oracle.py (K = 8, history planes, the book-rate lottery), which tests/test_selfplay_oracle_cpu.py
pins to both.  The network is the exact stub of tests/stub_net.py, as in test_gpu_search.py.  "Red" is the side that
moves first from the book position."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import selfplay_oracle as so
import stub_net
from oracle import xq_oracle as xo
from test_gpu_search import gpu, play_config, stub_eval  # noqa: F401  (gpu: fixture)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gold():
    with open(os.path.join(GOLDEN, "book_games.json")) as f:
        return json.load(f)


def _pc_of(c, K=1, **kw):
    d = dict(simulation_num_per_move=c["sims"], search_threads=K, c_puct=c["c_puct"], tau_decay_rate=c["tau"],
             max_game_length=c["max_game_length"], enable_resign_rate=c["enable_resign_rate"],
             resign_threshold=c["resign_threshold"], min_resign_turn=c["min_resign_turn"])
    d.update(kw)
    return play_config(**d)


def _engine_cfg(pc, **engine):
    from cchess_alphazero.config import Config
    cfg = Config("mini")
    for k, v in vars(pc).items():
        setattr(cfg.play, k, v)
    for k, v in engine.items():
        setattr(cfg.engine, k, v)
    return cfg


def _play(gpu, pc, spec, G, seed, book, rate=1.0, stop=None, max_rounds=60000, every=16, **kw):
    """Self-play through SelfPlayEngine with a stub evaluator; returns every drained game, in drain order, and the
    counters.  stop(games) -> True ends the run (checked at every drain); default: each slot has finished two games."""
    from cchess_alphazero.engine import SelfPlayEngine
    eng = SelfPlayEngine(_engine_cfg(pc), G, evaluator=stub_eval(gpu, spec), seed=seed, book=book, book_rate=rate, **kw)
    games = []
    if stop is None:
        def stop(gs):
            return min(sum(1 for g in gs if g["game_id"] % G == s) for s in range(G)) >= 2
    try:
        eng.start(0, 0)
        for r in range(max_rounds):
            eng.step()
            if r % every == every - 1:
                games += eng.drain()
                if stop(games):
                    break
        else:
            raise AssertionError(f"not finished after {max_rounds} rounds: {len(games)} games")
        ctr = eng.counters()
    finally:
        eng.close()
    assert ctr["tree_resets"] == 0 and ctr["overflow_sims"] == 0
    assert len({g["game_id"] for g in games}) == len(games)
    return games, ctr


def _moves(g):
    return [item[0] for item in g["data"][1:]]


def _assert_game(g, ref, init_state, book_index, what):
    assert g["data"][0] == init_state, what
    assert g["book_index"] == book_index, what
    assert _moves(g) == ref["moves"], (what, _moves(g), ref["moves"])
    assert (g["turns"], g["value"], g["store"]) == (ref["turns"], int(ref["value"]), ref["store"]), what
    v = g["value"]
    assert [item[1] for item in g["data"][1:]] == [v if i % 2 == 0 else -v for i in range(g["turns"])], what


def _two_per_slot_and_position(G, n):
    def stop(gs):
        slots = [sum(1 for g in gs if g["game_id"] % G == s) for s in range(G)]
        pos = [sum(1 for g in gs if g["book_index"] == p) for p in range(n)]
        return min(slots) >= 2 and min(pos) >= 2
    return stop


# ---- 1. parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 1])
def test_book_selfplay_reproduces_the_reference_games(gpu, ci):
    """rate = 1, K = 1: every drained game is the reference's own start_game from that book position, for its game id."""
    gold = _gold()
    book, c = gold["book"], gold["configs"][ci]
    ref = {g["game_id"]: g for g in c["games"]}
    G, n = 4, len(book)
    games, ctr = _play(gpu, _pc_of(c), c["stub"], G, c["seed"], book, stop=_two_per_slot_and_position(G, n))
    assert len(games) >= 2 * G
    for g in games:
        gid = g["game_id"]
        assert gid in ref, f"game {gid} is beyond the recorded ids: record more in make_golden_book.py"
        assert ref[gid]["position"] == book[gid % n]
        _assert_game(g, ref[gid], book[gid % n], gid % n, (c["name"], gid))
    assert ctr["games"] >= len(games)
    # the counters read "red" as the first mover: they add up over the finished games that were drained and those that were not
    assert ctr["red_wins"] + ctr["black_wins"] + ctr["draws"] == ctr["games"]


@pytest.mark.parametrize("ci,K", [(0, 8), (1, 8), (0, 3)])
def test_book_selfplay_matches_the_restated_oracle_at_K_gt_1(gpu, ci, K):
    gold = _gold()
    book, c = gold["book"], gold["configs"][ci]
    pc = _pc_of(c, K=K)
    G, n = 5, len(book)
    games, _ = _play(gpu, pc, c["stub"], G, c["seed"], book, stop=_two_per_slot_and_position(G, n))
    cfg = so.oracle_cfg(pc)
    for g in games:
        gid = g["game_id"]
        ref = so.selfplay_game(cfg, c["stub"], c["seed"], gid, init_state=book[gid % n])
        _assert_game(g, ref, book[gid % n], gid % n, (c["name"], K, gid))
        assert g["resigned"] == ref["resigned"]


# ---- 2. the book-rate lottery ------------------------------------------------------------------------------------------
def test_book_rate_lottery(gpu):
    gold = _gold()
    book, c = gold["book"], gold["configs"][0]
    pc = _pc_of(c, K=4, max_game_length=10)
    G, n, seed = 6, len(book), 777
    games, _ = _play(gpu, pc, c["stub"], G, seed, book, rate=0.5)
    assert len(games) >= 2 * G
    from_book = {g["game_id"] for g in games if g["book_index"] is not None}
    expect = {g["game_id"] for g in games if stub_net.philox_uniform(seed, g["game_id"], 0, 2) < 0.5}
    assert from_book == expect and 0 < len(from_book) < len(games)
    cfg = so.oracle_cfg(pc)
    for g in games:
        gid = g["game_id"]
        init = book[gid % n] if gid in expect else xo.INIT_STATE
        ref = so.selfplay_game(cfg, c["stub"], seed, gid, init_state=init)
        _assert_game(g, ref, init, gid % n if gid in expect else None, gid)


def _raw_records(gpu, pc, spec, G, seed, rounds, setup):
    """The record ring's bytes and the counters after a fixed number of rounds."""
    s = gpu.S.Search(pc, G, seed=seed)
    setup(s)
    ev = stub_eval(gpu, spec)
    s.start_selfplay(seed=seed, first_game_id=0)
    for _ in range(rounds):
        s.round()
        p, v = ev(s.planes)
        s.policy.copy_(p)
        s.value.copy_(v)
    buf = np.zeros((4096, s.record_stride), dtype=np.uint8)
    n = C.c_int(0)
    cur = C.c_uint(0)
    gpu.N.check(s.L.cz_search_drain_records(s.h, C.byref(cur), buf.ctypes.data, 4096, C.byref(n), s._stream()), "drain")
    ctr = s.counters()
    s.close()
    # a record = its 16-byte header and the `turns` moves it holds; games that end in one launch reach the ring in any order
    recs = []
    for i in range(n.value):
        turns = int(buf[i, 4:8].view(np.int32)[0])
        recs.append(buf[i, :16 + 2 * turns].tobytes())
    recs.sort(key=lambda b: int.from_bytes(b[:4], "little"))
    return recs, {k: ctr[k] for k in ("games", "plies", "sims", "expansions", "red_wins", "black_wins", "draws", "resigns")}


def test_rate_0_and_an_empty_book_change_nothing(gpu):
    gold = _gold()
    boards = np.stack([xo.state_to_board(s) for s in gold["book"]])
    pc = play_config(simulation_num_per_move=16, search_threads=4, tau_decay_rate=0.9, max_game_length=8,
                     enable_resign_rate=0.5, resign_threshold=-0.4, min_resign_turn=4)
    spec = dict(kind="hash", salt=5)
    base, ctr0 = _raw_records(gpu, pc, spec, 8, 31, 400, lambda s: None)
    assert len(base) >= 16
    rate0, ctr1 = _raw_records(gpu, pc, spec, 8, 31, 400, lambda s: s.set_book(boards, 0.0))
    empty, ctr2 = _raw_records(gpu, pc, spec, 8, 31, 400, lambda s: (s.set_book(boards, 1.0), s.set_book(None)))
    assert rate0 == base and empty == base
    assert ctr0 == ctr1 and ctr0 == ctr2
    # ... and the book does: same seed, rate 1
    with_book, _ = _raw_records(gpu, pc, spec, 8, 31, 400, lambda s: s.set_book(boards, 1.0))
    assert with_book != base


# ---- 3. visit records --------------------------------------------------------------------------------------------------
def test_first_visit_entry_lists_the_book_positions_moves(gpu):
    gold = _gold()
    book, c = gold["book"], gold["configs"][0]
    pc = _pc_of(c, K=4, max_game_length=8)
    G, n = 4, len(book)
    games, _ = _play(gpu, pc, c["stub"], G, 11, book, record_visits=True, stop=_two_per_slot_and_position(G, n))
    seen = set()
    for g in games:
        assert g["visits"] is not None, g["game_id"]
        first = g["visits"][0]
        legal = xo.get_legal_moves(book[g["book_index"]])
        assert [xo.label_str(int(m)) for m in first.moves] == legal, g["game_id"]
        assert first.ply == 0 and first.sum_n == pc.simulation_num_per_move
        if len(g["data"][1]) == 3:                          # the record's pi of ply 0 names moves of the book position
            assert {m for m, _ in g["data"][1][2]} <= set(legal)
        seen.add(g["book_index"])
    assert seen == set(range(n))


# ---- 4. history planes -------------------------------------------------------------------------------------------------
def test_book_games_with_history_planes(gpu):
    """28 input planes: the root of ply 0 has no history (second block zero), as in a game from INIT_STATE."""
    gold = _gold()
    book, c = gold["book"], gold["configs"][0]
    pc = _pc_of(c, K=4, max_game_length=10)
    G, n, seed = 4, len(book), 23
    games, _ = _play(gpu, pc, c["stub"], G, seed, book, use_history=True, stop=_two_per_slot_and_position(G, n))
    cfg = so.oracle_cfg(pc, use_history=True)
    differs = 0
    for g in games:
        gid = g["game_id"]
        ref = so.selfplay_game(cfg, c["stub"], seed, gid, init_state=book[gid % n])
        _assert_game(g, ref, book[gid % n], gid % n, gid)
        differs += ref["moves"] != so.selfplay_game(so.oracle_cfg(pc), c["stub"], seed, gid, init_state=book[gid % n])["moves"]
    assert differs > 0                                      # (the second plane block reaches the stub network)


# ---- 5. trainer --------------------------------------------------------------------------------------------------------
def test_book_records_load_into_the_replay_window(gpu, tmp_path, monkeypatch):
    import torch
    from cchess_alphazero.config import Config
    from cchess_alphazero.environment.static_env import state_to_array
    from cchess_alphazero.lib.data_helper import PlayDataWriter, get_game_data_filenames
    from cchess_alphazero.lib.record_decoder import expand_records
    from cchess_alphazero.lib.replay_window import ReplayWindow
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    gold = _gold()
    book, c = gold["book"], gold["configs"][1]
    pc = _pc_of(c, K=4, max_game_length=8)
    G, n = 4, len(book)
    games, _ = _play(gpu, pc, c["stub"], G, 5, book, stop=_two_per_slot_and_position(G, n))
    cfg = Config("mini")
    cfg.play_data.nb_game_in_file = 3
    writer = PlayDataWriter(cfg)
    kept = [g for g in games if g["turns"] > 0]
    kept = kept[:len(kept) // 3 * 3]
    for g in kept:
        writer.add_game(g["data"])
    files = get_game_data_filenames(cfg.resource)
    assert len(files) == len(kept) // 3
    win = ReplayWindow(10 ** 6)
    for f in files:
        win.load_file(f)
    assert len(win) == sum(g["turns"] for g in kept)
    off = np.concatenate([[0], np.cumsum([g["turns"] for g in kept])])
    boards = win.boards[:len(win)].cpu().numpy()
    for g, o in zip(kept, off[:-1]):
        assert np.array_equal(boards[o], state_to_array(book[g["book_index"]])), g["game_id"]
    planes, _, vals, offsets = expand_records([g["data"] for g in kept])
    assert np.array_equal(offsets, off)
    idx = torch.arange(len(win), dtype=torch.int32, device="cuda")
    assert torch.equal(win.planes(idx), planes.float())
    assert torch.equal(win.z[:len(win)], vals)


def test_worker_reads_the_book_from_the_config_and_writes_its_positions(gpu, tmp_path, monkeypatch):
    """config.engine.book_path / book_rate (what --book / --book-rate set) -> the engine loads the file with the package's
    rule kernels and hands it to the search; the worker's record files begin with the games' real first states."""
    from cchess_alphazero.config import Config
    from cchess_alphazero.engine import SelfPlayEngine
    from cchess_alphazero.lib.data_helper import get_game_data_filenames, read_game_data_from_file
    from cchess_alphazero.lib.record_decoder import split_games
    from cchess_alphazero.worker.self_play import SelfPlayWorker
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    book = _gold()["book"]
    cfg = Config("mini")
    for k, v in dict(simulation_num_per_move=12, search_threads=4, max_game_length=8, noise_eps=0.0,
                     tau_decay_rate=0.98).items():
        setattr(cfg.play, k, v)
    cfg.engine.games_per_gpu, cfg.engine.report_every_rounds = 16, 16
    cfg.engine.book_path, cfg.engine.book_rate = os.path.join(GOLDEN, "book.txt"), 0.5
    cfg.play_data.max_file_num = 1000
    w = SelfPlayWorker(cfg)
    w.engine = SelfPlayEngine(cfg, 16, evaluator=stub_eval(gpu, dict(kind="hash", salt=21)), seed=9)
    assert w.engine.book == book and w.engine.book_rate == 0.5 and w.engine.search.book_size == len(book)
    w.engine.start(0, 0)
    seen = []
    drain = w.engine.drain

    def spy(*a, **k):
        out = drain(*a, **k)
        seen.extend(out)
        return out
    w.engine.drain = spy
    w.run(max_rounds=4000, max_games=60)
    w.close()
    stored = [g["data"] for g in seen if g["store"]]
    written = [g for p in get_game_data_filenames(cfg.resource) for g in split_games(read_game_data_from_file(p))]
    assert len(written) >= 20 and written == stored[:len(written)]
    firsts = {g[0] for g in written}
    assert xo.INIT_STATE in firsts and len(firsts & set(book)) >= 3 and firsts <= set(book) | {xo.INIT_STATE}
    for g in seen:
        hit = stub_net.philox_uniform(9, g["game_id"], 0, 2) < 0.5
        assert g["book_index"] == (g["game_id"] % len(book) if hit else None)
        assert g["data"][0] == (book[g["game_id"] % len(book)] if hit else xo.INIT_STATE)


# ---- 6. arena ----------------------------------------------------------------------------------------------------------
def test_arena_plays_each_book_position_once_per_colour(gpu, tmp_path, monkeypatch):
    from arena_oracle import arena_game
    from cchess_alphazero.config import Config
    from cchess_alphazero.worker.evaluator import EvaluateWorker, book_states, position_table, score_table
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    cfg = Config("mini")
    for k, v in dict(simulation_num_per_move=24, search_threads=4, noise_eps=0.0, tau_decay_rate=0.9, c_puct=1.0,
                     max_game_length=12).items():
        setattr(cfg.play, k, v)
    cfg.opts.evaluate = False
    book = _gold()["book"]
    specs = (dict(kind="hash", salt=41), dict(kind="hash", salt=42))
    evs = tuple((lambda planes, s=s: stub_net.hash_stub_torch(planes, s["salt"])) for s in specs)

    def u_fn(g, turns):
        return stub_net.philox_uniform(99, g, 1, turns)
    n = 2 * len(book) + 2
    starts = book_states(book, range(n))
    assert all(starts[2 * k] == starts[2 * k + 1] == book[k % len(book)] for k in range(n // 2))
    trace = {}
    got = EvaluateWorker(cfg, evaluators=evs, seed=5).play_games(n, u_fn=u_fn, init_state=starts, trace=trace)
    exp = [arena_game(i, cfg.play, specs, u_fn, init_state=starts[i])[:2] for i in range(n)]
    assert got == exp
    for i in range(n):                                       # both colours searched the same first position
        assert trace[i][0]["state"] == starts[i]
    # the single init_state keeps working
    one = EvaluateWorker(cfg, evaluators=evs, seed=5).play_games(2, u_fn=u_fn, init_state=book[1])
    assert one == [arena_game(i, cfg.play, specs, u_fn, init_state=book[1])[:2] for i in range(2)]
    rows = position_table(got, len(book))
    total = score_table(got)
    assert tuple(sum(r["table"][i] for r in rows) for i in range(7)) == total
    assert [r["games"] for r in rows] == [4] + [2] * (len(book) - 1)
    with pytest.raises(ValueError):
        EvaluateWorker(cfg, evaluators=evs, seed=5).play_games(3, u_fn=u_fn, init_state=starts[:2])


# ---- 7. argument errors, and load_book on the package's own rule kernels ------------------------------------------------
def test_set_book_argument_errors_leave_the_object_usable(gpu):
    gold = _gold()
    book, c = gold["book"], gold["configs"][0]
    boards = np.ascontiguousarray(np.stack([xo.state_to_board(s) for s in book]), dtype=np.int8)
    pc = _pc_of(c, K=4, max_game_length=6)
    s = gpu.S.Search(pc, 3, seed=c["seed"])
    ptr, st = boards.ctypes.data_as(C.c_void_p), s._stream()
    ERR_ARG = -1                                            # include/czero.h CZ_ERR_ARG
    s.set_book(boards, 1.0)
    for args in ((ptr, -1, 1.0), (None, 3, 1.0), (ptr, len(book), -0.01), (ptr, len(book), 1.01),
                 (ptr, len(book), float("nan")), (ptr, gpu.S.BOOK_MAX + 1, 1.0)):
        rc = s.L.cz_search_set_book(s.h, args[0], args[1], args[2], st)
        assert rc == ERR_ARG, args
    assert s.L.cz_search_set_book(None, ptr, len(book), 1.0, st) == ERR_ARG
    with pytest.raises(gpu.N.NativeError):
        s.set_book(boards, 2.0)
    # the book set before the failed calls is still in force
    ev = stub_eval(gpu, c["stub"])
    s.start_selfplay(seed=c["seed"], first_game_id=0)
    recs = []
    for r in range(4000):
        s.round()
        p, v = ev(s.planes)
        s.policy.copy_(p)
        s.value.copy_(v)
        if r % 32 == 31:
            recs += s.drain_records()
            if len(recs) >= 6:
                break
    s.close()
    assert len(recs) >= 6 and all(r["book_index"] == r["game_id"] % len(book) for r in recs)
    cfg = so.oracle_cfg(pc)
    for r in recs[:4]:
        ref = so.selfplay_game(cfg, c["stub"], c["seed"], r["game_id"], init_state=book[r["book_index"]])
        assert [xo.label_str(int(m)) for m in r["moves"]] == ref["moves"]


def test_load_book_on_the_rule_kernels(gpu, tmp_path):
    from cchess_alphazero.lib.book import load_book
    assert load_book(os.path.join(GOLDEN, "book.txt")) == _gold()["book"]
    row9 = "9/9/9/9/9/9/9"
    for bad, needle in ((f"4s4/{row9}/4R4/4S4", "already over"), (f"3s5/4m4/{row9}/4S4", "attack")):
        p = tmp_path / "bad.txt"
        p.write_text(f"{xo.INIT_STATE}\n# comment\n{bad}\n")
        with pytest.raises(ValueError) as e:
            load_book(str(p))
        assert str(e.value).startswith(f"{p}:3: ") and needle in str(e.value)
