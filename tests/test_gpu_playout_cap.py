"""-m gpu: playout cap randomization (cz_search_set_playout_cap, run.py self --fast-sims N --full-rate P).

The device game loop is compared, game by game and with no tolerance, with tests/playout_cap_oracle.py -- the oracle's
self-play loop with the ply's budget written into its one player before each move, which tests/test_playout_cap_cpu.py
pins to tests/selfplay_oracle.py where the two must agree.  The network is the exact stub of tests/stub_net.py.  With the
cap off, and at rate 1, the record ring holds the bytes it holds without the call.

GPU time of this file on an MI355X: see EXPERIMENTS.md ("Playout cap randomization")."""
import json
import logging
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import playout_cap_oracle as pco
import selfplay_oracle as so
from oracle import xq_oracle as xo
from test_gpu_book import GOLDEN, _engine_cfg, _raw_records
from test_gpu_search import assert_root_equal, boards_tensor, gpu, oracle_cfg, play_config, stub_eval  # noqa: F401  (gpu: fixture)
from test_gpu_trainer import small_config, window_of

pytestmark = pytest.mark.gpu
ERR_ARG = -1                                                # include/czero.h CZ_ERR_ARG
SPEC = dict(kind="hash", salt=5)
G = 32                                                      # games per configuration: one per slot at least


def _book():
    with open(os.path.join(GOLDEN, "book_games.json")) as f:
        return json.load(f)["book"]


def _play(gpu, pc, G, seed, fast_sims, rate, book=None, book_rate=1.0, max_rounds=120000, **kw):
    """Self-play through SelfPlayEngine with the stub evaluator until every slot has finished a game.  Returns every
    finished game and, per slot, the slot's `sims` counter as it stood at the end of the round in which its last game
    finished: the new game in the slot has only expanded its root by then (nothing backed up), so the sum over the slots
    is the number of simulations of the finished games."""
    from cchess_alphazero.engine import SelfPlayEngine
    eng = SelfPlayEngine(_engine_cfg(pc), G, evaluator=stub_eval(gpu, SPEC), seed=seed, book=book, book_rate=book_rate,
                         fast_sims=fast_sims, full_rate=rate, **kw)
    i_sims, i_games = gpu.S.COUNTER_NAMES.index("sims"), gpu.S.COUNTER_NAMES.index("games")
    games = []
    at_boundary = np.zeros(G, dtype=np.uint64)
    n_done = np.zeros(G, dtype=np.uint64)
    try:
        eng.start(0, 0)
        for r in range(max_rounds):
            eng.step()
            gc = eng.search.game_counters()
            fin = gc[:, i_games] != n_done
            at_boundary[fin] = gc[fin, i_sims]
            n_done = gc[:, i_games].copy()
            if r % 16 == 15:
                games += eng.drain()
            if n_done.min() >= 1:
                break
        else:
            raise AssertionError(f"not finished after {max_rounds} rounds: {len(games)} games")
        games += eng.drain()
        ctr = eng.counters()
    finally:
        eng.close()
    assert ctr["tree_resets"] == 0 and ctr["overflow_sims"] == 0
    assert len({g["game_id"] for g in games}) == len(games) == int(n_done.sum()) >= G
    return games, int(at_boundary.sum()), ctr


def _moves(g):
    return [item[0] for item in g["data"][1:]]


def _flags(g):
    """The per-move fast flags as the record items carry them: a four-element item with weight 0."""
    for item in g["data"][1:]:
        assert len(item) in (2, 3) or (len(item) == 4 and item[3] == 0), item
    return [len(item) == 4 for item in g["data"][1:]]


def _compare(games, pc, seed, fast_sims, rate, use_history=False, book=None, book_rate=1.0, visits=False):
    """Every game against the capped oracle.  Returns (the oracle's simulations, full plies, fast plies, fast plies that
    searched nothing)."""
    cfg = so.oracle_cfg(pc, use_history=use_history)
    sims = full = fast = idle = 0
    for g in games:
        gid = g["game_id"]
        init = book[gid % len(book)] if book and so.book_lottery(seed, gid, book_rate) else xo.INIT_STATE
        trace = []
        ref = pco.capped_selfplay_game(cfg, SPEC, seed, gid, fast_sims, rate, init_state=init, trace=trace)
        what = (gid, pc.search_threads, rate)
        assert g["data"][0] == init, what
        assert _moves(g) == ref["moves"], (what, _moves(g), ref["moves"])
        assert (g["turns"], g["value"], g["store"], g["resigned"]) == \
               (ref["turns"], int(ref["value"]), ref["store"], ref["resigned"]), what
        assert _flags(g) == pco.move_flags(ref), what
        assert g["fast_plies"] == sum(pco.move_flags(ref)), what
        if visits:
            vis = g["visits"]
            assert vis is not None and len(vis) == len(trace), what           # one entry per searched ply, fast ones included
            for e, t in zip(vis, trace):
                assert np.array_equal(e.moves, t["moves"]) and np.array_equal(e.n, t["n"]), (what, e.ply)
                assert (e.sum_n, e.fast, e.resign) == (t["sum_n"], t["fast"], t["action"] is None), (what, e.ply)
        sims += ref["sims"]
        full += len(ref["fast"]) - sum(ref["fast"])
        fast += sum(ref["fast"])
        idle += ref["idle_fast"]
    return sims, full, fast, idle


# (the record ring holds 2 G + 64 = 128 games and _raw_records drains once, at the end: 120 rounds of these 16-ply games
#  at >= 2 rounds a ply finish fewer than that, so no record is overwritten and the comparison does not depend on the
#  order in which games that end in one launch reach the ring)
ROUNDS_1 = 120


# ---- 1. off is off -----------------------------------------------------------------------------------------------------
def test_cap_off_and_rate_1_leave_every_record_byte_and_counter(gpu):
    pc = play_config(simulation_num_per_move=16, search_threads=4, tau_decay_rate=0.9, max_game_length=8,
                     enable_resign_rate=0.5, resign_threshold=-0.4, min_resign_turn=4)
    base, ctr0 = _raw_records(gpu, pc, SPEC, G, 31, ROUNDS_1, lambda s: None)
    assert len(base) >= G
    off, ctr1 = _raw_records(gpu, pc, SPEC, G, 31, ROUNDS_1, lambda s: s.set_playout_cap(0, 0.25))
    rate1, ctr2 = _raw_records(gpu, pc, SPEC, G, 31, ROUNDS_1, lambda s: s.set_playout_cap(6, 1.0))
    back, ctr3 = _raw_records(gpu, pc, SPEC, G, 31, ROUNDS_1, lambda s: (s.set_playout_cap(6, 0.5), s.set_playout_cap(0, 0.5)))
    assert off == base and rate1 == base and back == base
    assert ctr0 == ctr1 == ctr2 == ctr3
    # ... and the cap does: same seed, rate 0.5
    mixed, ctr4 = _raw_records(gpu, pc, SPEC, G, 31, ROUNDS_1, lambda s: s.set_playout_cap(6, 0.5))
    assert mixed != base and ctr4["plies"] > ctr0["plies"]
    # the same with root noise on: the cap off draws the rows it drew
    noisy = play_config(**dict(vars(pc), noise_eps=0.25))
    nbase, nc0 = _raw_records(gpu, noisy, SPEC, G, 31, ROUNDS_1, lambda s: None)
    noff, nc1 = _raw_records(gpu, noisy, SPEC, G, 31, ROUNDS_1, lambda s: s.set_playout_cap(6, 1.0))
    assert nbase != base and noff == nbase and nc0 == nc1


# ---- 2. all fast -------------------------------------------------------------------------------------------------------
def _records(gpu, pc, seed, rounds, setup):
    s = gpu.S.Search(pc, G, seed=seed)
    setup(s)
    ev = stub_eval(gpu, SPEC)
    s.start_selfplay(seed=seed, first_game_id=0)
    recs = []
    for r in range(rounds):
        s.round()
        p, v = ev(s.planes)
        s.policy.copy_(p)
        s.value.copy_(v)
        if r % 16 == 15:                                    # (before the ring of 2 G + 64 records can wrap)
            recs += s.drain_records()
    recs = sorted(recs + s.drain_records(), key=lambda r: r["game_id"])
    ctr = s.counters()
    s.close()
    keys = ("games", "plies", "sims", "expansions", "terminal_sims", "red_wins", "black_wins", "draws", "resigns")
    return recs, {k: ctr[k] for k in keys}


def _plain(r):
    return (r["game_id"], r["turns"], r["value"], r["store"], r["resigned"], r["moves"].tolist())


@pytest.mark.parametrize("noise_eps", [0.0, 0.25])
def test_rate_0_is_a_search_of_fast_sims_without_root_noise(gpu, noise_eps):
    """noise_eps > 0 pins "no root noise on fast plies" exactly: the capped search is configured with noise and must still
    play the games of a noiseless search of fast_sims simulations."""
    kw = dict(search_threads=4, tau_decay_rate=0.9, max_game_length=8, enable_resign_rate=0.5, resign_threshold=-0.4,
              min_resign_turn=4)
    small = play_config(simulation_num_per_move=6, noise_eps=0.0, **kw)
    capped = play_config(simulation_num_per_move=16, noise_eps=noise_eps, **kw)
    want, ctr_w = _records(gpu, small, 31, 120, lambda s: None)
    got, ctr_g = _records(gpu, capped, 31, 120, lambda s: s.set_playout_cap(6, 0.0))
    assert len(want) >= G
    assert [_plain(r) for r in got] == [_plain(r) for r in want]
    assert ctr_g == ctr_w
    for r, w in zip(got, want):
        ref = so.selfplay_game(so.oracle_cfg(small), SPEC, 31, r["game_id"])
        assert [xo.label_str(int(m)) for m in r["moves"]] == ref["moves"], r["game_id"]
        searched = ref["searched"]                          # (the appended king capture is not a searched ply)
        assert r["fast"] == [True] * searched + [False] * (r["turns"] - searched), r["game_id"]
        assert not any(w["fast"])
    if noise_eps:                                           # the noise is still there on full plies
        half_noisy, _ = _records(gpu, capped, 31, 120, lambda s: s.set_playout_cap(6, 0.5))
        quiet = play_config(simulation_num_per_move=16, noise_eps=0.0, **kw)
        half_quiet, _ = _records(gpu, quiet, 31, 120, lambda s: s.set_playout_cap(6, 0.5))
        assert [_plain(r) for r in half_noisy] != [_plain(r) for r in half_quiet]


# ---- 3. mixed schedules against the oracle -----------------------------------------------------------------------------
def _pc(K, **kw):
    d = dict(simulation_num_per_move=200, search_threads=K, tau_decay_rate=0.98, max_game_length=12)
    d.update(kw)
    return play_config(**d)


@pytest.mark.parametrize("rate", [0.25, 0.5])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_mixed_schedule_matches_the_capped_oracle(gpu, K, rate):
    pc = _pc(K)
    games, sims_gpu, ctr = _play(gpu, pc, G, 11, 40, rate)
    sims, full, fast, idle = _compare(games, pc, 11, 40, rate)
    print(f"K={K} rate={rate}: {len(games)} games, {full} full and {fast} fast plies, {idle} fast plies searched nothing, "
          f"{sims} simulations")
    assert full > 0 and fast > 0
    if K == 1:
        assert idle >= 1                                    # a fast ply whose reused root exceeded the budget
    assert sims_gpu == sims
    assert ctr["sims"] >= sims


def test_mixed_schedule_with_history_planes(gpu):
    pc = _pc(4, simulation_num_per_move=64)
    games, sims_gpu, _ = _play(gpu, pc, G, 23, 16, 0.25, use_history=True)
    sims, full, fast, _ = _compare(games, pc, 23, 16, 0.25, use_history=True)
    assert full > 0 and fast > 0 and sims_gpu == sims
    plain = so.oracle_cfg(pc)                               # (the second plane block reaches the stub network)
    assert any(_moves(g) != pco.capped_selfplay_game(plain, SPEC, 23, g["game_id"], 16, 0.25)["moves"] for g in games)


def test_mixed_schedule_with_a_book_at_rate_half(gpu):
    book = _book()
    pc = _pc(4, simulation_num_per_move=64)
    games, sims_gpu, _ = _play(gpu, pc, G, 777, 16, 0.5, book=book, book_rate=0.5)
    sims, full, fast, _ = _compare(games, pc, 777, 16, 0.5, book=book, book_rate=0.5)
    assert full > 0 and fast > 0 and sims_gpu == sims
    from_book = [g["book_index"] is not None for g in games]
    assert any(from_book) and not all(from_book)


def test_mixed_schedule_with_visit_records_and_resignation(gpu):
    # (resign_threshold 0.05 from ply 8: on the oracle 14 of game ids 0-31 resign, on fast plies and on full ones)
    pc = _pc(1, enable_resign_rate=0.5, resign_threshold=0.05, min_resign_turn=8)
    games, sims_gpu, ctr = _play(gpu, pc, G, 11, 40, 0.25, record_visits=True)
    sims, full, fast, idle = _compare(games, pc, 11, 40, 0.25, visits=True)
    assert full > 0 and fast > 0 and idle >= 1 and sims_gpu == sims
    assert ctr["visits_dropped"] == 0
    assert any(g["resigned"] for g in games)
    entries = [e for g in games for e in g["visits"]]
    assert any(e.fast and e.sum_n > 40 for e in entries)    # the idle fast plies show in the entries
    assert any(e.resign and e.fast for e in entries) and any(e.resign and not e.fast for e in entries)


# ---- 4. records to trainer ---------------------------------------------------------------------------------------------
def _strip(game):
    return [game[0]] + [item[:2] if len(item) < 3 or item[2] is None else item[:3] for item in game[1:]]


def test_records_reach_the_trainer_with_their_weights(gpu, tmp_path, monkeypatch):
    import torch
    from cchess_alphazero.agent.model import CChessModel
    from cchess_alphazero.lib.record_decoder import expand_records
    from cchess_alphazero.worker.optimize import OptimizeWorker, validation_split
    pc = _pc(4, simulation_num_per_move=24, max_game_length=10)
    seed, n, rate = 5, 6, 0.5
    with_pi, _, _ = _play(gpu, pc, G, seed, n, rate, record_visits=True)
    without, _, _ = _play(gpu, pc, G, seed, n, rate)
    assert {g["game_id"]: _moves(g) for g in with_pi} == {g["game_id"]: _moves(g) for g in without}
    cfg = so.oracle_cfg(pc)
    # item shapes
    kinds = set()
    for games, pi in ((with_pi, True), (without, False)):
        for g in games:
            ref = pco.capped_selfplay_game(cfg, SPEC, seed, g["game_id"], n, rate)
            flags = pco.move_flags(ref)
            v = g["value"]
            assert len(g["data"]) - 1 == g["turns"] == len(flags)
            for i, (item, f) in enumerate(zip(g["data"][1:], flags)):
                assert item[0] == ref["moves"][i] and item[1] == (v if i % 2 == 0 else -v)
                searched = i < ref["searched"]
                if f:
                    assert len(item) == 4 and item[3] == 0 and searched
                    assert (isinstance(item[2], list) and item[2]) if pi else item[2] is None
                else:
                    assert len(item) == (3 if pi and searched else 2)
                kinds.add((pi, f, searched))
            assert g["fast_plies"] == sum(flags)
            assert json.loads(json.dumps(g["data"])) == g["data"]            # None travels as null
    assert kinds >= {(True, True, True), (True, False, True), (False, True, True), (False, False, True)}
    assert (True, False, False) in kinds or (False, False, False) in kinds   # a king capture: two elements, never fast
    # the window keeps every position and knows which rows train
    games = [g["data"] for g in with_pi if g["turns"] > 0]
    win = window_of(games)
    bare = window_of([_strip(g) for g in games])
    flags = np.array([len(item) == 4 for g in games for item in g[1:]])
    assert len(win) == len(bare) == len(flags) and flags.any() and not flags.all()
    assert win.trainable.dtype == np.uint8 and np.array_equal(win.trainable, (~flags).astype(np.uint8))
    assert np.array_equal(win.training_rows(), np.flatnonzero(~flags))
    assert bare.trainable.all() and np.array_equal(bare.training_rows(), np.arange(len(bare)))
    m = len(win)
    assert torch.equal(win.boards[:m], bare.boards[:m]) and torch.equal(win.prev[:m], bare.prev[:m])
    assert torch.equal(win.played[:m], bare.played[:m]) and torch.equal(win.z[:m], bare.z[:m])
    assert torch.equal(win.row_ptr[:m + 1], bare.row_ptr[:m + 1]) and win.nnz == bare.nnz
    # record_decoder.expand_records stays expanding_data: every position, the extras ignored
    for targets in ("played", "visits"):
        a, b = expand_records(games, targets=targets), expand_records([_strip(g) for g in games], targets=targets)
        assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and np.array_equal(a[3], b[3])
    none_games = [g["data"] for g in without if g["turns"] > 0]
    a, b = expand_records(none_games, targets="visits"), expand_records([_strip(g) for g in none_games], targets="visits")
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    assert np.array_equal(window_of(none_games).trainable, np.array(
        [len(item) != 4 for g in none_games for item in g[1:]], dtype=np.uint8))
    # one epoch of the worker draws trainable rows only
    cfg_t = small_config(tmp_path, monkeypatch, batch_size=16, policy_targets="visits")
    ow = OptimizeWorker(cfg_t)
    ow.model = CChessModel(cfg_t)
    ow.model.build(seed=5)
    ow.model.model.cuda().train()
    ow.compile_model()
    ow.update_learning_rate(0)
    ow.window = win
    drawn = dict(step=[], evaluate=[])
    step, evaluate = ow.step, ow.evaluate

    def spy_step(idx, mirror=None):
        drawn["step"].append(idx.cpu().numpy().copy())
        return step(idx, mirror)

    def spy_eval(idx_all, mirror=False):
        drawn["evaluate"].append(idx_all.cpu().numpy().copy())
        return evaluate(idx_all, mirror)
    ow.step, ow.evaluate = spy_step, spy_eval
    tr, va = validation_split(m)
    rows = win.training_rows()
    steps = ow.train_epoch(1)
    got = np.concatenate(drawn["step"])
    assert np.array_equal(np.sort(got), np.intersect1d(tr, rows)) and len(got) < len(tr)
    assert len(drawn["evaluate"]) == 1 and np.array_equal(drawn["evaluate"][0], np.intersect1d(va, rows))
    assert steps == len(rows) // 16 and ow.skipped_rows == int(flags.sum())
    assert all(np.isfinite(x) for x in ow.history[-1]["train"])
    # a malformed weight names the game and the ply; the window is unchanged
    long = sorted(games, key=len)[-2:]
    assert len(long[1]) > 3
    bad = [list(long[0]), [long[1][0]] + [list(i) for i in long[1][1:]]]
    bad[1][2] = bad[1][2][:2] + [None, 2]
    for w in (2, -1, 0.5, "0", None, True):
        bad[1][2][3] = w
        with pytest.raises(ValueError, match=r"game 1, ply 1"):
            win.add_games(bad)
    assert len(win) == m and len(win.trainable) == m
    for w in (0, 1):
        bad[1][2][3] = w
        fresh = window_of(bad)
        assert fresh.trainable[len(bad[0]) - 1 + 1] == w


# ---- 5. the command line -----------------------------------------------------------------------------------------------
def test_run_py_self_with_a_playout_cap_then_opt(tmp_path, monkeypatch):
    from cchess_alphazero import manager
    from cchess_alphazero.agent.model import CChessModel
    from cchess_alphazero.lib.data_helper import get_game_data_filenames, read_game_data_from_file
    from cchess_alphazero.lib.record_decoder import split_games
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "chinesechess-alphazero_amd")
    env = dict(os.environ, DATA_DIR=str(tmp_path / "data"), PROJECT_DIR=str(tmp_path), PYTHONPATH=pkg)
    r = subprocess.run([sys.executable, os.path.join(pkg, "cchess_alphazero", "run.py"), "self", "--type", "mini",
                        "--games-per-gpu", "64", "--fast-sims", "8", "--full-rate", "0.5", "--record-visits",
                        "--max-games", "8"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(tmp_path / "logs" / "play.log") as f:
        log = f.read()
    assert "playout cap" in log and re.search(r"drained \d+ full plies \(training rows\) and \d+ fast plies", log)
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    build = manager.build_config

    def small(args):                                        # the command line's config at test size
        cfg = build(args)
        cfg.model.cnn_filter_num, cfg.model.res_layer_num = 32, 2
        cfg.trainer.batch_size = 16
        return cfg
    monkeypatch.setattr(manager, "build_config", small)
    cfg = small(manager.create_parser().parse_args(["opt"]))
    rc = cfg.resource
    files = get_game_data_filenames(rc)
    assert files
    items = [it for p in files for g in split_games(read_game_data_from_file(p)) for it in g[1:]]
    four = [it for it in items if len(it) == 4]
    assert four and all(it[3] == 0 and isinstance(it[2], list) for it in four)
    assert any(len(it) == 3 for it in items)
    model = CChessModel(cfg)
    model.build(seed=0)
    model.save(rc.model_best_config_path, rc.model_best_weight_path)
    monkeypatch.setattr(sys, "argv", ["run.py", "opt", "--type", "mini", "--policy-targets", "visits"])
    handlers, level = list(logging.getLogger().handlers), logging.getLogger().level
    try:
        total = manager.start()
    finally:
        logging.getLogger().setLevel(level)
        for h in logging.getLogger().handlers[len(handlers):]:
            logging.getLogger().removeHandler(h)
            h.close()
    assert total > 0
    with open(rc.opt_log_path) as f:
        m = re.search(r"(\d+) of (\d+) positions carry the training weight 0", f.read())
    assert m and 0 < int(m.group(1)) < int(m.group(2))


# ---- 6. arguments, and the modes the cap does not touch ----------------------------------------------------------------
def test_set_playout_cap_argument_errors_leave_the_setting(gpu):
    pc = play_config(simulation_num_per_move=16, search_threads=4, max_game_length=6)
    s = gpu.S.Search(pc, 2, seed=1)
    st = s._stream()
    s.set_playout_cap(6, 0.5)
    for args in ((-1, 0.5), (17, 0.5), (6, -0.01), (6, 1.01), (6, float("nan"))):
        assert s.L.cz_search_set_playout_cap(s.h, args[0], args[1], st) == ERR_ARG, args
    assert s.L.cz_search_set_playout_cap(None, 6, 0.5, st) == ERR_ARG
    with pytest.raises(gpu.N.NativeError):
        s.set_playout_cap(6, 2.0)
    assert (s.fast_sims, s.full_rate) == (6, 0.5)
    assert s.L.cz_search_set_sims(s.h, 5) == ERR_ARG        # the full budget never goes below the fast one
    s.set_playout_cap(16, 0.0)                              # the bounds themselves are fine
    s.set_playout_cap(1, 1.0)
    s.set_playout_cap(0, 7.0)                               # off: the rate means nothing
    s.close()


def test_external_mode_never_looks_at_the_cap(gpu):
    states = [xo.INIT_STATE, xo.step(xo.INIT_STATE, '1242')]
    pc = play_config(simulation_num_per_move=60, search_threads=4, noise_eps=0.0)
    s = gpu.S.Search(pc, len(states), seed=7)
    s.set_playout_cap(10, 0.0)                              # every self-play ply would be fast
    s.set_roots(boards_tensor(gpu, states))
    s.run_until_idle(stub_eval(gpu, SPEC))
    st = s.root_stats()
    for g, state in enumerate(states):
        pl = xo.Player(oracle_cfg(pc), SPEC)
        pl.search(state)
        assert pl.node_stats(state)["sum_n"] == 60
        assert_root_equal(st, g, pl.node_stats(state), f"game {g}")
        pl.close()
    s.close()
