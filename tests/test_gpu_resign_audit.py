"""-m gpu: the max-q record and the resignation audit (cz_search_record_maxq, cz_search_drain_visits_cols,
cz_search_root_maxq, cz_root_maxq, cz_search_set_resign_threshold; run.py self --resign-audit, --resign-fp-target).

The yardsticks are tests/resign_audit_oracle.py: the C oracle's games with the max q of every searched ply (float64, a
maximum of correctly rounded quotients: compared for equality), and the per-game restatement of the audit that
tests/test_resign_audit_cpu.py pins lib/resign_audit.py to."""
import ctypes as C
import json

import numpy as np
import pytest

import resign_audit_oracle as ro
import search_model as sm
import selfplay_oracle as so
from oracle import xq_oracle as xo
from selfplay_raw import drain_cols, selfplay_raw
from test_gpu_book import _engine_cfg
from test_gpu_search import boards_tensor, gpu, no_act_tensors, play_config, stub_eval  # noqa: F401  (gpu: fixture)

pytestmark = pytest.mark.gpu
ERR_ARG = -1                                                # include/czero.h CZ_ERR_ARG
G = 16
MRT = 4
M = 128


# ---- the worker on the oracle's configuration ------------------------------------------------------------------------------
def _worker(gpu, tmp_path, monkeypatch, **engine):
    """SelfPlayWorker on the hash stub (the engine handed in) with the configuration of tests/resign_audit_oracle.py;
    every drained game is kept in worker.seen."""
    from cchess_alphazero.engine import SelfPlayEngine
    from cchess_alphazero.worker.self_play import SelfPlayWorker
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    cfg = _engine_cfg(ro.play_config(), games_per_gpu=G, report_every_rounds=32, record_visits=True, resign_audit=True,
                      audit_every_rounds=None, reload_seconds=None, **engine)
    cfg.play_data.max_file_num = 1000
    w = SelfPlayWorker(cfg)
    w.engine = SelfPlayEngine(cfg, G, evaluator=stub_eval(gpu, ro.SPEC), seed=ro.SEED)
    assert w.engine.resign_audit and w.engine.search.maxq_on
    w.engine.start(0, 0)
    w.seen = {}
    drain = w.engine.drain

    def keep(*a, **kw):
        out = drain(*a, **kw)
        for g in out:
            w.seen[g["game_id"]] = g
        return out
    w.engine.drain = keep
    return w


def _run_until_first_games(w, gpu, chunk=128, max_chunks=40):
    i_games = gpu.S.COUNTER_NAMES.index("games")
    for _ in range(max_chunks):
        w.run(max_rounds=chunk)
        if w.engine.search.game_counters()[:, i_games].min() >= 1:
            break
    else:
        raise AssertionError(f"games 0 .. {G - 1} not finished: {sorted(w.seen)}")
    ctr = w.engine.counters()
    assert ctr["visits_dropped"] == 0 and ctr["tree_resets"] == 0 and ctr["overflow_sims"] == 0, ctr
    assert all(i in w.seen for i in ro.GAME_IDS)
    return ctr


def test_maxq_of_every_ply_equals_the_oracle_and_the_worker_audits_it(gpu, tmp_path, monkeypatch):
    from cchess_alphazero.lib.resign_audit import ResignAudit
    w = _worker(gpu, tmp_path, monkeypatch)
    try:
        _run_until_first_games(w, gpu)
        threshold = w.engine.resign_threshold
    finally:
        w.close()
    n_entries = 0
    for gid, g in sorted(w.seen.items()):
        ref = ro.game(gid)
        vis = g["visits"]
        assert vis is not None and g["value"] == ref["value"] and g["turns"] == ref["turns"], gid
        assert [e.ply for e in vis] == [p for p, _ in ref["trace"]], gid
        for e, (ply, mq) in zip(vis, ref["trace"]):
            assert e.no_resign and not e.resign, (gid, ply)              # bit 5: enable_resign_rate 1.0, nobody resigns
            assert e.maxq == mq, (gid, ply, e.maxq, mq)                  # float64, exactly
            n_entries += 1
    assert n_entries > 1000
    # the worker's histogram is the CPU module's on the oracle's games -- and, at the table's points, the specification's
    assert w.resign_audit.skipped == 0 and sorted(w.resign_audited) == sorted(w.seen)
    want = ResignAudit(MRT)
    for gid in w.seen:
        want.add_trace(ro.game(gid)["trace"], ro.game(gid)["value"])
    assert w.resign_audit.games == want.games == len(w.seen)
    assert (w.resign_audit.would == want.would).all() and (w.resign_audit.fp == want.fp).all()
    for k, T in enumerate(want.grid):
        assert (int(want.would[k]), int(want.fp[k])) == ro.restate([ro.game(i) for i in w.seen], float(T), MRT), T
    first = ResignAudit(MRT)
    for gid in ro.GAME_IDS:
        first.add_game(w.seen[gid]["visits"], w.seen[gid]["value"])
    for T, (would, fp) in ro.TABLE.items():
        if T <= 0.0:
            assert first.at(T) == (would, fp, T)
    assert threshold == -0.92 and w.resign_threshold_log == []           # no target: the threshold stays
    with open(tmp_path / "data" / "play_data" / "resign_audit_0.json") as f:
        d = json.load(f)
    assert d["threshold"] == -0.92 and len(d["grid"]) == len(d["would"]) == len(d["fp"]) == 101
    assert 0 < d["games"] <= want.games and d["skipped"] == 0


def test_worker_adapts_the_threshold_to_the_target(gpu, tmp_path, monkeypatch):
    from cchess_alphazero.lib.resign_audit import default_grid
    w = _worker(gpu, tmp_path, monkeypatch, resign_fp_target=0.3, resign_audit_min_events=5)
    try:
        _run_until_first_games(w, gpu)
        threshold = w.engine.resign_threshold
        low = w.engine.search.resign_threshold
    finally:
        w.close()
    assert w.resign_threshold_log, "the audit never reached five events: the test shows nothing"
    running = -0.92
    for games, t in w.resign_threshold_log:
        # the games audited so far, their traces from the oracle, the threshold from the restatement
        so_far = [ro.game(gid) for gid in w.resign_audited[:games]]
        assert len(so_far) == games
        want = ro.choose_restated(so_far, default_grid(), 0.3, 5, MRT)
        assert want is not None and t == want and t != running, (games, t, want)
        running = t
    assert threshold == low == running
    # every game still plays on without resignation, so the games are the oracle's whatever the threshold became
    assert all(g["value"] == ro.game(gid)["value"] and not g["resigned"] for gid, g in w.seen.items())
    assert w.resign_audit.skipped == 0


# ---- resignation enabled for some games ------------------------------------------------------------------------------------
def _engine_run(gpu, pc, seed, graph=False, before_start=None, mid=None, rounds_before=0, stop=None, max_rounds=6000):
    """SelfPlayEngine on the hash stub with the visit and the max-q record; mid(eng, entries so far) runs once after
    rounds_before rounds.  Returns ({game id: game}, counters)."""
    from cchess_alphazero.engine import SelfPlayEngine
    eng = SelfPlayEngine(_engine_cfg(pc), G, evaluator=stub_eval(gpu, ro.SPEC), seed=seed, record_visits=True,
                         resign_audit=True)
    i_games = gpu.S.COUNTER_NAMES.index("games")
    out = {}
    try:
        if before_start:
            before_start(eng)
        eng.start(0, 0)
        if graph:
            eng.capture_graph()
        for r in range(1, max_rounds + 1):
            eng.step()
            if mid is not None and r == rounds_before:
                for g in eng.drain():
                    out[g["game_id"]] = g
                mid(eng, out)
            if r % 16 == 0:
                for g in eng.drain():
                    out[g["game_id"]] = g
                if r > rounds_before and (stop(eng) if stop else eng.search.game_counters()[:, i_games].min() >= 1):
                    break
        else:
            raise AssertionError(f"not finished after {max_rounds} rounds: {len(out)} games")
        for g in eng.drain():
            out[g["game_id"]] = g
        ctr = eng.counters()
    finally:
        eng.close()
    assert ctr["visits_dropped"] == 0
    return out, ctr


def test_resign_enabled_games_lack_the_flag_and_resign_below_the_threshold(gpu):
    pc = ro.play_config(enable_resign_rate=0.5, resign_threshold=0.1)
    games, ctr = _engine_run(gpu, pc, ro.SEED)
    cfg = so.oracle_cfg(pc)
    n_resigned = n_on = n_off = 0
    for gid, g in games.items():
        enabled = bool(so.resign_enabled(cfg, ro.SEED, gid))
        vis = g["visits"]
        assert vis is not None
        n_on += enabled
        n_off += not enabled
        assert all(e.no_resign == (not enabled) for e in vis), gid
        assert all(e.maxq is not None for e in vis), gid
        assert g["resigned"] == any(e.resign for e in vis)
        for i, e in enumerate(vis):
            if e.resign:
                assert enabled and i == len(vis) - 1 and e.ply > MRT and e.maxq < 0.1, (gid, e.ply, e.maxq)
                n_resigned += 1
            elif enabled and e.ply > MRT:
                assert e.maxq >= 0.1, (gid, e.ply, e.maxq)               # the test would have fired
    assert n_resigned > 0 and n_on > 0 and n_off > 0, (n_resigned, n_on, n_off)
    assert ctr["resigns"] >= n_resigned


# ---- record on versus off ----------------------------------------------------------------------------------------------------
def _without_bit_5(entries):
    out = []
    for row, *_ in entries:
        b = bytearray(row)
        b[7] &= 0xFF ^ 32
        out.append(bytes(b))
    return sorted(out)


@pytest.mark.parametrize("K", [1, 8])
def test_record_on_changes_bit_5_and_nothing_else(gpu, K):
    pc = play_config(simulation_num_per_move=16, search_threads=K, tau_decay_rate=0.9, max_game_length=8,
                     enable_resign_rate=0.5, resign_threshold=-0.4, min_resign_turn=4)
    rounds = 400 if K == 1 else 120
    base, vis0, c0 = selfplay_raw(gpu, pc, 31, rounds, 32)
    off, vis1, c1 = selfplay_raw(gpu, pc, 31, rounds, 32, setup_after=lambda s: (s.record_maxq(True), s.record_maxq(False)))
    on, vis2, c2 = selfplay_raw(gpu, pc, 31, rounds, 32, setup_after=lambda s: s.record_maxq(True))
    assert len(base) >= 32 and len(vis0) > len(base)
    assert off == base and vis1 == vis0 and c1 == c0            # off: every byte what it was
    assert on == base and c2 == c0                              # on: records and counters byte for byte
    assert all(not row[7] & 32 for row, *_ in vis0)
    flagged = sum(bool(row[7] & 32) for row, *_ in vis2)
    assert 0 < flagged < len(vis2)                              # both kinds of game occur
    assert _without_bit_5(vis2) == sorted(row for row, *_ in vis0)
    # the flag is the game's lottery
    cfg = so.oracle_cfg(pc)
    for row, *_ in vis2:
        gid = int(np.frombuffer(row[:4], dtype=np.uint32)[0])
        assert bool(row[7] & 32) == (not so.resign_enabled(cfg, 31, gid)), gid


# ---- root_maxq and root_maxq_rows ----------------------------------------------------------------------------------------------
def _want_maxq(st, g, bans):
    c = int(st["counts"][g])
    lab = sm.banned_labels(st["moves"][g, :c], bans)
    return ro.root_maxq(lab, st["n"][g, :c], st["w"][g, :c]), lab


@pytest.mark.parametrize("K", [1, 8])
def test_root_maxq_against_numpy_on_root_stats(gpu, K):
    t = gpu.torch
    cases = {c["name"]: c for c in sm.cases()}
    names = ["init", "pos100", "pos250", "pos400", "pos550", "pos625", "wide", "pos250"]
    states = [cases[n]["state"] for n in names]
    assert len(xo.get_legal_moves(cases["wide"]["state"])) > 64          # both halves of the root's edges
    ev = stub_eval(gpu, ro.SPEC)
    s = gpu.S.Search(play_config(simulation_num_per_move=64, search_threads=K), 8, seed=7)
    assert np.isnan(s.root_maxq()).all()                                 # no root is in the tree
    # the ban: what the unbanned search of the position plays (slot 2) is banned in slot 7, with two more moves
    s.set_roots(boards_tensor(gpu, states))
    s.run_until_idle(ev)
    st = s.root_stats()
    got = s.root_maxq()
    rows = []
    for g in range(8):
        want, lab = _want_maxq(st, g, [])
        assert got[g] == want and -2.0 <= want <= 2.0, (g, got[g], want)
        rows.append((lab, st["n"][g], st["w"][g], int(st["counts"][g])))
    c = int(st["counts"][2])
    best = xo.label_str(int(st["moves"][2, int(st["n"][2, :c].argmax())]))
    bans = [[]] * 7 + [[best] + [m for m in xo.get_legal_moves(states[7]) if m != best][:2]]
    na, nn = no_act_tensors(gpu, bans)
    s.set_roots(boards_tensor(gpu, states), no_act=na, n_no_act=nn)
    s.run_until_idle(ev)
    st = s.root_stats()
    got = s.root_maxq()
    for g in range(8):
        want, lab = _want_maxq(st, g, bans[g])
        assert got[g] == want, (g, got[g], want)
        rows.append((lab, st["n"][g], st["w"][g], int(st["counts"][g])))
    c = int(st["counts"][7])
    j = [xo.label_str(int(mv)) for mv in st["moves"][7, :c]].index(best)
    assert st["n"][7, j] > 0                                             # the banned edge holds visits of the first search
    s.close()
    # a root never selected from: one simulation expands the root and ends
    s = gpu.S.Search(play_config(simulation_num_per_move=1, search_threads=K), 8, seed=7)
    s.set_roots(boards_tensor(gpu, states))
    s.run_until_idle(ev)
    st = s.root_stats()
    assert all(int(st["counts"][g]) > 0 and int(st["n"][g, :int(st["counts"][g])].sum()) == 0 for g in range(8))
    assert (s.root_maxq() == 0.0).all()
    s.close()
    # the arithmetic on rows: the roots above and the cases a search does not produce
    special = [
        (np.array([1 | ro.BANNED, 2 | ro.BANNED], dtype=np.uint16), [3, 4], [1.0, 1.0], 2, -100.0),    # every edge banned
        (np.array([], dtype=np.uint16), [], [], 0, -100.0),                                             # no edge
        (np.array([1, 2, 3], dtype=np.uint16), [0, 0, 0], [0.0, 0.0, 0.0], 3, 0.0),                    # never selected from
        (np.array([1, 2 | ro.BANNED, 3], dtype=np.uint16), [4, 10, 4], [-2.0, 10.0, -3.0], 3, -0.5),   # the best edge banned
        (np.array([1, 2], dtype=np.uint16), [3, 0], [-3.0, 5.0], 2, 0.0),                               # n = 0 counts as 0.0
    ]
    rng = np.random.default_rng(3)
    n2 = rng.integers(1, 50, 100).astype(np.int32)
    lab2 = rng.permutation(2086)[:100].astype(np.uint16)
    lab2[:64] |= ro.BANNED                                                # only the lanes' second edges count
    w2 = rng.uniform(-2, 2, 100) * n2
    special.append((lab2, n2, w2, 100, ro.root_maxq(lab2, n2, w2)))
    R = len(rows) + len(special)
    lab = np.zeros((R, M), dtype=np.uint16)
    n = np.full((R, M), 1, dtype=np.int32)
    w = np.full((R, M), 50.0, dtype=np.float64)                           # past n_edges: values that would win if read
    ne = np.zeros(R, dtype=np.uint8)
    want = np.zeros(R, dtype=np.float64)
    for i, (l, nn_, ww, c) in enumerate(rows):
        lab[i, :c], n[i, :c], w[i, :c], ne[i] = l, nn_[:c], ww[:c], c
        want[i] = ro.root_maxq(l, nn_[:c], ww[:c])
    for i, (l, nn_, ww, c, v) in enumerate(special, start=len(rows)):
        lab[i, :c], n[i, :c], w[i, :c], ne[i], want[i] = l, nn_, ww, c, v
    args = [t.from_numpy(lab.view(np.int16)).cuda().view(t.uint16), t.from_numpy(n).cuda(), t.from_numpy(w).cuda(),
            t.from_numpy(ne).cuda()]
    out = gpu.S.root_maxq_rows(*args).cpu().numpy()
    assert gpu.S.Search.root_maxq_rows is gpu.S.root_maxq_rows
    assert out.tobytes() == want.tobytes(), (out, want)
    L = gpu.N.lib()
    po = C.c_void_p(t.empty(R, dtype=t.float64, device="cuda").data_ptr())
    ptr = [C.c_void_p(x.data_ptr()) for x in args]
    stream = C.c_void_p(t.cuda.current_stream().cuda_stream)
    for i in range(4):
        assert L.cz_root_maxq(*(ptr[:i] + [None] + ptr[i + 1:]), R, po, stream) == ERR_ARG, i
    assert L.cz_root_maxq(*ptr, R, None, stream) == ERR_ARG
    assert L.cz_root_maxq(*ptr, -1, po, stream) == ERR_ARG
    assert L.cz_root_maxq(*ptr, 0, po, stream) == 0


# ---- set_resign_threshold ------------------------------------------------------------------------------------------------------
def _records(games):
    return [(gid, g["turns"], g["value"], g["resigned"], g["store"], g["data"],
             [(e.ply, e.resign, e.no_resign, e.maxq, e.n.tobytes(), e.moves.tobytes()) for e in g["visits"]])
            for gid, g in sorted(games.items())]


@pytest.mark.parametrize("graph", [False, True])
def test_threshold_set_before_start_plays_the_games_of_an_engine_created_with_it(gpu, graph):
    kw = dict(simulation_num_per_move=24, search_threads=4, max_game_length=12, enable_resign_rate=0.0)
    stop = lambda eng: eng.rounds >= 640  # noqa: E731  (a fixed number of rounds: the same games in both runs)
    made, c0 = _engine_run(gpu, ro.play_config(resign_threshold=0.1, **kw), 5, graph=graph, stop=stop)

    def setter(eng):
        assert eng.resign_threshold == -0.92
        eng.set_resign_threshold(0.1)
        assert eng.resign_threshold == eng.search.resign_threshold == 0.1
    set_, c1 = _engine_run(gpu, ro.play_config(resign_threshold=-0.92, **kw), 5, graph=graph, before_start=setter, stop=stop)
    assert len(made) >= G and c0["resigns"] > 0
    assert _records(set_) == _records(made) and c1 == c0
    # ... and not those of the engine left at -0.92
    left, c2 = _engine_run(gpu, ro.play_config(resign_threshold=-0.92, **kw), 5, graph=graph, stop=stop)
    assert c2["resigns"] < c0["resigns"] and _records(left) != _records(made)


@pytest.mark.parametrize("graph", [False, True])
def test_threshold_set_in_mid_run_resigns_only_at_plies_chosen_after_the_call(gpu, graph):
    pc = ro.play_config(simulation_num_per_move=24, search_threads=4, max_game_length=30, enable_resign_rate=0.0,
                        resign_threshold=-5.0)
    before = {}

    def mid(eng, drained):
        # everything chosen so far: the finished games and what waits for its game's record
        for gid, g in drained.items():
            before[gid] = list(g["visits"])
        for gid, ents in eng.search.waiting_visits().items():
            before[gid] = list(ents)
        old = eng._graph
        assert (old is not None) == graph
        eng.set_resign_threshold(0.1)
        assert (eng._graph is not None) == graph and (not graph or eng._graph is not old)     # captured again
        with pytest.raises(ValueError):
            eng.set_resign_threshold(float("nan"))
        assert eng.resign_threshold == 0.1
    games, ctr = _engine_run(gpu, pc, 9, graph=graph, mid=mid, rounds_before=96)
    seen_before = {(gid, e.ply) for gid, ents in before.items() for e in ents}
    assert seen_before and not any(e.resign for ents in before.values() for e in ents)
    # the old threshold was in force: plies the new one would have resigned at were played on
    assert any(e.ply > MRT and e.maxq < 0.1 for ents in before.values() for e in ents)
    n_resigned = 0
    for gid, g in games.items():
        for e in g["visits"]:
            if (gid, e.ply) in seen_before:
                assert not e.resign, (gid, e.ply)
            elif e.ply > MRT:
                assert e.resign == (e.maxq < 0.1), (gid, e.ply, e.maxq)  # chosen after the call: the new threshold
                n_resigned += e.resign
    assert n_resigned > 0 and ctr["resigns"] == n_resigned


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_settings(gpu):
    pc = play_config(simulation_num_per_move=16, search_threads=4, max_game_length=6)
    s = gpu.S.Search(pc, 2, seed=1)
    st, L = s._stream(), s.L
    assert L.cz_search_record_maxq(s.h, 1, st) == ERR_ARG               # without the visit ring
    with pytest.raises(gpu.N.NativeError):
        s.record_maxq(True)
    assert not s.maxq_on
    assert L.cz_search_record_maxq(s.h, 0, st) == 0 and L.cz_search_record_maxq(None, 1, st) == ERR_ARG
    n = C.c_int(-1)
    buf = np.zeros((64, gpu.S.VISIT_STRIDE), dtype=np.uint8)
    mb = np.zeros(64, dtype=np.float64)
    s.record_visits(True, capacity=64)
    assert drain_cols(s, buf, (None, None, mb), 64, C.byref(n)) == ERR_ARG     # a buffer for a record that is off
    s.record_maxq(True)
    assert s.maxq_on
    assert drain_cols(s, None, (None, None, None), 0, C.byref(n)) == 0 and n.value == 0
    # a NULL column for a record that is on: not copied, no error, and the record stays on
    assert drain_cols(s, buf, (None, None, None), 64, C.byref(n)) == 0 and n.value == 0 and s.maxq_on
    assert drain_cols(s, buf, (mb, None, mb), 64, C.byref(n)) == ERR_ARG       # a q column with the value record off
    assert drain_cols(s, buf, (None, None, mb), 64, C.byref(n)) == 0
    assert L.cz_search_root_maxq(s.h, None, st) == ERR_ARG
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert L.cz_search_set_resign_threshold(s.h, bad, st) == ERR_ARG
        with pytest.raises(gpu.N.NativeError):
            s.set_resign_threshold(bad)
    assert L.cz_search_set_resign_threshold(None, 0.0, st) == ERR_ARG
    assert s.resign_threshold == pc.resign_threshold
    # the plain drain keeps working with columns on, and the entries carry the number through the binding
    s.start_selfplay(seed=1)
    ev = stub_eval(gpu, ro.SPEC)
    for _ in range(40):
        s.round()
        p, v = ev(s.planes)
        s.policy.copy_(p)
        s.value.copy_(v)
    ents = [e for es in s.waiting_visits().values() for e in es]
    assert ents and all(e.maxq is not None and e.no_resign and e.q is None and e.s is None for e in ents)
    for _ in range(8):
        s.round()
        p, v = ev(s.planes)
        s.policy.copy_(p)
        s.value.copy_(v)
    assert L.cz_search_drain_visits(s.h, buf.ctypes.data, 64, C.byref(n), None, st) == 0 and n.value > 0
    s.record_visits(False)                                               # the visit ring going takes this ring with it
    assert not s.maxq_on and L.cz_search_record_maxq(s.h, 1, st) == ERR_ARG
    s.close()
    from cchess_alphazero.engine import SelfPlayEngine
    with pytest.raises(ValueError, match="record_visits"):
        SelfPlayEngine(_engine_cfg(pc), 2, evaluator=stub_eval(gpu, ro.SPEC), resign_audit=True)


# ---- the command line --------------------------------------------------------------------------------------------------------------
def test_run_py_self_with_resign_audit(tmp_path):
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "chinesechess-alphazero_amd")
    env = dict(os.environ, DATA_DIR=str(tmp_path / "data"), PROJECT_DIR=str(tmp_path), PYTHONPATH=pkg)
    run = [sys.executable, os.path.join(pkg, "cchess_alphazero", "run.py"), "self", "--type", "mini"]
    r = subprocess.run(run + ["--resign-audit"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "needs --record-visits" in r.stderr
    r = subprocess.run(run + ["--games-per-gpu", "32", "--record-visits", "--resign-audit", "--resign-fp-target", "0.3",
                              "--max-games", "8"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(tmp_path / "logs" / "play.log") as f:
        log = f.read()
    assert "resignation audit of the no-resign games, threshold -0.92, false-positive target 0.3" in log
    m = re.findall(r"resign audit: (\d+) games audited \((\d+) skipped\); at threshold (-?[0-9.]+) (\d+) would have resigned, "
                   r"(\d+) of them false positives", log)
    # (at `mini` nine games in ten may resign, enable_resign_rate 0.1, and are skipped: whether one of the first eight is
    #  audited is the lottery's business; the histogram itself is tested above)
    assert m and int(m[-1][0]) + int(m[-1][1]) >= 8 and int(m[-1][4]) <= int(m[-1][3]) <= int(m[-1][0])
    with open(tmp_path / "data" / "play_data" / "resign_audit_0.json") as f:
        d = json.load(f)
    assert d["games"] == int(m[-1][0]) and d["skipped"] == int(m[-1][1]) and len(d["would"]) == 101
    tool = subprocess.run([sys.executable, os.path.join(root, "tools", "resign_audit.py"), "--target", "0.3",
                           str(tmp_path / "data" / "play_data" / "resign_audit_0.json")], capture_output=True, text=True,
                          timeout=120)
    assert tool.returncode == 0 and f"{d['games']} games audited, {d['skipped']} skipped, 1 file(s)" in tool.stdout
