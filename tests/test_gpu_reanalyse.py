"""-m gpu: scripted games (cz_search_set_script, SelfPlayEngine(script=...), run.py reanalyse).

The device walks stored games again: the moves, the turns and the result are the script's, and every ply's search is compared,
entry by entry and with no tolerance, with tests/reanalyse_oracle.py -- selfplay_oracle's game loop played by one oracle
player whose move is the script's.  The network is the exact stub of tests/stub_net.py, as in test_gpu_book.py; the scripts
come from games the CPU oracle played under ANOTHER stub and seed, so that most scripted moves are not the search's own."""
import functools
import json
import os

import numpy as np
import pytest

import game_endings as ge
import playout_cap_oracle as pco
import q_record_oracle as qo
import reanalyse_oracle as ro
import selfplay_oracle as so
import surprise_oracle as sur
from conftest import load_golden
from oracle import xq_oracle as xo
from test_gpu_book import _engine_cfg
from test_gpu_search import gpu, play_config, stub_eval  # noqa: F401  (gpu: fixture)

pytestmark = pytest.mark.gpu
GEN_SPEC, GEN_SEED = dict(kind="hash", salt=31), 77          # who played the stored games
RUN_SPEC, RUN_SEED = dict(kind="hash", salt=5), 19           # who walks them again
G = 4
BANNED = 0x8000


def _pc(K=1, sims=20, mgl=8, **kw):
    return play_config(simulation_num_per_move=sims, search_threads=K, tau_decay_rate=0.9, max_game_length=mgl, noise_eps=0.0,
                       enable_resign_rate=0.5, resign_threshold=-0.4, min_resign_turn=4, **kw)


def _record(init, moves, z):
    return [init] + [[m, z if i % 2 == 0 else -z] for i, m in enumerate(moves)]


@functools.lru_cache(maxsize=None)
def stored_games():
    """Six games of the CPU oracle under GEN_SPEC / GEN_SEED, as (init_state, moves, z): four from the opening position, two
    from book positions; computed once and never changed."""
    book = load_golden("book_games.json")["book"]
    cfg = so.oracle_cfg(_pc(sims=16))
    out = []
    for gid in range(6):
        g = so.selfplay_game(cfg, GEN_SPEC, GEN_SEED, gid, init_state=None if gid < 4 else book[gid % len(book)])
        # (these short games all end drawn at the length cap; a script's z is whatever its producer says, so say more)
        out.append((g["init_state"], tuple(g["moves"]), (1, -1, 0)[gid % 3]))
    return tuple(out)


def _walk(gpu, pc, games, spec=RUN_SPEC, seed=RUN_SEED, max_rounds=20000, **kw):
    """Walk `games` [(init_state, moves, z)] through SelfPlayEngine(script=...) on G slots until no slot is searching.
    Returns (the drained games by script index, what 32 further rounds drained, the counters)."""
    from cchess_alphazero.engine import SelfPlayEngine
    from cchess_alphazero.lib import reanalyse as ra
    scripts, kept, aside = ra.pack_scripts([_record(*g) for g in games], 2 * pc.max_game_length + 3)
    assert not aside and len(kept) == len(games)
    eng = SelfPlayEngine(_engine_cfg(pc), G, evaluator=stub_eval(gpu, spec), seed=seed, record_visits=True, script=scripts, **kw)
    out = []
    try:
        eng.start(0)
        for r in range(max_rounds):
            eng.step()
            if r % 16 == 15:
                idle = eng.search.pending() == 0
                out += eng.drain()
                if idle:
                    break
        else:
            raise AssertionError(f"still searching after {max_rounds} rounds: {len(out)} games")
        for _ in range(32):
            eng.step()
        late = eng.drain()
        ctr = eng.counters()
    finally:
        eng.close()
    assert ctr["tree_resets"] == 0 and ctr["overflow_sims"] == 0 and ctr["visits_dropped"] == 0
    assert all(g["script_index"] == g["game_id"] for g in out)
    return {g["script_index"]: g for g in out}, late, ctr


def _moves(g):
    return [item[0] for item in g["data"][1:]]


def _assert_script(g, game, what):
    """The drained game is the script: start position, moves, turns, z; stored, not resigned, no mismatch."""
    init, moves, z = game
    assert g["data"][0] == init, what
    assert _moves(g) == list(moves) and g["turns"] == len(moves), (what, _moves(g), moves)
    assert [it[1] for it in g["data"][1:]] == [z if i % 2 == 0 else -z for i in range(len(moves))], what
    assert (g["value"], g["store"], g["resigned"], g["script_mismatch"], g["book_index"]) == (z, True, False, False, None), what


def _assert_entries(g, trace, what):
    """Every visit entry is the scripted oracle's root of that ply: moves, counts, the root's own count; no tolerance."""
    vis = g["visits"]
    assert vis is not None and len(vis) == len(trace), (what, len(vis or []), len(trace))
    for t, (e, ref) in enumerate(zip(vis, trace)):
        assert e.ply == t and e.sum_n == ref["sum_n"], (what, t, e.sum_n, ref["sum_n"])
        assert len(e.moves) == len(ref["moves"]) and (e.moves == ref["moves"]).all(), (what, t)
        assert (e.n == ref["n"]).all(), (what, t, e.n, ref["n"])
        assert [xo.label_str(int(m)) for m, b in zip(e.moves, e.banned) if b] == \
               [m for m in map(xo.label_str, map(int, e.moves)) if m in ref["no_act"]], (what, t)
        assert e.resign == (ref["scripted"] is None), (what, t)


def _oracle(pc, K, gid, game, **kw):
    trace = []
    out = ro.scripted_game(so.oracle_cfg(pc, K=K), RUN_SPEC, RUN_SEED, gid, game[1], init_state=game[0], trace=trace, **kw)
    return out, trace


# ---- 1. parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8])
def test_scripted_games_are_searched_as_the_oracle_searches_them(gpu, K):
    """6 scripts on 4 slots: two slots take a second script, two go idle."""
    games = stored_games()
    pc = _pc(K=K)
    traces = [_oracle(pc, K, i, g) for i, g in enumerate(games)]
    # (CPU side) the scripts hold what the kernel has to get right: moves the search never visited, and visited moves that
    # are not the search's own choice
    plies = [e for _, tr in traces for e in tr if e["scripted"] is not None]
    visits_of = lambda e: int(e["n"][[xo.label_str(int(m)) for m in e["moves"]].index(e["scripted"])])  # noqa: E731
    unvisited = sum(1 for e in plies if visits_of(e) == 0)
    other = sum(1 for e in plies if visits_of(e) > 0 and e["scripted"] != e["action"])
    assert unvisited >= 5 and other >= 5, (unvisited, other, len(plies))
    got, late, ctr = _walk(gpu, pc, games)
    assert sorted(got) == list(range(6)) and late == []             # exactly six records, and further rounds produce none
    for i, game in enumerate(games):
        _assert_script(got[i], game, (K, i))
        out, trace = traces[i]
        assert out["moves"][:out["searched"]] == list(game[1][:out["searched"]])
        _assert_entries(got[i], trace, (K, i))
        # a record item per move: pi where the ply was searched, the two-field form for an appended king capture
        for t, it in enumerate(got[i]["data"][1:]):
            assert len(it) == (3 if t < out["searched"] else 2), (K, i, t)
    assert ctr["games"] == 6 and ctr["script_mismatch"] == 0 and ctr["resigns"] == 0
    assert ctr["plies"] == sum(len(tr) for _, tr in traces)


# ---- 2. endings ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _endings():
    c = load_golden("endings_games.json")["configs"][0]
    return c, {g["game_id"]: (g["position"], tuple(g["moves"]), int(g["value"])) for g in c["games"]}


def _ban_line():
    """A recorded game up to a ply at which the loop bans a move, followed by that banned move: (game, ply)."""
    c, games = _endings()
    init, moves, _ = games[6]
    cl = ge.classify(init, list(moves), c["max_game_length"])
    t = cl["ban_plies"][0]
    return (init, moves[:t] + (cl["bans"][t][0],), 1), t


def test_endings_king_capture_cut_and_a_banned_scripted_move(gpu):
    c, games = _endings()
    capture = games[3]                                              # its last move is the king capture the loop appends
    cl = ge.classify(capture[0], list(capture[1]), c["max_game_length"])
    assert cl["ending"] == "king_capture" and cl["searched"] == cl["turns"] - 1
    cut = (games[13][0], games[13][1][:10], -1)                     # stops while the rules say play on; z is the script's
    assert ge.classify(cut[0], list(cut[1]), c["max_game_length"])["ending"] == "resign"
    ban, t_ban = _ban_line()
    cb = ge.classify(ban[0], list(ban[1]), c["max_game_length"])
    assert cb["ending"] == "resign" and ban[1][t_ban] in cb["bans"][t_ban]
    pc = _pc(K=4, sims=16, mgl=c["max_game_length"])
    scripts = [capture, cut, ban]
    got, late, ctr = _walk(gpu, pc, scripts)
    assert sorted(got) == [0, 1, 2] and late == [] and ctr["script_mismatch"] == 0
    for i, game in enumerate(scripts):
        _assert_script(got[i], game, i)
        out, trace = _oracle(pc, 4, i, game)
        _assert_entries(got[i], trace, i)
    # the king capture: the script's last move, not searched
    assert len(got[0]["visits"]) == got[0]["turns"] - 1 == cl["searched"] and len(got[0]["data"][-1]) == 2
    # the cut script: the position after its last move is searched and says "no move"; z kept, no resigned flag
    assert len(got[1]["visits"]) == 11 and got[1]["visits"][-1].resign and got[1]["value"] == -1 and not got[1]["resigned"]
    # the banned move: its edge is flagged, it is not in the record's pi, and the board went on to the position behind it
    e = got[2]["visits"][t_ban]
    j = [xo.label_str(int(m)) for m in e.moves].index(ban[1][t_ban])
    assert e.banned[j] and ban[1][t_ban] not in [m for m, _ in got[2]["data"][1 + t_ban][2]]
    after = cb["states"][t_ban + 1]
    assert [xo.label_str(int(m)) for m in got[2]["visits"][t_ban + 1].moves] == xo.get_legal_moves(after)


def test_ending_at_the_length_cap_on_the_scripts_last_move(gpu):
    c, games = _endings()
    init, moves, _ = games[13]
    game = (init, moves[:12], 0)
    assert ge.classify(init, list(moves[:12]), 6)["ending"] == "length"
    pc = _pc(K=4, sims=16, mgl=6)
    got, late, ctr = _walk(gpu, pc, [game])
    assert sorted(got) == [0] and late == [] and ctr["script_mismatch"] == 0
    _assert_script(got[0], game, "length")
    out, trace = _oracle(pc, 4, 0, game)
    assert len(trace) == 12                                         # the rules ended it: no search after the last move
    _assert_entries(got[0], trace, "length")


# ---- 3. mismatch ---------------------------------------------------------------------------------------------------------
def test_mismatches_are_flagged_counted_and_never_stepped(gpu):
    c, games = _endings()
    good = stored_games()
    # an illegal move in the middle: a label the position at ply 5 does not have
    init, moves, z = good[0]
    state = init
    for m in moves[:5]:
        state, _ = xo.new_step(state, m)
    legal = set(xo.get_legal_moves(state))
    bad = next(xo.label_str(i) for i in range(2086) if xo.label_str(i) not in legal)
    illegal = (init, moves[:5] + (bad,) + moves[6:], z)
    # two extra moves after the rules have ended the game
    cap = games[3]
    extra = (cap[0], cap[1] + moves[:2], cap[2])
    n_cap = len(cap[1])
    scripts = [illegal, extra, good[1], good[2], good[3], good[4]]   # slots 0 and 1 go on with scripts 4 and 5
    pc = _pc(K=4, sims=16, mgl=8)
    got, late, ctr = _walk(gpu, pc, scripts)
    assert sorted(got) == list(range(6)) and late == []
    assert ctr["script_mismatch"] == 2 and ctr["games"] == 6
    a, b = got[0], got[1]
    assert a["script_mismatch"] and not a["store"] and not a["resigned"]
    assert a["turns"] == 5 and _moves(a) == list(moves[:5])         # the moves before the bad one, and nothing of it
    assert len(a["visits"]) == 6                                    # plies 0 .. 5 were searched, none after
    assert b["script_mismatch"] and not b["store"]
    assert b["turns"] == n_cap - 1 and _moves(b) == list(cap[1][:n_cap - 1])     # the king capture is not appended either
    assert len(b["visits"]) == n_cap - 1
    # the scripts after them, in the same slots and in the others, come out right: their first root is their own start
    for i in range(2, 6):
        _assert_script(got[i], scripts[i], i)
        out, trace = _oracle(pc, 4, i, scripts[i])
        _assert_entries(got[i], trace, i)
        assert [xo.label_str(int(m)) for m in got[i]["visits"][0].moves] == xo.get_legal_moves(scripts[i][0])


def test_the_librarys_refusals_are_the_python_tables(gpu):
    """cz_search_set_script beside each excluded feature, and each of them beside a script; a book and the max-q record."""
    from cchess_alphazero import search_options as sopt
    from cchess_alphazero.lib import reanalyse as ra
    from test_gpu_search_options import ERR_ARG, FEATURES
    scripts, _, _ = ra.pack_scripts([_record(*stored_games()[0])], 19)
    s = gpu.S.Search(_pc(K=4, sims=16), 2, seed=1)
    st = s._stream()
    err = lambda: s.L.cz_last_error().decode()  # noqa: E731
    try:
        with pytest.raises(gpu.N.NativeError):                      # needs the visit record
            s.set_script(*scripts)
        s.record_visits(True)
        excluded = {k for k, _ in sopt.SCRIPT_EXCLUDES}
        for key, f in FEATURES.items():
            f.wrap_on(s)
            if key in excluded:
                with pytest.raises(gpu.N.NativeError):
                    s.set_script(*scripts)
                assert err() == f"cz_search_set_script: {f.phrase}"
            else:
                s.set_script(*scripts)
                s.set_script()
            f.wrap_off(s)
            s.set_script(*scripts)
            rc = f.on(s.L, s.h, st)
            assert (rc == ERR_ARG) == (key in excluded), key
            if key in excluded:
                assert err() == f"{f.entry}: a script is set (cz_search_set_script)"
            assert f.off(s.L, s.h, st) == 0
            s.set_script()
        boards = np.stack([xo.state_to_board(xo.INIT_STATE)])
        s.set_book(boards, 1.0)
        with pytest.raises(gpu.N.NativeError):
            s.set_script(*scripts)
        s.set_book(None)
        s.record_maxq(True)
        with pytest.raises(gpu.N.NativeError):
            s.set_script(*scripts)
        s.record_maxq(False)
        s.set_script(*scripts)
        for call in (lambda: s.set_book(boards, 1.0), lambda: s.record_maxq(True), lambda: s.record_visits(False)):
            with pytest.raises(gpu.N.NativeError):
                call()
            assert err().endswith("a script is set (cz_search_set_script)")
        assert s.counters()["script_mismatch"] == 0
    finally:
        s.close()


# ---- 4. with options -----------------------------------------------------------------------------------------------------
def test_scripted_games_with_q_surprise_and_a_playout_cap(gpu):
    t = gpu.torch
    games = stored_games()[:4]
    pc = _pc(K=1, sims=20)
    got, late, ctr = _walk(gpu, pc, games, record_q=True, record_surprise=True, fast_sims=8, full_rate=0.5)
    assert sorted(got) == list(range(4)) and late == []
    n_fast = n_full = 0
    for i, game in enumerate(games):
        _assert_script(got[i], game, i)
        out, trace = _oracle(pc, 1, i, game, fast_sims=8, full_rate=0.5)
        _assert_entries(got[i], trace, i)
        vis = got[i]["visits"]
        rows = len(trace)
        lab = np.zeros((rows, 128), np.uint16)
        n = np.zeros((rows, 128), np.int32)
        w = np.zeros((rows, 128), np.float64)
        p = np.zeros((rows, 128), np.float32)
        for r, e in enumerate(trace):
            c = len(e["moves"])
            ban = np.array([xo.label_str(int(m)) in e["no_act"] for m in e["moves"]])
            lab[r, :c] = np.where(ban, e["moves"] | BANNED, e["moves"])
            n[r, :c], w[r, :c], p[r, :c] = e["n"], e["w"], e["p"]
        dev = [t.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x).cuda() for x in (lab, n, w, p)]
        dev[0] = dev[0].view(t.uint16)
        ne = t.tensor([len(e["moves"]) for e in trace], dtype=t.uint8, device="cuda")
        want_q = gpu.S.root_value_rows(dev[0], dev[1], dev[1], dev[2], ne).cpu().numpy()
        want_s = gpu.S.root_surprise_rows(dev[0], dev[1], dev[3], ne).cpu().numpy()
        for r, (e, ref) in enumerate(zip(vis, trace)):
            fast = not pco.ply_is_full(RUN_SEED, i, r, 8, 0.5)
            assert e.fast == fast == ref["fast"], (i, r)
            assert qo.same_value(qo.NAN if e.q is None else e.q, float(want_q[r]), 1e-13), (i, r, e.q, want_q[r])
            _, A = sur.surprise(lab[r, :len(ref["moves"])], ref["n"], ref["p"])
            assert sur.same(sur.NAN if e.s is None else e.s, float(want_s[r]), A), (i, r, e.s, want_s[r])
            if ref["scripted"] is None:
                continue
            it = got[i]["data"][1 + r]
            assert len(it) == 6 and it[3] == (0 if fast else 1), (i, r, it)
            assert it[4] == (None if e.q is None else round(e.q, 6)) and it[5] == (None if e.s is None else round(e.s, 6))
            n_fast += fast
            n_full += not fast
    assert n_fast >= 5 and n_full >= 5


# ---- 5. end to end -------------------------------------------------------------------------------------------------------
def test_run_py_reanalyse_end_to_end(gpu, tmp_path, monkeypatch):
    """run.py reanalyse through the command line's configuration: three small files, one in the reference's two-field form,
    a random-init best model."""
    from cchess_alphazero import manager
    from cchess_alphazero.lib.data_helper import read_game_data_from_file
    from cchess_alphazero.lib.record_decoder import split_games
    from cchess_alphazero.lib.replay_window import ReplayWindow
    from cchess_alphazero.worker import reanalyse as wr
    from cchess_alphazero.worker.self_play import load_model
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    monkeypatch.delenv("CZ_BOOK", raising=False)
    games = stored_games()
    records, out_dir = tmp_path / "data" / "trained", tmp_path / "data" / "play_data"
    records.mkdir(parents=True)
    files = {"play_a.json": [_record(*games[0]), _record(*games[4])],                         # the reference's own form
             "play_b.json": [[g[0]] + [it + [[[it[0], 3]]] for it in g[1:]] for g in map(lambda x: _record(*x), games[1:3])],
             "play_c.json": [_record(*games[3]), _record(*games[5])]}
    for name, gs in files.items():
        (records / name).write_text(json.dumps([x for g in gs for x in g]))
    cfg = manager.build_config(manager.create_parser().parse_args(
        ["reanalyse", "--type", "mini", "--sims", "16", "--games-per-gpu", "4", "--reanalyse-plies", "40", "--record-q"]))
    cfg.play.max_game_length, cfg.play.noise_eps = 8, 0.0
    cfg.engine.report_every_rounds, cfg.engine.use_hip_graph = 8, False
    assert cfg.engine.record_visits and wr.ReanalyseWorker(cfg).records_dir == str(records)
    cfg.resource.create_directories()
    model, _ = load_model(cfg)
    w = wr.ReanalyseWorker(cfg, model=model)
    seen = []
    make = w._engine_for

    def spy(scripts):                                               # every drained game, with its visit entries
        eng = make(scripts)
        if not hasattr(eng, "_drain"):
            eng._drain = eng.drain
            eng.drain = lambda *a, **k: [seen.append(g) or g for g in eng._drain(*a, **k)]
        return eng
    w._engine_for = spy
    try:
        total = w.run()
    finally:
        w.close()
    visits = {(g["data"][0], tuple(it[0] for it in g["data"][1:])): g["visits"] for g in seen}
    assert len(seen) == len(visits) == 6
    n_games, n_plies = 6, sum(len(g[1]) for g in games)
    assert (total["files"], total["games"], total["plies"], total["mismatches"], total["skipped"]) == (3, n_games, n_plies, 0, 0)
    assert sorted(os.listdir(records / "reanalysed")) == sorted(files) and not list(records.glob("*.json"))
    win = ReplayWindow(10 ** 5)
    for name, gs in files.items():
        back = split_games(read_game_data_from_file(str(out_dir / name)))
        assert [(g[0], [it[:2] for it in g[1:]]) for g in back] == [(g[0], [it[:2] for it in g[1:]]) for g in gs], name
        for g in back:
            for it in g[1:]:
                if len(it) == 2:
                    continue                                         # an appended king capture
                assert len(it) == 5 and it[3] == 1
        for g in back:                                               # every full ply's pi sums to the ply's root visits
            vis = visits[(g[0], tuple(it[0] for it in g[1:]))]
            for t, it in enumerate(g[1:]):
                if len(it) > 2:
                    assert sum(c for _, c in it[2]) == int(vis[t].n[~vis[t].banned].sum()) > 0, (name, t)
        assert win.load_file(str(out_dir / name)) == sum(len(g) - 1 for g in gs)
    idx = gpu.torch.arange(len(win), dtype=gpu.torch.int32, device="cuda")
    dense = win.dense_targets(idx, targets="visits")
    dense = np.asarray(dense.cpu() if hasattr(dense, "cpu") else dense, dtype=np.float64)
    assert dense.shape == (n_plies, 2086) and np.abs(dense.sum(1) - 1.0).max() < 1e-5
