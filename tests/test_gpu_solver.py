"""-m gpu: the MCTS solver (cz_search_set_solver, cz_search_node_proof, cz_search_root_decided; run.py self / eval --solver).

The yardstick is tests/solver_oracle.py, a Python restatement of the reference's search for one search thread with the
solver's definitions (include/czero.h) in it; tests/test_solver_cpu.py pins it to forced_playouts_oracle.Search with the
rules off and to a minimax for soundness.  K = 1 searches and played lines are compared with it exactly -- no tolerance: no
transcendental function is involved --, K = 8 is held by invariants, and a search that had the solver switched on and off
again is the search that never had it, bit for bit."""
import ctypes as C
import json

import numpy as np
import pytest

import forced_playouts_oracle as fo
import solver_oracle as so
from oracle import xq_oracle as xo
from test_gpu_book import _engine_cfg
from test_gpu_search import (assert_root_equal, boards_tensor, gpu, no_act_tensors, play_config, stub_eval)  # noqa: F401

pytestmark = pytest.mark.gpu
ERR_ARG = -1                                                # include/czero.h CZ_ERR_ARG
OPEN, WIN, LOSS = so.OPEN, so.WIN, so.LOSS
COUNTERS = ("sims", "expansions", "terminal_sims", "repetition_sims", "proven_sims")


def _pc(sims, K=1, **kw):
    return play_config(simulation_num_per_move=sims, search_threads=K, noise_eps=0.0, tau_decay_rate=0.0, **kw)


def _searches():
    """(name, state, salt, sims) of every single search: the fixtures at each of their budgets, the nine ordinary positions."""
    out = [(p["name"], p["state"], so.SALT, sims) for p in so.positions() for sims in p["sims"]]
    return out + [("fo:" + c["name"], c["state"], c["salt"], 64) for c in fo.cases()]


def _assert_proof_equal(got, want, nm, what):
    """got: node_proof() of a G = 1 search; want: Search.proof() or None (the position is not a node of the tree)."""
    if want is None:
        assert int(got["status"][0]) == -1, what
        return
    assert (int(got["status"][0]), int(got["dist"][0])) == (want["status"], want["dist"]), (what, got["status"], got["dist"], want)
    assert got["mark"][0, :nm].tolist() == want["mark"], (what, got["mark"][0, :nm], want["mark"])
    assert got["mark_dist"][0, :nm].tolist() == want["mark_dist"], (what, got["mark_dist"][0, :nm], want["mark_dist"])
    assert not got["mark"][0, nm:].any() and not got["mark_dist"][0, nm:].any(), what


def _assert_counters(ctr, o, what, base=None):
    for key in COUNTERS:
        assert ctr[key] - (base[key] if base else 0) == getattr(o, key), (what, key, ctr[key], getattr(o, key))


# ---- 1. K = 1 single searches against the oracle ---------------------------------------------------------------------------
def test_single_searches_match_the_oracle(gpu):
    seen = set()
    for name, state, salt, sims in _searches():
        o = so.Search(so.play_cfg(sims), salt)
        ran = o.search(state)
        s = gpu.S.Search(_pc(sims), 1, seed=7)
        s.set_solver(True)
        s.set_roots(boards_tensor(gpu, [state]))
        s.run_until_idle(stub_eval(gpu, dict(kind="hash", salt=salt)))
        what = f"{name} at {sims}"
        assert_root_equal(s.root_stats(), 0, o.node_stats(state), what)
        ctr = s.counters()
        _assert_counters(ctr, o, what)
        assert ctr["sims"] == ran and ctr["overflow_sims"] == 0 and ctr["tree_resets"] == 0, what
        root = o.tree[state]
        nm = len(root.moves)
        _assert_proof_equal(s.node_proof(), o.proof(state), nm, what)
        assert bool(s.root_decided()[0]) == o.decided(), what
        for j, mv in enumerate(root.moves):                 # every root child: a node, or -1 (terminal / never reached)
            child = xo.step(state, mv)
            linked = root.n[j] > 0 and not root.term[j]
            want = o.proof(child) if linked else None
            _assert_proof_equal(s.node_proof([root.labels[j]]), want, len(o.tree[child].moves) if want else 0, f"{what} child {j}")
        seen.add((o.proof(state)["status"], ran < sims, o.rule1(root) >= 64, o.proven_sims > 0))
        s.close()
    # the set shows what it is there for: OPEN / WIN / LOSS roots, early stops, a proof through edge >= 64, an arrival
    assert {st for st, _, _, _ in seen} == {OPEN, WIN, LOSS}
    assert any(early for _, early, _, _ in seen) and any(wide for _, _, wide, _ in seen) and any(arr for _, _, _, arr in seen)


# ---- 2. K = 1 played lines in external mode ------------------------------------------------------------------------------------
def _first_move(name, sims):
    pos = {p["name"]: p for p in so.positions()}[name]
    o = so.Search(so.play_cfg(sims), so.SALT)
    o.search(pos["state"])
    return o.play(pos["state"])


@pytest.mark.parametrize("name,sims,ban_first", [("m2", 128, False), ("wide_m2", 128, False), ("m1", 64, True)])
def test_played_lines_match_the_oracle(gpu, name, sims, ban_first):
    pos = {p["name"]: p for p in so.positions()}[name]
    bans = {0: [_first_move(name, sims)]} if ban_first else None       # ban_first: the ply whose winning edge is banned
    o = so.Search(so.play_cfg(sims), so.SALT)
    line, end = o.play_line(pos["state"], bans=bans)
    assert xo.done(end)[0] and len(line) >= 2
    t = gpu.torch
    s = gpu.S.Search(_pc(sims), 1, seed=7)
    s.set_solver(True)
    ev = stub_eval(gpu, dict(kind="hash", salt=so.SALT))
    idle = 0
    for ply, step in enumerate(line):
        na, nn = no_act_tensors(gpu, [step["no_act"]])
        before = s.counters()
        s.set_roots(boards_tensor(gpu, [step["state"]]), turns=t.tensor([ply], dtype=t.int32, device="cuda"), no_act=na, n_no_act=nn)
        s.run_until_idle(ev)
        what = f"{name} ply {ply}"
        assert s.counters()["sims"] - before["sims"] == step["ran"], what
        assert_root_equal(s.root_stats(), 0, step["stats"], what)
        _assert_proof_equal(s.node_proof(), step["proof"], len(step["stats"]["moves"]), what)
        assert xo.label_str(int(s.choose(None)[0])) == step["move"], what
        idle += step["ran"] == 0
    assert idle >= 1                                                    # plies that run no simulation
    if ban_first:
        assert line[0]["proof"]["status"] == WIN and line[0]["move"] != bans[0][0]
    else:
        assert len(line) == pos["want"]["dist"] - 1 and idle == len(line) - 1
    s.close()


# ---- 3. self-play from a book ----------------------------------------------------------------------------------------------------
def test_selfplay_from_a_book_wins_what_is_won(gpu):
    from cchess_alphazero.engine import SelfPlayEngine
    pos = {p["name"]: p for p in so.positions()}
    names = ["m1", "m2", "wide_m1"]
    book = [pos[n]["state"] for n in names]
    G = len(book)
    pc = _pc(128, max_game_length=100)
    eng = SelfPlayEngine(_engine_cfg(pc), G, evaluator=stub_eval(gpu, dict(kind="hash", salt=so.SALT)), seed=5, book=book,
                         book_rate=1.0, solver=True)
    i_games = gpu.S.COUNTER_NAMES.index("games")
    games = []
    try:
        eng.start(0, 0)
        for r in range(4000):
            eng.step()
            if r % 8 == 7:
                games += eng.drain()
                if eng.search.game_counters()[:, i_games].min() >= 1:
                    break
        else:
            raise AssertionError(f"not finished: {len(games)} games")
        games += eng.drain()
        ctr = eng.counters()
    finally:
        eng.close()
    assert ctr["tree_resets"] == 0 and ctr["overflow_sims"] == 0
    first = {g["game_id"]: g for g in games if g["game_id"] < G}
    assert sorted(first) == list(range(G))
    for gid, name in enumerate(names):
        g, d = first[gid], pos[name]["want"]["dist"]
        assert g["book_index"] == gid and g["data"][0] == book[gid]
        assert json.loads(json.dumps(g["data"])) == g["data"]           # the record parses
        moves = [it[0] for it in g["data"][1:]]
        # d - 1 searched plies, then the appended king capture; the first mover ("red") wins
        assert len(moves) == d and g["value"] == 1 and not g["resigned"], (name, moves)
        state = book[gid]
        for mv in moves[:d - 1]:
            assert not xo.done(state)[0] and mv in xo.get_legal_moves(state), (name, mv)
            state = xo.step(state, mv)
        assert xo.done(state)[:2] == (True, 1), name
        # ply 0 is the oracle's: the same search, the same move
        o = so.Search(so.play_cfg(128), so.SALT)
        o.search(book[gid])
        assert moves[0] == o.play(book[gid]), name


# ---- 4. K = 8 by invariants ----------------------------------------------------------------------------------------------------
def test_k_8_is_sound_stops_at_a_decided_root_and_counts(gpu):
    names = ["m1", "m2", "wide_m2", "lost"]
    pos = {p["name"]: p for p in so.positions()}
    states = [pos[n]["state"] for n in names]
    G, sims = len(states), 256
    s = gpu.S.Search(_pc(sims, K=8), G, seed=11)
    s.set_solver(True)
    ev = stub_eval(gpu, dict(kind="hash", salt=so.SALT))
    s.set_roots(boards_tensor(gpu, states))
    s.run_until_idle(ev)
    st, pr, ctr = s.root_stats(), s.node_proof(), s.counters()
    assert ctr["overflow_sims"] == 0 and ctr["tree_resets"] == 0
    memo, checked = {}, 0

    def sound(state, status, dist, what):
        nonlocal checked
        if status in (WIN, LOSS) and dist <= 5:
            assert so.minimax(state, max(0, dist - 1), memo) == status, (what, status, dist)
            checked += 1
    for g, name in enumerate(names):
        nm = int(st["counts"][g])
        # visit sums: every simulation but the one that made the root went through one root edge, all are backed up
        assert int(st["n"][g, :nm].sum()) == int(st["sum_n"][g]) - 1 and (st["n"][g, :nm] >= 0).all(), name
        assert int(st["sum_n"][g]) <= sims
        status, dist = int(pr["status"][g]), int(pr["dist"][g])
        sound(states[g], status, dist, name)
        if name in ("m1", "lost"):                                      # a mate in one of 36 moves, three moves that all lose
            assert status == pos[name]["want"]["status"], name
        moves = xo.get_legal_moves(states[g])
        for j in range(nm):
            mk, md = int(pr["mark"][g, j]), int(pr["mark_dist"][g, j])
            # a mark is the child's status from the CHILD's mover's view
            sound(xo.step(states[g], moves[j]), mk, md, f"{name} edge {j}")
        if status == WIN:                                               # the derive rule, on what the tree holds
            win = [int(pr["mark_dist"][g, j]) for j in range(nm) if pr["mark"][g, j] == LOSS]
            assert win and dist >= 1 + min(win)                         # (the first proof is final: later marks may be nearer)
        if status == LOSS:
            assert (pr["mark"][g, :nm] == WIN).all() and dist == min(so.DIST_MAX, 1 + int(pr["mark_dist"][g, :nm].max()))
    assert checked >= 8 and ctr["sims"] == int(st["sum_n"].sum())
    decided = s.root_decided().astype(bool)
    assert decided[names.index("m1")] and decided[names.index("lost")]
    assert (decided == np.isin(pr["status"], (WIN, LOSS))).all()           # (no bans: a proven root is a decided one)
    i_sims = gpu.S.COUNTER_NAMES.index("sims")
    per_game = s.game_counters()[:, i_sims].astype(np.int64)
    assert (per_game == st["sum_n"]).all() and (per_game[decided] < sims).all()
    # a decided root starts no batch: the same roots again cost those games no simulation, and their statistics stay
    s.set_roots(boards_tensor(gpu, states))
    s.run_until_idle(ev)
    st2 = s.root_stats()
    assert (s.game_counters()[:, i_sims].astype(np.int64)[decided] == per_game[decided]).all()
    assert st2["n"][decided].tobytes() == st["n"][decided].tobytes() and st2["w"][decided].tobytes() == st["w"][decided].tobytes()
    # the move of a won root is a winning edge
    act = s.choose(None)
    for g, name in enumerate(names):
        if int(pr["status"][g]) == WIN:
            j = st["moves"][g].tolist().index(int(act[g]))
            assert pr["mark"][g, j] == LOSS, name
    s.close()


# ---- 5. off is off ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8])
def test_solver_switched_off_again_is_a_search_that_never_had_it(gpu, K):
    states = [p["state"] for p in so.positions()] + [c["state"] for c in fo.cases()[:3]]
    G = len(states)
    ev = stub_eval(gpu, dict(kind="hash", salt=so.SALT))
    out = []
    for setup in (lambda s: None, lambda s: (s.set_solver(True), s.set_solver(False)), lambda s: s.set_solver(True)):
        s = gpu.S.Search(_pc(96, K=K), G, seed=3)
        setup(s)
        s.set_roots(boards_tensor(gpu, states))
        s.run_until_idle(ev)
        st = s.root_stats()
        out.append((st["n"].tobytes(), st["w"].tobytes(), st["p"].tobytes(), st["sum_n"].tobytes(), s.counters(),
                    s.node_proof()["status"].tolist(), s.choose(None).tolist()))
        s.close()
    plain, back, on = out
    assert back == plain
    assert plain[4]["proven_sims"] == 0 and plain[5] == [OPEN] * G         # the terminal codes alone prove nothing
    assert on[:4] != plain[:4] and WIN in on[5] and LOSS in on[5]           # ... and the solver does change the search


# ---- 6. arguments ------------------------------------------------------------------------------------------------------------------
def test_argument_refusals(gpu):
    t = gpu.torch
    s = gpu.S.Search(_pc(16, K=4), 2, seed=1)
    st = s._stream()
    L = s.L
    assert L.cz_search_set_solver(None, 1, st) == ERR_ARG
    for bad in (-1, 2, 7):
        assert L.cz_search_set_solver(s.h, bad, st) == ERR_ARG
    # the solver with Gumbel, with forced playouts, with the evaluation cache: refused both ways round
    s.set_gumbel(8)
    assert L.cz_search_set_solver(s.h, 1, st) == ERR_ARG
    s.set_gumbel(0)
    s.set_forced_playouts(2.0)
    assert L.cz_search_set_solver(s.h, 1, st) == ERR_ARG
    s.set_forced_playouts(0.0)
    s.set_eval_cache(10)
    assert L.cz_search_set_solver(s.h, 1, st) == ERR_ARG
    s.set_eval_cache(0)
    with pytest.raises(gpu.N.NativeError):
        s.set_gumbel(8), s.set_solver(True)
    s.set_gumbel(0)
    assert not s.solver
    s.set_solver(True)
    assert s.solver
    assert L.cz_search_set_gumbel(s.h, 8, 50.0, 1.0, st) == ERR_ARG
    assert L.cz_search_set_forced_playouts(s.h, 2.0, st) == ERR_ARG
    assert L.cz_search_set_eval_cache(s.h, 10, st) == ERR_ARG
    assert L.cz_search_set_gumbel(s.h, 0, 50.0, 1.0, st) == 0              # switching the others OFF is never refused
    assert L.cz_search_set_forced_playouts(s.h, 0.0, st) == 0
    # bad pointers, path_len out of range
    status = t.empty(2, dtype=t.int8, device="cuda")
    dist = t.empty(2, dtype=t.uint8, device="cuda")
    mark = t.empty((2, 128), dtype=t.uint8, device="cuda")
    path = t.zeros((2, 4), dtype=t.int16, device="cuda")
    p = [C.c_void_p(x.data_ptr()) for x in (path, status, dist, mark)]
    assert L.cz_search_node_proof(None, None, 0, p[1], p[2], p[3], p[3], st) == ERR_ARG
    assert L.cz_search_node_proof(s.h, None, 0, None, p[2], p[3], p[3], st) == ERR_ARG
    assert L.cz_search_node_proof(s.h, None, 0, p[1], None, p[3], p[3], st) == ERR_ARG
    assert L.cz_search_node_proof(s.h, None, 4, p[1], p[2], p[3], p[3], st) == ERR_ARG      # a path length without a path
    assert L.cz_search_node_proof(s.h, p[0], -1, p[1], p[2], p[3], p[3], st) == ERR_ARG
    assert L.cz_search_node_proof(s.h, p[0], 129, p[1], p[2], p[3], p[3], st) == ERR_ARG
    assert L.cz_search_node_proof(s.h, p[0], 4, p[1], p[2], None, None, st) == 0            # the per-edge outputs are optional
    assert L.cz_search_root_decided(None, p[2], st) == ERR_ARG
    assert L.cz_search_root_decided(s.h, None, st) == ERR_ARG
    # nothing searched yet: no root is linked, nothing is decided
    assert s.node_proof()["status"].tolist() == [-1, -1] and s.root_decided().tolist() == [0, 0]
    s.close()
    # the engine and the command line refuse the pairs before the library has to
    from cchess_alphazero import manager
    from cchess_alphazero.engine import SelfPlayEngine
    ev = stub_eval(gpu, dict(kind="hash", salt=1))
    for kw, msg in ((dict(gumbel=8, record_visits=True), "gumbel"), (dict(forced_playouts=2.0, record_visits=True), "forced"),
                    (dict(eval_cache=10), "eval_cache")):
        with pytest.raises(ValueError, match=msg):
            SelfPlayEngine(_engine_cfg(_pc(16, K=4)), 2, evaluator=ev, solver=True, **kw)
    for extra in (["--gumbel", "8", "--record-visits"], ["--forced-playouts", "2", "--record-visits"], ["--eval-cache", "10"]):
        with pytest.raises(SystemExit, match="--solver excludes"):
            manager.build_config(manager.create_parser().parse_args(["self", "--solver"] + extra))
    assert manager.build_config(manager.create_parser().parse_args(["eval", "--solver"])).engine.solver is True
    assert manager.build_config(manager.create_parser().parse_args(["self"])).engine.solver is False
