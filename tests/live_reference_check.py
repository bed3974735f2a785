"""The oracle against the reference's own functions on freshly drawn positions, in two forms:

  * LIVE: imports the reference from its checkout (REF) -- whose package name, cchess_alphazero, is also the name of this
    repository's host package, so the two must not share an interpreter: this script runs in its own process -- and
    compares both sides on the spot;
  * GOLDEN (--golden): compares the oracle with the reference's results for the same draws as recorded in
    tests/golden/live_reference.json (`record`, run where the reference is present, writes that file).  Needs nothing
    outside the repository: this is what tests/test_oracle_live_reference.py runs.

    python tests/live_reference_check.py [--golden] rules   SEED GAMES MAX_PLIES CAPTURE_BIAS
    python tests/live_reference_check.py [--golden] history SEED GAMES MAX_PLIES CAPTURE_BIAS
    python tests/live_reference_check.py [--golden] mcts    SEED N_POSITIONS SIMS
    python tests/live_reference_check.py [--golden] games   SEED N_GAMES
    python tests/live_reference_check.py [--golden] arena   SEED N_GAMES
    python tests/live_reference_check.py [--golden] kgt1    SEED N_POSITIONS K SIMS RUNS
    python tests/live_reference_check.py record            (the cases of GOLDEN_CASES -> tests/golden/live_reference.json)

Each mode is a pair: ref_<mode> computes the reference's side (a JSON-able record), cmp_<mode> checks the oracle against
such a record.  Exit status 0 and a line "ok <mode> <count>" when everything matched; an AssertionError names the first
difference.
"""
import hashlib
import json
import os
import random
import sys

import numpy as np

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "live_reference.json")
sys.path.insert(0, ROOT)                                   # `from oracle import xq_oracle` (tests/arena_oracle.py)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import xq_oracle as xo  # noqa: E402

# the parameter sets of tests/test_oracle_live_reference.py's default run (mode, *args): what `record` stores
GOLDEN_CASES = [("rules", 101, 20, 120, 0.3), ("rules", 303, 24, 300, 0.9), ("history", 404, 10, 80, 0.5),
                ("mcts", 505, 8, 150), ("games", 606, 6), ("arena", 707, 3), ("kgt1", 909, 1, 8, 120, 2)]


def case_key(mode, *args):
    return " ".join([mode] + [str(a) for a in args])


def _reference():
    """the reference's static_env (imports the reference: live mode only)"""
    for p in (os.path.join(REF, "cchess_alphazero"), REF):
        if p not in sys.path:
            sys.path.insert(0, p)
    import cchess_alphazero.environment.static_env as senv
    return senv


def _gm():
    """configuration / stub helpers of the golden generator (imports the reference, patches its sleep)"""
    _reference()
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_mcts as gm
    return gm


def _digest(obj):
    return hashlib.sha256(json.dumps(obj, sort_keys=True).encode()).hexdigest()[:24]


def _occupancy(env, state):
    """(x, y) -> whether that square holds a piece (the reference's board is rows of characters, the oracle's a flat
    array of piece codes, 0 = empty)"""
    board = env.state_to_board(state)
    if env is xo:
        return lambda x, y: board[y * 9 + x] != 0
    return lambda x, y: board[y][x] != '.'


def playout_positions(env, seed, games, max_plies, capture_bias):
    """Random playouts with `env`'s move generator (the reference's static_env or the oracle: both have the same API);
    positions are always 'red to move' strings, as everywhere in the reference (step() flips the board)."""
    rng = random.Random(seed)
    out = []
    for _ in range(games):
        state = env.INIT_STATE
        hist = [state]
        for _ply in range(max_plies):
            moves = env.get_legal_moves(state)
            if not moves or env.done(state)[0]:
                break
            out.append((state, list(hist)))
            occupied = _occupancy(env, state)
            captures = [m for m in moves if occupied(int(m[2]), int(m[3]))]
            mv = rng.choice(captures) if captures and rng.random() < capture_bias else rng.choice(moves)
            state = env.step(state, mv)
            hist.append(mv)
            hist.append(state)
    return out


def rules_facts(env, state, rng):
    """Everything the rules check compares for one position, as plain JSON values:
    get_legal_moves (order included), done(need_check=True), state_to_planes, fliped_state, has_attack_chessman,
    new_step for every legal move (the reference raises when a king is captured, static_env.py:93-95: None), and
    will_check_or_catch / be_catched for up to 4 moves drawn with rng."""
    moves = list(env.get_legal_moves(state))
    d = env.done(state, need_check=True)
    planes = np.asarray(env.state_to_planes(state), dtype=np.float32)
    steps = []
    for mv in moves:
        try:
            s = env.new_step(state, mv)
            steps.append([s[0], bool(s[1])])
        except ValueError:
            steps.append(None)
    catch = [[mv, bool(env.will_check_or_catch(state, mv)), bool(env.be_catched(state, mv))]
             for mv in rng.sample(moves, min(4, len(moves)))]
    return {"moves": moves, "done": [bool(d[0]), int(d[1]), d[2], bool(d[3])],
            "planes": [list(planes.shape), hashlib.sha256(planes.tobytes()).hexdigest()[:24]],
            "flip": env.fliped_state(state), "attack": bool(env.has_attack_chessman(state)), "new_step": steps,
            "catch": catch}


def _positions_record(positions):
    return {"count": len(positions), "positions": _digest([s for s, _ in positions])}


def _check_positions(rec, positions):
    assert len(positions) == rec["count"], ("playout positions", len(positions), rec["count"])
    assert _digest([s for s, _ in positions]) == rec["positions"], "playout positions differ from the reference's"


# ---- rules ----
def ref_rules(seed, games, max_plies, capture_bias):
    senv = _reference()
    positions = playout_positions(senv, seed, games, max_plies, capture_bias)
    rng = random.Random(seed + 1)
    return dict(_positions_record(positions), facts=[_digest(rules_facts(senv, s, rng)) for s, _ in positions])


def cmp_rules(rec, seed, games, max_plies, capture_bias):
    positions = playout_positions(xo, seed, games, max_plies, capture_bias)
    _check_positions(rec, positions)
    rng = random.Random(seed + 1)
    for (state, _), want in zip(positions, rec["facts"]):
        got = rules_facts(xo, state, rng)
        assert _digest(got) == want, (state, got)
    return len(positions)


# ---- history planes ----
def history_digest(env, state, hist):
    p = np.asarray(env.state_history_to_planes(state, hist), dtype=np.float32)
    return [list(p.shape), hashlib.sha256(p.tobytes()).hexdigest()[:24]]


def ref_history(seed, games, max_plies, capture_bias):
    senv = _reference()
    positions = playout_positions(senv, seed, games, max_plies, capture_bias)
    return dict(_positions_record(positions), planes=[history_digest(senv, s, h) for s, h in positions])


def cmp_history(rec, seed, games, max_plies, capture_bias):
    positions = playout_positions(xo, seed, games, max_plies, capture_bias)
    _check_positions(rec, positions)
    for (state, hist), want in zip(positions, rec["planes"]):
        assert history_digest(xo, state, hist) == want, (state, len(hist))
    return len(positions)


# ---- search (K = 1) ----
def _mcts_picks(env, seed, n_positions):
    positions = playout_positions(env, seed, 6, 70, 0.3)
    return [s for s, _ in random.Random(seed).sample(positions, n_positions)]


def _mcts_setting(seed, i):
    return dict(kind="hash", salt=seed + i), ((1.5, 3) if i % 2 == 0 else (5.0, 1))


def ref_mcts(seed, n_positions, sims):
    """The reference's CChessPlayer (search_threads = 1, no noise, tests/stub_net.py as the network): action, visit
    counts, W (float64 bits) and priors (float32 bits) of every root edge."""
    gm = _gm()
    import stub_net
    np.random.dirichlet = lambda alpha, size=None: np.full(len(alpha), 1.0 / len(alpha))
    out = []
    for i, state in enumerate(_mcts_picks(_reference(), seed, n_positions)):
        spec, (c_puct, vl) = _mcts_setting(seed, i)
        cfg = gm.make_cfg(sims, c_puct=c_puct, vl=vl)
        pl = gm.ref_player.CChessPlayer(cfg, search_tree=None, pipes=stub_net.StubPipe(gm.stub_fn(spec)),
                                        enable_resign=False, debugging=False)
        action, _policy = pl.action(state, 0, None)
        out.append(dict(gm.root_stats(pl, state), state=state, action=action))
        pl.close()
    return {"searches": out}


def cmp_mcts(rec, seed, n_positions, sims):
    picked = _mcts_picks(xo, seed, n_positions)
    assert len(picked) == len(rec["searches"])
    for i, (state, want) in enumerate(zip(picked, rec["searches"])):
        assert state == want["state"], (i, state, want["state"])
        spec, (c_puct, vl) = _mcts_setting(seed, i)
        ocfg = xo.play_cfg(simulation_num_per_move=sims, search_threads=1, c_puct=c_puct, virtual_loss=vl)
        op = xo.Player(ocfg, spec)
        got_action, _ = op.action(state, 0)
        st = op.node_stats(state)
        op.close()
        assert got_action == want["action"], (state, got_action, want["action"])
        assert " ".join(xo.label_str(m) for m in st["moves"]) == want["moves"], state
        assert [int(x) for x in st["n"]] == want["n"], (state, list(st["n"]), want["n"])
        assert [float(x).hex() for x in st["w"]] == want["w_hex"], state
        assert [float(np.float32(x)).hex() for x in st["p"]] == want["p_hex"], state
    return len(picked)


# ---- self-play games ----
def _game_specs(seed, n_games):
    rng = random.Random(seed)
    specs = []
    for i in range(n_games):
        spec = dict(name=f"live_{seed}_{i}", salt=seed + i, seed=seed * 7 + i,
                    sims=rng.choice([4, 6, 10, 25, 40]), tau=rng.choice([0.0, 0.9, 0.98]),
                    max_game_length=rng.choice([16, 30, 60]), c_puct=rng.choice([0.5, 1.5, 3.0]))
        if i % 3 == 2:
            spec.update(enable_resign_rate=0.0, resign_threshold=rng.choice([-0.35, 0.3]), min_resign_turn=6)
        specs.append(spec)
    return specs


def ref_games(seed, n_games):
    """The reference's own SelfPlayWorker.start_game (tests/golden/make_golden_mcts.py::record_game: stub network, the
    engine's counter-based uniforms behind np.random.choice / random.random): length, result, every move, the
    visit-count CRC of every action() call, the evaluation count."""
    gm = _gm()
    gm._shim_tf()
    import cchess_alphazero.worker.self_play as sp
    out = []
    for spec in _game_specs(seed, n_games):
        g = gm.record_game(sp, spec)
        out.append({"turns": g["turns"], "value": g["value"], "store": g["store"],
                    "record": g["record"], "crc": [p["crc"] for p in g["plies"]], "nn_positions": g["nn_positions"]})
    return {"games": out}


def cmp_games(rec, seed, n_games):
    specs = _game_specs(seed, n_games)
    assert len(specs) == len(rec["games"])
    for spec, gmr in zip(specs, rec["games"]):
        cfg = xo.play_cfg(simulation_num_per_move=spec["sims"], search_threads=1, c_puct=spec["c_puct"],
                          tau_decay_rate=spec["tau"], max_game_length=spec["max_game_length"],
                          enable_resign_rate=spec.get("enable_resign_rate", 1.0),
                          resign_threshold=spec.get("resign_threshold", -0.92),
                          min_resign_turn=spec.get("min_resign_turn", 20))
        r = xo.selfplay_game(cfg, {"kind": "hash", "salt": spec["salt"]}, spec["seed"], 0)
        assert r["turns"] == gmr["turns"], (spec, r["turns"], gmr["turns"])
        assert r["value"] == gmr["value"] and r["store"] == gmr["store"], spec
        if gmr["record"] is not None:
            rec_ = gmr["record"]
            assert rec_[0] == xo.INIT_STATE
            assert r["moves"] == [m for m, _ in rec_[1:]], spec
        assert r["visit_crc"][:len(gmr["crc"])].tolist() == gmr["crc"], spec
        assert r["counters"]["nn_positions"] == gmr["nn_positions"], spec
    return n_games


# ---- arena games ----
ENDGAME = '3s5/4m4/9/9/4p4/2R6/9/4C4/4M4/3MS4'


def _arena_specs(seed, n_games):
    rng = random.Random(seed)
    specs = []
    for i in range(n_games):
        spec = dict(name=f"live_arena_{seed}_{i}", idx=i, salts=(seed + 2 * i, seed + 2 * i + 1), seed=seed * 5 + i,
                    sims=rng.choice([4, 6, 8, 12, 30]), max_game_length=rng.choice([20, 40, 80]),
                    c_puct=rng.choice([0.5, 1.0, 1.5]), evaluate=bool(i % 4 == 3))
        if i % 3 == 1:
            spec["init_state"] = ENDGAME
        specs.append(spec)
    return specs


def ref_arena(seed, n_games):
    """The reference's own EvaluateWorker.start_game (two players, two stub networks, colours by game index, the arena's
    repetition handling; tests/golden/make_golden_mcts.py::_arena_game): ply by ply state, action, visit CRC, bans and
    temperature flags, result."""
    gm = _gm()
    gm._shim_tf()
    import cchess_alphazero.worker.evaluator as ev
    out = []
    for spec in _arena_specs(seed, n_games):
        g = gm._arena_game(ev, spec)
        out.append({"value": g["value"], "turns": g["turns"],
                    "plies": [{k: r[k] for k in ("state", "action", "crc", "sum_n", "no_act", "inc")} for r in g["plies"]]})
    return {"games": out}


def cmp_arena(rec, seed, n_games):
    import types
    import stub_net
    from arena_oracle import arena_game
    specs = _arena_specs(seed, n_games)
    assert len(specs) == len(rec["games"])
    for spec, g in zip(specs, rec["games"]):
        pc = types.SimpleNamespace(simulation_num_per_move=spec["sims"], search_threads=1, c_puct=spec["c_puct"],
                                   dirichlet_alpha=0.2, tau_decay_rate=0.0, virtual_loss=3,
                                   max_game_length=spec["max_game_length"])
        trace = []
        value, turns, _evals = arena_game(spec["idx"], pc, tuple(dict(kind="hash", salt=x) for x in spec["salts"]),
                                          lambda idx, ply, _s=spec["seed"]: stub_net.philox_uniform(_s, idx, 1, ply),
                                          init_state=spec.get("init_state"), evaluate=spec["evaluate"], trace=trace)
        assert (value, turns) == (g["value"], g["turns"]), (spec, value, turns, g["value"], g["turns"])
        assert len(trace) == len(g["plies"]), spec
        for t, r in zip(trace, g["plies"]):
            t = json.loads(json.dumps({k: t[k] for k in r}, default=_plain))       # (tuples / numpy scalars as JSON has them)
            assert (t["state"], t["action"], t["crc"], t["sum_n"]) == (r["state"], r["action"], r["crc"], r["sum_n"]), spec
            assert t["no_act"] == r["no_act"] and t["inc"] == r["inc"], spec
    return n_games


# ---- search_threads = K > 1 ----
def _kgt1_picks(env, seed, n_positions):
    positions = playout_positions(env, seed, 8, 60, 0.3)
    return [s for s, _ in random.Random(seed).sample(positions, n_positions)]


def ref_kgt1(seed, n_positions, K, sims, runs):
    """The unmodified reference (its own thread timing: 1 ms sender sleep, 5 ms switch interval, as in
    tests/golden/make_golden_kgt1.py) searched `runs` times per freshly drawn position: the visit vectors."""
    import time
    gm = _gm()
    import stub_net
    gm.ref_player.sleep = time.sleep
    sys.setswitchinterval(0.005)
    np.random.dirichlet = lambda alpha, size=None: np.full(len(alpha), 1.0 / len(alpha))
    out = []
    for i, state in enumerate(_kgt1_picks(_reference(), seed, n_positions)):
        spec = dict(kind="hash", salt=seed + i)
        visits = []
        for _run in range(runs):
            cfg = gm.make_cfg(sims)
            cfg.play.search_threads = K
            pl = gm.ref_player.CChessPlayer(cfg, search_tree=None, pipes=stub_net.StubPipe(gm.stub_fn(spec)),
                                            enable_resign=False)
            pl.action(state, 0, None)
            node = pl.tree[state]
            visits.append([int(node.a[mv].n) if mv in node.a else 0 for mv in node.legal_moves])
            pl.close()
        out.append({"state": state, "visits": visits})
    return {"positions": out}


def cmp_kgt1(rec, seed, n_positions, K, sims, runs):
    """Against the oracle's canonical order: where the reference's runs all agree the oracle must give
    exactly that visit vector; where they differ it must have a top move some run has and lie no further from their mean
    than 1.5 x the furthest run (few runs: a crude spread)."""
    picked = _kgt1_picks(xo, seed, n_positions)
    assert len(picked) == len(rec["positions"])
    exact_n = deterministic = 0
    for i, (state, want) in enumerate(zip(picked, rec["positions"])):
        assert state == want["state"], (i, state, want["state"])
        visits = want["visits"]
        assert len(visits) == runs
        ocfg = xo.play_cfg(simulation_num_per_move=sims, search_threads=K)
        op = xo.Player(ocfg, dict(kind="hash", salt=seed + i))
        op.search(state)
        n = [int(x) for x in op.node_stats(state)["n"]]
        op.close()
        assert sum(n) == sum(visits[0]), (state, sum(n), sum(visits[0]))
        v = np.array(visits, dtype=np.float64)
        p = v / v.sum(1, keepdims=True)
        mean = p.mean(0)
        far = float((0.5 * np.abs(p - mean).sum(1)).max())
        q = np.array(n, dtype=np.float64) / sum(n)
        tv = float(0.5 * np.abs(q - mean).sum())
        same = len({tuple(x) for x in visits}) == 1
        exact = tuple(n) in {tuple(x) for x in visits}
        deterministic += same
        exact_n += exact
        print("kgt1", i, "distinct reference vectors", len({tuple(x) for x in visits}), "tv %.4f far %.4f" % (tv, far),
              "exact" if exact else "", flush=True)
        if same:
            assert exact, (state, n, visits[0])
        else:
            assert int(np.argmax(q)) in {int(np.argmax(r)) for r in p}, state
            assert tv <= 1.5 * far + 1e-9, (state, tv, far)
    print("kgt1: deterministic positions", deterministic, "of", n_positions, "; oracle equals a recorded run in", exact_n)
    return n_positions


MODES = {"rules": (ref_rules, cmp_rules, (int, int, int, float)), "history": (ref_history, cmp_history, (int, int, int, float)),
         "mcts": (ref_mcts, cmp_mcts, (int, int, int)), "games": (ref_games, cmp_games, (int, int)),
         "arena": (ref_arena, cmp_arena, (int, int)), "kgt1": (ref_kgt1, cmp_kgt1, (int, int, int, int, int))}


def _plain(x):
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, np.ndarray):
        return x.tolist()
    raise TypeError(type(x))


def record():
    """The reference's side of every GOLDEN_CASES entry -> tests/golden/live_reference.json"""
    out = {"generator": "tests/live_reference_check.py record", "numpy": np.__version__,
           "python": sys.version.split()[0], "cases": {}}
    for mode, *args in GOLDEN_CASES:
        ref, cmp_, _types = MODES[mode]
        rec = json.loads(json.dumps(ref(*args), default=_plain))
        n = cmp_(rec, *args)                                # (a record the oracle does not match is not written)
        out["cases"][case_key(mode, *args)] = rec
        print("recorded", mode, *args, n, flush=True)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    argv = sys.argv[1:]
    xo.build()
    if argv == ["record"]:
        record()
        raise SystemExit(0)
    golden = argv[0] == "--golden"
    if golden:
        argv = argv[1:]
    mode = argv[0]
    if mode not in MODES:
        raise SystemExit("mode?")
    ref, cmp_, types_ = MODES[mode]
    args = [t(a) for t, a in zip(types_, argv[1:])]
    if len(args) != len(types_):
        raise SystemExit(f"{mode}: {len(types_)} arguments")
    if golden:
        with open(GOLDEN) as f:
            cases = json.load(f)["cases"]
        key = case_key(mode, *args)
        if key not in cases:
            raise SystemExit(f"no recorded case '{key}' in {GOLDEN} (recorded: {sorted(cases)})")
        rec = cases[key]
    else:
        rec = json.loads(json.dumps(ref(*args), default=_plain))
    print("ok", mode, cmp_(rec, *args))
