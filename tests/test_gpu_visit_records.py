"""-m gpu: root visit records of self-play (cz_search_record_visits, engine.record_visits).  Every searched ply's root
visit counts, captured when the move is chosen, against the per-ply fingerprints recorded from the reference's own
SelfPlayWorker (tests/golden/games_k1.json, plies[*].crc) and against the oracle's self-play (oracle/xq_mcts.c); the
record writer's [move, value, pi] items; the decoder's visit targets; a ring too small for the run."""

import numpy as np
import pytest

from arena_oracle import visit_crc
from oracle import xq_oracle as xo
from test_gpu_search import _golden, gpu, oracle_cfg, play_config, stub_eval  # noqa: F401

pytestmark = pytest.mark.gpu


def run_selfplay_visits(gpu, pc, spec, G, seed, games_wanted, record=True, capacity=0, drain_every=64,
                        max_rounds=200000, **kw):
    """Like test_gpu_search.run_selfplay, with the visit record on: the ring holds every entry of drain_every rounds
    unless `capacity` says otherwise.  Returns ({game id: record}, counters)."""
    s = gpu.S.Search(pc, G, seed=seed, **kw)
    if record:
        s.record_visits(True, capacity=capacity or 8 * drain_every * G)
    ev = stub_eval(gpu, spec)
    s.start_selfplay(seed=seed, first_game_id=0)
    recs = {}
    for r in range(max_rounds):
        s.round()
        p, v = ev(s.planes)
        s.policy.copy_(p)
        s.value.copy_(v)
        if r % drain_every == drain_every - 1:
            for rec in s.drain_records(with_visits=record):
                recs[rec["game_id"]] = rec
            if all(g in recs for g in range(games_wanted)):
                break
    ctr = s.counters()
    s.close()
    return recs, ctr


def crcs(visits):
    return [visit_crc(e.moves, e.n) for e in visits]


def same_games(a, b, gids):
    for g in gids:
        assert [int(m) for m in a[g]["moves"]] == [int(m) for m in b[g]["moves"]], g
        for k in ("turns", "value", "store", "resigned"):
            assert a[g][k] == b[g][k], (g, k)


GAME_KEYS = ("sims", "expansions", "terminal_sims", "repetition_sims", "parked", "plies", "games", "red_wins",
             "black_wins", "draws", "resigns", "tree_resets", "overflow_sims", "root_reused_sims")


def test_reference_games_carry_the_reference_visit_counts(gpu):
    """All 15 games of the reference's SelfPlayWorker: per searched ply the fingerprint of (moves, n) in edge order, the
    root's sum_n and the banned edges; one entry per action() call (the resignation ply counts, the appended king capture
    does not).  At the `resign` game's banned ply the record's pi leaves the banned move out, as calc_policy does."""
    from cchess_alphazero.environment.lookup_tables import ActionLabelsRed
    from cchess_alphazero.lib.data_helper import pi_from_visits
    data = _golden("games_k1.json")
    assert any(g["sims"] == 800 for g in data["games"])
    banned_checked = 0
    for gm in data["games"]:
        pc = play_config(simulation_num_per_move=gm["sims"], search_threads=1, c_puct=gm.get("c_puct", 1.5),
                         tau_decay_rate=gm["tau"], max_game_length=gm["max_game_length"],
                         enable_resign_rate=gm.get("enable_resign_rate", 1.0),
                         resign_threshold=gm.get("resign_threshold", -0.92),
                         min_resign_turn=gm.get("min_resign_turn", 20))
        recs, ctr = run_selfplay_visits(gpu, pc, dict(kind="hash", salt=gm["salt"]), 1, gm["seed"], 1)
        got = recs[0]
        name = gm["name"]
        assert got["turns"] == gm["turns"] and ctr["visits_dropped"] == 0, name
        vis = got["visits"]
        plies = gm["plies"]
        assert vis is not None and len(vis) == len(plies), (name, None if vis is None else len(vis), len(plies))
        assert [e.ply for e in vis] == list(range(len(plies)))
        assert crcs(vis) == [p["crc"] for p in plies], name
        assert [e.sum_n for e in vis] == [p["sum_n"] for p in plies], name
        for i, (e, p) in enumerate(zip(vis, plies)):
            assert sorted(xo.label_str(int(m)) for m in e.moves[e.banned]) == sorted(p["no_act"]), (name, i)
            if p["no_act"]:
                pi = pi_from_visits(e.moves, e.n, e.banned, ActionLabelsRed)
                keep = [(xo.label_str(int(m)), int(c)) for m, c, b in zip(e.moves, e.n, e.banned) if not b and c > 0]
                assert [tuple(x) for x in pi] == keep and not any(m in p["no_act"] for m, _ in pi), (name, i)
                total = sum(c for _, c in pi)
                assert total == int(e.n[~e.banned].sum()), (name, i)
                banned_checked += 1
        assert vis[-1].resign == got["resigned"], name
    assert banned_checked >= 1                               # the `resign` game's ban of 3134


@pytest.mark.parametrize("K,tau", [(1, 0.0), (1, 0.9), (4, 0.0), (4, 0.9)])
def test_selfplay_visits_match_oracle_and_change_no_game(gpu, K, tau):
    pc = play_config(simulation_num_per_move=24, search_threads=K, tau_decay_rate=tau, max_game_length=16,
                     enable_resign_rate=0.5, resign_threshold=-0.4, min_resign_turn=4)
    spec = dict(kind="hash", salt=31)
    G, seed = 12, 4242
    recs, ctr = run_selfplay_visits(gpu, pc, spec, G, seed, G)
    off, ctr_off = run_selfplay_visits(gpu, pc, spec, G, seed, G, record=False)
    assert ctr["visits_dropped"] == 0 and "visits_dropped" not in ctr_off
    same_games(recs, off, range(G))
    for gid in range(G):
        ref = xo.selfplay_game(oracle_cfg(pc), spec, seed, gid)
        got = recs[gid]
        assert [xo.label_str(int(m)) for m in got["moves"]] == ref["moves"], gid
        vis = got["visits"]
        assert vis is not None, gid
        assert crcs(vis) == [int(c) for c in ref["visit_crc"][:len(vis)]], gid
        # one entry per action() call: every move but an appended king capture, plus the resignation ply
        n_calls = got["turns"] + (1 if got["resigned"] else 0)
        assert len(vis) in (n_calls, n_calls - 1) and (len(vis) == n_calls or not got["resigned"]), gid
    # both runs stop at the same round: the whole search agrees, not only the drained games
    assert {k: ctr[k] for k in GAME_KEYS} == {k: ctr_off[k] for k in GAME_KEYS}


def test_root_noise_run_records_everything_and_changes_no_game(gpu):
    pc = play_config(simulation_num_per_move=24, search_threads=4, tau_decay_rate=0.9, max_game_length=16,
                     noise_eps=0.25, enable_resign_rate=0.5, resign_threshold=-0.4, min_resign_turn=4)
    spec = dict(kind="hash", salt=5)
    G, seed = 16, 77
    recs, ctr = run_selfplay_visits(gpu, pc, spec, G, seed, G, max_rounds=20000)
    off, _ = run_selfplay_visits(gpu, pc, spec, G, seed, G, record=False, max_rounds=20000)
    assert ctr["visits_dropped"] == 0
    same_games(recs, off, range(G))
    for gid in range(G):
        vis = recs[gid]["visits"]
        assert vis is not None and len(vis) >= recs[gid]["turns"] - 1, gid
        assert all(int(e.n.sum()) >= 1 for e in vis if not e.resign), gid


# ---- full size: the normal self-play shape -------------------------------------------------------------------------
def _engine_config(pc, G, **engine):
    from cchess_alphazero.config import Config
    cfg = Config("normal")
    for k, v in vars(pc).items():
        setattr(cfg.play, k, v)
    cfg.engine.games_per_gpu = G
    for k, v in engine.items():
        setattr(cfg.engine, k, v)
    return cfg


def test_normal_selfplay_records_every_ply_at_the_default_cadence(gpu):
    """4096 games x K = 8 x 800 simulations through SelfPlayEngine with the stub network, drained at the worker's default
    report_every_rounds (200): the engine's own ring cadence drops nothing; 16 sampled games' visit fingerprints equal
    the oracle's.  Stops once every slot has finished its first game."""
    from cchess_alphazero import engine as engine_mod
    from cchess_alphazero.engine import SelfPlayEngine
    from test_gpu_full_size import normal_selfplay_play, whole_game_pool
    pc, G = normal_selfplay_play()
    K = pc.search_threads
    assert K == 8 and pc.simulation_num_per_move == 800
    spec = dict(kind="hash", salt=43)
    seed = 31
    cfg = _engine_config(pc, G, record_visits=True)
    every = cfg.engine.report_every_rounds
    assert every == 200
    eng = SelfPlayEngine(cfg, G, evaluator=stub_eval(gpu, spec), seed=seed, pool_chunks=G * whole_game_pool(gpu, pc))
    try:
        assert eng.record_visits and eng.search.visit_capacity == 8 * engine_mod.VISIT_DRAIN_ROUNDS * G
        eng.start(0, 0)
        got = {}
        for r in range(1, 6001):
            eng.step()
            if r % every == 0:
                for g in eng.drain():
                    got[g["game_id"]] = g
                if all(i in got for i in range(G)):
                    break
        c = eng.counters()
    finally:
        eng.close()
    assert all(i in got for i in range(G))
    assert c["visits_dropped"] == 0 and c["overflow_sims"] == 0 and c["tree_resets"] == 0, c
    assert all(got[i]["visits"] is not None for i in range(G))
    rng = np.random.default_rng(16)
    for gid in [0, G - 1] + sorted(rng.choice(np.arange(1, G - 1), 14, replace=False).tolist()):
        ref = xo.selfplay_game(oracle_cfg(pc), spec, seed, gid)
        vis = got[gid]["visits"]
        assert [m for m, *_ in got[gid]["data"][1:]] == ref["moves"], gid
        assert crcs(vis) == [int(x) for x in ref["visit_crc"][:len(vis)]], gid


def _engine_games(gpu, graph, rounds=1200):
    from cchess_alphazero.engine import SelfPlayEngine
    pc = play_config(simulation_num_per_move=24, search_threads=4, tau_decay_rate=0.9, max_game_length=12,
                     enable_resign_rate=0.5, resign_threshold=-0.4, min_resign_turn=4)
    cfg = _engine_config(pc, 16, record_visits=True)
    eng = SelfPlayEngine(cfg, 16, evaluator=stub_eval(gpu, dict(kind="hash", salt=11)), seed=3)
    out = {}
    try:
        eng.start(0, 0)
        if graph:
            eng.capture_graph()
        for r in range(rounds):
            eng.step()
            if r % 100 == 99:
                for g in eng.drain():
                    out[g["game_id"]] = g
        for g in eng.drain():
            out[g["game_id"]] = g
        c = eng.counters()
    finally:
        eng.close()
    assert c["visits_dropped"] == 0
    return out


def test_graph_replays_record_the_same_visits_as_direct_rounds(gpu):
    direct = _engine_games(gpu, False)
    graph = _engine_games(gpu, True)
    common = sorted(set(direct) & set(graph))
    assert len(common) >= 32
    for gid in common:
        assert direct[gid]["data"] == graph[gid]["data"], gid
        assert any(len(it) == 3 for it in graph[gid]["data"][1:]), gid


# ---- records on disk, decoder ---------------------------------------------------------------------------------------
def _worker_games(gpu, tmp_path, monkeypatch, record):
    """SelfPlayWorker on the stub network (the engine handed in); returns ({game id: drained game}, files' data)."""
    from cchess_alphazero.config import Config
    from cchess_alphazero.engine import SelfPlayEngine
    from cchess_alphazero.lib.data_helper import get_game_data_filenames, read_game_data_from_file
    from cchess_alphazero.worker.self_play import SelfPlayWorker
    d = tmp_path / ("on" if record else "off")
    monkeypatch.setenv("DATA_DIR", str(d / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(d))
    cfg = Config("mini")
    for k, v in dict(simulation_num_per_move=12, search_threads=4, max_game_length=8, noise_eps=0.25,
                     tau_decay_rate=0.98).items():
        setattr(cfg.play, k, v)
    cfg.engine.games_per_gpu = 16
    cfg.engine.report_every_rounds = 16
    cfg.engine.record_visits = record
    cfg.play_data.max_file_num = 1000
    w = SelfPlayWorker(cfg)
    w.engine = SelfPlayEngine(cfg, 16, evaluator=stub_eval(gpu, dict(kind="hash", salt=21)), seed=0)
    w.engine.start(0, 0)
    seen = {}
    drain = w.engine.drain

    def spy(*a, **k):
        out = drain(*a, **k)
        for g in out:
            seen[g["game_id"]] = g
        return out
    w.engine.drain = spy
    w.run(max_rounds=4000, max_games=40)
    w.close()
    files = [read_game_data_from_file(p) for p in get_game_data_filenames(cfg.resource)]
    return seen, files


def test_worker_writes_pi_records_and_the_same_games(gpu, tmp_path, monkeypatch):
    from cchess_alphazero.environment.lookup_tables import ActionLabelsRed
    from cchess_alphazero.lib.data_helper import pi_from_visits
    from cchess_alphazero.lib.record_decoder import split_games
    on, files_on = _worker_games(gpu, tmp_path, monkeypatch, True)
    off, files_off = _worker_games(gpu, tmp_path, monkeypatch, False)
    common = sorted(set(on) & set(off))
    assert len(common) >= 24
    for gid in common:
        a, b = on[gid]["data"], off[gid]["data"]
        assert a[0] == b[0] and [it[:2] for it in a[1:]] == b[1:], gid
        assert all(len(it) == 2 for it in off[gid]["data"][1:])
    n_pi = 0
    for gid, g in on.items():
        vis = g["visits"]
        assert vis is not None, gid
        for i, it in enumerate(g["data"][1:]):
            if i < len(vis) and not vis[i].resign:
                e = vis[i]
                assert len(it) == 3 and it[2] == pi_from_visits(e.moves, e.n, e.banned, ActionLabelsRed), (gid, i)
                n_pi += 1
            else:
                assert len(it) == 2 and i == len(g["data"]) - 2, (gid, i)      # only an appended king capture
    assert n_pi > 100
    stored_on = [json_norm(g["data"]) for g in on.values() if g["store"]]
    games_on = [json_norm(x) for f in files_on for x in split_games(f)]
    assert games_on and all(x in stored_on for x in games_on)
    assert sum(len(split_games(f)) for f in files_off) > 0


def json_norm(x):
    import json
    return json.loads(json.dumps(x))


def test_decoder_visit_targets(gpu, tmp_path, monkeypatch):
    import torch
    from cchess_alphazero.environment.lookup_tables import label_index
    from cchess_alphazero.lib.record_decoder import expand_records
    on, _ = _worker_games(gpu, tmp_path, monkeypatch, True)
    games = [json_norm(g["data"]) for _, g in sorted(on.items())][:20]
    planes, pol, vals, offsets = expand_records(games, targets="visits")
    items = [it for g in games for it in g[1:]]
    assert pol.shape == (len(items), 2086) and pol.dtype == torch.float32
    P = pol.cpu().numpy()
    assert np.allclose(P.sum(1), 1.0, atol=1e-5)
    n_two = 0
    for r, it in enumerate(items):
        exp = np.zeros(2086, dtype=np.float32)
        if len(it) == 3:
            tot = sum(c for _, c in it[2])
            for m, c in it[2]:
                exp[label_index(m)] = np.float32(c / tot)
        else:
            exp[label_index(it[0])] = 1.0
            n_two += 1
        assert (P[r] == exp).all(), r
    assert n_two < len(items)
    stripped = [[g[0]] + [it[:2] for it in g[1:]] for g in games]
    a = expand_records(games)
    b = expand_records(stripped)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all() and (a[3] == b[3]).all()
    assert (planes == a[0]).all() and (vals == a[2]).all()


# ---- overrun --------------------------------------------------------------------------------------------------------
def test_tiny_ring_counts_its_drops_and_changes_no_game(gpu, monkeypatch):
    """A ring of 4 entries drained every 64 rounds: entries are dropped and counted, the games that lost one come out
    without visits (two-element items), the games themselves are those of a run without recording."""
    from cchess_alphazero import engine as engine_mod
    from cchess_alphazero.engine import SelfPlayEngine
    pc = play_config(simulation_num_per_move=24, search_threads=4, tau_decay_rate=0.9, max_game_length=12)
    spec = dict(kind="hash", salt=13)
    G, seed = 8, 9
    recs, ctr = run_selfplay_visits(gpu, pc, spec, G, seed, G, capacity=4)
    off, _ = run_selfplay_visits(gpu, pc, spec, G, seed, G, record=False)
    assert ctr["visits_dropped"] > 0
    same_games(recs, off, range(G))
    assert any(recs[g]["visits"] is None for g in range(G))
    # the same through the engine: items of a game that lost an entry keep the two-element form
    eng = SelfPlayEngine(_engine_config(pc, G, record_visits=True), G, evaluator=stub_eval(gpu, spec), seed=seed)
    monkeypatch.setattr(engine_mod, "VISIT_DRAIN_ROUNDS", 10 ** 9)     # (no pull between the drains)
    try:
        eng.search.record_visits(True, capacity=4)
        eng.start(0, 0)
        got = {}
        for r in range(1, 20001):
            eng.step()
            if r % 64 == 0:
                for g in eng.drain():
                    got[g["game_id"]] = g
                if all(i in got for i in range(G)):
                    break
        c = eng.counters()
    finally:
        eng.close()
    assert c["visits_dropped"] > 0
    lost = [g for g in range(G) if got[g]["visits"] is None]
    assert lost
    for g in lost:
        assert all(len(it) == 2 for it in got[g]["data"][1:])
        assert [m for m, _ in got[g]["data"][1:]] == [xo.label_str(int(m)) for m in off[g]["moves"]]
