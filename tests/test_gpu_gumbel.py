"""-m gpu: Gumbel root search with sequential halving (cz_search_set_gumbel, cz_search_root_started,
cz_search_gumbel_draws, cz_search_gumbel_targets, cz_gumbel_policy_target; run.py self --gumbel M --record-visits).

The yardstick is tests/gumbel_oracle.py: the definitions of include/czero.h in plain float64 and a Python search for one
search thread with the root rule in it; tests/test_gumbel_cpu.py holds it to hand-written schedules and to the plain
search at M = 0, and shows that on the inputs used here no selection is decided by less than 1e-9 -- so `started`, n, W,
p and the move are compared exactly although exp and log are two libraries'; a target may differ by 1.  K = 8 is held by
the invariants of the halving.  With M = 0 a search is what it was."""
import numpy as np
import pytest

import forced_playouts_oracle as fo
import gumbel_oracle as go
from oracle import xq_oracle as xo
from test_gpu_book import _engine_cfg
from test_gpu_search import (assert_root_equal, boards_tensor, gpu, no_act_tensors, oracle_cfg, play_config,  # noqa: F401
                             stub_eval)

pytestmark = pytest.mark.gpu
SIMS, M, SEED = 64, 16, 7
WIDE = '3s5/9/9/2K3K2/R7R/1C5C1/P1P1P1P1P/9/9/4S4'          # more than 64 moves


# ---- 1. the draws ---------------------------------------------------------------------------------------------------------
def test_draws_are_gumbel_of_the_philox_stream(gpu):
    t = gpu.torch
    states = [xo.INIT_STATE, WIDE, fo.cases()[1]["state"], fo.cases()[4]["state"]]
    turns = [0, 5, 40, 3]
    seed = 11
    s = gpu.S.Search(play_config(simulation_num_per_move=16, search_threads=4), 4, seed=seed)
    s.set_gumbel(M)
    s.set_roots(boards_tensor(gpu, states), turns=t.tensor(turns, dtype=t.int32, device="cuda"))
    got = s.gumbel_draws()
    assert len(xo.get_legal_moves(WIDE)) > 64
    worst = 0.0
    for g in range(4):
        want = go.draws_for(seed, 0, g, turns[g])           # (external mode: game id 0, the slot tells the games apart)
        rel = np.abs(got[g] - want) / np.abs(want)
        worst = max(worst, float(rel.max()))
        assert (rel <= 1e-12).all(), (g, int(rel.argmax()), float(rel.max()))
    print(f"draws: worst relative difference {worst:.3e}")
    assert (s.root_started() == 0).all()
    assert len({got[g].tobytes() for g in range(4)}) == 4
    s.close()


# ---- 2. single searches at K = 1 against the oracle -------------------------------------------------------------------------
def test_single_searches_match_the_oracle(gpu):
    pc = play_config(simulation_num_per_move=SIMS, search_threads=1, noise_eps=0.0, tau_decay_rate=0.0)
    kinds = set()
    for c in fo.cases():
        s = gpu.S.Search(pc, 1, seed=SEED)
        s.set_gumbel(M)
        ev = stub_eval(gpu, dict(kind="hash", salt=c["salt"]))
        s.set_roots(boards_tensor(gpu, [c["state"]]))           # (nothing is searched yet: this is for the ply's draws)
        draws = s.gumbel_draws()[0].copy()
        res, osearch = go.run_case(c, M, SIMS, draws)
        for r in res:
            na, nn = no_act_tensors(gpu, [r["no_act"]])
            s.set_roots(boards_tensor(gpu, [r["state"]]), no_act=na, n_no_act=nn)
            assert s.gumbel_draws()[0].tobytes() == draws.tobytes()     # same game, same ply number: the same draws
            s.run_until_idle(ev)
            what = f"{c['name']} {r['state']}"
            nm = len(r["started"])
            assert_root_equal(s.root_stats(), 0, r["stats"], what)
            started = s.root_started()[0]
            assert started[:nm].tolist() == r["started"], (what, started[:nm], r["started"])
            assert (started[nm:] == 0).all(), what
            assert xo.label_str(int(s.choose()[0])) == r["best"], what
            tg = s.gumbel_targets()
            assert int(tg["raw_total"][0]) == r["raw_total"], what
            assert np.abs(tg["n"][0, :nm] - r["targets"]).max() <= 1, (what, tg["n"][0, :nm], r["targets"])
            assert (tg["n"][0, nm:] == 0).all(), what
            assert (s.root_targets()["n"] == tg["n"]).all()     # with the option on the recorded counts ARE these targets
        ctr = s.counters()
        for key in ("sims", "expansions", "terminal_sims", "repetition_sims"):
            assert ctr[key] == getattr(osearch, key), (c["name"], key)
        kinds.add(c["kind"])
        kinds.add("wide" if len(res[0]["started"]) > 64 else None)
        s.close()
    assert kinds >= {"ban", "reuse", "wide"}


# ---- 3. the target arithmetic alone ---------------------------------------------------------------------------------------
def _random_row(rng, nm, ban=0.0, visited=0.7):
    n = (rng.integers(1, 60, nm) * (rng.random(nm) < visited)).astype(np.int32)
    q = rng.uniform(-2, 2, nm)                                  # |q| up to 2: terminal values, clamped by q01
    p = rng.random(nm) ** 4
    p[rng.random(nm) < 0.1] = 0.0
    if p.sum() == 0.0:
        p[0] = 1.0
    p = (p / p.sum()).astype(np.float32)
    lab = rng.permutation(2086)[:nm].astype(np.uint16)
    lab[rng.random(nm) < ban] |= go.BANNED
    return dict(labels=lab, n=n, w=q * n, p=p)


def test_policy_target_rows(gpu):
    t = gpu.torch
    rng = np.random.default_rng(23)
    sizes = [1, 2, 63, 64, 65, 127, 128] + [int(rng.integers(1, 129)) for _ in range(57)]
    rows = [_random_row(rng, nm, ban=0.15 * (i % 3), visited=(0.0 if i == 7 else 0.7)) for i, nm in enumerate(sizes)]
    rows[8]["labels"] |= go.BANNED                              # every edge banned
    R = len(rows)
    assert R == 64 and sum(len(r["n"]) > 64 for r in rows) > 8
    lab = np.zeros((R, 128), dtype=np.uint16)
    n = np.full((R, 128), 10 ** 6, dtype=np.int32)              # past n_edges: values that would show if they were read
    w = np.full((R, 128), 1e6, dtype=np.float64)
    p = np.ones((R, 128), dtype=np.float32)
    ne = np.zeros(R, dtype=np.uint8)
    for i, r in enumerate(rows):
        k = len(r["n"])
        ne[i] = k
        lab[i, :k], n[i, :k], w[i, :k], p[i, :k] = r["labels"], r["n"], r["w"], r["p"]
    args = [t.from_numpy(lab.view(np.int16)).cuda().view(t.uint16), t.from_numpy(n).cuda(), t.from_numpy(w).cuda(),
            t.from_numpy(p).cuda(), t.from_numpy(ne).cuda()]
    for c_visit, c_scale in ((50.0, 1.0), (0.0, 0.1), (50.0, 0.0)):
        out, raw = gpu.S.gumbel_policy_target(*args, c_visit, c_scale)
        out, raw = out.cpu().numpy(), raw.cpu().numpy()
        for i, r in enumerate(rows):
            k = len(r["n"])
            want, S = go.target(r["labels"], r["n"], r["w"], r["p"], c_visit, c_scale)
            assert int(raw[i]) == S, i
            assert np.abs(out[i, :k] - want).max() <= 1, (i, c_visit, c_scale, out[i, :k], want)
            assert (out[i, k:] == 0).all() and (out[i, :k][(r["labels"] & go.BANNED) != 0] == 0).all(), i
            assert (out[i, :k][r["p"] == 0] == 0).all(), i
    assert (out[8] == 0).all() and raw[8] == 0
    import ctypes as C
    L = gpu.N.lib()
    ptr = [C.c_void_p(x.data_ptr()) for x in args]
    o = [C.c_void_p(t.empty((R, 128), dtype=t.int32, device="cuda").data_ptr()),
         C.c_void_p(t.empty(R, dtype=t.int32, device="cuda").data_ptr())]
    st = C.c_void_p(t.cuda.current_stream().cuda_stream)
    for bad in (-1.0, float("nan"), float("inf")):
        assert L.cz_gumbel_policy_target(*ptr, R, bad, 1.0, *o, st) == -1
        assert L.cz_gumbel_policy_target(*ptr, R, 50.0, bad, *o, st) == -1
    assert L.cz_gumbel_policy_target(None, *ptr[1:], R, 50.0, 1.0, *o, st) == -1
    assert L.cz_gumbel_policy_target(*ptr, -1, 50.0, 1.0, *o, st) == -1
    assert L.cz_gumbel_policy_target(*ptr, 0, 50.0, 1.0, *o, st) == 0


# ---- 4. K = 8 by invariant ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [4, 16])
def test_k_8_keeps_the_halving_invariants(gpu, m):
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "positions_1k.json")) as f:
        pos = [p["state"] for p in json.load(f)["positions"]]
    states = [c["state"] for c in fo.cases()] + [pos[i] for i in (10, 160, 310, 460, 610, 760, 910)]
    assert len(states) == 16
    bans = [None] * 16
    bans[2] = xo.get_legal_moves(states[2])[:3]
    bans[5] = [xo.get_legal_moves(states[5])[-1]]
    pc = play_config(simulation_num_per_move=SIMS, search_threads=8, virtual_loss=3, noise_eps=0.25, tau_decay_rate=0.9)
    s = gpu.S.Search(pc, 16, seed=5)
    s.set_gumbel(m)
    na, nn = no_act_tensors(gpu, bans)
    s.set_roots(boards_tensor(gpu, states), no_act=na, n_no_act=nn)
    s.run_until_idle(stub_eval(gpu, dict(kind="hash", salt=4)))
    st, started, act = s.root_stats(), s.root_started(), s.choose()
    ctr = s.counters()
    assert ctr["tree_resets"] == 0 and ctr["overflow_sims"] == 0
    for g in range(16):
        nm = int(st["counts"][g])
        labels = [xo.label_str(int(l)) for l in st["moves"][g, :nm]]
        live = np.array([mv not in (bans[g] or ()) for mv in labels])
        sg = started[g, :nm]
        total = int(sg.sum())
        # every selection at the root adds 1 to the root's count, which starts at 1 when the root is expanded
        assert total == int(st["sum_n"][g]) - 1 == SIMS - 1, (g, total, int(st["sum_n"][g]))
        assert (sg[~live] == 0).all() and (started[g, nm:] == 0).all(), g
        used = go.seq(min(m, int(live.sum())), SIMS)[:total]
        for v in range(max(used) + 2):
            assert int((sg > v).sum()) == used.count(v), (g, v, sg.tolist())
        top = {labels[j] for j in range(nm) if live[j] and sg[j] == sg[live].max()}
        assert xo.label_str(int(act[g])) in top, g
        assert int(st["n"][g, :nm].sum()) == total and (st["n"][g, :nm] >= 0).all()     # no virtual loss left behind
    s.close()


# ---- 5. self-play at K = 1 against the oracle's loop ------------------------------------------------------------------------
def test_selfplay_games_match_the_oracle(gpu):
    from cchess_alphazero.engine import SelfPlayEngine
    G, seed, salt, m = 4, 13, 5, 8
    # (root noise and a temperature are configured: a Gumbel ply must use neither, the oracle has neither)
    pc = play_config(simulation_num_per_move=32, search_threads=1, noise_eps=0.25, tau_decay_rate=0.9, max_game_length=3,
                     enable_resign_rate=0.5, resign_threshold=-0.3, min_resign_turn=1)
    eng = SelfPlayEngine(_engine_cfg(pc), G, evaluator=stub_eval(gpu, dict(kind="hash", salt=salt)), seed=seed,
                         record_visits=True, gumbel=m)
    games = []
    try:
        eng.start(0, 0)
        for r in range(4000):
            eng.step()
            if r % 16 == 15:
                games += eng.drain()
                if len({g["game_id"] for g in games if g["game_id"] < G}) == G:
                    break
        ctr = eng.counters()
    finally:
        eng.close()
    assert ctr["tree_resets"] == 0 and ctr["overflow_sims"] == 0 and ctr["visits_dropped"] == 0
    ocfg = oracle_cfg(play_config(**dict(vars(pc), noise_eps=0.0, tau_decay_rate=0.0)))
    first = {g["game_id"]: g for g in games if g["game_id"] < G}
    assert len(first) == G
    for gid, g in sorted(first.items()):
        ref = go.gumbel_selfplay_game(ocfg, salt, seed, gid, gid % G, m)
        assert [it[0] for it in g["data"][1:]] == ref["moves"], gid
        assert (g["turns"], g["value"], g["store"], g["resigned"]) == (ref["turns"], ref["value"], ref["store"], ref["resigned"])
        vis = g["visits"]
        assert len(vis) == len(ref["plies"]) > 0
        for e, r in zip(vis, ref["plies"]):
            assert e.gumbel and not e.pruned and not e.fast and e.resign == r["resign"], (gid, e.ply)
            assert (e.moves == r["labels"]).all() and (e.banned == r["banned"]).all() and e.sum_n == r["sum_n"]
            assert e.raw_total == r["raw_total"], (gid, e.ply)
            assert np.abs(e.n - r["targets"]).max() <= 1, (gid, e.ply, e.n, r["targets"])
            assert abs(int(e.n.sum()) - 65536) <= len(e.n)
        for item, e in zip(g["data"][1:], vis):                 # pi is the entry, zero targets omitted
            assert sorted(c for _, c in item[2]) == sorted(int(c) for c in e.n[~e.banned] if c > 0)


# ---- 6. off is off --------------------------------------------------------------------------------------------------------
def test_m_0_after_the_option_was_on_is_the_plain_search(gpu):
    pc = play_config(simulation_num_per_move=SIMS, search_threads=4, noise_eps=0.25)
    cs = fo.cases()
    ev = stub_eval(gpu, dict(kind="hash", salt=9))
    states = [cs[1]["state"], cs[7]["state"]]
    plain = gpu.S.Search(pc, 2, seed=3)
    plain.set_roots(boards_tensor(gpu, states))
    plain.run_until_idle(ev)
    want = plain.root_stats()
    s = gpu.S.Search(pc, 2, seed=3)
    s.set_gumbel(M)
    s.set_roots(boards_tensor(gpu, states))
    s.run_until_idle(ev)
    on = s.root_stats()
    assert s.root_started().sum() == 2 * (SIMS - 1)
    s.set_gumbel(0)
    s.reset_trees()
    s.set_roots(boards_tensor(gpu, states))
    s.run_until_idle(ev)
    got = s.root_stats()
    for k in ("moves", "n", "w", "p", "sum_n", "counts"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert on["n"].tobytes() != want["n"].tobytes()             # (the option would have shown)
    assert (s.root_targets()["n"] == plain.root_targets()["n"]).all()
    assert s.choose([0.3, 0.6]).tolist() == plain.choose([0.3, 0.6]).tolist()
    # arguments: refused values leave the setting
    st = s._stream()
    for bad in ((-1, 50.0, 1.0), (129, 50.0, 1.0), (4, -1.0, 1.0), (4, float("nan"), 1.0), (4, 50.0, float("inf"))):
        assert s.L.cz_search_set_gumbel(s.h, *bad, st) == -1, bad
    s.set_forced_playouts(2.0)
    assert s.L.cz_search_set_gumbel(s.h, 4, 50.0, 1.0, st) == -1
    s.set_forced_playouts(0.0)
    s.set_gumbel(4)
    assert s.L.cz_search_set_forced_playouts(s.h, 2.0, st) == -1 and s.L.cz_search_set_playout_cap(s.h, 8, 0.5, st) == -1
    s.close()
    plain.close()
