"""-m gpu: the full Gumbel search (cz_search_set_gumbel_full, cz_search_node_net_value, cz_gumbel_policy_target_v,
cz_gumbel_interior_pick; run.py self --gumbel M --gumbel-full).

The yardstick is tests/gumbel_full_oracle.py: the definitions of include/czero.h in plain float64 and gumbel_oracle's
search with the rule below the root in it.  tests/test_gumbel_full_cpu.py holds it to hand-computed rows and to the
root-only search with full off, and shows that on the inputs used here every selection -- at the root, below it, the
played move -- is decided by at least 1e-9 (the least margins: 4.9e-5 below the root and 5.8e-4 at it over the ten
searches, 5.4e-5 and 4.2e-4 over the four games, 8.8e-6 over the random rows), so picks, n, W, p, `started` and the moves
are compared exactly although exp is two libraries' and the sums run in two orders; a score may differ by 1e-12, a target
by 1.  K = 8 is held by invariants.  With full off a search is what cz_search_set_gumbel alone gives."""
import ctypes as C

import numpy as np
import pytest

import forced_playouts_oracle as fo
import gumbel_full_oracle as gf
import gumbel_oracle as go
import stub_net
from oracle import xq_oracle as xo
from test_gpu_book import _engine_cfg
from test_gpu_search import (assert_root_equal, boards_tensor, gpu, no_act_tensors, oracle_cfg, play_config,  # noqa: F401
                             stub_eval)

pytestmark = pytest.mark.gpu
SIMS, M, SEED = 64, 16, 7


# ---- 1. the rule and the target on rows ---------------------------------------------------------------------------------------
def _pack(t, rows):
    R = len(rows)
    lab = np.zeros((R, 128), dtype=np.uint16)
    n = np.full((R, 128), 10 ** 6, dtype=np.int32)              # past n_edges: values that would show if they were read
    w = np.full((R, 128), 1e6, dtype=np.float64)
    p = np.ones((R, 128), dtype=np.float32)
    ne = np.zeros(R, dtype=np.uint8)
    for i, r in enumerate(rows):
        k = len(r["n"])
        ne[i] = k
        lab[i, :k], n[i, :k], w[i, :k], p[i, :k] = r["labels"], r["n"], r["w"], r["p"]
    v = np.array([r["v"] for r in rows], dtype=np.float32)
    return [t.from_numpy(lab.view(np.int16)).cuda().view(t.uint16), t.from_numpy(n).cuda(), t.from_numpy(w).cuda(),
            t.from_numpy(p).cuda(), t.from_numpy(ne).cuda(), t.from_numpy(v).cuda()]


def test_interior_pick_and_full_target_rows(gpu):
    t = gpu.torch
    rows = gf.random_rows()
    nm0 = 5
    rows.append(dict(labels=np.arange(nm0, dtype=np.uint16), n=np.array([2, 1, 3, 1, 4], np.int32),
                     w=np.array([0.5, 0.1, -1.0, 0.3, 0.0]), p=np.zeros(nm0, np.float32), v=np.float32(0.5)))   # every prior 0
    rows.append(dict(labels=np.array([7], np.uint16), n=np.array([3], np.int32), w=np.array([-6.0]),
                     p=np.array([1.0], np.float32), v=np.float32(-1.0)))                                       # one edge
    rows.append(dict(labels=np.zeros(0, np.uint16), n=np.zeros(0, np.int32), w=np.zeros(0), p=np.zeros(0, np.float32),
                     v=np.float32(0.25)))                                                                      # no edge
    R = len(rows)
    lab, n, w, p, ne, v = args = _pack(t, rows)
    worst = 0.0
    for c_visit, c_scale in gf.PAIRS:
        pick, score = gpu.S.gumbel_interior_pick(n, w, p, ne, v, c_visit, c_scale)
        out, raw = gpu.S.gumbel_policy_target_v(lab, n, w, p, ne, v, c_visit, c_scale)
        pick, score, out, raw = pick.cpu().numpy(), score.cpu().numpy(), out.cpu().numpy(), raw.cpu().numpy()
        for i, r in enumerate(rows):
            k = len(r["n"])
            want, sc, _ = gf.interior_pick(r["n"], r["w"], r["p"], r["v"], c_visit, c_scale)
            assert int(pick[i]) == want, (i, c_visit, c_scale, int(pick[i]), want)
            diff = float(np.abs(score[i, :k] - np.array(sc)).max()) if k else 0.0
            worst = max(worst, diff)
            assert diff <= 1e-12, (i, c_visit, c_scale, diff)
            assert (score[i, k:] == 0.0).all(), i
            tg, S = gf.target_v(r["labels"], r["n"], r["w"], r["p"], r["v"], c_visit, c_scale)
            assert int(raw[i]) == S, i
            assert k == 0 or np.abs(out[i, :k] - tg).max() <= 1, (i, c_visit, c_scale, out[i, :k], tg)
            assert (out[i, k:] == 0).all() and (out[i, :k][(r["labels"] & gf.BANNED) != 0] == 0).all(), i
        assert int(pick[R - 3]) == 3 and int(pick[R - 2]) == 0 and int(pick[R - 1]) == -1
        assert (out[R - 3] == 0).all() and int(out[R - 2, 0]) == 65536
    print(f"interior scores: largest difference from the oracle {worst:.3e}")
    # nothing visited (row 7): the full target is the prior, whatever v
    k = len(rows[7]["n"])
    live = (rows[7]["labels"] & gf.BANNED) == 0
    pr = rows[7]["p"].astype(np.float64) * live
    assert np.abs(out[7, :k] - np.floor(65536.0 * pr / pr.sum() + 0.5)).max() <= 1
    # arguments
    L = gpu.N.lib()
    ptr = [C.c_void_p(x.data_ptr()) for x in args]
    lab_, n_, w_, p_, ne_, v_ = ptr
    keep = [t.empty((R, 128), dtype=t.int32, device="cuda"), t.empty(R, dtype=t.int32, device="cuda"),
            t.empty((R, 128), dtype=t.float64, device="cuda")]
    om, orw, osc = [C.c_void_p(x.data_ptr()) for x in keep]
    st = C.c_void_p(t.cuda.current_stream().cuda_stream)
    for bad in (-1.0, float("nan"), float("inf")):
        assert L.cz_gumbel_policy_target_v(lab_, n_, w_, p_, ne_, v_, R, bad, 1.0, om, orw, st) == -1
        assert L.cz_gumbel_policy_target_v(lab_, n_, w_, p_, ne_, v_, R, 50.0, bad, om, orw, st) == -1
        assert L.cz_gumbel_interior_pick(n_, w_, p_, ne_, v_, R, bad, 1.0, orw, osc, st) == -1
        assert L.cz_gumbel_interior_pick(n_, w_, p_, ne_, v_, R, 50.0, bad, orw, osc, st) == -1
    assert L.cz_gumbel_policy_target_v(lab_, n_, w_, p_, ne_, None, R, 50.0, 1.0, om, orw, st) == -1
    assert L.cz_gumbel_policy_target_v(lab_, n_, w_, p_, ne_, v_, -1, 50.0, 1.0, om, orw, st) == -1
    assert L.cz_gumbel_policy_target_v(lab_, n_, w_, p_, ne_, v_, 0, 50.0, 1.0, om, orw, st) == 0
    assert L.cz_gumbel_interior_pick(n_, w_, p_, ne_, None, R, 50.0, 1.0, orw, osc, st) == -1
    assert L.cz_gumbel_interior_pick(n_, w_, p_, ne_, v_, R, 50.0, 1.0, orw, None, st) == -1
    assert L.cz_gumbel_interior_pick(n_, w_, p_, ne_, v_, -1, 50.0, 1.0, orw, osc, st) == -1
    assert L.cz_gumbel_interior_pick(n_, w_, p_, ne_, v_, 0, 50.0, 1.0, orw, osc, st) == 0


# ---- 2. single searches at K = 1 against the oracle -------------------------------------------------------------------------
def _stub_value(state, salt):
    return np.float32(stub_net.hash_stub_numpy(xo.state_to_planes(state)[None], salt)[1][0])


def test_single_searches_match_the_oracle(gpu):
    pc = play_config(simulation_num_per_move=SIMS, search_threads=1, noise_eps=0.0, tau_decay_rate=0.0)
    kinds = set()
    for c in fo.cases():
        s = gpu.S.Search(pc, 1, seed=SEED)
        s.set_gumbel(M)
        s.set_gumbel_full(True)
        ev = stub_eval(gpu, dict(kind="hash", salt=c["salt"]))
        s.set_roots(boards_tensor(gpu, [c["state"]]))           # (nothing is searched yet: this is for the ply's draws)
        draws = s.gumbel_draws()[0].copy()
        assert np.isnan(s.node_net_value()[0])                  # the root is not in the tree yet
        res, osearch = gf.run_case(c, M, SIMS, draws)
        for r in res:
            na, nn = no_act_tensors(gpu, [r["no_act"]])
            s.set_roots(boards_tensor(gpu, [r["state"]]), no_act=na, n_no_act=nn)
            assert s.gumbel_draws()[0].tobytes() == draws.tobytes()
            s.run_until_idle(ev)
            what = f"{c['name']} {r['state']}"
            nm = len(r["started"])
            assert_root_equal(s.root_stats(), 0, r["stats"], what)
            started = s.root_started()[0]
            assert started[:nm].tolist() == r["started"], (what, started[:nm], r["started"])
            assert (started[nm:] == 0).all(), what
            assert xo.label_str(int(s.choose()[0])) == r["best"], what
            # the node under the played move, and the values the two nodes keep
            path = [xo.label_of_str(r["best"])]
            child = s.node_stats(path)
            rv, cv = s.node_net_value()[0], s.node_net_value(path)[0]
            assert rv.tobytes() == r["net_value"].tobytes() == _stub_value(r["state"], c["salt"]).tobytes(), what
            if r["child_stats"] is None:                        # a terminal position: not a node
                assert int(child["counts"][0]) == 0 and np.isnan(cv), what
            else:
                assert_root_equal(child, 0, r["child_stats"], what + " child")
                assert cv.tobytes() == r["child_value"].tobytes() == _stub_value(r["child_state"], c["salt"]).tobytes(), what
                kinds.add("child")
            tg = s.gumbel_targets()
            assert int(tg["raw_total"][0]) == r["raw_total"], what
            assert np.abs(tg["n"][0, :nm] - r["targets"]).max() <= 1, (what, tg["n"][0, :nm], r["targets"])
            assert (tg["n"][0, nm:] == 0).all(), what
            assert (s.root_targets()["n"] == tg["n"]).all()
        ctr = s.counters()
        for key in ("sims", "expansions", "terminal_sims", "repetition_sims"):
            assert ctr[key] == getattr(osearch, key), (c["name"], key)
        kinds.add(c["kind"])
        kinds.add("wide" if len(res[0]["started"]) > 64 else None)
        s.close()
    assert kinds >= {"ban", "reuse", "wide", "child"}


# ---- 3. K = 8 by invariant ------------------------------------------------------------------------------------------------
def _k8_run(gpu, m, states, bans):
    pc = play_config(simulation_num_per_move=SIMS, search_threads=8, virtual_loss=3, noise_eps=0.25, tau_decay_rate=0.9)
    s = gpu.S.Search(pc, 16, seed=5)
    s.set_gumbel(m)
    s.set_gumbel_full(True)
    na, nn = no_act_tensors(gpu, bans)
    s.set_roots(boards_tensor(gpu, states), no_act=na, n_no_act=nn)
    s.run_until_idle(stub_eval(gpu, dict(kind="hash", salt=4)))
    st, started, act = s.root_stats(), s.root_started(), s.choose()
    child = s.node_stats(np.asarray(act, dtype=np.uint16).reshape(16, 1))
    out = dict(st=st, started=started, act=act, child=child, ctr=s.counters(), tg=s.gumbel_targets(),
               rv=s.node_net_value())
    s.close()
    return out


@pytest.mark.parametrize("m", [4, 16])
def test_k_8_keeps_the_invariants(gpu, m):
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "positions_1k.json")) as f:
        pos = [p["state"] for p in json.load(f)["positions"]]
    states = [c["state"] for c in fo.cases()] + [pos[i] for i in (10, 160, 310, 460, 610, 760, 910)]
    assert len(states) == 16
    bans = [None] * 16
    bans[2] = xo.get_legal_moves(states[2])[:3]
    bans[5] = [xo.get_legal_moves(states[5])[-1]]
    a = _k8_run(gpu, m, states, bans)
    st, started, act, child, ctr = a["st"], a["started"], a["act"], a["child"], a["ctr"]
    assert ctr["tree_resets"] == 0 and ctr["overflow_sims"] == 0
    for g in range(16):
        nm = int(st["counts"][g])
        labels = [xo.label_str(int(l)) for l in st["moves"][g, :nm]]
        live = np.array([mv not in (bans[g] or ()) for mv in labels])
        sg = started[g, :nm]
        total = int(sg.sum())
        assert total == int(st["sum_n"][g]) - 1 == SIMS - 1, (g, total, int(st["sum_n"][g]))
        assert (sg[~live] == 0).all() and (started[g, nm:] == 0).all(), g
        used = go.seq(min(m, int(live.sum())), SIMS)[:total]
        for v in range(max(used) + 2):
            assert int((sg > v).sum()) == used.count(v), (g, v, sg.tolist())
        top = {labels[j] for j in range(nm) if live[j] and sg[j] == sg[live].max()}
        assert xo.label_str(int(act[g])) in top, g
        # no virtual loss left behind, at the root and at the node under the played move, where the new rule selected
        assert int(st["n"][g, :nm].sum()) == int(st["sum_n"][g]) - 1 and (st["n"][g, :nm] >= 0).all(), g
        cn = int(child["counts"][g])
        if cn:
            assert int(child["n"][g, :cn].sum()) == int(child["sum_n"][g]) - 1 and (child["n"][g, :cn] >= 0).all(), g
        assert a["rv"][g].tobytes() == _stub_value(states[g], 4).tobytes(), g
    assert int((child["sum_n"] > 2).sum()) >= 8                 # (the rule did select below the root)
    # a second object with the same seed gives the same bytes
    b = _k8_run(gpu, m, states, bans)
    for k in ("moves", "n", "w", "p", "sum_n", "counts"):
        assert a["st"][k].tobytes() == b["st"][k].tobytes() and a["child"][k].tobytes() == b["child"][k].tobytes(), k
    assert a["started"].tobytes() == b["started"].tobytes() and a["act"].tobytes() == b["act"].tobytes()
    assert a["tg"]["n"].tobytes() == b["tg"]["n"].tobytes()


# ---- 4. self-play at K = 1 against the oracle's loop ------------------------------------------------------------------------
def test_selfplay_games_match_the_oracle(gpu):
    from cchess_alphazero.engine import SelfPlayEngine
    G, seed, salt, m = 4, 13, 5, 8
    pc = play_config(simulation_num_per_move=32, search_threads=1, noise_eps=0.25, tau_decay_rate=0.9, max_game_length=3,
                     enable_resign_rate=0.5, resign_threshold=-0.3, min_resign_turn=1)
    eng = SelfPlayEngine(_engine_cfg(pc), G, evaluator=stub_eval(gpu, dict(kind="hash", salt=salt)), seed=seed,
                         record_visits=True, gumbel=m, gumbel_full=True)
    assert eng.gumbel_full and eng.search.gumbel_full
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
        ref = gf.gumbel_selfplay_game(ocfg, salt, seed, gid, gid % G, m)
        assert [it[0] for it in g["data"][1:]] == ref["moves"], gid
        assert (g["turns"], g["value"], g["store"], g["resigned"]) == (ref["turns"], ref["value"], ref["store"], ref["resigned"])
        vis = g["visits"]
        assert len(vis) == len(ref["plies"]) > 0
        for e, r in zip(vis, ref["plies"]):
            assert e.gumbel and not e.pruned and not e.fast and e.resign == r["resign"], (gid, e.ply)
            assert (e.moves == r["labels"]).all() and (e.banned == r["banned"]).all() and e.sum_n == r["sum_n"]
            assert e.raw_total == r["raw_total"], (gid, e.ply)
            assert np.abs(e.n - r["targets"]).max() <= 1, (gid, e.ply, e.n, r["targets"])


# ---- 5. off is off --------------------------------------------------------------------------------------------------------
def test_full_off_after_it_was_on_is_the_root_only_search(gpu):
    pc = play_config(simulation_num_per_move=SIMS, search_threads=4, noise_eps=0.25)
    cs = fo.cases()
    ev = stub_eval(gpu, dict(kind="hash", salt=9))
    states = [cs[1]["state"], cs[7]["state"]]

    def snap(x):
        st = x.root_stats()
        return [st[k].tobytes() for k in ("moves", "n", "w", "p", "sum_n", "counts")] + \
               [x.root_started().tobytes(), x.gumbel_targets()["n"].tobytes(), x.root_targets()["n"].tobytes(),
                x.choose([0.3, 0.6]).tobytes()]
    plain = gpu.S.Search(pc, 2, seed=3)
    plain.set_gumbel(M)
    plain.set_roots(boards_tensor(gpu, states))
    plain.run_until_idle(ev)
    want = snap(plain)
    s = gpu.S.Search(pc, 2, seed=3)
    s.set_gumbel(M)
    s.set_gumbel_full(True)
    s.set_roots(boards_tensor(gpu, states))
    s.run_until_idle(ev)
    on = snap(s)
    s.set_gumbel_full(False)
    s.reset_trees()
    s.set_roots(boards_tensor(gpu, states))
    s.run_until_idle(ev)
    assert snap(s) == want
    assert on[1] != want[1] and on[7] != want[7]                # (the option would have shown: counts and targets)
    # arguments: refused values leave the setting
    st = s._stream()
    L = s.L
    assert L.cz_search_set_gumbel_full(s.h, 2, st) == -1 and L.cz_search_set_gumbel_full(s.h, -1, st) == -1
    assert L.cz_search_set_gumbel_full(None, 1, st) == -1
    s.set_gumbel_full(True)
    assert L.cz_search_set_gumbel_full(s.h, 2, st) == -1
    s.reset_trees()
    s.set_roots(boards_tensor(gpu, states))
    s.run_until_idle(ev)
    assert snap(s) == on                                        # (still on after the refused call)
    s.set_gumbel(0)                                             # m = 0 clears the flag
    assert not s.gumbel_full
    assert L.cz_search_set_gumbel_full(s.h, 1, st) == -1        # ... and full needs m > 0
    s.set_gumbel(M)
    s.reset_trees()
    s.set_roots(boards_tensor(gpu, states))
    s.run_until_idle(ev)
    assert snap(s) == want                                      # (off: set_gumbel(0) switched it off in the library too)
    s.close()
    plain.close()
