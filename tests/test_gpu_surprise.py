"""-m gpu: the policy surprise record and the surprise weighting (cz_search_record_surprise, cz_search_drain_visits_cols,
cz_search_root_surprise, cz_root_surprise, cz_policy_value_loss_w; run.py self --record-surprise, run.py opt
--surprise-weight A).

The yardstick of the arithmetic is tests/surprise_oracle.py (math.log, math.fsum); its docstring derives the bound, 64 *
2^-53 * A + 1e-300 per row with A = sum |t_j log(t_j / r_j)|.  With the record off, the rings' bytes, the records and the
counters are what they were."""
import copy
import ctypes as C
import json
import logging
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import forced_playouts_oracle as fo
import stub_net
import surprise_oracle as so
from oracle import xq_oracle as xo
from selfplay_raw import drain_cols, selfplay_raw
from test_gpu_book import _engine_cfg
from test_gpu_forced_playouts import _entry_key
from test_gpu_q_record import _games_with_q, _play
from test_gpu_search import boards_tensor, gpu, no_act_tensors, play_config, stub_eval  # noqa: F401  (gpu: fixture)
from test_gpu_trainer import dev, random_games, small_config, window_of  # noqa: F401  (dev: fixture)
from test_surprise_cpu import six_element_games

pytestmark = pytest.mark.gpu
ERR_ARG = -1                                                # include/czero.h CZ_ERR_ARG
SPEC = dict(kind="hash", salt=5)
M = 128
B_ = so.BANNED


# ---- 1. the arithmetic alone ---------------------------------------------------------------------------------------------
def _row(labels, m, p):
    return dict(labels=np.asarray(labels, dtype=np.uint16), m=np.asarray(m, dtype=np.int32), p=np.asarray(p, dtype=np.float32))


def _random_row(rng, nm, ban=0.0, near=False, wide=False):
    """wide: Dirichlet(0.3) priors, which span far more than 2^22 -- rows for so.bound_wide(); otherwise so.random_priors()."""
    p = rng.dirichlet(np.full(nm, 0.3)).astype(np.float32) if wide else so.random_priors(rng, nm)
    m = (rng.integers(1, 60, nm) * (rng.random(nm) < 0.6)).astype(np.int32)
    if near:                                                # counts close to the priors: a small s
        m = np.round(p.astype(np.float64) * 3000).astype(np.int32)
    lab = rng.permutation(2086)[:nm].astype(np.uint16)
    lab[rng.random(nm) < ban] |= B_
    return _row(lab, m, p)


def _special_rows():
    rng = np.random.default_rng(5)
    rows = {
        "half_half": _row([1, 2], [5, 5], [0.25, 0.75]),
        "t_equals_r": _row([1, 2, 3], [1, 2, 1], [0.25, 0.5, 0.25]),
        "all_banned": _row([1 | B_, 2 | B_], [3, 4], [0.5, 0.5]),
        "banned_holds_the_mass": _row([1, 2 | B_, 3], [5, 100000, 5], [0.25, 100.0, 0.75]),
        "all_m_0": _row([1, 2, 3], [0, 0, 0], [0.2, 0.3, 0.5]),
        "p_sum_0": _row([1, 2], [3, 4], [0.0, 0.0]),
        "p_0_on_a_visited_edge": _row([1, 2], [1, 1], [0.0, 1.0]),
        "every_visit_on_p_0": _row([1, 2], [1000000, 0], [0.0, 1.0]),
        "one_edge_holds_every_visit": _row([1, 2, 3, 4], [0, 64, 0, 0], [0.1, 0.2, 0.3, 0.4]),
        "one_edge": _row([7], [9], [0.125]),
        "no_edge": _row([], [], []),
    }
    for nm in (0, 1, 2, 63, 64, 65, 127, 128):
        rows[f"edges_{nm}"] = _random_row(rng, nm)
    r = _random_row(rng, 100)
    r["labels"][:64] |= B_                                  # only the lanes' second edges count
    r["m"][64:] = np.maximum(r["m"][64:], 1)
    rows["second_half_only"] = r
    return rows


def test_root_surprise_alone(gpu):
    t = gpu.torch
    rows = _special_rows()
    rng = np.random.default_rng(11)
    for i in range(256):
        rows[f"random_{i}"] = _random_row(rng, int(rng.integers(1, 129)), ban=0.1 * (i % 3), near=i % 4 == 3)
    for i in range(64):                                     # priors of any span: P's own rounding on top of the bound
        rows[f"wide_{i}"] = _random_row(rng, int(rng.integers(1, 129)), ban=0.1 * (i % 3), near=i % 2 == 1, wide=True)
    names = list(rows)
    R = len(names)
    lab = np.zeros((R, M), dtype=np.uint16)
    m = np.zeros((R, M), dtype=np.int32)
    p = np.zeros((R, M), dtype=np.float32)
    ne = np.zeros(R, dtype=np.uint8)
    m[:], p[:] = 10 ** 6, 1e9                               # past n_edges: values that would change the result if read
    for i, name in enumerate(names):
        r = rows[name]
        k = len(r["m"])
        ne[i] = k
        lab[i, :k], m[i, :k], p[i, :k] = r["labels"], r["m"], r["p"]
    dev_args = [t.from_numpy(lab.view(np.int16)).cuda().view(t.uint16), t.from_numpy(m).cuda(), t.from_numpy(p).cuda(),
                t.from_numpy(ne).cuda()]
    got = gpu.S.root_surprise_rows(*dev_args).cpu().numpy()
    assert gpu.S.Search.root_surprise_rows is gpu.S.root_surprise_rows
    worst = worst_rel = worst_wide = 0.0
    for i, name in enumerate(names):
        r = rows[name]
        want, A = so.surprise(r["labels"], r["m"], r["p"])
        delta = abs(float(got[i]) - want) if want == want else 0.0
        wide = name.startswith("wide_")
        print(f"{name}: got {got[i]!r} want {want!r} delta {delta:.3e} bound {so.bound(A):.3e}")
        assert so.same(float(got[i]), want, A, wide=wide), (name, got[i], want, A)
        if want == want:
            assert 0.0 <= got[i] < so.S_BOUND, name
            if wide:
                worst_wide = max(worst_wide, delta / so.bound_wide(A))
                continue
            worst = max(worst, delta)
            worst_rel = max(worst_rel, delta / so.bound(A))
    print(f"cz_root_surprise: {R} rows, max |delta| = {worst:.3e}, max |delta| / bound = {worst_rel:.3f}; "
          f"wide priors: max |delta| / bound_wide = {worst_wide:.3f}")
    for name in ("all_banned", "all_m_0", "p_sum_0", "no_edge", "edges_0"):
        assert math.isnan(got[names.index(name)]), name
    assert not np.isnan(got[[i for i, nme in enumerate(names) if nme.startswith("random_")]]).all()
    assert got[names.index("t_equals_r")] == 0.0 and got[names.index("one_edge")] == 0.0
    assert got[names.index("banned_holds_the_mass")] == got[names.index("half_half")]
    assert abs(got[names.index("half_half")] - 0.14384103622589045) < 1e-15
    assert 68.0 < got[names.index("every_visit_on_p_0")] < so.S_BOUND
    assert got[names.index("second_half_only")] > 0.0
    # twice the same bits
    assert gpu.S.root_surprise_rows(*dev_args).cpu().numpy().tobytes() == got.tobytes()
    # arguments
    L = gpu.N.lib()
    out = t.empty(R, dtype=t.float64, device="cuda")
    ptr = [C.c_void_p(x.data_ptr()) for x in dev_args]
    st = C.c_void_p(t.cuda.current_stream().cuda_stream)
    po = C.c_void_p(out.data_ptr())
    for i in range(4):
        assert L.cz_root_surprise(*(ptr[:i] + [None] + ptr[i + 1:]), R, po, st) == ERR_ARG, i
    assert L.cz_root_surprise(*ptr, R, None, st) == ERR_ARG
    assert L.cz_root_surprise(*ptr, -1, po, st) == ERR_ARG
    assert L.cz_root_surprise(*ptr, 0, po, st) == 0


# ---- 2. single searches, external mode -----------------------------------------------------------------------------------
def _check_roots(s, bans, what):
    st, tg, sp = s.root_stats(), s.root_targets(), s.root_surprise()
    pruned = 0
    for g in range(s.G):
        c = int(st["counts"][g])
        lab = st["moves"][g, :c].copy()
        for j in range(c):
            if xo.label_str(int(lab[j])) in bans[g]:
                lab[j] |= B_
        want, A = so.surprise(lab, tg["n"][g, :c], st["p"][g, :c])
        assert want == want and 0.0 <= want < so.S_BOUND, (what, g)
        assert so.same(float(sp[g]), want, A), (what, g, sp[g], want, A)
        pruned += int((tg["n"][g, :c] != st["n"][g, :c]).any())
    return pruned, st


def test_root_surprise_of_single_searches(gpu, positions_1k):
    wide = [c for c in fo.cases() if c["name"] == "wide"][0]["state"]
    picks = [positions_1k[i]["state"] for i in (100, 250, 400, 550, 700)]
    states = [xo.INIT_STATE] + picks + [wide, picks[1]]
    assert len(states) == 8 and len(xo.get_legal_moves(wide)) == 74
    pc = play_config(simulation_num_per_move=64, search_threads=4)
    ev = stub_eval(gpu, SPEC)
    for k in (0.0, 2.0):
        s = gpu.S.Search(pc, 8, seed=7)
        assert np.isnan(s.root_surprise()).all()            # a root that is not in the tree has no surprise
        s.set_forced_playouts(k)
        bans = [[]] * 7 + [xo.get_legal_moves(states[7])[:3]]               # the golden position with a ban
        na, nn = no_act_tensors(gpu, bans)
        s.set_roots(boards_tensor(gpu, states), no_act=na, n_no_act=nn)
        s.run_until_idle(ev)
        pruned, st = _check_roots(s, bans, f"k={k} ply 0")
        # the reuse line's second ply: every game plays its most visited move and searches on in the kept subtree; the
        # last root stays and bans that move instead, so a banned edge holds visits
        best = []
        for g in range(8):
            c = int(st["counts"][g])
            n = st["n"][g, :c].astype(np.int64)
            n[[xo.label_str(int(mv)) in bans[g] for mv in st["moves"][g, :c]]] = -1
            best.append(xo.label_str(int(st["moves"][g, int(n.argmax())])))
        nxt = [xo.step(states[g], best[g]) for g in range(7)] + [states[7]]
        nxt = [states[g] if xo.done(x)[0] else x for g, x in enumerate(nxt)]
        bans2 = [[]] * 7 + [[best[7]]]
        na, nn = no_act_tensors(gpu, bans2)
        s.set_roots(boards_tensor(gpu, nxt), turns=gpu.torch.ones(8, dtype=gpu.torch.int32, device="cuda"), no_act=na,
                    n_no_act=nn)
        s.run_until_idle(ev)
        pruned2, st2 = _check_roots(s, bans2, f"k={k} ply 1")
        c = int(st2["counts"][7])
        j = [xo.label_str(int(mv)) for mv in st2["moves"][7, :c]].index(best[7])
        assert st2["n"][7, j] > 0                           # the banned edge's visits are in the tree, not in the surprise
        ctr = s.counters()
        assert ctr["tree_resets"] == 0 and ctr["overflow_sims"] == 0
        assert (pruned + pruned2 > 0) == (k > 0), (k, pruned, pruned2)
        s.close()


# ---- self-play helpers -----------------------------------------------------------------------------------------------------
_PRIORS = {}


def _priors(state):
    """(labels in edge order, float32 priors without noise) of `state` as the Python search oracle spreads them."""
    if state not in _PRIORS:
        node = fo._Node(state)
        pol, _ = stub_net.hash_stub_numpy(xo.state_to_planes(state)[None], SPEC["salt"])
        node.pending = pol[0]
        node.spread()
        _PRIORS[state] = (np.array(node.labels, dtype=np.uint16), np.array(node.p, dtype=np.float32))
    return _PRIORS[state]


def _want_s(state, moves, banned, n):
    lab, p = _priors(state)
    assert len(lab) == len(moves) and (lab == moves).all()
    return so.surprise(np.where(banned, moves | B_, moves), n, p)


# ---- 3. self-play through the engine -------------------------------------------------------------------------------------
def _strip_s(data):
    """The record without its surprise column: what the same run writes with record_surprise off (record_q on)."""
    return [data[0]] + [it[:5] if len(it) == 6 else it for it in data[1:]]


@pytest.mark.parametrize("k", [2.0, 0.0])
def test_selfplay_games_carry_the_oracles_surprise(gpu, k):
    G = 16
    pc = play_config(simulation_num_per_move=16, search_threads=1, noise_eps=0.0, tau_decay_rate=0.6, max_game_length=6,
                     enable_resign_rate=0.5, resign_threshold=-0.4, min_resign_turn=4)
    kw = dict(fast_sims=4, full_rate=0.5)
    games, ctr = _play(gpu, pc, G, 17, k, record_surprise=True, **kw)
    assert ctr["visits_dropped"] == 0 and ctr["tree_resets"] == 0 and ctr["overflow_sims"] == 0
    ply0 = {}
    n_s = n_fast = n_full = 0
    worst = 0.0
    for g in games:
        vis = g["visits"]
        assert vis is not None
        items = g["data"][1:]
        state = g["data"][0]
        for i, e in enumerate(vis):
            want, A = _want_s(state, e.moves, e.banned, e.n)        # the oracle's priors, the entry's counts
            got = so.NAN if e.s is None else e.s
            assert so.same(got, want, A), (g["game_id"], i, e.s, want, A)
            if want == want:
                worst = max(worst, abs(got - want) / so.bound(A))
                n_s += 1
            if i == 0:                                              # ... and at ply 0 the oracle's counts as well
                if e.fast not in ply0:
                    o = fo.Search(fo.play_cfg(4 if e.fast else 16), SPEC["salt"], 0.0 if e.fast else k)
                    o.search(state)
                    ply0[e.fast] = (o.targets(state)[0] if not e.fast else o.node_stats(state)["n"], o.node_stats(state)["p"])
                cnt, p = ply0[e.fast]
                assert (e.n == cnt).all() and (p.view(np.uint32) == _priors(state)[1].view(np.uint32)).all()
                assert e.pruned == (k > 0 and not e.fast)
            if e.resign:
                assert i == len(vis) - 1 and len(items) == i
                continue
            it = items[i]
            assert len(it) == 6 and it[3] == (0 if e.fast else 1), (g["game_id"], i, it)
            assert it[4] == (None if e.q is None else round(e.q, 6)) and it[5] == (None if e.s is None else round(e.s, 6))
            n_fast += e.fast
            n_full += not e.fast
            state = xo.step(state, it[0])
        for it in items[len(vis):]:                                 # the appended king capture
            assert len(it) == 2
    assert set(ply0) == {False, True}
    data = [g["data"] for g in games]
    assert json.loads(json.dumps(data)) == data
    print(f"k={k}: {len(games)} games, {n_s} surprises ({n_full} full, {n_fast} fast plies), max |delta| / bound = {worst:.3f}")
    assert n_s > 3 * G and n_fast > 0 and n_full > 0
    # the surprise column is the only addition: entries, values, records and counters of the same run without it
    off, ctr0 = _play(gpu, pc, G, 17, k, **kw)
    assert ctr0 == ctr
    assert [g["game_id"] for g in off] == [g["game_id"] for g in games]
    qbits = lambda e: None if e.q is None else np.float64(e.q).tobytes()  # noqa: E731
    for a, b in zip(off, games):
        assert a["data"] == _strip_s(b["data"]), a["game_id"]
        assert [_entry_key(e) + (qbits(e),) for e in a["visits"]] == [_entry_key(e) + (qbits(e),) for e in b["visits"]]
        assert all(e.s is None for e in a["visits"])
        assert {k_: v for k_, v in a.items() if k_ not in ("data", "visits")} == \
               {k_: v for k_, v in b.items() if k_ not in ("data", "visits")}
    # without the value record the q column is None and the surprises are the same bits
    from cchess_alphazero.engine import SelfPlayEngine
    eng = SelfPlayEngine(_engine_cfg(pc), 2, evaluator=stub_eval(gpu, SPEC), seed=17, record_visits=True,
                         record_surprise=True)
    assert eng.search.surprise_on and not eng.search.values_on
    eng.close()


# ---- 4. off means off, every drain, the full ring --------------------------------------------------------------------------
def _selfplay_raw(gpu, pc, seed, rounds, setup, columns=("q",), capacity=0, G=16, before=None):
    """selfplay_raw with the playout cap (4, 0.5) and `setup` AFTER the visit ring is on (`before`: ahead of it); entries
    (row, q bytes, s bytes, maxq bytes), -7.0 where the drain writes none; a ring of `capacity` may drop entries."""
    return selfplay_raw(gpu, pc, seed, rounds, G, setup_before=before, setup_after=setup, capacity=capacity,
                        playout_cap=(4, 0.5), columns=columns, fill=-7.0, no_drops=False)


def _check_raw_surprises(recs, entries):
    """Every entry whose game has finished: its s against the oracle, from the game's moves and the entry's own counts."""
    moves = {}
    for rec in recs:
        a = np.frombuffer(rec, dtype=np.uint8)
        moves[int(a[0:4].view(np.uint32)[0])] = [xo.label_str(int(l) & 0x7FFF) for l in a[16:].view(np.uint16)]
    checked = with_s = 0
    for row, _, sb, _ in entries:
        a = np.frombuffer(row, dtype=np.uint8)
        gid, ply, ne = int(a[0:4].view(np.uint32)[0]), int(a[4:6].view(np.uint16)[0]), int(a[6])
        if gid not in moves or ply > len(moves[gid]):
            continue
        state = xo.INIT_STATE
        for mv in moves[gid][:ply]:
            state = xo.step(state, mv)
        lab = a[16:16 + 2 * ne].view(np.uint16)
        n = a[16 + 2 * ne:16 + 6 * ne].view(np.int32)
        want, A = _want_s(state, lab & 0x7FFF, (lab & B_) != 0, n)
        got = float(np.frombuffer(sb, dtype=np.float64)[0])
        assert so.same(got, want, A), (gid, ply, got, want, A)
        checked += 1
        with_s += want == want
    return checked, with_s


def test_surprise_off_leaves_every_record_entry_value_and_counter(gpu):
    pc = play_config(simulation_num_per_move=16, search_threads=4, tau_decay_rate=0.9, max_game_length=8,
                     enable_resign_rate=0.5, resign_threshold=-0.4, min_resign_turn=4)
    rounds = 240
    q_on = lambda s: s.record_values(True)  # noqa: E731
    base, vis0, c0 = _selfplay_raw(gpu, pc, 31, rounds, q_on)
    assert len(base) >= 16 and len(vis0) > len(base) and c0["visits_dropped"] == 0
    rows_q = [(row, q) for row, q, _, _ in vis0]
    assert len({q for _, q in rows_q}) > 8
    # switched off, and switched on and off again: nothing differs
    for setup in (lambda s: (q_on(s), s.record_surprise(False)), lambda s: (q_on(s), s.record_surprise(True), s.record_surprise(False))):
        recs, vis, ctr = _selfplay_raw(gpu, pc, 31, rounds, setup)
        assert recs == base and vis == vis0 and ctr == c0
    # ON: the records, the visit ring, the value ring and the counters still hold the same bytes, through every drain
    both = lambda s: (q_on(s), s.record_surprise(True))  # noqa: E731
    recs, vis_qs, ctr = _selfplay_raw(gpu, pc, 31, rounds, both, columns=("q", "s"))
    assert recs == base and ctr == c0 and [(row, q) for row, q, _, _ in vis_qs] == rows_q
    checked, with_s = _check_raw_surprises(recs, vis_qs)
    assert checked > len(vis_qs) // 2 and with_s > checked // 2
    assert len({sb for _, _, sb, _ in vis_qs}) > 8                     # (surprises of their entries, not a constant)
    recs, vis, ctr = _selfplay_raw(gpu, pc, 31, rounds, both, columns=("q",))   # a column that is not asked for is dropped
    assert recs == base and ctr == c0 and vis == vis0
    recs, vis, ctr = _selfplay_raw(gpu, pc, 31, rounds, both, columns=())
    assert recs == base and ctr == c0 and [e[0] for e in vis] == [e[0] for e in vis0]
    # the surprise record alone, the q column NULL: the same entries and the same surprises
    recs, vis, ctr = _selfplay_raw(gpu, pc, 31, rounds, lambda s: s.record_surprise(True), columns=("s",))
    assert recs == base and ctr == c0 and [(row, sb) for row, _, sb, _ in vis] == [(row, sb) for row, _, sb, _ in vis_qs]
    # a ring that fills: an entry that finds it full is dropped with its surprise, the others keep theirs -- the ring
    # wraps many times here, so a surprise in the wrong slot would show
    recs, vis, ctr = _selfplay_raw(gpu, pc, 31, rounds, both, columns=("q", "s"), capacity=24)
    assert recs != [] and ctr["visits_dropped"] > 0 and 24 < len(vis) < len(vis0)
    assert set(vis) <= set(vis_qs)
    checked, with_s = _check_raw_surprises(recs, vis)
    assert checked > len(vis) // 2 and with_s > 0


@pytest.mark.parametrize("k", [0.0, 2.0])
def test_a_record_that_is_off_never_changes_the_others(gpu, k):
    """Values and surprise on against values only, surprise only and neither, with pruning (k = 2) as well: the records,
    the entries, the values, the surprises and the counters are the same bytes wherever two runs both have them."""
    pc = play_config(simulation_num_per_move=16, search_threads=4, tau_decay_rate=0.9, max_game_length=8,
                     enable_resign_rate=0.5, resign_threshold=-0.4, min_resign_turn=4)

    def run(values, surprise, columns):
        def setup(s):
            s.set_forced_playouts(k)
            s.record_values(values)
            s.record_surprise(surprise)
        recs, vis, ctr = _selfplay_raw(gpu, pc, 31, 240, setup, columns=columns)
        assert ctr["visits_dropped"] == 0
        return recs, vis, ctr
    recs, vis, ctr = run(True, True, ("q", "s"))
    assert len(recs) >= 16 and len(vis) > len(recs)
    assert len({q for _, q, _, _ in vis}) > 8 and len({sb for _, _, sb, _ in vis}) > 8
    assert any(row[7] & gpu.S.VISIT_PRUNED for row, _, _, _ in vis) == (k > 0)
    recs_q, vis_q, ctr_q = run(True, False, ("q",))
    assert recs_q == recs and ctr_q == ctr and [(row, q) for row, q, _, _ in vis_q] == [(row, q) for row, q, _, _ in vis]
    recs_s, vis_s, ctr_s = run(False, True, ("s",))
    assert recs_s == recs and ctr_s == ctr and [(row, sb) for row, _, sb, _ in vis_s] == [(row, sb) for row, _, sb, _ in vis]
    recs_p, vis_p, ctr_p = run(False, False, ())
    assert recs_p == recs and ctr_p == ctr and [e[0] for e in vis_p] == [e[0] for e in vis]


# ---- 5. the loss kernel -----------------------------------------------------------------------------------------------------
EPS, HI = np.float32(1e-7), np.float32(1.0 - 1e-7)


@pytest.mark.parametrize("B", [1, 3, 64, 65])
def test_loss_kernel_with_row_weights(dev, B):
    import torch
    from cchess_alphazero import _native
    from cchess_alphazero.lib.replay_window import mix_targets
    w = window_of(_games_with_q(41, 10))
    n = len(w)
    rng = np.random.default_rng(60 + B)
    idx_h = rng.integers(0, n, size=B).astype(np.int32)
    oob = 1 if B > 1 else None
    if oob is not None:
        idx_h[oob] = n                                      # one out-of-range index: zero loss and gradient
    idx = torch.from_numpy(idx_h).to(dev)
    logits = torch.from_numpy(rng.normal(0, 2, size=(B, 2086)).astype(np.float32)).to(dev)
    v = torch.from_numpy(np.tanh(rng.normal(size=B)).astype(np.float32)).to(dev)
    flags_h = rng.integers(0, 2, size=B).astype(np.uint8)
    flags = torch.from_numpy(flags_h).to(dev)
    rw_h = rng.choice(np.array([0.0, 0.25, 1.0, 3.5], dtype=np.float32), size=n)
    rw = torch.from_numpy(rw_h).to(dev)
    wp, wv, lam = 1.25, 0.75, 0.3
    args = (w.played[:n], w.z[:n], w.row_ptr[:n + 1], w.vis_label[:w.nnz], w.vis_count[:w.nnz], 1, wp, wv)
    plain = _native.policy_value_loss(logits, v, idx, *args, mirror=flags, q=w.q[:n], q_ratio=lam)
    pl, se, gl, gv = _native.policy_value_loss(logits, v, idx, *args, mirror=flags, q=w.q[:n], q_ratio=lam, row_w=rw)
    # the per-row losses stay the unweighted ones
    assert torch.equal(pl, plain[0]) and torch.equal(se, plain[1])
    # float64 restatement (tests/test_gpu_trainer.py), the row's scale times its weight
    ok = np.ones(B, dtype=bool)
    if oob is not None:
        ok[oob] = False
    safe = np.where(ok, idx_h, 0)
    t = w.dense_targets(safe, "visits", mirror=flags_h).astype(np.float64)
    zt = mix_targets(w.z[:n].cpu().numpy()[safe], w.q[:n].cpu().numpy()[safe], lam).astype(np.float64)
    wr = np.where(ok, rw_h[safe], 0.0).astype(np.float64)
    x = logits.cpu().numpy().astype(np.float64)
    p = np.exp(x - x.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    pc = np.clip(p, np.float64(EPS), np.float64(HI))
    lo_ref = np.where(ok, -(t * np.log(pc)).sum(1), 0.0)
    vv = v.cpu().numpy().astype(np.float64)
    se_ref = np.where(ok, (vv - zt) ** 2, 0.0)
    msk = (p > EPS) & (p < HI)
    S = (t * msk).sum(1, keepdims=True)
    g_ref = wp / B * wr[:, None] * (p * S - t * msk)
    gv_ref = wv * 2 * (vv - zt) / B * wr
    d_pl = np.abs(pl.cpu().numpy() - lo_ref).max()
    d_gl = np.abs(gl.cpu().numpy() - g_ref).max()
    d_gv = np.abs(gv.cpu().numpy() - gv_ref).max()
    print(f"B={B}: max |delta| policy_loss {d_pl:.3e} grad_logits {d_gl:.3e} grad_v {d_gv:.3e}")
    assert np.allclose(pl.cpu().numpy(), lo_ref, rtol=1e-6, atol=1e-7)
    assert np.allclose(se.cpu().numpy(), se_ref, rtol=1e-6, atol=1e-9)
    assert d_gl < 1e-6 and d_gv < 1e-6
    # the weight is one rounded float32 product on top of the unweighted scale
    wrow = torch.from_numpy(np.where(ok, rw_h[safe], 1.0).astype(np.float32)).to(dev)
    assert torch.equal(gv, plain[3] * wrow)
    zero = torch.from_numpy(~ok | (np.where(ok, rw_h[safe], 1.0) == 0)).to(dev)
    assert (gl[zero] == 0).all() and (gv[zero] == 0).all()
    one = torch.from_numpy(ok & (rw_h[safe] == 1.0)).to(dev)
    assert torch.equal(gl[one], plain[2][one]) and torch.equal(gv[one], plain[3][one])
    # all-ones weights and row_w = NULL: the bits of cz_policy_value_loss_q
    ones = _native.policy_value_loss(logits, v, idx, *args, mirror=flags, q=w.q[:n], q_ratio=lam, row_w=torch.ones_like(rw))
    assert all(torch.equal(a, b) for a, b in zip(ones, plain))
    L = _native.lib()
    out = [torch.empty_like(x_) for x_ in plain]
    ptr = lambda x_: None if x_ is None else C.c_void_p(x_.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.cz_policy_value_loss_w(ptr(logits), logits.stride(0), ptr(v), ptr(idx), ptr(flags), B, n, ptr(w.row_ptr),
                                  ptr(w.vis_label), ptr(w.vis_count), w.nnz, ptr(w.played), ptr(w.z), ptr(w.q), lam, None, 1,
                                  wp, wv, *[ptr(x_) for x_ in out], st)
    torch.cuda.synchronize()
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(out, plain))
    # without mirror flags and without q: the weighted form of the plain entry point
    a = _native.policy_value_loss(logits, v, idx, *args, row_w=torch.ones_like(rw))
    b = _native.policy_value_loss(logits, v, idx, *args)
    assert all(torch.equal(x_, y_) for x_, y_ in zip(a, b))


# ---- 6. the window ----------------------------------------------------------------------------------------------------------
def _games_with_s(seed, n_games, s_rate=0.8, fast_rate=0.3):
    """random_games with visit counts, every item widened to [move, value, pi or None, weight, q or None, s or None]; a game
    in three has no s at all and one in three is left in the two- and three-element forms."""
    rng = np.random.default_rng(seed)
    games = random_games(seed, n_games, max_plies=30, pi=True)
    for gi, g in enumerate(games):
        if gi % 3 == 2:
            continue
        for it in g[1:]:
            s = round(float(rng.gamma(0.5, 0.5)), 6) if gi % 3 == 0 and rng.random() < s_rate else None
            it += [None] * (3 - len(it)) + [0 if rng.random() < fast_rate else 1,
                                             None if rng.random() < 0.3 else round(float(rng.uniform(-2, 2)), 6), s]
    return games


def _expected_weights(games, alpha):
    from cchess_alphazero.lib.replay_window import surprise_weights
    items = [it for g in games for it in g[1:]]
    s = np.array([it[5] if len(it) >= 6 and it[5] is not None else np.nan for it in items], dtype=np.float32)
    tr = np.array([it[3] if len(it) >= 4 else 1 for it in items], dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(g) - 1 for g in games])])
    return s, tr, surprise_weights(s, tr, offs, alpha)


def test_window_holds_the_weights_and_refuses_a_malformed_surprise(dev):
    from cchess_alphazero.lib.replay_window import ReplayWindow
    games = _games_with_s(43, 9)
    w = ReplayWindow(10 ** 6, surprise_weight=0.5)
    w.add_games(games[:5])
    w.add_games(games[5:])                                  # a second load: its games' weights are their own
    n = len(w)
    s, tr, want = _expected_weights(games, 0.5)
    assert n == len(s) and (w.trainable == tr).all()
    assert w.s[:n].cpu().numpy().tobytes() == s.tobytes()
    got = w.w[:n].cpu().numpy()
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    assert np.isfinite(s).any() and np.isnan(s).any() and (got[tr == 0] == 0).all() and got.max() > 1.0 and 0.5 <= got[tr == 1].min() < 1.0
    # records with s only, and without any
    for sub in ([g for i, g in enumerate(games) if i % 3 == 0], [g for i, g in enumerate(games) if i % 3 != 0]):
        w1 = ReplayWindow(10 ** 6, surprise_weight=1.0)
        w1.add_games(sub)
        assert w1.w[:len(w1)].cpu().numpy().tobytes() == _expected_weights(sub, 1.0)[2].tobytes()
    # without the option no array exists and a weighted loss is refused
    w0 = window_of(games)
    assert w0.w is None and w0.surprise_weight == 0.0 and w0.s[:n].cpu().numpy().tobytes() == s.tobytes()
    import torch
    lg = torch.zeros((2, 2086), device=dev)
    with pytest.raises(ValueError, match="surprise_weight"):
        w0.loss(lg, torch.zeros(2, device=dev), torch.zeros(2, dtype=torch.int32, device=dev), surprise=True)
    for bad in (-0.1, 1.5, float("nan"), True):
        with pytest.raises(ValueError, match="surprise_weight"):
            ReplayWindow(10, surprise_weight=bad)
    # the weighted means of the window's loss: mean(w[idx] * loss), the kernel's gradients
    from cchess_alphazero import _native
    rng = np.random.default_rng(3)
    B = 48
    idx_h = rng.integers(0, n, size=B).astype(np.int32)
    idx = torch.from_numpy(idx_h).to(dev)
    logits = torch.from_numpy(rng.normal(0, 2, size=(B, 2086)).astype(np.float32)).to(dev)
    v = torch.from_numpy(np.tanh(rng.normal(size=B)).astype(np.float32)).to(dev)
    pl, se, gl, gv = _native.policy_value_loss(logits, v, idx, w.played[:n], w.z[:n], w.row_ptr[:n + 1], w.vis_label[:w.nnz],
                                               w.vis_count[:w.nnz], 1, 1.25, 0.75, row_w=w.w[:n])
    lg2, vg2 = logits.clone().requires_grad_(True), v.clone().requires_grad_(True)
    tot, pm, vm = w.loss(lg2, vg2, idx, "visits", (1.25, 0.75), surprise=True)
    tot.backward()
    wr = torch.from_numpy(want[idx_h]).to(dev)
    assert torch.equal(pm, (wr * pl).mean()) and torch.equal(vm, (wr * se).mean())
    assert torch.equal(tot, 1.25 * pm + 0.75 * vm) and torch.equal(lg2.grad, gl) and torch.equal(vg2.grad, gv)
    # a malformed s raises, names the game and the ply, and leaves the window as it was
    snap = lambda: (len(w), w.nnz, w.n_games, w.s[:len(w)].cpu().numpy().tobytes(), w.w[:len(w)].cpu().numpy().tobytes(),  # noqa: E731
                    w.q[:len(w)].cpu().numpy().tobytes(), w.z[:len(w)].cpu().numpy().tobytes())
    before = snap()
    long = next(g for g in games[::3] if len(g) >= 3)
    for bad in (-0.1, 71, float("nan"), "1", True):
        g = [copy.deepcopy(long), copy.deepcopy(long)]
        g[1][2][5] = bad
        with pytest.raises(ValueError, match=r"game 1, ply 1"):
            w.add_games(g)
        assert snap() == before
    for ok in (0, 0.0, 70, 69.077553, None):
        g = [copy.deepcopy(long)]
        g[0][1][5] = ok
        got = window_of(g).s[0].item()
        assert math.isnan(got) if ok is None else got == np.float32(ok)


def test_expand_records_takes_six_element_items(dev):
    import torch
    from cchess_alphazero.lib.record_decoder import expand_records
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_records.json")) as f:
        games = [g["data"] for g in json.load(f)["games"]][:6]
    a = expand_records(games)
    b = expand_records(six_element_games(games))
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(torch.as_tensor(x), torch.as_tensor(y))


# ---- 7. a trainer pass ------------------------------------------------------------------------------------------------------
def test_trainer_pass_with_and_without_the_weights(dev, tmp_path, monkeypatch):
    import torch
    from cchess_alphazero.agent.model import CChessModel
    from cchess_alphazero.worker.optimize import OptimizeWorker
    games = _games_with_s(21, 12, fast_rate=0.0)
    # (the convolutions' backward pass repeats bit for bit only in the library's deterministic mode, as
    #  tests/test_gpu_q_record.py found)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    runs = {}
    for name, extra in (("none", {}), ("0", dict(surprise_weight=0.0)), ("0.5", dict(surprise_weight=0.5))):
        cfg = small_config(tmp_path, monkeypatch, batch_size=32, policy_targets="visits", **extra)
        ow = OptimizeWorker(cfg)
        assert ow.surprise_weight == extra.get("surprise_weight", 0.0)
        ow.model = CChessModel(cfg)
        ow.model.build(seed=3)
        ow.model.model.cuda().train()
        ow.compile_model()
        ow.update_learning_rate(0)
        ow.window = ow.new_window()
        ow.window.add_games(games)
        assert (ow.window.w is not None) == (name == "0.5")
        val0 = ow.evaluate(torch.arange(32, dtype=torch.int32, device=dev))     # equal parameters: never weighted
        rng = np.random.default_rng(0)
        losses = []
        for _ in range(3):
            idx = rng.permutation(len(ow.window))[:32].astype(np.int32)
            losses.append([x.item() for x in ow.step(torch.from_numpy(idx).to(dev))])
        val = ow.evaluate(torch.arange(32, dtype=torch.int32, device=dev))
        runs[name] = (losses, val0, val, {k: v.clone() for k, v in ow.model.model.state_dict().items()})
    assert runs["none"][:3] == runs["0"][:3]
    for k, a in runs["none"][3].items():
        assert torch.equal(a, runs["0"][3][k]), k
    assert runs["0.5"][1] == runs["0"][1]                   # the validation losses do not depend on the option
    assert all(math.isfinite(x) for row in runs["0.5"][0] for x in row) and all(math.isfinite(x) for x in runs["0.5"][2])
    assert runs["0.5"][0] != runs["0"][0]
    assert any(not torch.equal(a, runs["0.5"][3][k]) for k, a in runs["0"][3].items())
    w = ow.window.w[:len(ow.window)].cpu().numpy()
    assert w.min() < 1.0 < w.max()
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="surprise_weight"):
            OptimizeWorker(small_config(tmp_path, monkeypatch, surprise_weight=bad))


# ---- 8. arguments -----------------------------------------------------------------------------------------------------------
def test_record_surprise_argument_errors_leave_the_setting(gpu):
    pc = play_config(simulation_num_per_move=16, search_threads=4, max_game_length=6)
    s = gpu.S.Search(pc, 2, seed=1)
    st = s._stream()
    L = s.L
    # without the visit ring: refused, and the object stays off
    assert L.cz_search_record_surprise(s.h, 1, st) == ERR_ARG
    with pytest.raises(gpu.N.NativeError):
        s.record_surprise(True)
    assert not s.surprise_on
    assert L.cz_search_record_surprise(s.h, 0, st) == 0         # switching off what is off is no error
    assert L.cz_search_record_surprise(None, 1, st) == ERR_ARG
    s.record_visits(True, capacity=64)
    n = C.c_int(-1)
    buf = np.zeros((64, gpu.S.VISIT_STRIDE), dtype=np.uint8)
    qb = np.zeros(64, dtype=np.float64)
    sb = np.zeros(64, dtype=np.float64)

    def drain(host, q, sp, max_entries, n_out):
        return drain_cols(s, host, (q, sp, None), max_entries, n_out)
    # a buffer for a record that is off is refused; all NULL is the plain drain
    assert drain(buf, None, sb, 64, C.byref(n)) == ERR_ARG
    assert drain(buf, qb, None, 64, C.byref(n)) == ERR_ARG
    assert drain(buf, None, None, 64, C.byref(n)) == 0 and n.value == 0
    s.record_surprise(True)
    assert s.surprise_on and not s.values_on
    assert drain(None, None, None, 0, C.byref(n)) == 0 and n.value == 0
    assert drain(buf, qb, sb, 64, C.byref(n)) == ERR_ARG
    assert drain(buf, None, sb, -1, C.byref(n)) == ERR_ARG
    assert drain(buf, None, sb, 64, None) == ERR_ARG
    assert L.cz_search_root_surprise(s.h, None, st) == ERR_ARG
    assert L.cz_search_root_surprise(None, C.c_void_p(gpu.torch.empty(2, dtype=gpu.torch.float64, device="cuda").data_ptr()),
                                     st) == ERR_ARG
    # the setting is kept after the refusals: a short self-play run still hands out surprises
    s.start_selfplay(seed=1)
    ev = stub_eval(gpu, SPEC)
    for _ in range(40):
        s.round()
        p, v = ev(s.planes)
        s.policy.copy_(p)
        s.value.copy_(v)
    ents = [e for es in s.waiting_visits().values() for e in es]
    assert ents and sum(e.s is not None for e in ents) > 0 and all(e.q is None for e in ents)
    assert all(e.s is None or 0.0 <= e.s < so.S_BOUND for e in ents)
    # the visit ring going takes the surprise ring with it
    s.record_visits(False)
    assert not s.surprise_on
    assert L.cz_search_record_surprise(s.h, 1, st) == ERR_ARG
    s.close()
    from cchess_alphazero.engine import SelfPlayEngine
    with pytest.raises(ValueError, match="record_visits"):
        SelfPlayEngine(_engine_cfg(pc), 2, evaluator=stub_eval(gpu, SPEC), record_surprise=True)


# ---- 9. the command line ----------------------------------------------------------------------------------------------------
def test_run_py_self_with_record_surprise_then_opt_with_surprise_weight(tmp_path, monkeypatch):
    from cchess_alphazero import manager
    from cchess_alphazero.agent.model import CChessModel
    from cchess_alphazero.lib.data_helper import get_game_data_filenames, read_game_data_from_file
    from cchess_alphazero.lib.record_decoder import split_games
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "chinesechess-alphazero_amd")
    env = dict(os.environ, DATA_DIR=str(tmp_path / "data"), PROJECT_DIR=str(tmp_path), PYTHONPATH=pkg)
    run = [sys.executable, os.path.join(pkg, "cchess_alphazero", "run.py"), "self", "--type", "mini"]
    r = subprocess.run(run + ["--record-surprise"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "needs --record-visits" in r.stderr
    r = subprocess.run(run + ["--games-per-gpu", "32", "--record-visits", "--record-surprise", "--fast-sims", "8",
                              "--max-games", "8"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(tmp_path / "logs" / "play.log") as f:
        log = f.read()
    assert "policy surprise s" in log
    m = re.search(r"policy surprise of (\d+) full plies written, mean s = ([0-9.]+); of (\d+) fast plies, mean s = ([0-9.]+)", log)
    assert m and int(m.group(1)) > 0 and 0.0 <= float(m.group(2)) < so.S_BOUND and 0.0 <= float(m.group(4)) < so.S_BOUND
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
    six = [it for it in items if len(it) == 6]
    assert six and {it[3] for it in six} == {0, 1} and all(it[4] is None for it in six)
    assert any(it[5] is not None for it in six) and all(it[5] is None or 0.0 <= it[5] < so.S_BOUND for it in six)
    assert all(len(it) in (2, 6) for it in items)
    model = CChessModel(cfg)
    model.build(seed=0)
    model.save(rc.model_best_config_path, rc.model_best_weight_path)
    digest0 = model.digest
    monkeypatch.setattr(sys, "argv", ["run.py", "opt", "--type", "mini", "--surprise-weight", "0.5", "--policy-targets",
                                      "visits"])
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
        m = re.search(r"weighted by policy surprise, A = 0.5: (\d+) of (\d+) carry an s; weights min ([0-9.]+) mean ([0-9.]+) "
                      r"max ([0-9.]+)", f.read())
    assert m and 0 < int(m.group(1)) <= int(m.group(2))
    assert 0.5 <= float(m.group(3)) <= float(m.group(4)) <= float(m.group(5))
    best = CChessModel(cfg)
    assert best.load(rc.model_best_config_path, rc.model_best_weight_path) and best.digest != digest0
