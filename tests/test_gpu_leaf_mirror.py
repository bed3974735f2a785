"""-m gpu: the random leaf mirror of the search (cz_search_set_leaf_mirror; run.py self / eval --leaf-mirror P).

A new leaf may be shown to the network as the left-right mirror image of its position; its policy row is then read at
column M(a) for move a (M = cz_label_mirror), its value as it is.  The yardstick is the engine itself at rate 0 under
stub_net.hash_stub_torch -- asymmetric: every plane element and every label matters -- which tests/test_gpu_search.py pins
to the oracle.  A stand-in network that is told which rows are mirrored (the per-slot flags) and undoes the mirror on both
sides must leave every statistic of the search bit for bit where it was; so must a network that is exactly
mirror-equivariant without being told anything."""
import json
import math
import os

import numpy as np
import pytest

import forced_playouts_oracle as fo
import stub_net
from oracle import xq_oracle as xo
from test_gpu_search import END, MID, boards_tensor, gpu, play_config, stub_eval  # noqa: F401

pytestmark = pytest.mark.gpu
ERR_ARG = -1                                                # include/czero.h CZ_ERR_ARG
G, SIMS = 32, 64
WIDE = [c for c in fo.cases() if c["name"] == "wide"][0]["state"]
CTRS = ("sims", "expansions", "terminal_sims", "repetition_sims")


def _states():
    """G root positions from tests/golden: INIT, a middlegame, an endgame, the root with more than 64 moves, then a spread
    of the 1k suite."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "positions_1k.json")) as f:
        pos = json.load(f)["positions"]
    out = [xo.INIT_STATE, MID, END, WIDE] + [pos[i]["state"] for i in range(5, 1000, 35)]
    return out[:G]


STATES = _states()
WIDE_G = 3


def _two_ply_lines(states):
    """For the 28-plane cases: (roots, prev, kind).  Odd games search the position two plies down a line from their state
    with the line's first position as the game history (hist_kind 1: fresh simulations take the second block from
    g_prev_board); even games, the wide root and lines that end early have no game history (hist_kind 0: the second block
    comes from the simulation's own path once it is two plies deep)."""
    roots, prev, kind = [], [], []
    for g, s0 in enumerate(states):
        line = [s0]
        while g % 2 == 1 and g != WIDE_G and len(line) < 3 and not xo.done(line[-1])[0]:
            line.append(xo.step(line[-1], xo.get_legal_moves(line[-1])[g % 3]))
        ok = len(line) == 3 and not xo.done(line[-1])[0]
        roots.append(line[-1] if ok else s0)
        prev.append(line[0] if ok else s0)
        kind.append(1 if ok else 0)
    return roots, prev, kind


@pytest.fixture(scope="module")
def M(gpu):
    return gpu.torch.from_numpy(gpu.N.label_mirror().astype(np.int64)).cuda()


def flag_aware(ev, M):
    """The stand-in network behind the flags: a flagged row is un-mirrored before `ev` sees it (planes flipped along the
    file axis) and its policy row is written so that column M(a) holds ev's entry for a (M is an involution: a gather
    through M).  Unflagged rows go through unchanged."""
    def f(planes, flags):
        fl = flags.bool()
        x = planes.clone()
        x[fl] = planes[fl].flip(-1)
        out = ev(x)                                             # (policy, value, and what else the search reads: as it is)
        p = out[0].clone()
        p[fl] = p[fl][:, M]
        return (p,) + tuple(out[1:])
    return f


def drive(gpu, M, K, rate, logits=False, boards_only=False, hist=False, compact=False, spec=None, seed=7, sims=SIMS,
          evaluate=None, flags=True, setup=None, probe=None):
    """One search of STATES driven round by round through round() / leaf_rows() (or the compact queue) with the flag-aware
    stand-in.  rate None: set_leaf_mirror is never called.  setup(s): further setters, before the roots are set; an `evaluate`
    with a third output writes it to the rows that setup's option reads (moves_left_x or wdl_rows).  Returns
    dict(st=root_stats, ctr, flags=[(slot, flag)] of every leaf written, in round order; probe: probe(s) after the search)."""
    t = gpu.torch
    pc = play_config(simulation_num_per_move=sims, search_threads=K)
    s = gpu.S.Search(pc, G, seed=seed, use_history=hist)
    if logits:
        s.policy_logits(True)
    if boards_only:
        s.leaf_masks(True)
        s.leaf_planes(False)
    for r in rate if isinstance(rate, tuple) else (rate,):          # (a tuple: one call after the other)
        if r is not None:
            s.set_leaf_mirror(r, flags=flags)
    if setup:
        setup(s)
    if hist:
        roots, prev, kind = _two_ply_lines(STATES)
        s.set_roots(boards_tensor(gpu, roots), prev_boards=boards_tensor(gpu, prev),
                    hist_kind=t.tensor(kind, dtype=t.uint8, device="cuda"))
    else:
        s.set_roots(boards_tensor(gpu, STATES))
    ev = evaluate or flag_aware(stub_eval(gpu, spec or dict(kind="hash", salt=3)), M)
    seen = []
    for _ in range(10000):
        s.round(compact=compact)
        pending, rows = s.leaf_rows()
        if pending == 0:
            break
        n = rows.numel()
        if compact:
            n = int(s.q_count.item())
            rows = s.q_rows[:n].long()
        if not n:
            continue
        fl = s.mirrored[rows] if s.mirrored is not None else t.zeros(n, dtype=t.uint8, device="cuda")
        seen += sorted(zip(rows.tolist(), fl.tolist()))          # (the order of the rows within a round is arbitrary)
        p, v, *more = ev(s.queue_planes(rows=rows), fl)
        if logits:
            p = t.log(p.double()).float()
        extra = s.wdl_rows if s.draw_on else s.moves_left_x
        if compact:
            s.policy[:n] = p
            s.value[:n] = v
            if more:
                extra[:n] = more[0]
        else:
            s.policy.index_copy_(0, rows, p)
            s.value.index_copy_(0, rows, v)
            if more:
                extra.index_copy_(0, rows, more[0])
    out = dict(st=s.root_stats(), ctr=s.counters(), flags=seen, K=s.K)
    if probe:
        out["probe"] = probe(s)
    s.close()
    return out


def assert_same_search(a, b, what=""):
    sa, sb = a["st"], b["st"]
    assert (sa["counts"] == sb["counts"]).all(), what
    for g in range(G):
        c = int(sa["counts"][g])
        assert (sa["moves"][g, :c] == sb["moves"][g, :c]).all(), (what, g)
        assert (sa["n"][g, :c] == sb["n"][g, :c]).all(), (what, g, sa["n"][g, :c], sb["n"][g, :c])
        assert (sa["w"][g, :c].view(np.uint64) == sb["w"][g, :c].view(np.uint64)).all(), (what, g)
        assert (sa["p"][g, :c].view(np.uint32) == sb["p"][g, :c].view(np.uint32)).all(), (what, g)
    assert (sa["sum_n"] == sb["sum_n"]).all(), what
    for k in CTRS:
        assert a["ctr"][k] == b["ctr"][k], (what, k, a["ctr"][k], b["ctr"][k])


# ---- 1. exactness under a flag-aware stand-in network ----------------------------------------------------------------------
# (K, policy_logits, boards only, 28 planes, compact queue): every value of every parameter with both K = 1 and K = 8,
# and K = 80 for the slot-by-slot attach
CASES = [
    (1, False, False, False, False),
    (8, False, False, False, False),
    (1, True, True, False, False),
    (8, True, True, False, True),
    (1, False, False, True, True),
    (8, True, False, True, False),
    (8, False, True, True, True),
    (1, True, True, True, False),
    (80, False, False, False, False),
    (80, True, False, True, True),
]


@pytest.mark.parametrize("K,logits,boards_only,hist,compact", CASES)
def test_flag_aware_stand_in_gives_the_rate_0_search_bit_for_bit(gpu, M, K, logits, boards_only, hist, compact):
    """Rates 0.5 and 1 against the search in which set_leaf_mirror was never called: moves, n, W bits, p bits, sum_n and
    the sims / expansions / terminal_sims / repetition_sims counters.

    Which attach code a case reaches: K = 1 and K = 8 (at most 64 slots per game, paths of at most 64 levels: 64
    simulations cannot go deeper) attach through the prefetched chain leaf_pre_a / leaf_pre_b / attach_and_backup; K = 80
    (more than 64 slots per game) takes k_sim's slot-by-slot form, attach_policy.  Both read a mirrored leaf's row through
    M, for the labels of `lane` and of `lane + 64` (the root of game 3 has more than 64 moves)."""
    kw = dict(logits=logits, boards_only=boards_only, hist=hist, compact=compact)
    base = drive(gpu, M, K, None, **kw)
    assert int(base["st"]["counts"][WIDE_G]) > 64
    assert base["ctr"]["expansions"] > G * SIMS // 2
    for rate in (0.5, 1.0):
        got = drive(gpu, M, K, rate, **kw)
        assert_same_search(base, got, f"rate {rate}")
        fl = np.array([f for _, f in got["flags"]])
        assert len(fl) == got["ctr"]["expansions"]
        assert fl.all() if rate == 1.0 else (0 < fl.sum() < len(fl))
        wide_root = [f for slot, f in got["flags"] if slot // got["K"] == WIDE_G][0]
        assert rate < 1.0 or wide_root == 1
    assert not any(f for _, f in base["flags"])


def test_the_mirror_is_seen_by_a_stand_in_that_ignores_the_flags(gpu, M):
    """The same asymmetric stub without the flags: the search changes -- so test 1 passes because both sides of the
    mirror are undone, not because nothing is mirrored."""
    base = drive(gpu, M, 8, None)
    plain = stub_eval(gpu, dict(kind="hash", salt=3))
    got = drive(gpu, M, 8, 1.0, evaluate=lambda planes, flags: plain(planes))
    assert any((base["st"]["n"][g] != got["st"]["n"][g]).any() for g in range(G))


# ---- 2. the same in self-play mode --------------------------------------------------------------------------------------------
def _entry_key(e):
    return (e.ply, e.moves.tolist(), e.n.tolist(), e.banned.tolist(), e.sum_n, e.resign, e.fast, e.pruned, e.raw_total)


def _selfplay(gpu, M, K, rate, rounds, seed=31):
    pc = play_config(simulation_num_per_move=16, search_threads=K, tau_decay_rate=0.9, max_game_length=8,
                     enable_resign_rate=0.5, resign_threshold=-0.4, min_resign_turn=4)
    t = gpu.torch
    s = gpu.S.Search(pc, G, seed=seed)
    s.record_visits(True)
    if rate is not None:
        s.set_leaf_mirror(rate, flags=True)
    ev = flag_aware(stub_eval(gpu, dict(kind="hash", salt=5)), M)
    s.start_selfplay(seed=seed, first_game_id=0)
    recs, mirrored, written = [], 0, 0
    for r in range(rounds):
        s.round()
        fl = s.mirrored if s.mirrored is not None else t.zeros(s.slots, dtype=t.uint8, device="cuda")
        p, v = ev(s.planes, fl)         # (a slot without a new leaf keeps its old planes and its old flag: a consistent pair)
        s.policy.copy_(p)
        s.value.copy_(v)
        if r % 16 == 15 or r == rounds - 1:
            _, rows = s.leaf_rows()
            mirrored += int(fl[rows].sum())
            written += rows.numel()
            for g in s.drain_records(with_visits=True):
                recs.append((g["game_id"], g["turns"], g["value"], g["store"], g["resigned"], g["moves"].tolist(), g["fast"],
                             [_entry_key(e) for e in g["visits"]]))
    ctr = s.counters()
    s.close()
    assert ctr["visits_dropped"] == 0
    return sorted(recs), ctr, mirrored, written


@pytest.mark.parametrize("K", [1, 8])
def test_selfplay_records_entries_and_counters_are_those_of_rate_0(gpu, M, K):
    rounds = 400 if K == 1 else 120
    base, c0, m0, _ = _selfplay(gpu, M, K, None, rounds)
    assert len(base) >= G and m0 == 0 and sum(len(r[7]) for r in base) > len(base)
    for rate in (0.5, 1.0):
        recs, c, m, n = _selfplay(gpu, M, K, rate, rounds)
        assert recs == base, rate
        assert c == c0, rate
        assert m == n if rate == 1.0 else 0 < m < n


# ---- 3. an exactly equivariant network needs no flags ----------------------------------------------------------------------
def test_equivariant_network_without_flags_searches_as_at_rate_0(gpu, M):
    """policy[a] = h(x)[a] + h(Mx)[M(a)], value = 0.5 (v(x) + v(Mx)): float addition commutes, so the network's answer for
    Mx read through M is its answer for x to the last bit."""
    h = stub_eval(gpu, dict(kind="hash", salt=11))

    def net(planes, flags):
        p0, v0 = h(planes)
        p1, v1 = h(planes.flip(-1))
        return p0 + p1[:, M], 0.5 * (v0 + v1)
    for K in (1, 8):
        base = drive(gpu, M, K, None, evaluate=net)
        got = drive(gpu, M, K, 0.5, evaluate=net, flags=False)
        assert_same_search(base, got, f"K {K}")
        assert int(base["st"]["counts"][WIDE_G]) > 64


# ---- 4. the coin ---------------------------------------------------------------------------------------------------------------
def test_the_coin(gpu, M):
    kw = dict(spec=dict(kind="hash", salt=17), sims=160)
    never = drive(gpu, M, 8, None, **kw)
    ones = drive(gpu, M, 8, 1.0, **kw)
    assert ones["flags"] and all(f == 1 for _, f in ones["flags"])

    # back to 0: every flag 0, and the run is the one in which the setter was never called
    zero = drive(gpu, M, 8, (1.0, 0.0), **kw)
    assert zero["flags"] and not any(f for _, f in zero["flags"])
    assert_same_search(never, zero, "rate 0")
    assert [slot for slot, _ in zero["flags"]] == [slot for slot, _ in never["flags"]]

    # a fair coin: the share over N leaves within five standard deviations, both kinds in every game with 64 leaves
    P = 0.5
    half = drive(gpu, M, 8, P, **kw)
    fl = np.array([f for _, f in half["flags"]], dtype=np.int64)
    game = np.array([slot // 8 for slot, _ in half["flags"]])
    N, k = len(fl), int(fl.sum())
    assert N >= 4000 and N == half["ctr"]["expansions"]
    assert abs(k / N - P) <= 5.0 * math.sqrt(P * (1 - P) / N), (k, N)
    big = [g for g in range(G) if (game == g).sum() >= 64]
    assert len(big) >= G // 2
    for g in big:
        assert 0 < fl[game == g].sum() < (game == g).sum(), g

    # the flags are a function of the seed
    again = drive(gpu, M, 8, P, **kw)
    other = drive(gpu, M, 8, P, seed=8, **kw)
    assert again["flags"] == half["flags"]
    assert [f for _, f in other["flags"]] != [f for _, f in half["flags"]]
    assert_same_search(never, other, "another seed")        # (the search itself does not depend on the coin)


# ---- 5. arguments ----------------------------------------------------------------------------------------------------------------
def test_bad_rates_are_refused_and_leave_the_rate(gpu, M):
    pc = play_config(simulation_num_per_move=SIMS, search_threads=8)
    s = gpu.S.Search(pc, G, seed=7)
    s.set_leaf_mirror(1.0, flags=True)
    for bad in (-0.1, 1.5, float("nan")):
        rc = s.L.cz_search_set_leaf_mirror(s.h, bad, None, s._stream())
        assert rc == ERR_ARG, bad
        with pytest.raises(gpu.N.NativeError):
            s.set_leaf_mirror(bad)
        assert s.leaf_mirror == 1.0
    assert s.L.cz_search_set_leaf_mirror(None, 0.5, None, s._stream()) == ERR_ARG
    s.set_roots(boards_tensor(gpu, STATES))
    s.round()
    _, rows = s.leaf_rows()
    assert rows.numel() >= G - 1 and bool(s.mirrored[rows].all())        # rate 1 and the flag array are still in force
    s.close()


# ---- 6. the engine ---------------------------------------------------------------------------------------------------------------
def _engine(leaf_mirror, rounds=80, **kw):
    import torch as t
    from cchess_alphazero.config import Config
    from cchess_alphazero.engine import SelfPlayEngine
    cfg = Config("mini")
    cfg.model.cnn_filter_num, cfg.model.res_layer_num = 128, 2
    cfg.play.simulation_num_per_move, cfg.play.search_threads, cfg.play.noise_eps = 8, 8, 0.0
    cfg.play.max_game_length = 8
    if leaf_mirror is not None:
        kw["leaf_mirror"] = leaf_mirror
    eng = SelfPlayEngine(cfg, G, dtype=t.float32, seed=11, **kw)
    assert eng.compact and eng.leaf_mirror == (leaf_mirror or 0.0) == eng.search.leaf_mirror
    eng.start()
    games, before = [], 0
    for r in range(rounds):
        eng.step()
        now = eng.counters()["expansions"]
        assert int(eng.search.q_count.item()) == now - before      # every new leaf is in the queue, mirrored or not
        before = now
        if r % 16 == 15:                                           # (before the record ring can fill)
            games += eng.drain()
    games += eng.drain()
    assert eng.counters()["ring_dropped"] == 0
    eng.close()
    return games


def test_engine_with_a_leaf_mirror_plays_legal_games_on_the_mini_network(gpu):
    games = _engine(0.5)
    assert len(games) >= G
    for g in games:
        state = g["data"][0]
        assert state == xo.INIT_STATE and len(g["data"]) - 1 == g["turns"]
        for i, item in enumerate(g["data"][1:]):
            assert item[0] in xo.get_legal_moves(state), (g["game_id"], i)
            state = xo.step(state, item[0])


def test_engine_at_rate_0_is_the_engine_without_the_argument(gpu):
    key = lambda games: sorted((g["game_id"], g["turns"], g["value"], g["store"], g["resigned"], json.dumps(g["data"]))
                               for g in games)
    a, b = _engine(None), _engine(0.0)
    assert len(a) >= G and key(a) == key(b)
