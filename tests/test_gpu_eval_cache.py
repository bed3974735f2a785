"""-m gpu: the cross-game evaluation cache of the search (cz_search_set_eval_cache; run.py self --eval-cache LOG2).

A table of network results keyed by position and leaf-mirror bit, shared by all games of a search object and kept across
reset_trees() / set_roots() / new self-play games.  A new leaf the table holds takes no queue row, its priors and value
come from the entry, and it is attached one round later at its place in simulation order -- so a search with the cache on
must produce THE SAME BITS as one with it off.  That equality is what this file checks, on the helpers of
tests/test_gpu_leaf_mirror.py (its 32 STATES, its assert_same_search: moves, n, the bits of w and p, sum_n and the
counters sims / expansions / terminal_sims / repetition_sims) under the asymmetric hash stub, driven round by round so
that the rows the network is asked about can be counted.

Shapes: G = 32 games, 64 simulations.  Every case calls set_eval_cache, which the library before this option lacks."""
import numpy as np
import pytest

from test_gpu_book import _engine_cfg
from test_gpu_leaf_mirror import CTRS, G, SIMS, STATES, assert_same_search
from test_gpu_search import boards_tensor, gpu, play_config, stub_eval  # noqa: F401

pytestmark = pytest.mark.gpu
ERR_ARG = -1                                                # include/czero.h CZ_ERR_ARG
STRIDE = 576                                                # CZ_EVAL_CACHE_STRIDE
SPEC = dict(kind="hash", salt=3)
INFO = ("probes", "hits", "stores")


def phases(gpu, K, cache, n_phases=2, logits=False, boards_only=False, compact=False, mirror=None, gumbel=0, full=False,
           clear_before=(), seed=7):
    """n_phases searches of STATES on ONE search object, driven round by round through round() / leaf_rows() (or the compact
    queue) with the plain hash stub, which is told nothing about mirrored rows.  Between two phases: reset_trees() and
    set_roots() with the same states -- nothing else, so what the table holds survives; `clear_before`: the phases that
    start with clear_eval_cache().  cache: log2 of the table's entries, None = set_eval_cache is never called.
    Returns one dict per phase: st = root_stats, ctr = the phase's share of the counters, rows = queue rows evaluated,
    probes / hits / stores = the phase's share of eval_cache_info(), v = node_net_value() of the roots (Gumbel)."""
    t = gpu.torch
    pc = play_config(simulation_num_per_move=SIMS, search_threads=K)
    s = gpu.S.Search(pc, G, seed=seed)
    if logits:
        s.policy_logits(True)
    if boards_only:
        s.leaf_masks(True)
        s.leaf_planes(False)
    if mirror is not None:
        s.set_leaf_mirror(mirror)
    if gumbel:
        s.set_gumbel(gumbel)
        if full:
            s.set_gumbel_full(True)
    if cache is not None:
        s.set_eval_cache(cache)
        assert s.eval_cache_info() == dict(entries=1 << cache, probes=0, hits=0, stores=0)
    ev = stub_eval(gpu, SPEC)
    out = []
    for ph in range(n_phases):
        if ph:
            s.reset_trees()
        if ph in clear_before:
            s.clear_eval_cache()
        ctr0, info0 = s.counters(), s.eval_cache_info()
        s.set_roots(boards_tensor(gpu, STATES))
        n_rows = 0
        for _ in range(10000):
            s.round(compact=compact)
            pending, rows = s.leaf_rows()
            if pending == 0:
                break
            n = rows.numel()
            if compact:
                n = int(s.q_count.item())
                assert n == rows.numel()                            # both lists hold the evaluated leaves, no cached one
                rows = s.q_rows[:n].long()
            if not n:
                continue
            n_rows += n
            p, v = ev(s.queue_planes(rows=rows))
            if logits:
                p = t.log(p.double()).float()
            if compact:
                s.policy[:n] = p
                s.value[:n] = v
            else:
                s.policy.index_copy_(0, rows, p)
                s.value.index_copy_(0, rows, v)
        else:
            raise AssertionError("the search did not finish")
        ctr1, info1 = s.counters(), s.eval_cache_info()
        d = dict(st=s.root_stats(), ctr={k: ctr1[k] - ctr0[k] for k in CTRS}, rows=n_rows, entries=info1["entries"])
        d.update({k: info1[k] - info0[k] for k in INFO})
        if gumbel:
            d["v"] = s.node_net_value()
        out.append(d)
    s.close()
    return out


def check_phase(ph, off, what):
    assert_same_search(off, ph, what)
    # every expansion either took a queue row or was answered by the table
    assert ph["rows"] + ph["hits"] == ph["ctr"]["expansions"], (what, ph["rows"], ph["hits"], ph["ctr"]["expansions"])
    assert ph["hits"] <= ph["probes"] <= ph["ctr"]["expansions"], what


# ---- 1. two phases at K = 1: the second one asks the network almost nothing ----------------------------------------------------
# (policy_logits, boards only, compact queue)
CASES_K1 = [(False, False, False), (True, False, True), (False, True, True), (True, True, False)]


@pytest.mark.parametrize("logits,boards_only,compact", CASES_K1)
def test_k1_the_second_search_is_answered_by_the_table_and_is_the_same_search(gpu, logits, boards_only, compact):
    """Phase A searches STATES, then reset_trees() + set_roots() with the same states and phase B, then clear_eval_cache()
    and phase C.  A, B, C and a search that never switches the cache on are the same search; in each phase rows + hits ==
    expansions.

    With K = 1 nothing parks, so every expansion is made in the selection launch and probes.  Phase B asks for the
    positions phase A asked for; what it still evaluates is what the direct-mapped table lost: n positions in 2^20 slots
    lose about n^2 / 2^21 entries to shared slots, about 2 for the ~2100 positions here.  The bound is 2 % of phase A's
    rows: a factor of 20 above that, and far below a cache that does not work (100 %).  After the clear phase C evaluates
    exactly what phase A did."""
    kw = dict(logits=logits, boards_only=boards_only, compact=compact)
    off = phases(gpu, 1, None, n_phases=1, **kw)[0]
    assert off["rows"] == off["ctr"]["expansions"] > G * SIMS // 2 and off["entries"] == 0
    a, b, c = phases(gpu, 1, 20, n_phases=3, clear_before=(2,), **kw)
    for name, ph in (("A", a), ("B", b), ("C", c)):
        check_phase(ph, off, f"phase {name}")
        assert ph["probes"] == ph["ctr"]["expansions"], name            # K = 1: every expansion probes
    print(f"rows evaluated: off {off['rows']}, A {a['rows']} (hits {a['hits']}), B {b['rows']} (hits {b['hits']}), "
          f"C {c['rows']}; stores A {a['stores']} B {b['stores']}")
    assert b["rows"] <= 0.02 * a["rows"], (a["rows"], b["rows"])
    assert c["rows"] == a["rows"] and c["hits"] == a["hits"]


# ---- 2. K = 8: parked simulations, leaves made in the backup launch ---------------------------------------------------------------
@pytest.mark.parametrize("logits,boards_only,compact", [(False, False, False), (True, True, True)])
def test_k8_two_phases_are_the_same_search(gpu, logits, boards_only, compact):
    """K = 8: simulations park on waiting leaves -- on cached ones exactly as on evaluated ones -- and a resumed simulation
    makes its leaf in the backup launch, which does not probe: no share of hits is asserted, only that there are some."""
    kw = dict(logits=logits, boards_only=boards_only, compact=compact)
    off = phases(gpu, 8, None, n_phases=1, **kw)[0]
    a, b = phases(gpu, 8, 20, **kw)
    check_phase(a, off, "phase A")
    check_phase(b, off, "phase B")
    print(f"K = 8: rows A {a['rows']} B {b['rows']}, hits A {a['hits']} B {b['hits']}, probes B {b['probes']}")
    assert b["hits"] > 0


def test_k80_the_slot_by_slot_attach_takes_cached_slots_too(gpu):
    """More than 64 slots per game: k_sim's slot-by-slot attach (attach_policy), the other path a cached slot joins."""
    off = phases(gpu, 80, None, n_phases=1)[0]
    a, b = phases(gpu, 80, 20)
    check_phase(a, off, "phase A")
    check_phase(b, off, "phase B")
    assert b["hits"] > 0


# ---- 3. a table smaller than the search ---------------------------------------------------------------------------------------
def test_a_table_of_1024_entries_is_overwritten_all_the_time_and_changes_nothing(gpu):
    """2^10 entries for some 2000 positions per phase: entries are overwritten all the time and writers meet in one
    launch (the loser drops its store)."""
    off = phases(gpu, 8, None, n_phases=1)[0]
    a, b = phases(gpu, 8, 10)
    check_phase(a, off, "phase A")
    check_phase(b, off, "phase B")
    assert a["entries"] == 1024
    print(f"2^10 entries: stores {a['stores']} + {b['stores']}, hits {a['hits']} + {b['hits']}")
    assert a["stores"] + b["stores"] > a["entries"]
    assert a["stores"] <= a["rows"] and b["stores"] <= b["rows"]        # (at most one store per evaluated row)


# ---- 4. the mirror bit is part of the key -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8])
def test_leaf_mirror_a_row_is_only_reused_under_the_coin_it_was_evaluated_under(gpu, K):
    """Rate 0.5 with the plain hash stub, which is not mirror-equivariant and is not told the flags: the row of a position
    and the row of its mirror image differ in every entry.  The same search as cache-off at rate 0.5 -- a key without the
    mirror bit would hand a leaf the other frame's row."""
    off = phases(gpu, K, None, n_phases=1, mirror=0.5)[0]
    plain = phases(gpu, K, None, n_phases=1)[0]
    assert any((off["st"]["n"][g] != plain["st"]["n"][g]).any() for g in range(G))     # (the mirror is seen by this stub)
    a, b = phases(gpu, K, 20, mirror=0.5)
    check_phase(a, off, "phase A")
    check_phase(b, off, "phase B")
    assert b["hits"] > 0


# ---- 5. Gumbel: the net value of a cached attach ------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True])
def test_gumbel_the_cached_attach_keeps_the_network_value(gpu, full):
    """set_gumbel(16), with and without set_gumbel_full: every attach keeps the leaf's network value in the node (the full
    search selects with it below the root), a cached attach from the entry.  Same search, same node_net_value() of the
    roots -- which phase B takes from the table."""
    off = phases(gpu, 8, None, n_phases=1, gumbel=16, full=full)[0]
    a, b = phases(gpu, 8, 20, gumbel=16, full=full)
    for name, ph in (("A", a), ("B", b)):
        check_phase(ph, off, f"phase {name}")
        assert ph["v"].view(np.uint32).tolist() == off["v"].view(np.uint32).tolist(), name
    fin = off["v"][np.isfinite(off["v"])]                               # (NaN: a root that is not searched, e.g. a finished position)
    assert len(fin) >= G - 2 and len(set(fin.tolist())) > G // 2
    assert b["hits"] > 0


# ---- 6. self-play through the engine ------------------------------------------------------------------------------------------
def _selfplay(gpu, eval_cache, rounds=None):
    """16 games x 16 simulations, K = 4, short games, through SelfPlayEngine on an evaluator callable.  rounds None: until
    every slot has finished three games.  Returns (drained games, rounds played, eval_cache_info)."""
    from cchess_alphazero.engine import SelfPlayEngine
    pc = play_config(simulation_num_per_move=16, search_threads=4, tau_decay_rate=0.9, max_game_length=8,
                     enable_resign_rate=0.5, resign_threshold=-0.4, min_resign_turn=4)
    eng = SelfPlayEngine(_engine_cfg(pc), 16, evaluator=stub_eval(gpu, dict(kind="hash", salt=31)), seed=31,
                         record_visits=True, eval_cache=eval_cache)
    assert eng.eval_cache == eval_cache == eng.search.eval_cache
    games, r = [], 0
    try:
        eng.start()
        while r < (rounds or 4000):
            eng.step()
            r += 1
            if r % 16 == 0:
                games += eng.drain()
                if rounds is None and int(eng.search.game_counters()[:, 10].min()) >= 3:    # column 10: games
                    break
        games += eng.drain()
        assert eng.counters()["ring_dropped"] == 0
        info = eng.search.eval_cache_info()
    finally:
        eng.close()
    return games, r, info


def test_selfplay_records_are_equal_item_for_item(gpu):
    """Cache 2^16 against off, same seed, enough rounds for every slot to finish at least three games: the drained records
    are equal item for item (moves, values, pi), and later games, which replay the opening, hit the table."""
    from cchess_alphazero._native_search import COUNTER_NAMES
    assert COUNTER_NAMES[10] == "games"
    on, rounds, info = _selfplay(gpu, 16)
    assert rounds < 4000 and len(on) >= 48
    off, _, info_off = _selfplay(gpu, 0, rounds=rounds)
    assert info_off == dict(entries=0, probes=0, hits=0, stores=0)
    # (games that end in the same round reach the record ring in the order their waves get there: compared by game id)
    on, off = sorted(on, key=lambda g: g["game_id"]), sorted(off, key=lambda g: g["game_id"])
    assert [g["game_id"] for g in on] == [g["game_id"] for g in off]
    assert len({g["game_id"] for g in on}) == len(on)
    for a, b in zip(on, off):
        assert a["data"] == b["data"], a["game_id"]
        assert {k: v for k, v in a.items() if k not in ("data", "visits")} == \
               {k: v for k, v in b.items() if k not in ("data", "visits")}
    assert any(len(item) == 3 for g in on for item in g["data"][1:])     # (the items carry pi)
    print(f"self-play: {len(on)} games in {rounds} rounds, cache {info}")
    assert info["entries"] == 1 << 16 and info["hits"] > 0 and info["stores"] > 0


# ---- 7. refusals and bookkeeping ----------------------------------------------------------------------------------------------
def test_refusals_and_bookkeeping(gpu):
    pc = play_config(simulation_num_per_move=SIMS, search_threads=8)
    s = gpu.S.Search(pc, G, seed=7)
    st = s._stream()
    assert s.eval_cache_info() == dict(entries=0, probes=0, hits=0, stores=0)     # the setter was never called
    base = s.device_bytes()
    for bad in (9, 25, -1, 1):
        with pytest.raises(ValueError, match="10 <= LOG2 <= 24"):
            s.set_eval_cache(bad)
        assert s.L.cz_search_set_eval_cache(s.h, bad, st) == ERR_ARG                 # the library itself, with a message
        assert "10 .. 24" in s.L.cz_last_error().decode()
        assert s.device_bytes() == base and s.eval_cache == 0
    assert s.L.cz_search_set_eval_cache(None, 16, st) == ERR_ARG
    for log2 in (10, 16):
        s.set_eval_cache(log2)
        assert s.device_bytes() == base + (STRIDE << log2)
        assert s.memory_info()["eval_cache_bytes"] == STRIDE << log2
        assert s.eval_cache_info()["entries"] == 1 << log2
    # a search fills it; a clear zeroes the numbers; switching it off gives the memory back
    s.set_roots(boards_tensor(gpu, STATES))
    s.run_until_idle(stub_eval(gpu, SPEC))
    info = s.eval_cache_info()
    assert info["stores"] > 0 and info["probes"] > 0
    s.clear_eval_cache()
    assert s.eval_cache_info() == dict(entries=1 << 16, probes=0, hits=0, stores=0)
    s.set_eval_cache(0)
    assert s.device_bytes() == base and s.memory_info()["eval_cache_bytes"] == 0
    assert s.eval_cache_info() == dict(entries=0, probes=0, hits=0, stores=0)
    s.clear_eval_cache()                                                 # (nothing to do, no error)
    s.close()
    # 28 input planes: the network input is not a function of the position
    h = gpu.S.Search(pc, 4, seed=7, use_history=True)
    with pytest.raises(gpu.N.NativeError, match="28-plane"):
        h.set_eval_cache(16)
    assert h.eval_cache == 0 and h.eval_cache_info()["entries"] == 0
    h.set_eval_cache(0)                                                  # (off is not refused)
    h.close()
    from cchess_alphazero.engine import SelfPlayEngine
    with pytest.raises(ValueError, match="use_history"):
        SelfPlayEngine(_engine_cfg(pc), 2, evaluator=stub_eval(gpu, SPEC), use_history=True, eval_cache=16)


# ---- 8. a network change empties the table ------------------------------------------------------------------------------------
def test_set_network_empties_the_table_and_the_graph_replays(gpu):
    """SelfPlayEngine on a real 1-block 128-filter network, its own compact queue with raw logits: a few rounds fill the
    table; set_network with other weights passes through _install, which empties it -- stores == 0 before the next round;
    a graph captured then, fill kernel included, replays and the table fills from the new network."""
    import torch as t
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.config import Config
    from cchess_alphazero.engine import SelfPlayEngine
    cfg = Config("mini")
    cfg.model.cnn_filter_num, cfg.model.res_layer_num = 128, 1
    cfg.play.simulation_num_per_move, cfg.play.search_threads, cfg.play.noise_eps = 8, 8, 0.0
    cfg.play.max_game_length = 8
    t.manual_seed(0)
    eng = SelfPlayEngine(cfg, 16, net=CChessNet.from_model_config(cfg.model), dtype=t.float32, seed=11, eval_cache=16)
    try:
        assert eng.compact and eng.search.eval_cache == 16
        eng.start()
        for _ in range(12):
            eng.step()
        first = eng.search.eval_cache_info()
        assert first["entries"] == 1 << 16 and first["stores"] > 0
        t.manual_seed(1)
        eng.set_network(CChessNet.from_model_config(cfg.model))
        cleared = eng.search.eval_cache_info()                           # before the next round
        assert cleared == dict(entries=1 << 16, probes=0, hits=0, stores=0)
        eng.capture_graph()
        assert eng._graph is not None
        for _ in range(12):
            eng.step()
        t.cuda.synchronize()
        again = eng.search.eval_cache_info()
        assert again["stores"] > 0 and again["probes"] > 0
        c = eng.counters()
        assert c["overflow_sims"] == 0 and c["expansions"] > 0
    finally:
        eng.close()
