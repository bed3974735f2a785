"""The peaked exact stub and the oracle's run-time limits (max_depth, max_nodes: oracle/xq_mcts.h), CPU only.  They are
what tests/test_gpu_search_limits.py compares the engine's long paths and counted cut-offs with."""
import numpy as np
import pytest

import stub_net
from oracle import xq_oracle as xo
from search_limits import (LONG_CASES, MID, PEAKED, oracle_stub, sims_end_one_way, tree_defects, walk_oracle_tree,
                           zero_prior_node)


def _search(state=MID, spec=PEAKED, **cfg):
    pl = xo.Player(xo.play_cfg(**cfg), oracle_stub(spec))
    pl.search(state)
    return pl


@pytest.mark.parametrize("in_planes", [14, 28])
def test_peaked_stub_numpy_and_torch_are_bit_identical(in_planes):
    import torch
    rng = np.random.default_rng(in_planes)
    planes = (rng.random((64, in_planes, 10, 9)) < 0.03).astype(np.float32)
    planes[0] = 0
    for salt, S, value in [(5, 8, 0.0), (6, 8, 0.25), (1, 0, -1.0), (2, 3, 0.0), (3, 11, 0.0)]:
        p, v = stub_net.peaked_stub_numpy(planes, salt, S, value)
        pt, vt = stub_net.peaked_stub_torch(torch.from_numpy(planes), salt, S, value)
        assert p.dtype == np.float32 and pt.dtype == torch.float32 and p.shape == (64, stub_net.N_LABELS)
        assert np.array_equal(pt.numpy().view(np.uint32), p.view(np.uint32)), (salt, S)
        assert np.array_equal(vt.numpy().view(np.uint32), v.view(np.uint32)) and (v == np.float32(value)).all()
        assert ((p == 0) | (p >= stub_net.PEAK_FLOOR)).all() and (p <= 1).all()
        if S == 0:      # the hash stub's own policy with its entries below the floor zeroed
            h, _ = stub_net.hash_stub_numpy(planes, salt)
            assert np.array_equal(p, np.where(h < stub_net.PEAK_FLOOR, np.float32(0), h))
        if S == 8:      # x^2048 >= 2^-60 needs x >= 2^(-60/2048) = 0.98: 42 +- 6.4 of a row's 2086 entries survive
            assert ((p != 0).sum(axis=1) > 0).all() and (p != 0).sum(axis=1).max() <= 100
    # the spec form the searches use
    p, v = stub_net.stub_numpy(PEAKED)(planes)
    q, _ = stub_net.peaked_stub_numpy(planes, 5, 8, 0.0)
    assert np.array_equal(p, q) and (v == 0).all()


@pytest.mark.parametrize("K,sims,state,in_planes", LONG_CASES)
def test_peaked_stub_drives_the_oracle_past_64_plies(K, sims, state, in_planes):
    pl = _search(state, simulation_num_per_move=sims, search_threads=K, use_history=int(in_planes == 28))
    c = pl.counters()
    assert c["max_depth"] > 64 and c["depth_overflow"] == 0 and c["overflow_sims"] == 0, c
    assert c["repetition_sims"] > 0 and c["sims"] == sims and sims_end_one_way(c), c
    count, bad = tree_defects(pl, state)
    assert count > 100 and not bad, bad[:3]
    pl.close()


def test_a_row_without_any_prior_is_searched():
    """spread_priors' all_p == 0 -> 1: under the peaked stub some positions give every legal move the prior 0."""
    pl = _search(simulation_num_per_move=400, search_threads=1)
    found = zero_prior_node(pl, MID)
    assert found is not None
    path, st = found
    assert len(path) >= 1 and not st["p"].any() and st["n"].sum() == st["sum_n"] - 1 > 0
    # every edge scores q + 0: `>=` keeps the last of equals, so the first visit went to the last move
    assert st["n"][-1] > 0
    pl.close()


def test_depth_limit_of_one():
    n_root = len(xo.get_legal_moves(MID))
    for K in (1, 8):
        pl = _search(simulation_num_per_move=300, search_threads=K, max_depth=1)
        c, st = pl.counters(), pl.node_stats(MID)
        assert c["max_depth"] == 1 and c["expansions"] <= 1 + n_root and c["depth_overflow"] > 0, c
        assert c["sims"] == 300 and sims_end_one_way(c), c
        assert st["sum_n"] == 300 and st["n"].sum() == st["sum_n"] - 1 and (st["n"] >= 0).all()
        assert pl.tree_size() == c["expansions"]
        count, bad = tree_defects(pl, MID)
        assert count == c["expansions"] and not bad, bad[:3]
        pl.close()


END = '3s5/4m4/9/9/4p4/2R6/9/4C4/4M4/3MS4'


@pytest.mark.parametrize("K", [1, 8])
def test_depth_limit_cut_returns_every_virtual_loss_and_the_old_order_does_not(K):
    """max_depth = 7.  The cut before the selection (the engine's order) leaves every node consistent.  The cut after
    sum_n += 1 and the virtual loss of the selected edge -- where this oracle had its compile-time cut -- backs up only
    the path, so that edge keeps its virtual loss: sum n_j == sum_n - 1 fails at the nodes where it fired.  That identity
    is what the engine's heap-exhaustion test relies on.  The root's own statistics differ between the two orders only
    where a node that was cut at depth 7 is also reached on a shorter path and selected from with the stale edge in it:
    an endgame with few pieces (many transpositions) and the hash stub's non-zero values show it."""
    spec = dict(kind="hash", salt=5)
    kw = dict(simulation_num_per_move=1200, search_threads=K, max_depth=7)
    new, old = _search(END, spec, **kw), _search(END, spec, cut_after_select=1, **kw)
    cn, co = new.counters(), old.counters()
    assert cn["depth_overflow"] > 0 and co["depth_overflow"] > 0 and cn["max_depth"] == co["max_depth"] == 7
    assert sims_end_one_way(cn) and cn["sims"] == 1200
    count, bad = tree_defects(new, END)
    assert count > 50 and not bad, bad[:3]
    _, bad_old = tree_defects(old, END)
    assert bad_old and all(len(path) <= 7 and "sum n_j" in what for path, what in bad_old), bad_old[:3]
    # each lost virtual loss leaves v - 1 = 2 visits too many: together, exactly the cuts
    excess = 0
    for path, _, st in walk_oracle_tree(old, END):
        excess += int(st["n"].sum()) - (st["sum_n"] - 1)
    assert excess == 2 * co["depth_overflow"]
    a, b = new.node_stats(END), old.node_stats(END)
    assert a["sum_n"] == b["sum_n"] == 1200 and a["n"].sum() == b["n"].sum() == 1199
    assert not (np.array_equal(a["n"], b["n"]) and np.array_equal(a["w"], b["w"]))
    new.close()
    old.close()


def test_depth_limit_beyond_the_deepest_path_changes_nothing():
    ref = _search(simulation_num_per_move=400, search_threads=1)
    deepest = ref.counters()["max_depth"]
    lim = _search(simulation_num_per_move=400, search_threads=1, max_depth=deepest + 1)
    a, b = ref.node_stats(MID), lim.node_stats(MID)
    assert np.array_equal(a["n"], b["n"]) and np.array_equal(a["w"], b["w"]) and lim.counters() == ref.counters()
    cut = _search(simulation_num_per_move=400, search_threads=1, max_depth=deepest - 1)
    assert cut.counters()["depth_overflow"] > 0 and cut.counters()["max_depth"] == deepest - 1
    for p in (ref, lim, cut):
        p.close()


@pytest.mark.parametrize("K,spec", [(1, PEAKED), (8, PEAKED), (8, dict(kind="hash", salt=5))])
def test_node_limit(K, spec):
    pl = _search(spec=spec, simulation_num_per_move=500, search_threads=K, max_nodes=200)
    c = pl.counters()
    assert c["expansions"] == 200 == pl.tree_size() and c["overflow_sims"] > 0 and c["depth_overflow"] == 0, c
    assert c["sims"] == 500 and sims_end_one_way(c), c
    count, bad = tree_defects(pl, MID)
    assert count > 50 and not bad, bad[:3]
    st = pl.node_stats(MID)
    assert st["sum_n"] == 500 and st["n"].sum() == 499
    pl.close()


def test_node_limit_refuses_the_root():
    """A tree that is full before the search starts: every simulation is refused at the root, depth 0."""
    pl = xo.Player(xo.play_cfg(simulation_num_per_move=40, search_threads=4, max_nodes=30), oracle_stub(PEAKED))
    pl.search(MID)
    c0 = pl.counters()
    assert pl.tree_size() == 30 and c0["sims"] == 40 and c0["overflow_sims"] > 0
    other = xo.fliped_state(xo.step(MID, xo.get_legal_moves(MID)[0]))
    assert pl.node_stats(other) is None
    pl.search(other)
    c = pl.counters()
    assert pl.node_stats(other) is None and pl.tree_size() == 30
    assert c["overflow_sims"] == c0["overflow_sims"] + 40 and c["sum_depth"] == c0["sum_depth"]
    assert c["sims"] == 80 and sims_end_one_way(c), c
    pl.close()
