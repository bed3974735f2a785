"""-m gpu: the parts of the tree search (csrc/xq_search_sim.h, xq_search_tree.h) that the hash stub never reaches, against the oracle with the
same limits (oracle/xq_mcts.h max_depth / max_nodes), bit for bit like tests/test_gpu_search.py:
  1. paths longer than 64 plies: the second pass of every lane loop over a path (backup, find_in_path, load_path), the
     path rows [G][K][max_depth] and the LDS copy past index 64, history_board two plies up such a path;
  2. the depth limit (Search(max_depth=)): a simulation cut at an evaluated node backs up 0 and counts depth_overflow;
  3. a hash table that fills up inside one ply (set_sims beyond hash_cap): refused expansions count overflow_sims;
  4. a heap that runs out inside one ply: the oracle has no granules, so invariants instead of parity.
The peaked exact stub (tests/stub_net.py) is what makes the paths long.  Every host loop here is bounded."""
import numpy as np
import pytest

from oracle import xq_oracle as xo
from search_limits import (LONG_CASES, MID, PARITY_COUNTERS, PEAKED, node_defect, oracle_stub, sims_end_one_way,
                           walk_oracle_tree, zero_prior_node)
from test_gpu_search import END, assert_root_equal, boards_tensor, gpu, oracle_cfg, play_config, stub_eval   # noqa: F401

pytestmark = pytest.mark.gpu

NOMOVE = 0xFFFF
HASH5 = dict(kind="hash", salt=5)


def ocfg(pc, **kw):
    c = oracle_cfg(pc, use_history=kw.pop("use_history", 0))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def game_counters(gpu, s):
    rows = s.game_counters()
    return [{k: int(rows[g, i]) for i, k in enumerate(gpu.S.COUNTER_NAMES[:s.n_counters])} for g in range(s.G)]


def assert_counters_equal(gpu, s, players, what=""):
    """The counters the engine and the oracle both keep, game by game (both accumulate over the plies of a line)."""
    got = game_counters(gpu, s)
    for g, pl in enumerate(players):
        ref = pl.counters()
        for k in PARITY_COUNTERS:
            assert got[g][k] == ref[k], (what, g, k, got[g][k], ref[k])
    return got


def node_at(s, g, path):
    """Engine statistics of the node `path` (labels) below game g's root, in the oracle's node_stats form."""
    pa = np.full((s.G, max(1, len(path))), NOMOVE, dtype=np.uint16)
    pa[g, :len(path)] = path
    st = s.node_stats(pa)
    c = int(st["counts"][g])
    return dict(moves=st["moves"][g, :c], n=st["n"][g, :c], w=st["w"][g, :c], p=st["p"][g, :c], sum_n=int(st["sum_n"][g]))


def assert_node_equal(s, g, path, ref, what=""):
    pa = np.full((s.G, max(1, len(path))), NOMOVE, dtype=np.uint16)
    pa[g, :len(path)] = path
    assert_root_equal(s.node_stats(pa), g, ref, (what, len(path)))


def assert_tree_equal(s, g, pl, state, what=""):
    """Every node of the oracle's tree below `state`, edge for edge, in the engine's tree.  The root alone does not show
    a wrong update 70 plies down; these nodes do.  Returns (nodes compared, longest path to one)."""
    count = deepest = 0
    for path, _, ref in walk_oracle_tree(pl, state):
        assert_node_equal(s, g, list(path), ref, what)
        count, deepest = count + 1, max(deepest, len(path))
    return count, deepest


def assert_line_equal(s, g, pl, state, what="", max_len=128):
    """The same for the nodes of the oracle's most visited line only (until it ends or runs into itself).  Returns the
    number of nodes compared."""
    board, path, seen = xo.state_to_board(state), [], set()
    for _ in range(max_len):
        ref = pl.node_stats(board)
        if ref is None or len(ref["n"]) == 0 or board.tobytes() in seen:
            break
        seen.add(board.tobytes())
        assert_node_equal(s, g, path, ref, what)
        j = int(np.argmax(ref["n"]))
        if ref["n"][j] == 0:
            break
        path.append(int(ref["moves"][j]))
        board, _ = xo.step_board(board, path[-1])
        if xo.done_board(board)[0]:
            break
    return len(path)


# ---- 1. long paths -----------------------------------------------------------------------------------------------
def _hist_line(state, picks=(7, 1)):
    """(root, prev): the position two plies down a line from `state`, and `state` as the game position two plies before."""
    line = [state]
    for k in picks:
        line.append(xo.step(line[-1], xo.get_legal_moves(line[-1])[k]))
    return line[-1], line[0]


@pytest.mark.parametrize("K,sims,in_planes", sorted({(K, sims, pl) for K, sims, _, pl in LONG_CASES}))
def test_long_paths_match_oracle(gpu, K, sims, in_planes):
    """The searches that tests/search_limits.py lists (deepest path 68 .. 89 in the oracle), by their (K, simulations,
    planes) in one Search each.  With 28 planes a second game has a real game history (hist_kind 1: fresh simulations
    take the second block from g_prev_board, resumed ones from their own path), the first has none."""
    t = gpu.torch
    hist = in_planes == 28
    states = [st for k, n, st, pl in LONG_CASES if (k, n, pl) == (K, sims, in_planes)]
    hists = [None] * len(states)
    kw = {}
    if hist:
        root, prev = _hist_line(MID)
        states.append(root)
        hists.append([prev, None, None, None, root])                 # (action(hist=...): hist[-5] is all that is read)
        kw = dict(prev_boards=boards_tensor(gpu, [h[0] if h else s for s, h in zip(states, hists)]),
                  hist_kind=t.tensor([1 if h else 0 for h in hists], dtype=t.uint8, device="cuda"))
    pc = play_config(simulation_num_per_move=sims, search_threads=K)
    s = gpu.S.Search(pc, len(states), seed=7, use_history=hist)
    assert s.max_depth == 128
    s.set_roots(boards_tensor(gpu, states), **kw)
    s.run_until_idle(stub_eval(gpu, PEAKED), max_rounds=4 * sims)
    st = s.root_stats()
    players = []
    for g, state in enumerate(states):
        pl = xo.Player(ocfg(pc, use_history=int(hist)), oracle_stub(PEAKED))
        pl.set_history(hists[g])
        pl.search(state)
        players.append(pl)
        c = pl.counters()
        print(f"long path K={K} sims={sims} planes={in_planes} game {g}: deepest {c['max_depth']}, "
              f"repetitions {c['repetition_sims']}, terminals {c['terminal_sims']}, parked {c['parked']}")
        assert c["max_depth"] > 64 and c["depth_overflow"] == 0 and c["overflow_sims"] == 0, (g, c)
        assert_root_equal(st, g, pl.node_stats(state), f"game {g}")
        if K == 1:
            count, reach = assert_tree_equal(s, g, pl, state, f"game {g}")
            assert count == c["expansions"] and reach > 64
        else:
            assert_line_equal(s, g, pl, state, f"game {g}")
    got = assert_counters_equal(gpu, s, players)
    assert all(c["depth_overflow"] == 0 and c["overflow_sims"] == 0 and c["tree_resets"] == 0 for c in got)
    if not hist:
        # a node whose legal moves all got the prior 0 (all_p == 0 -> 1), found in the oracle's tree: the same in the engine
        found = zero_prior_node(players[0], states[0])
        assert found is not None
        path, ref = found
        assert not ref["p"].any() and ref["sum_n"] > 1
        assert_node_equal(s, 0, list(path), ref, "zero-prior node")
        assert not node_at(s, 0, list(path))["p"].any()
    for pl in players:
        pl.close()
    s.close()


def test_long_paths_over_three_plies_with_reuse(gpu):
    """Three plies of one line, the tree kept from ply to ply: long paths through nodes of earlier searches."""
    t = gpu.torch
    pc = play_config(simulation_num_per_move=600, search_threads=8)
    states = [MID, xo.fliped_state(MID)]
    G = len(states)
    s = gpu.S.Search(pc, G, seed=3)
    players = [xo.Player(ocfg(pc), oracle_stub(PEAKED)) for _ in range(G)]
    deepest = [0] * G
    for ply in range(3):
        s.set_roots(boards_tensor(gpu, states), turns=t.full((G,), ply, dtype=t.int32, device="cuda"))
        s.run_until_idle(stub_eval(gpu, PEAKED), max_rounds=2400)
        st = s.root_stats()
        act = s.choose(None)
        for g in range(G):
            before = players[g].counters()["sims"]
            a, _ = players[g].action(states[g], ply, None, False, 0.5)
            assert_root_equal(st, g, players[g].node_stats(states[g]), f"ply {ply} game {g}")
            assert xo.label_str(int(act[g])) == a
            if ply > 0:
                assert 0 < players[g].counters()["sims"] - before < 600          # the subtree was reused
            deepest[g] = assert_line_equal(s, g, players[g], states[g], f"ply {ply} game {g}")
            states[g] = xo.step(states[g], a)
        got = assert_counters_equal(gpu, s, players, f"ply {ply}")
    for g in range(G):
        c = players[g].counters()
        print(f"three plies game {g}: deepest {c['max_depth']}")
        assert c["max_depth"] > 64 and got[g]["depth_overflow"] == 0 and got[g]["tree_resets"] == 0, c
        players[g].close()
    s.close()


# ---- 2. the depth limit --------------------------------------------------------------------------------------------
LIMIT_STATES = [xo.INIT_STATE, MID, END, xo.fliped_state(MID), MID]      # (games 1 and 4: the same search, side by side)

# (D, K, stub, simulations): every pairing in which the oracle cuts at least one simulation.  The hash stub's paths end
# near depth 10 (none reaches 7 at K = 80), only the peaked stub's lines reach 40, at K = 8 only in a longer search, and
# K = 80 stays near depth 12 with either stub.
DEPTH_CASES = ([(D, K, spec, 480 if K == 80 else 300) for D in (1, 2, 7) for K in (1, 8, 80) for spec in (HASH5, PEAKED)
                if (D, K, spec["kind"]) != (7, 80, "hash")]
               + [(40, 1, PEAKED, 300), (40, 8, PEAKED, 1600)])


@pytest.mark.parametrize("D,K,spec,sims", DEPTH_CASES, ids=lambda v: v["kind"] if isinstance(v, dict) else str(v))
def test_depth_limit_matches_oracle(gpu, D, K, spec, sims):
    """Search(max_depth=D) against the oracle with the same D: five games in one search, so that the [K][D] path rows of
    neighbouring simulations and games adjoin -- a write at index D of a row lands in the next one."""
    pc = play_config(simulation_num_per_move=sims, search_threads=K)
    s = gpu.S.Search(pc, len(LIMIT_STATES), seed=7, max_depth=D)
    assert s.max_depth == D
    s.set_roots(boards_tensor(gpu, LIMIT_STATES))
    s.run_until_idle(stub_eval(gpu, spec), max_rounds=4 * sims)
    st = s.root_stats()
    players = []
    for g, state in enumerate(LIMIT_STATES):
        pl = xo.Player(ocfg(pc, max_depth=D), oracle_stub(spec))
        pl.search(state)
        players.append(pl)
        assert_root_equal(st, g, pl.node_stats(state), f"game {g}")
        assert_line_equal(s, g, pl, state, f"game {g}")
    got = assert_counters_equal(gpu, s, players)
    cuts = [pl.counters()["depth_overflow"] for pl in players]
    print(f"depth limit D={D} K={K} {spec['kind']}: depth_overflow per game {cuts}, "
          f"deepest {[pl.counters()['max_depth'] for pl in players]}")
    assert sum(cuts) > 0 and max(c["max_depth"] for c in got) == D
    for g, c in enumerate(got):
        assert c["overflow_sims"] == 0 and c["tree_resets"] == 0 and c["sims"] == sims and sims_end_one_way(c), (g, c)
        assert node_defect(dict(n=st["n"][g], w=st["w"][g], sum_n=int(st["sum_n"][g]))) is None
    for pl in players:
        pl.close()
    s.close()


def test_depth_limit_over_six_plies_with_reuse(gpu):
    t = gpu.torch
    D = 7
    pc = play_config(simulation_num_per_move=200, search_threads=8)
    states = [MID, END, xo.fliped_state(MID)]
    G = len(states)
    s = gpu.S.Search(pc, G, seed=3, max_depth=D)
    players = [xo.Player(ocfg(pc, max_depth=D), oracle_stub(PEAKED)) for _ in range(G)]
    for ply in range(6):
        s.set_roots(boards_tensor(gpu, states), turns=t.full((G,), ply, dtype=t.int32, device="cuda"))
        s.run_until_idle(stub_eval(gpu, PEAKED), max_rounds=800)
        st = s.root_stats()
        act = s.choose(None)
        for g in range(G):
            a, _ = players[g].action(states[g], ply, None, False, 0.5)
            assert_root_equal(st, g, players[g].node_stats(states[g]), f"ply {ply} game {g}")
            assert xo.label_str(int(act[g])) == a
            assert_line_equal(s, g, players[g], states[g], f"ply {ply} game {g}")
            states[g] = xo.step(states[g], a)
        got = assert_counters_equal(gpu, s, players, f"ply {ply}")
    print("six plies at D=7: depth_overflow per game", [c["depth_overflow"] for c in got])
    assert all(c["depth_overflow"] > 0 and c["max_depth"] == D and c["tree_resets"] == 0 for c in got), got
    for pl in players:
        pl.close()
    s.close()


# ---- 3. the hash table fills up inside a ply -----------------------------------------------------------------------
def _reservation_fails(pl, state, sims, hash_cap):
    """begin_search / reserve_ply restated for a game whose heap is not the limit: the ply's tasks (the reuse rule of
    player.py:153-158 without bans) cannot be reserved when node count + tasks + 1 exceeds 7/8 of the hash table."""
    root = pl.node_stats(state)
    done_n = root["sum_n"] if root is not None else 0
    if done_n == sims:
        done_n = 0
    tasks = max(0, sims - done_n)
    return tasks > 0 and pl.tree_size() + tasks + 1 > hash_cap * 7 // 8


@pytest.mark.parametrize("spec", [HASH5, PEAKED], ids=lambda v: v["kind"])
def test_hash_table_full_inside_a_ply(gpu, spec):
    """A search longer than the game's hash table (set_sims is documented not to refuse it).  reserve_ply's first test
    fails for such a ply whatever the tree holds (node count + tasks + 1 > 7/8 hash_cap), so begin_search drops the
    tree -- one tree_resets per game -- and its second reserve_ply fails the same test before it takes any chunk: the
    search runs on the chunks the game keeps.  hash_lookup probes at most hash_cap slots and reports slot -1 only when
    none of them is empty, so expansions are refused exactly while the tree holds hash_cap nodes: the oracle's
    max_nodes = hash_cap."""
    t = gpu.torch
    sims0, sims, K = 100, 700, 8
    pc0 = play_config(simulation_num_per_move=sims0, search_threads=K)
    pc = play_config(simulation_num_per_move=sims, search_threads=K)
    states = [xo.INIT_STATE, MID, END]
    G = len(states)
    s = gpu.S.Search(pc0, G, seed=1, max_nodes_per_game=300)
    assert s.hash_cap == 512 and sims + 1 > s.hash_cap * 7 // 8
    s.set_sims(sims)
    s.set_roots(boards_tensor(gpu, states))
    s.run_until_idle(stub_eval(gpu, spec), max_rounds=4 * sims)
    st = s.root_stats()
    m = s.memory_info()
    players = []
    for g, state in enumerate(states):
        pl = xo.Player(ocfg(pc, max_nodes=s.hash_cap), oracle_stub(spec))
        assert _reservation_fails(pl, state, sims, s.hash_cap)
        pl.search(state)
        players.append(pl)
        assert_root_equal(st, g, pl.node_stats(state), f"game {g}")
        assert_line_equal(s, g, pl, state, f"game {g}")
    got = assert_counters_equal(gpu, s, players)
    print(f"hash table full ({spec['kind']}): overflow_sims per game {[c['overflow_sims'] for c in got]}, "
          f"expansions {[c['expansions'] for c in got]}, memory {m}")
    # the hash table was the limit in at least one game, the heap in none: what the fullest game uses of its chunks leaves
    # room for any record (a node of MAXMOVES moves and its statistics: 4 + 48 + 128 granules of 16 bytes)
    assert max(c["overflow_sims"] for c in got) > 0 and m["nodes_max_game"] == s.hash_cap
    assert all(c["expansions"] == s.hash_cap for c in got if c["overflow_sims"] > 0)
    held = m["held_chunks"] // G
    assert m["held_chunks"] == G * held and m["tree_bytes_max_game"] + 180 * 16 < held << 20, m
    assert all(c["tree_resets"] == 1 and c["depth_overflow"] == 0 and sims_end_one_way(c) for c in got), got
    # two more plies at the length the search was created with, the oracle's trees kept.  A game whose new root has fewer
    # visits than that finds the table as the long search left it (512 nodes + tasks + 1 > 448): its tree is dropped
    # again and the ply is a search on an empty tree; a root that already has as many visits searches nothing; the ply
    # after reuses the subtree.  Exact parity again, the resets derived from reserve_ply's rule.
    act = s.choose(None)
    s.set_sims(sims0)
    resets = G
    for ply in (1, 2):
        states = [xo.step(state, xo.label_str(int(a))) for state, a in zip(states, act)]
        for g, pl in enumerate(players):
            pl.set_sims(sims0)
            if _reservation_fails(pl, states[g], sims0, s.hash_cap):
                pl.clear_tree()
                resets += 1
        s.set_roots(boards_tensor(gpu, states), turns=t.full((G,), ply, dtype=t.int32, device="cuda"))
        s.run_until_idle(stub_eval(gpu, spec), max_rounds=4 * sims0)
        st = s.root_stats()
        act = s.choose(None)
        for g, pl in enumerate(players):
            a, _ = pl.action(states[g], ply, None, False, 0.5)
            assert_root_equal(st, g, pl.node_stats(states[g]), f"ply {ply} game {g}")
            assert xo.label_str(int(act[g])) == a
        assert_counters_equal(gpu, s, players, f"ply {ply}")
    c = s.counters()
    assert G < resets <= 2 * G and c["tree_resets"] == resets, (c, resets)
    assert c["overflow_sims"] == sum(x["overflow_sims"] for x in got)
    for pl in players:
        pl.close()
    s.close()


# ---- 4. the heap runs out inside a ply -----------------------------------------------------------------------------
def _round(s, ev):
    """One round and the evaluation of its new leaves; returns the number of games still searching."""
    s.round()
    pending, rows = s.leaf_rows()
    if pending and rows.numel():
        p, v = ev(s.planes.index_select(0, rows))
        s.policy.index_copy_(0, rows, p)
        s.value.index_copy_(0, rows, v)
    return pending


def _tree_nodes(s, interior, limit=1200):
    """Breadth first over the engine's tree of game 0 along each node's three most visited edges (the principal variation
    and its siblings): [(path, stats)] of the nodes that have edges, until `interior` of them below the root have been
    selected from (or `limit` nodes were read)."""
    out, queue, have = [], [[]], 0
    while queue and have < interior and len(out) < limit:
        nxt = []
        for path in queue:
            st = node_at(s, 0, path)
            if len(st["n"]) == 0:
                continue                      # a terminal child, or one whose expansion was refused
            out.append((path, st))
            have += int(len(path) > 0 and st["sum_n"] > 1)
            if have >= interior or len(out) >= limit:
                break
            order = np.argsort(-st["n"], kind="stable")
            nxt.extend(path + [int(st["moves"][j])] for j in order[:3] if st["n"][j] > 0)
        queue = nxt
    return out


@pytest.mark.parametrize("spec", [PEAKED, HASH5], ids=lambda v: v["kind"])
def test_heap_exhausted_inside_a_ply(gpu, spec):
    """One game whose chunks run out before its hash table does: created for 40 simulations with the smallest pool (the
    chunk it keeps and one spare), then asked for 8000.  The oracle has no granules, so no parity: the search must end,
    count what it refused, leave every node consistent (tests/search_limits.py: a virtual loss that is not returned
    breaks sum n_j == sum_n - 1), keep its chunk accounting, and not touch the search object that runs beside it."""
    t = gpu.torch
    K, sims = 64, 8000
    pc0 = play_config(simulation_num_per_move=40, search_threads=K)
    # the neighbour: two games, default memory; alone first
    pcb = play_config(simulation_num_per_move=200, search_threads=8)
    bstates = [MID, END]

    def neighbour():
        b = gpu.S.Search(pcb, 2, seed=2)
        b.set_roots(boards_tensor(gpu, bstates))
        return b
    b = neighbour()
    b.run_until_idle(stub_eval(gpu, HASH5), max_rounds=800)
    alone = b.root_stats()
    b.close()

    s = gpu.S.Search(pc0, 1, seed=1, pool_chunks=1, max_nodes_per_game=8000)
    assert s.pool_chunks == s.keep_chunks + 1 and s.hash_cap == 16384
    b = neighbour()
    s.set_sims(sims)
    s.set_roots(boards_tensor(gpu, [MID]))
    ev, evb = stub_eval(gpu, spec), stub_eval(gpu, HASH5)
    rounds, b_pending = None, 1
    for r in range(4 * sims // K):                                   # (sims / K batches, each a few rounds at most)
        if b_pending:
            b_pending = _round(b, evb)
        if _round(s, ev) == 0:
            rounds = r + 1
            break
    assert rounds is not None and s.pending() == 0, "the starved search did not finish"
    for _ in range(800):
        if not b_pending:
            break
        b_pending = _round(b, evb)
    assert b_pending == 0
    c, m = s.counters(), s.memory_info()
    print(f"heap exhausted ({spec['kind']}): {rounds} rounds, counters "
          f"{ {k: c[k] for k in PARITY_COUNTERS + ('tree_resets', 'chunks_taken', 'stat_blocks')} }, memory {m}")
    # it happened, and the heap -- not the hash table -- was the limit
    assert c["overflow_sims"] > 0 and m["nodes"] < s.hash_cap, (c, m)
    assert m["free_chunks"] == 0 and m["held_chunks"] == s.pool_chunks == m["pool_chunks"]
    assert c["sims"] == sims and sims_end_one_way(c), c
    assert c["expansions"] == m["nodes"] and c["tree_resets"] == 1
    root = s.root_stats()
    assert int(root["sum_n"][0]) == sims
    nodes = _tree_nodes(s, 200)
    interior = [x for x in nodes if len(x[0]) > 0 and x[1]["sum_n"] > 1]
    assert len(interior) >= 200, (len(interior), len(nodes))
    for path, st in nodes:
        assert node_defect(st) is None, (path, node_defect(st), st)
    # the neighbour's games are what they are alone, and what the oracle says
    bst = b.root_stats()
    for g, state in enumerate(bstates):
        cnt = int(alone["counts"][g])
        ref = dict(moves=alone["moves"][g, :cnt], n=alone["n"][g, :cnt], w=alone["w"][g, :cnt], p=alone["p"][g, :cnt],
                   sum_n=int(alone["sum_n"][g]))
        assert_root_equal(bst, g, ref, f"neighbour game {g}")
        pl = xo.Player(ocfg(pcb), HASH5)
        pl.search(state)
        assert_root_equal(bst, g, pl.node_stats(state), f"neighbour game {g} against the oracle")
        pl.close()
    b.close()
    # afterwards: the trees dropped, a search of the length the object was created for is the oracle's again
    s.set_sims(40)
    s.reset_trees()
    m = s.memory_info()
    assert m["nodes"] == 0 and m["held_chunks"] == s.keep_chunks and m["free_chunks"] + m["held_chunks"] == m["pool_chunks"]
    s.set_roots(boards_tensor(gpu, [MID]))
    s.run_until_idle(ev, max_rounds=200)
    pl = xo.Player(ocfg(pc0), oracle_stub(spec))
    pl.search(MID)
    assert_root_equal(s.root_stats(), 0, pl.node_stats(MID), "after reset_trees")
    pl.close()
    c2 = s.counters()
    assert c2["overflow_sims"] == c["overflow_sims"] and c2["sims"] == sims + 40
    s.close()
