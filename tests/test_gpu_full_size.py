"""-m gpu: the BASELINE.json configurations at their published sizes against the oracle (oracle/xq_mcts.c) and float64.

The rest of the suite pins the kernels at small sizes (<= 943 trees, <= 800 simulations, <= 1500 queue rows).  Several
paths run only at the sizes the figures come from, and each case below asserts the sizing it exists for, so that a later
change of defaults cannot quietly turn it into a small-size test:
  deep    1600 simulations: a third base chunk per game (keep_chunks == 3), 2^19 hash entries per game -- 2^31 entries
          at 4096 games, past int32 --, longer paths against MAXD_LDS, a 20x256 fp16 network on 32 768 queue rows;
  normal  4096 games x K = 8 = 32 768 queue rows, 4096 records finishing in the same rounds, the real network with the
          compact queue and root reuse across a ply boundary;
  eval    the 200-game arena at 400 simulations.
G, K and the simulations are the configurations' own (configs/_tables.py::benchmark_overrides, built the way bench.py
builds them); a case overrides only what it must and says why.  Each case frees its device memory before the next."""
import types

import numpy as np
import pytest

import stub_net
from oracle import xq_oracle as xo
from test_gpu_search import (END, MATE, MID, assert_root_equal, boards_tensor, gpu, oracle_cfg,  # noqa: F401
                             play_config, run_selfplay, stub_eval)

pytestmark = pytest.mark.gpu
PLAY_FIELDS = ("simulation_num_per_move", "search_threads", "c_puct", "noise_eps", "dirichlet_alpha", "tau_decay_rate",
               "virtual_loss", "resign_threshold", "min_resign_turn", "max_game_length", "enable_resign_rate")


def bench_config(name):
    """The Config object bench.py runs for `--config name` (bench.py::build_config, no command-line overrides)."""
    import bench
    return bench.build_config(types.SimpleNamespace(config=name, games=None, sims_per_round=None, dtype=None, trunk=None))


def config_play(name, **override):
    cfg = bench_config(name)
    d = {k: getattr(cfg.play, k) for k in PLAY_FIELDS}
    d.update(override)
    return play_config(**d), cfg


def live_positions(positions_1k):
    """Indices of the 1k suite's positions that are not over and whose mover has a move."""
    return [i for i, p in enumerate(positions_1k) if not p["done"][0] and p["moves"].split()]


def suite_picks(positions_1k):
    """Three roots of the 1k suite: the most legal moves, the first one in check, the first whose mover ends the game
    with one of its moves (a search that meets terminal positions near the root)."""
    live = live_positions(positions_1k)
    most = max(live, key=lambda i: len(positions_1k[i]["moves"].split()))
    check = next(i for i in live if len(positions_1k[i]["done"]) > 3 and positions_1k[i]["done"][3])
    mate = next(i for i in live if i not in (most, check) and
                any(xo.done(xo.step(positions_1k[i]["state"], m))[0] for m in positions_1k[i]["moves"].split()))
    return [positions_1k[i]["state"] for i in (most, check, mate)]


def assert_clean(c, *extra):
    for k in ("overflow_sims", "depth_overflow", "tree_resets") + extra:
        assert c[k] == 0, (k, c[k])


# ---- deep: 1600 simulations per move ------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8])
def test_deep_searches_match_oracle(gpu, positions_1k, K):
    # noise_eps = 0: the engine's Dirichlet draws are not the oracle's RNG callback, so noise on cannot match bit for bit
    pc, _ = config_play("deep", search_threads=K, noise_eps=0.0)
    assert pc.simulation_num_per_move == 1600
    spec = dict(kind="hash", salt=5)
    states = [xo.INIT_STATE, MID, END, MATE, xo.fliped_state(MID), xo.step(xo.INIT_STATE, '1242')]
    states += suite_picks(positions_1k)
    s = gpu.S.Search(pc, len(states), seed=7)
    assert s.keep_chunks == 3                          # a third base chunk: what the 1600-simulation tree needs
    s.set_roots(boards_tensor(gpu, states))
    s.run_until_idle(stub_eval(gpu, spec))
    st = s.root_stats()
    ctr = s.counters()
    s.close()
    tot = dict(sims=0, expansions=0, terminal_sims=0, repetition_sims=0, parked=0)
    for g, state in enumerate(states):
        pl = xo.Player(oracle_cfg(pc), spec)
        pl.search(state)
        assert_root_equal(st, g, pl.node_stats(state), f"game {g} K={K}")
        c = pl.counters()
        for k in tot:
            tot[k] += c[k]
        pl.close()
    for k, v in tot.items():
        assert ctr[k] == v, (k, ctr[k], v)
    assert_clean(ctr)


def test_deep_tree_is_reused_across_plies(gpu):
    """test_multi_ply_reuse_matches_oracle at 1600 simulations: the game outgrows its three base chunks (takes chunks
    from the pool) while every ply still equals the oracle's whole-game tree."""
    pc, _ = config_play("deep", noise_eps=0.0)                           # (noise off: bit-for-bit comparison)
    assert pc.search_threads == 8
    spec = dict(kind="hash", salt=11)
    G = 4
    s = gpu.S.Search(pc, G, seed=1)
    keep = s.keep_chunks
    assert keep == 3
    players = [xo.Player(oracle_cfg(pc), spec) for _ in range(G)]
    states = [xo.INIT_STATE, xo.step(xo.INIT_STATE, '7242'), MID, END]
    t = gpu.torch
    for ply in range(4):
        s.set_roots(boards_tensor(gpu, states), turns=t.full((G,), ply, dtype=t.int32, device="cuda"))
        s.run_until_idle(stub_eval(gpu, spec))
        st = s.root_stats()
        act = s.choose(None)
        for g in range(G):
            a, _ = players[g].action(states[g], ply, None, False, 0.5)
            assert_root_equal(st, g, players[g].node_stats(states[g]), f"ply {ply} game {g}")
            assert xo.label_str(int(act[g])) == a
            states[g] = xo.step(states[g], a)
    c, m = s.counters(), s.memory_info()
    s.close()
    for p in players:
        p.close()
    assert_clean(c)
    assert m["nodes"] == c["expansions"]
    assert m["held_chunks_max_game"] > keep, m             # chunks taken beyond keep_chunks at this size
    assert c["chunks_taken"] > 0, c


def test_deep_one_ply_at_4096_games(gpu, positions_1k):
    """4096 trees of 1600 simulations: G x hash_cap = 2^31 hash entries (17 GB), the first size whose entry index does
    not fit an int32."""
    pc, cfg = config_play("deep", noise_eps=0.0)                         # (noise off: bit-for-bit comparison)
    G = cfg.engine.games_per_gpu
    assert G == 4096 and pc.search_threads == 8 and pc.max_game_length == 100
    live = live_positions(positions_1k)
    pool = [positions_1k[i]["state"] for i in live]
    pool += [positions_1k[i]["flip"] for i in live
             if not xo.done(positions_1k[i]["flip"])[0] and xo.get_legal_moves(positions_1k[i]["flip"])]
    states = [pool[g % len(pool)] for g in range(G)]
    spec = dict(kind="hash", salt=37)
    # pool_chunks explicit: the default takes up to 80 % of the free device memory; one ply on empty trees needs the
    # games' base chunks (G x keep_chunks) and nothing more
    s = gpu.S.Search(pc, G, seed=3, pool_chunks=G * 3 + 1024)
    try:
        assert s.hash_cap == 2 ** 19 and s.keep_chunks == 3
        assert G * s.hash_cap == 2 ** 31
        s.set_roots(boards_tensor(gpu, states))
        s.run_until_idle(stub_eval(gpu, spec))
        st = s.root_stats()
        ctr = s.counters()
    finally:
        s.close()
    assert (st["sum_n"] == 1600).all() and (st["n"].sum(axis=1) == 1600 - 1).all()
    assert_clean(ctr)
    rng = np.random.default_rng(4096)
    sample = [0, G - 1] + sorted(rng.choice(np.arange(1, G - 1), 48, replace=False).tolist())
    for g in sample:
        pl = xo.Player(oracle_cfg(pc), spec)
        pl.search(states[g])
        assert_root_equal(st, g, pl.node_stats(states[g]), f"game {g}")
        pl.close()


def test_deep_network_on_the_full_slot_queue(gpu, positions_1k):
    """The 20x256 fp16 network of `deep` on the engine's whole slot queue (it takes no compact queue): 32 768 rows, ~128
    boards per workgroup of every persistent kernel.  Rows are batch-independent bit for bit and near the fp32 module."""
    import torch
    import bench
    from cchess_alphazero.agent.model import CChessNet, calibration_planes, guarded_inference_net
    cfg = bench_config("deep")
    assert (cfg.model.res_layer_num, cfg.model.cnn_filter_num, cfg.engine.net_dtype) == (20, 256, "float16")
    n = cfg.engine.games_per_gpu * cfg.play.search_threads
    assert n == 32768
    torch.manual_seed(0)
    ref = CChessNet.from_model_config(cfg.model)                         # (bench.py's weights)
    net = guarded_inference_net(ref, torch.float16, trunk="mfma", arith=cfg.engine.net_arith)     # (what the engine builds)
    assert net.trunk == "mfma" and not net.supports_compact_queue()
    # the queue: 1k-suite positions, calibration playouts, and empty slots (a round that left them unwritten)
    suite = torch.from_numpy(np.stack([xo.state_to_planes(positions_1k[i]["state"])
                                       for i in live_positions(positions_1k)]).astype(np.uint8)).cuda()
    calib = calibration_planes(4096, 14, seed=77)
    src = torch.cat([suite, calib, torch.zeros((1, 14, 10, 9), dtype=torch.uint8, device="cuda")])
    rng = np.random.default_rng(20)
    kind = rng.choice(3, n, p=[0.3, 0.6, 0.1])
    pick = np.where(kind == 0, rng.integers(0, suite.shape[0], n),
                    np.where(kind == 1, suite.shape[0] + rng.integers(0, calib.shape[0], n), src.shape[0] - 1))
    pick[0], pick[-1] = 0, suite.shape[0]                                # (first and last rows hold a position)
    planes = src[torch.from_numpy(pick).cuda()].contiguous()
    p_all, v_all = (x.clone() for x in net(planes))
    torch.cuda.synchronize()
    assert torch.isfinite(p_all).all() and torch.isfinite(v_all).all()
    # a sample evaluated alone, in batches of 64: first and last rows, the rows around the persistent kernels' strides
    # (one workgroup per CU, one or two boards per tile), the rest random
    edges = {0, n - 1}
    for k in (1, 2, 3, 4, 8, 16, 32, 64, 127, 128):
        for b in (128 * k, 256 * k):
            edges.update(r for r in (b - 1, b, b + 1) if 0 <= r < n)
    rest = rng.choice(np.setdiff1d(np.arange(n), sorted(edges)), 512 - len(edges), replace=False)
    rows = np.array(sorted(edges) + sorted(rest.tolist()))
    assert len(rows) == 512
    rt = torch.from_numpy(rows).cuda()
    for b in range(0, 512, 64):
        r = rt[b:b + 64]
        p, v = net(planes[r].contiguous())
        assert torch.equal(p.view(torch.int32), p_all[r].view(torch.int32)), rows[b:b + 64]
        assert torch.equal(v.view(torch.int32), v_all[r].view(torch.int32)), rows[b:b + 64]
    # 64 of them against the fp32 CPU module, with the tolerance bench.py's numerics_check applies to this config
    q = planes[rt[::8]].contiguous()
    eng = types.SimpleNamespace(queue_planes=lambda k: q[:k], net=net, trunk=net.trunk)
    chk = bench.numerics_check(eng, ref, cfg, nq=64)
    assert chk["positions"] == 64
    assert chk["tolerance"] == bench.fp16_tolerance(20, 256), chk["tolerance"]
    assert chk["within_tolerance"], chk


# ---- normal: 4096 games x K = 8 x 800 simulations -----------------------------------------------------------------
def normal_selfplay_play(**override):
    # noise_eps = 0 for the bit-for-bit comparison; max_game_length 10 (21 plies at most) bounds the oracle's replay
    pc, cfg = config_play("normal", **dict(dict(noise_eps=0.0, max_game_length=10), **override))
    assert cfg.engine.games_per_gpu == 4096 and pc.search_threads == 8 and pc.simulation_num_per_move == 800
    return pc, cfg.engine.games_per_gpu


def whole_game_pool(gpu, pc):
    """Chunks for every game's whole-game tree (what the default pool asks for when the device has room), passed
    explicitly: the default would size itself by the free device memory of a shared machine."""
    probe = gpu.S.Search(pc, 1, seed=0, pool_chunks=1)
    mc = probe.max_chunks
    probe.close()
    return mc


def assert_accounting(s, c, G, K):
    m = s.memory_info()
    assert m["free_chunks"] + m["held_chunks"] == m["pool_chunks"], m
    # every finished simulation ended one way; the difference is the leaves still waiting for their evaluation
    in_flight = c["expansions"] + c["terminal_sims"] + c["repetition_sims"] - c["sims"]
    assert 0 <= in_flight <= G * K, (c, in_flight)


def test_normal_selfplay_4096_games_match_oracle(gpu):
    pc, G = normal_selfplay_play()
    assert pc.tau_decay_rate == 0.9                                      # Philox-driven move sampling
    K = pc.search_threads
    spec = dict(kind="hash", salt=43)
    seed = 31
    drained = []
    seen = {}

    def inspect(s):
        seen["mem"] = s.memory_info()
        seen["ctr"] = s.counters()
        assert_accounting(s, seen["ctr"], G, K)
    recs, ctr = run_selfplay(gpu, pc, spec, G, seed, G, max_rounds=6000, drained=drained, before_close=inspect,
                             pool_chunks=G * whole_game_pool(gpu, pc))
    assert G * K == 32768
    assert_clean(ctr, "ring_dropped", "no_act_truncated")
    first = [r["game_id"] for r in drained if r["game_id"] < G]
    assert sorted(first) == list(range(G))                               # each first game drained exactly once
    assert all(0 < recs[g]["turns"] <= 2 * pc.max_game_length + 1 for g in range(G))
    rng = np.random.default_rng(G)
    sample = [0, G - 1] + sorted(rng.choice(np.arange(1, G - 1), 64, replace=False).tolist())
    for gid in sample:
        ref = xo.selfplay_game(oracle_cfg(pc), spec, seed, gid)
        got = recs[gid]
        moves = [xo.label_str(int(m)) for m in got["moves"]]
        assert moves == ref["moves"], (gid, moves, ref["moves"])
        assert got["turns"] == ref["turns"] and got["value"] == int(ref["value"]) and got["store"] == ref["store"], gid


def test_normal_root_noise_at_4096_games(gpu):
    """The same 4096 games with the configuration's root noise (noise_eps = 0.15) for two plies.  No oracle match is
    possible; the bookkeeping must hold and the noise must act: without it every first root (INIT, same stub) would
    get the same visit vector."""
    pc, G = normal_selfplay_play(noise_eps=0.15)
    K, sims = pc.search_threads, pc.simulation_num_per_move
    spec = dict(kind="hash", salt=43)
    t = gpu.torch
    s = gpu.S.Search(pc, G, seed=31, pool_chunks=G * whole_game_pool(gpu, pc))
    try:
        states = [xo.INIT_STATE] * G
        rng = np.random.default_rng(15)
        firsts = None
        for ply in range(2):
            s.set_roots(boards_tensor(gpu, states), turns=t.full((G,), ply, dtype=t.int32, device="cuda"))
            s.run_until_idle(stub_eval(gpu, spec))
            st = s.root_stats()
            c = s.counters()
            assert (st["sum_n"] == sims).all() and (st["n"].sum(axis=1) == sims - 1).all(), ply
            assert_clean(c, "no_act_truncated")
            assert_accounting(s, c, G, K)
            if ply == 0:
                firsts = st["n"].copy()
            act = s.choose(rng.random(G))
            states = [xo.step(states[g], xo.label_str(int(act[g]))) for g in range(G)]
        assert c["root_reused_sims"] > 0
    finally:
        s.close()
    pl = xo.Player(oracle_cfg(play_config(**{k: getattr(pc, k) for k in PLAY_FIELDS if k != "noise_eps"})), spec)
    pl.search(xo.INIT_STATE)
    quiet = pl.node_stats(xo.INIT_STATE)["n"]
    pl.close()
    c0 = len(quiet)
    assert len({tuple(r) for r in firsts[:, :c0]}) > G // 2
    assert (firsts[:, :c0] != quiet[None, :]).any(axis=1).sum() > G // 2


def test_normal_engine_with_the_real_network(gpu):
    """SelfPlayEngine as bench.py builds it (normal: 4096 games, 7x128 float32 network, c6 tower behind the load-time
    guard, compact queue) for 120 rounds -- across the first ply boundary, so root reuse runs with the real network."""
    import torch
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.engine import SelfPlayEngine
    cfg = bench_config("normal")
    G, K = cfg.engine.games_per_gpu, cfg.play.search_threads
    assert G * K == 32768 and cfg.play.simulation_num_per_move == 800 and cfg.play.max_game_length == 100
    torch.manual_seed(0)
    ref_net = CChessNet.from_model_config(cfg.model)
    # pool_chunks explicit (the default sizes itself by the free memory of a shared device): the base chunks plus four
    # per game for the second ply's reservation
    eng = SelfPlayEngine(cfg, G, net=ref_net, dtype=torch.float32, seed=20260923, pool_chunks=G * 6)
    try:
        s = eng.search
        assert eng.compact and eng.net_arith_effective == "c6" and s.keep_chunks == 2
        eng.start()
        rounds = 120
        checks = {0, rounds // 2, rounds - 1}
        prev = eng.counters()["expansions"]
        rng = np.random.default_rng(7)
        for r in range(rounds):
            eng.step()
            qc = int(s.q_count.item())
            c = eng.counters()
            assert 0 < qc <= G * K, (r, qc)
            # a leaf is expanded (expand_node counts it) in the launch that writes it to its slot, and k_sim(SELECT)
            # lists every slot holding a leaf of this round in q_rows: the same round, no lag
            assert c["expansions"] - prev == qc, (r, c["expansions"] - prev, qc)
            prev = c["expansions"]
            if r in checks:
                a = eng.audit_network(1024)
                assert a is not None and a["ok"], (r, a)
                idx = np.unique(np.concatenate([[0, qc - 1], rng.integers(0, qc, 510)]))
                it = torch.from_numpy(idx).cuda()
                rows = s.q_rows[it].long()
                planes = s.queue_planes(rows=rows)
                p, v = eng.net(planes, logits=eng.policy_logits)
                assert eng.policy_logits
                assert torch.equal(p.view(torch.int32), s.policy[it].view(torch.int32)), r
                assert torch.equal(v.view(torch.int32), s.value[it].view(torch.int32)), r
        c = eng.counters()
        assert c["plies"] > 0 and c["root_reused_sims"] > 0, c
        assert_clean(c, "no_act_truncated")
        m = s.memory_info()
        assert m["free_chunks"] + m["held_chunks"] == m["pool_chunks"], m
    finally:
        eng.close()


# ---- eval: 400 simulations, 200 paired games ----------------------------------------------------------------------
def test_eval_arena_200_games_match_oracle(gpu):
    from arena_oracle import arena_game
    from cchess_alphazero.worker.evaluator import EvaluateWorker, score_table
    cfg = bench_config("eval")
    # noise_eps = 0: bit-for-bit comparison; max_game_length 12 bounds the oracle's replay
    cfg.play.noise_eps = 0.0
    cfg.play.max_game_length = 12
    cfg.opts.evaluate = False                              # like bench.py's arena (run.py eval of the reference)
    n = cfg.engine.games_per_gpu
    assert n == 200 and cfg.play.simulation_num_per_move == 400 and cfg.play.search_threads == 8
    assert cfg.play.c_puct == 1 and cfg.play.tau_decay_rate == 0
    specs = (dict(kind="hash", salt=51), dict(kind="hash", salt=52))
    evs = tuple((lambda planes, s=s: stub_net.hash_stub_torch(planes, s["salt"])) for s in specs)

    def u_fn(g, turns):
        return stub_net.philox_uniform(77, g, 1, turns)
    w = EvaluateWorker(cfg, evaluators=evs, seed=5)
    stats = {}
    got = w.play_games(n, u_fn=u_fn, stats=stats)
    assert len(got) == n
    assert stats["overflow_sims"] == 0 and stats["tree_resets"] == 0, stats
    table = score_table(got)
    assert sum(table[1:]) == n and 0 <= table[0] <= n
    rng = np.random.default_rng(200)
    sample = sorted({0, n - 1} | set(rng.choice(np.arange(0, n, 2), 8, replace=False).tolist())
                    | set(rng.choice(np.arange(1, n, 2), 8, replace=False).tolist()))
    assert len(sample) >= 17 and any(i % 2 == 0 for i in sample) and any(i % 2 == 1 for i in sample)
    for i in sample:
        assert got[i] == arena_game(i, cfg.play, specs, u_fn)[:2], i
