"""The MCTS solver on the CPU: tests/solver_oracle.py, the Python restatement the GPU tests compare with, is pinned here.

  * with the solver rules disabled the subclass is forced_playouts_oracle.Search bit for bit;
  * every status with d <= 5 it proves on the fixtures agrees with a depth-limited minimax over the rule functions;
  * derive() / winning_edge(), the two functions its walk and its rule 1 go through, on hand-computed rows;
  * the played lines end in done() after exactly d - 1 plies;
  * tests/golden/solver_positions.json says what the oracle shows, and the set has the cases the GPU tests need."""
import functools

import numpy as np
import pytest

import forced_playouts_oracle as fo
import solver_oracle as so
from oracle import xq_oracle as xo

OPEN, WIN, LOSS = so.OPEN, so.WIN, so.LOSS


# ---- 1. off is off ---------------------------------------------------------------------------------------------------------
def _same_stats(a, b, what):
    assert (a["moves"] == b["moves"]).all() and (a["n"] == b["n"]).all() and a["sum_n"] == b["sum_n"], what
    assert a["w"].tobytes() == b["w"].tobytes() and a["p"].tobytes() == b["p"].tobytes(), what


@pytest.mark.parametrize("case", fo.cases(), ids=lambda c: c["name"])
def test_rules_off_is_the_parent_search(case):
    sims = 96
    want, ws = fo.run_case(case, 0.0, sims)
    got, gs = fo.run_case(case, 0.0, sims, search_cls=functools.partial(so.Search, solver=False))
    assert len(want) == len(got)
    for a, b in zip(want, got):
        assert a["state"] == b["state"] and a["no_act"] == b["no_act"] and a["best"] == b["best"]
        _same_stats(a["stats"], b["stats"], case["name"])
    for key in ("sims", "expansions", "terminal_sims", "repetition_sims"):
        assert getattr(ws, key) == getattr(gs, key), key
    assert gs.proven_sims == 0 and all(n.status == OPEN and not any(n.mark) for n in gs.tree.values())
    assert set(ws.tree) == set(gs.tree)


def test_rules_off_on_the_fixtures():
    for pos in so.positions():
        a, b = fo.Search(so.play_cfg(64), so.SALT), so.Search(so.play_cfg(64), so.SALT, solver=False)
        a.search(pos["state"])
        assert b.search(pos["state"]) == 64
        _same_stats(a.node_stats(pos["state"]), b.node_stats(pos["state"]), pos["name"])
        assert (a.sims, a.terminal_sims, a.expansions) == (b.sims, b.terminal_sims, b.expansions)


# ---- 2. the fixtures and soundness -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def searched():
    """name -> {sims: Search} of every fixture at its budgets, and of the nine ordinary positions at 64."""
    out = {}
    for pos in so.positions():
        out[pos["name"]] = {}
        for sims in pos["sims"]:
            s = so.Search(so.play_cfg(sims), so.SALT)
            s.ran = s.search(pos["state"])
            out[pos["name"]][sims] = s
    for c in fo.cases():
        s = so.Search(so.play_cfg(64), c["salt"])
        s.ran = s.search(c["state"])
        out["fo:" + c["name"]] = {64: s}
    return out


def test_golden_file_says_what_the_oracle_shows(searched):
    for pos in so.positions():
        s = searched[pos["name"]][max(pos["sims"])]
        pr, w = s.proof(pos["state"]), pos["want"]
        node = s.tree[pos["state"]]
        assert (pr["status"], pr["dist"], s.ran, s.rule1(node), len(node.moves)) == \
               (w["status"], w["dist"], w["ran"], w["edge"], w["moves"]), pos["name"]
        assert s.decided() and s.sims == s.ran
        if "open_at" in pos:
            o = searched[pos["name"]][pos["open_at"]]
            assert o.proof(pos["state"])["status"] == OPEN and o.ran == pos["open_at"] and not o.decided()


def test_the_set_has_the_cases_the_gpu_tests_need(searched):
    big = {p["name"]: searched[p["name"]][max(p["sims"])] for p in so.positions()}
    state = {p["name"]: p["state"] for p in so.positions()}
    assert any(s.rule1(s.tree[state[n]]) >= 64 for n, s in big.items())             # a proof through the second half
    assert any(n.status == LOSS for s in big.values() for n in s.tree.values())
    assert big["lost"].tree[state["lost"]].status == LOSS
    assert any("open_at" in p for p in so.positions())
    assert any(s.proven_sims > 0 for s in big.values())                             # an arrival
    nine = [searched["fo:" + c["name"]][64] for c in fo.cases()]
    assert len(nine) == 9 and sum(len(so.proven_nodes(s, so.DIST_MAX)) for s in nine) == 2
    assert sum(s.ran == 64 for s in nine) == 8                                      # ordinary positions: the full budget


def test_every_short_proof_agrees_with_the_minimax(searched):
    memo, checked = {}, {WIN: 0, LOSS: 0}
    for name, runs in searched.items():
        for sims, s in runs.items():
            for state, status, dist in so.proven_nodes(s, 5):
                # (d counts the king capture itself: done() shows the end one ply earlier, d - 1 plies deep)
                assert so.minimax(state, max(0, dist - 1), memo) == status, (name, sims, state, status, dist)
                checked[status] += 1
    assert checked[WIN] >= 8 and checked[LOSS] >= 8
    # the yardstick itself, on positions whose answer is known by hand
    m1 = "4s4/R8/9/9/9/8R/9/9/9/3S5"
    assert so.minimax(m1, 1, memo) == OPEN and so.minimax(m1, 2, memo) == WIN
    lost = "5s3/9/9/9/9/9/9/9/8r/r3S4"
    assert so.minimax(lost, 0, memo) == OPEN and so.minimax(lost, 1, memo) == LOSS
    assert so.minimax(xo.INIT_STATE, 2, memo) == OPEN


# ---- 3. derive and rule 1 by hand ------------------------------------------------------------------------------------------
def test_derive_rows():
    d = so.derive
    assert d([], []) == (OPEN, 0)                                                   # nm = 0: never LOSS
    assert d([OPEN, OPEN], [0, 0]) == (OPEN, 0)
    assert d([LOSS], [0]) == (WIN, 1)                                               # a king capture: WIN(1)
    assert d([WIN], [1]) == (LOSS, 2)                                               # every move allows it: LOSS(2)
    assert d([WIN, LOSS, LOSS, OPEN], [9, 6, 4, 0]) == (WIN, 5)                     # 1 + MIN d over the winning edges
    assert d([WIN, WIN, WIN], [1, 7, 3]) == (LOSS, 8)                               # 1 + MAX d over all edges
    assert d([WIN, WIN, OPEN], [1, 7, 0]) == (OPEN, 0)                              # one edge unmarked: stays OPEN
    assert d([LOSS], [254]) == (WIN, 255) and d([LOSS], [255]) == (WIN, 255)        # saturation
    assert d([WIN, WIN], [255, 3]) == (LOSS, 255)
    assert d([WIN] * 128, list(range(128))) == (LOSS, 128)                          # both halves of a wave


def test_rule_1_rows():
    w = so.winning_edge
    assert w([OPEN, WIN], [0, 1], [False, False]) == -1
    assert w([LOSS, LOSS, LOSS], [4, 2, 2], [False] * 3) == 1                       # least d, the first on a tie
    assert w([LOSS, LOSS, LOSS], [4, 2, 2], [False, True, False]) == 2              # a banned winning edge is passed over
    assert w([LOSS], [0], [True]) == -1                                             # ... and the root is then not decided
    assert w([OPEN] * 70 + [LOSS], [0] * 71, [False] * 71) == 70


def test_a_banned_winning_edge_leaves_the_root_won_but_searched():
    pos = {p["name"]: p for p in so.positions()}["m1"]
    s = so.Search(so.play_cfg(64), so.SALT)
    s.search(pos["state"])
    node = s.tree[pos["state"]]
    ban = node.moves[s.rule1(node)]
    before = s.sims
    s.no_act = (ban,)
    assert node.status == WIN and not s.decided()                  # proven, not decided: the ply is searched
    ran = s.search(pos["state"], [ban])
    assert 0 < ran <= 64 and s.sims == before + ran
    mv = s.play(pos["state"], [ban])
    assert mv != ban
    if ran < 64:                                                    # stopped early: on the second mate the rooks have
        assert s.decided() and s.edge_mark(node, node.moves.index(mv)) == LOSS
    # a first proof is final, and bans play no part in a status
    assert (node.status, node.dist) == (WIN, 3)


# ---- 4. played lines ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m1", "m2", "wide_m1", "wide_m2"])
def test_played_line_ends_after_d_minus_1_plies(name):
    pos = {p["name"]: p for p in so.positions()}[name]
    s = so.Search(so.play_cfg(max(pos["sims"])), so.SALT)
    line, end = s.play_line(pos["state"])
    d = pos["want"]["dist"]
    assert len(line) == d - 1 and xo.done(end)[:2] == (True, 1)
    assert [l["ran"] for l in line] == [pos["want"]["ran"]] + [0] * (d - 2)         # the later plies run no simulation
    assert [(l["proof"]["status"], l["proof"]["dist"]) for l in line] == \
           [(WIN if i % 2 == 0 else LOSS, d - i) for i in range(d - 1)]


# ---- 5. the host layers that need no device --------------------------------------------------------------------------------
def test_uci_option_and_mate_score_without_a_gpu(monkeypatch):
    import io
    from cchess_alphazero import manager, uci
    from cchess_alphazero.config import Config
    monkeypatch.setattr(uci.senv, "step", lambda state, move: state)               # (the ponder lookup steps on the device)
    # N = (d - 1) / 2 for WIN(d), -(d - 2) / 2 for LOSS(d): the king capture that d counts is never played
    assert [uci.mate_in(WIN, d) for d in (1, 3, 5, 17)] == [0, 1, 2, 8]
    assert [uci.mate_in(LOSS, d) for d in (2, 4, 16)] == [0, -1, -7]
    assert uci.mate_in(OPEN, 0) is None
    cfg = Config(config_type="mini")
    assert cfg.engine.solver is False                                               # off by default
    out = io.StringIO()
    u = uci.UCI(cfg, out=out)
    assert any(line.startswith("option name Solver") for line in uci.ENGINE_ID)
    u.handle("setoption name Solver value true")
    assert cfg.engine.solver is True
    u.handle("setoption name Solver value false")
    assert cfg.engine.solver is False
    # `info ... score mate N` where the root is proven, the centipawn-style score otherwise
    u.start_time, u.is_red_turn, u.state = 0.0, True, "4s4/R8/9/9/9/8R/9/9/9/3S5"
    u.info_best_move("8489", 0.25, 1, (WIN, 3))
    u.info_best_move("8489", 0.25, 1, (OPEN, 0))
    u.info_best_move("8489", 0.25, 1)
    lines = [l for l in out.getvalue().splitlines() if l.startswith("info")]
    assert " score mate 1 " in lines[0] and " score 250 " in lines[1] and " score 250 " in lines[2]
    # the command line: --solver for self and eval, refused with the options that have a root rule or a kernel of their own
    parse = manager.create_parser().parse_args
    assert manager.build_config(parse(["self", "--solver"])).engine.solver is True
    assert manager.build_config(parse(["eval"])).engine.solver is False
    for extra in (["--gumbel", "8", "--record-visits"], ["--forced-playouts", "2", "--record-visits"], ["--eval-cache", "10"]):
        with pytest.raises(SystemExit, match="--solver excludes"):
            manager.build_config(parse(["self", "--solver"] + extra))
    with pytest.raises(SystemExit, match="--solver is an option"):
        manager.build_config(parse(["opt", "--solver"]))
