"""tests/search_model.py and the game loop of tests/selfplay_oracle.py, the two pieces every feature oracle is built on:
that each exists once, that the Gumbel players' games are start_game's (held to tests/game_endings.py, which shares no
code with the loop), and that every node keeps the stub's value."""
import inspect

import numpy as np
import pytest

import forced_playouts_oracle as fo
import game_endings
import gumbel_full_oracle as gf
import gumbel_oracle as go
import search_model as sm
import solver_oracle
import stop_oracle
import stub_net
from oracle import xq_oracle as xo


# ---- structure ----------------------------------------------------------------------------------------------------------
def test_one_simulation_loop_and_one_puct_loop():
    for mod in (go, gf, solver_oracle, stop_oracle):
        assert issubclass(mod.Search, sm.Search) and "_simulate" not in vars(mod.Search), mod.__name__
        assert "_puct" not in vars(mod.Search), mod.__name__
    assert fo.Search is sm.Search and fo._Node is sm.Node
    assert not hasattr(gf, "_Node") and issubclass(solver_oracle._Node, sm.Node)
    assert solver_oracle.Search.node_cls is solver_oracle._Node and go.Search.node_cls is sm.Node
    # the solver's selection ends in the model's loop: no second one, under any name
    assert not hasattr(solver_oracle.Search, "_select_reference")
    src = inspect.getsource(solver_oracle)
    assert "self._puct(node, is_root, skip)" in src and "c_puct" not in src and "sqrt" not in src


def _games_cfg():
    """The configuration of test_gumbel_full_cpu.py's test_margins_of_the_games_carry_the_gpu_comparison."""
    from test_gpu_search import oracle_cfg, play_config
    return oracle_cfg(play_config(simulation_num_per_move=32, search_threads=1, noise_eps=0.0, tau_decay_rate=0.0,
                                  max_game_length=3, enable_resign_rate=0.5, resign_threshold=-0.3, min_resign_turn=1))


def test_the_full_game_leaves_gumbel_oracle_as_it_was():
    plain = go.Search
    gf.gumbel_selfplay_game(_games_cfg(), 5, 13, 0, 0, 8)
    assert go.Search is plain
    with pytest.raises(ValueError, match="needs the Gumbel root search"):       # raised by the player's constructor
        gf.gumbel_selfplay_game(_games_cfg(), 5, 13, 0, 0, 0)
    assert go.Search is plain


# ---- the Gumbel players' games are the loop's ------------------------------------------------------------------------------
def test_gumbel_games_agree_with_the_classifier():
    """The four full games of the margins test and the four root-only games of the same arguments, replayed without a
    search: value, turns and searched, the position of every ply and the moves banned there."""
    cfg = _games_cfg()
    games = [(f"{mod.__name__} {gid}", mod.gumbel_selfplay_game(cfg, 5, 13, gid, gid, 8)) for mod in (gf, go) for gid in range(4)]
    scans = resigned = 0
    for what, g in games:
        c = game_endings.classify(g["init_state"], g["moves"], cfg.max_game_length)
        assert (c["value"], c["turns"], c["searched"]) == (g["value"], g["turns"], g["searched"]), what
        assert c["final_state"] == g["final_state"] and (c["ending"] == "resign") == g["resigned"], what
        assert c["states"] == [p["state"] for p in g["plies"]], what
        for t, p in enumerate(g["plies"]):
            banned = [xo.label_str(int(l)) for l, b in zip(p["labels"], p["banned"]) if b]
            assert sorted(set(c["bans"][t])) == sorted(banned), (what, t)
        scans += len(c["scans"])
        resigned += g["resigned"]
    print(f"{len(games)} games: {scans} repetition scans that found the position again, {resigned} resignations"
          + ("" if scans and resigned else " -- these games do not reach every branch of the loop"))


# ---- the kept value --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0.0, 2.0])
def test_every_node_keeps_the_stubs_value(k):
    nodes = 0
    for case in (fo.cases()[0], fo.cases()[3]):
        res, s = sm.run_case(case, k, sims=64)
        assert len(s.tree) > 16
        for state, node in s.tree.items():
            want = stub_net.hash_stub_numpy(xo.state_to_planes(state)[None], case["salt"])[1][0]
            assert node.state == state and node.v.dtype == np.float32
            assert node.v.tobytes() == np.float32(want).tobytes(), (case["name"], state)
            nodes += 1
    print(f"k = {k}: {nodes} nodes")
