"""Forced playouts and policy target pruning without a GPU: tests/forced_playouts_oracle.py -- the yardstick of
test_gpu_forced_playouts.py -- is pinned to the C oracle where the two must agree (k = 0), its inputs are shown to
exercise forcing and pruning at k = 2, and the command line is checked against config.engine."""
import json
import os

import numpy as np
import pytest

import forced_playouts_oracle as fo
from oracle import xq_oracle as xo


@pytest.fixture(scope="module")
def cases():
    cs = fo.cases()
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "positions_1k.json")) as f:
        golden = {p["state"] for p in json.load(f)["positions"]}
    assert cs[0]["state"] == xo.INIT_STATE
    assert len({c["state"] for c in cs[1:]} & golden - {xo.INIT_STATE}) >= 7
    assert any(c["kind"] == "ban" for c in cs) and any(c["kind"] == "reuse" for c in cs)
    return cs


def test_python_search_is_the_oracle_search_at_k_0(cases):
    """The pin: at k = 0 the Python search equals xo.Player.search + node_stats on n, w (bit for bit), p and sum_n, on
    every position, with the ban and along the two-ply reuse line; the counters agree as well."""
    for c in cases:
        res, s = fo.run_case(c, 0.0)
        pl = xo.Player(fo.play_cfg(), dict(kind="hash", salt=c["salt"]))
        assert len(res) == (2 if c["kind"] == "reuse" else 1)
        for r in res:
            assert bool(r["no_act"]) == (c["kind"] == "ban")
            pl.search(r["state"], 0, r["no_act"])
            ref, st = pl.node_stats(r["state"]), r["stats"]
            assert (st["moves"] == ref["moves"]).all(), c["name"]
            assert st["sum_n"] == ref["sum_n"], c["name"]
            assert (st["n"] == ref["n"]).all(), c["name"]
            assert (st["w"].view(np.uint64) == ref["w"].view(np.uint64)).all(), c["name"]
            assert (st["p"].view(np.uint32) == ref["p"].view(np.uint32)).all(), c["name"]
            # nothing forced, nothing pruned
            assert r["raw_total"] == sum(int(n) for n, m in zip(st["n"], st["moves"])
                                         if xo.label_str(int(m)) not in r["no_act"])
            assert (r["targets"] == st["n"]).all()
        ctr = pl.counters()
        for key in ("sims", "expansions", "terminal_sims", "repetition_sims"):
            assert ctr[key] == getattr(s, key), (c["name"], key)
        assert s.forced_picks == 0
        if c["kind"] == "reuse":
            assert fo.SIMS < s.sims < 2 * fo.SIMS           # the second search started from the first one's subtree
        if c["kind"] == "ban":
            assert res[0]["best"] != res[0]["no_act"][0]
        pl.close()


def test_inputs_force_and_prune_at_k_2(cases):
    """A condition on the inputs (the salts were chosen for it): at k = 2 at least half of the positions see forced picks
    and at least half lose visits to pruning.  And on every position: the pruned counts sum to no more than S, c* keeps
    its count, no count grows."""
    forced = pruned = 0
    for c in cases:
        res, s = fo.run_case(c, 2.0)
        forced += s.forced_picks > 0
        removed = 0
        for r in res:
            st = r["stats"]
            live = np.array([xo.label_str(int(m)) not in r["no_act"] for m in st["moves"]])
            S = int(st["n"][live].sum())
            assert r["raw_total"] == S
            assert int(r["targets"][live].sum()) <= S
            assert (r["targets"] <= st["n"]).all() and (r["targets"] >= 0).all()
            assert (r["targets"][~live] == st["n"][~live]).all()                  # banned edges keep their raw count
            star = min(np.flatnonzero(live), key=lambda j: (-int(st["n"][j]), int(st["moves"][j])))
            assert r["targets"][star] == st["n"][star] and xo.label_str(int(st["moves"][star])) == r["best"]
            assert int(r["targets"][live].max()) == int(r["targets"][star])       # still the greatest target
            removed += S - int(r["targets"][live].sum())
        pruned += removed > 0
    assert 2 * forced >= len(cases), forced
    assert 2 * pruned >= len(cases), pruned


def test_command_line_flags():
    from cchess_alphazero import manager
    from cchess_alphazero.config import Config
    assert Config("mini").engine.forced_playouts == 0.0
    p = manager.create_parser()
    cfg = manager.build_config(p.parse_args(["self"]))
    assert cfg.engine.forced_playouts == 0.0
    cfg = manager.build_config(p.parse_args(["self", "--record-visits", "--forced-playouts", "2"]))
    assert cfg.engine.forced_playouts == 2.0 and cfg.engine.record_visits
    cfg = manager.build_config(p.parse_args(["self", "--forced-playouts", "0"]))       # off needs no visit record
    assert cfg.engine.forced_playouts == 0.0
    for bad, needle in ((["--record-visits", "--forced-playouts", "-1"], "--forced-playouts -1"),
                        (["--record-visits", "--forced-playouts", "inf"], "--forced-playouts inf"),
                        (["--record-visits", "--forced-playouts", "nan"], "--forced-playouts nan"),
                        (["--forced-playouts", "2"], "needs --record-visits")):
        with pytest.raises(SystemExit) as e:
            manager.build_config(p.parse_args(["self"] + bad))
        assert needle in str(e.value), bad
