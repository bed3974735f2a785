"""play records written by the engine (tests/golden/engine_records.json, produced on an MI355X by
tools/make_engine_records.py) are valid input for the reference's trainer.  The oracle replays every record; the
reference's own ``expanding_data`` (worker/optimize.py:234-281) parsed them into the planes / policies / values recorded
in tests/golden/trainer_records.json (tests/golden/make_golden_trainer.py), and the oracle's replay must give the same."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import xq_oracle as xo

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "engine_records.json")


def _games():
    if not os.path.exists(FIXTURE):
        pytest.skip("engine_records.json not generated yet")
    with open(FIXTURE) as f:
        return json.load(f)["games"]


def test_engine_records_replay_with_oracle():
    games = _games()
    assert len(games) >= 20
    for g in games:
        data = g["data"]
        assert data[0] == xo.INIT_STATE and len(data) - 1 == g["turns"]
        state = data[0]
        for i, (mv, v) in enumerate(data[1:]):
            assert mv in xo.get_legal_moves(state), (g["game_id"], i)
            assert v == (g["value"] if i % 2 == 0 else -g["value"])
            state = xo.step(state, mv)
        over = xo.done(state)[0]
        # a decided game ends in a terminal position: the king capture appended (self_play.py:177-184) or the
        # two kings facing each other (static_env.py:39-49) -- unless it ended by resignation
        if g["value"] != 0 and not g["resigned"]:
            assert over


def test_reference_trainer_parses_engine_records():
    """The reference's expanding_data on every engine record, as recorded by tests/golden/make_golden_trainer.py
    (trainer_records.json): the same planes / policies / values as the oracle's replay of the record."""
    with open(os.path.join(HERE, "golden", "trainer_records.json")) as f:
        ref = {r["game_id"]: r for r in json.load(f)["games"]}
    games = _games()
    assert sorted(ref) == sorted(g["game_id"] for g in games)
    for g in games:
        r = ref[g["game_id"]]
        n = g["turns"]
        assert r["planes_shape"] == [n, 14, 10, 9] and r["policy_shape"] == [n, 2086] and r["value_shape"] == [n]
        planes = []
        state = g["data"][0]
        for i, (mv, v) in enumerate(g["data"][1:]):
            planes.append(np.asarray(xo.state_to_planes(state), dtype=np.float32))
            assert r["policy_argmax"][i] == xo.label_of_str(mv) and r["policy_sum"][i] == 1
            assert r["value"][i] == v
            state = xo.step(state, mv)
        got = hashlib.sha256(np.ascontiguousarray(np.stack(planes), dtype=np.float32).tobytes()).hexdigest()
        assert got == r["planes_sha256"], g["game_id"]
