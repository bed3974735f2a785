"""Records with five-element items ([move, value, pi or None, weight, q]: run.py self --record-visits --record-q) are still
valid input for the reference's trainer, which reads item[0] and item[1] only (worker/optimize.py:245-246).  The
reference's own ``expanding_data`` parsed the engine records of tests/golden/engine_records.json rewritten in that form
(tests/q_record_oracle.py five_element_games) into tests/golden/trainer_records_q.json
(tests/golden/make_golden_trainer_q.py): the same planes / policies / values as from the two-element records, and as the
oracle's replay."""
import hashlib
import json
import os

import numpy as np

import q_record_oracle as qo
from oracle import xq_oracle as xo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)["games"]


def test_the_rewritten_records_carry_every_item_form():
    games = _load("engine_records.json")
    five = qo.five_element_games([g["data"] for g in games])
    items = [it for g in five for it in g[1:]]
    assert {len(it) for it in items} == {2, 5}
    assert any(it[4] is None for it in items if len(it) == 5) and any(it[4] is not None for it in items if len(it) == 5)
    assert {it[3] for it in items if len(it) == 5} == {0, 1}
    assert json.loads(json.dumps(five)) == five
    for g, d in zip(games, five):
        assert [it[:2] for it in d[1:]] == [list(it[:2]) for it in g["data"][1:]] and d[0] == g["data"][0]


def test_reference_trainer_parses_five_element_records():
    games = _load("engine_records.json")
    five = qo.five_element_games([g["data"] for g in games])
    ref = {r["game_id"]: r for r in _load("trainer_records_q.json")}
    plain = {r["game_id"]: r for r in _load("trainer_records.json")}
    assert sorted(ref) == sorted(g["game_id"] for g in games)
    assert ref == plain                                     # what the reference made of the two-element records
    for g, data in zip(games, five):
        r = ref[g["game_id"]]
        n = g["turns"]
        assert r["planes_shape"] == [n, 14, 10, 9] and r["policy_shape"] == [n, 2086] and r["value_shape"] == [n]
        planes = []
        state = data[0]
        for i, it in enumerate(data[1:]):
            planes.append(np.asarray(xo.state_to_planes(state), dtype=np.float32))
            assert r["policy_argmax"][i] == xo.label_of_str(it[0]) and r["policy_sum"][i] == 1
            assert r["value"][i] == it[1]
            state = xo.step(state, it[0])
        got = hashlib.sha256(np.ascontiguousarray(np.stack(planes), dtype=np.float32).tobytes()).hexdigest()
        assert got == r["planes_sha256"], g["game_id"]
