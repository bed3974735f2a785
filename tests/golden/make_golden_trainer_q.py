"""Reference side of tests/test_q_record_roundtrip.py: the reference's expanding_data (worker/optimize.py:234-281) applied
to the engine records of engine_records.json REWRITTEN with five-element items (tests/q_record_oracle.py
five_element_games: [move, value, pi or None, weight, q]).  Output: trainer_records_q.json, the fields of
trainer_records.json.

    python tests/golden/make_golden_trainer_q.py      (where the reference checkout is present)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "chinesechess-alphazero_amd"))
from q_record_oracle import five_element_games  # noqa: E402

games5 = None


def main():
    global games5
    with open(os.path.join(HERE, "engine_records.json")) as f:
        games = json.load(f)["games"]
    games5 = five_element_games([g["data"] for g in games])      # (with this package's modules, before the reference's)
    for name in [n for n in sys.modules if n == "cchess_alphazero" or n.startswith("cchess_alphazero.")]:
        del sys.modules[name]
    sys.path.pop(0)
    sys.path.pop(0)
    sys.path.insert(0, HERE)
    import make_golden_trainer as ref                            # mocks keras, imports the REFERENCE's optimize
    out = []
    for g, data in zip(games, games5):
        planes, policy, value = ref.opt.expanding_data(data)
        out.append({"game_id": g["game_id"], "planes_shape": list(planes.shape), "policy_shape": list(policy.shape),
                    "value_shape": list(value.shape), "planes_sha256": ref.planes_digest(planes),
                    "policy_argmax": [int(x) for x in policy.argmax(1)], "policy_sum": [float(x) for x in policy.sum(1)],
                    "value": [float(x) for x in value]})
    with open(os.path.join(HERE, "trainer_records_q.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_trainer_q.py",
                   "reference": "worker/optimize.py expanding_data on engine_records.json with five-element items",
                   "games": out}, f)
        f.write("\n")
    print("games", len(out))


if __name__ == "__main__":
    main()
