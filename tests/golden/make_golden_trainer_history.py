"""Reference side of the history-mode tests of tests/test_gpu_trainer.py: the reference's own trainer input path with
use_history=True, expanding_data(data, True) (worker/optimize.py:234-281: 28 planes, the last 14 from history[-5], the
position two plies back), applied to every engine record of engine_records.json.  Output: trainer_records_history.json
-- per game the shapes, a digest of the planes (float32 bytes), the policy rows' argmax and the values.

    python tests/golden/make_golden_trainer_history.py      (where the reference checkout is present)
"""
import hashlib
import json
import os
import sys
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from live_reference_check import REF  # noqa: E402  (where the reference checkout lives)

sys.path[:0] = [REF, os.path.join(REF, "cchess_alphazero")]
for name in ("tensorflow", "keras", "keras.engine", "keras.engine.topology", "keras.engine.training",
             "keras.layers", "keras.layers.convolutional", "keras.layers.core", "keras.layers.merge",
             "keras.layers.normalization", "keras.regularizers", "keras.backend", "keras.models",
             "keras.optimizers", "keras.callbacks", "keras.utils", "keras.utils.training_utils"):
    sys.modules.setdefault(name, MagicMock())
import cchess_alphazero.worker.optimize as opt  # noqa: E402  (the REFERENCE's)


def planes_digest(planes):
    return hashlib.sha256(np.ascontiguousarray(planes, dtype=np.float32).tobytes()).hexdigest()


def main():
    with open(os.path.join(HERE, "engine_records.json")) as f:
        games = json.load(f)["games"]
    out = []
    for g in games:
        planes, policy, value = opt.expanding_data(g["data"], use_history=True)
        out.append({"game_id": g["game_id"], "planes_shape": list(planes.shape), "planes_sha256": planes_digest(planes),
                    "policy_argmax": [int(x) for x in policy.argmax(1)], "value": [float(x) for x in value]})
    with open(os.path.join(HERE, "trainer_records_history.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_trainer_history.py",
                   "reference": "worker/optimize.py expanding_data(data, use_history=True) on engine_records.json",
                   "games": out}, f)
        f.write("\n")
    print("games", len(out))


if __name__ == "__main__":
    main()
