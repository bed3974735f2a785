"""The positions of the legal-mask tests (test_policy_mask_cpu.py, test_gpu_policy_mask.py): one-ply games from boards whose move
lists straddle the 64 entries a lane pass marks, from the shortest lists of the family and from the two longest written-out
positions.  NumPy and the oracle only."""
import functools

import numpy as np

import rule_boards
from oracle import xq_oracle as xo

CLASSES = ("63", "64", "65", "66", "short", "long")
EXPECTED = {"63": 26, "64": 15, "65": 11, "66": 7, "short": 2, "long": 2}


@functools.lru_cache(maxsize=None)
def class_boards():
    """{class: int8 [n, 90]}: the boards of rule_boards.legal_placement(5, 4096) with exactly 63, 64, 65 and 66 moves, the two
    with fewer than 8, and rule_boards.LONG_STATES (74 and 68 moves)"""
    fam = rule_boards.legal_placement(5, 4096)
    out = {str(k): v for k, v in rule_boards.with_move_count(fam).items()}
    out["short"] = fam[rule_boards.raw_counts(fam) < 8]
    out["long"] = np.stack([xo.state_to_board(s) for s in rule_boards.LONG_STATES])
    return out


def one_ply_games(seed=0):
    """-> (games, classes): games [state, [a legal move, z]] of every board of class_boards(), and each game's class"""
    rng = np.random.default_rng(seed)
    games, classes = [], []
    for name in CLASSES:
        for b in class_boards()[name]:
            state = xo.board_to_state(b)
            moves = xo.get_legal_moves(state)
            games.append([state, [moves[int(rng.integers(len(moves)))], int(rng.integers(-1, 2))]])
            classes.append(name)
    return games, classes


def legal_mask_of_states(states):
    """bool [n, 2086] from the oracle's move lists"""
    lab = {m: i for i, m in enumerate(xo.labels())}
    out = np.zeros((len(states), len(lab)), dtype=bool)
    for r, s in enumerate(states):
        out[r, [lab[m] for m in xo.get_legal_moves(s)]] = True
    return out


def mirror_board(b):
    """file x -> 8 - x"""
    return np.ascontiguousarray(np.asarray(b, dtype=np.int8).reshape(10, 9)[:, ::-1]).reshape(90)
