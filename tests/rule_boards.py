"""Seeded board families for the rule kernels' tests (test_rule_boards_cpu.py, test_gpu_rules_paths.py).  NumPy and the oracle
only; every function returns read-only int8 [n, 90] arrays (y = 0 first, the mover's pieces positive) and is deterministic.

The rule kernels are defined on PLACEMENT-LEGAL boards with at most 128 moves per side ("The domain of the rule
kernels"): every piece stands on a square its type can stand on.  In the mover's frame: the king in the palace (x 3..5, y 0..2),
advisors on its 5 points, elephants on their 7 points, pawns on files 0/2/4/6/8 at y 3..4 or anywhere at y >= 5, rooks, knights
and cannons anywhere; the opponent's pieces on the same squares rotated by s -> 89 - s.  Which side has how many pieces of a type
is NOT part of the domain (overfull()).  A board whose raw oracle move count (xqo_legal_moves: it counts past 128 and stores 128)
exceeds 128 for the mover or for the flipped board is dropped here, so that no test can send one to a device: a MoveList holds
128 entries.  dropped(family, seed, n) tells how many that were."""
import ctypes as C
import functools

import numpy as np

from oracle import xq_oracle as xo

PAWN, CANNON, ROOK, KNIGHT, ELEPHANT, ADVISOR, KING = 1, 2, 3, 4, 5, 6, 7
MAXMOVES = xo.MAXMOVES


def _sq(x, y):
    return 9 * y + x


def _mask(squares):
    m = np.zeros(90, dtype=bool)
    m[[_sq(x, y) for x, y in squares]] = True
    return m


# the squares a mover's piece of each type can stand on
ALLOWED = {
    KING: _mask([(x, y) for x in (3, 4, 5) for y in (0, 1, 2)]),
    ADVISOR: _mask([(3, 0), (5, 0), (4, 1), (3, 2), (5, 2)]),
    ELEPHANT: _mask([(2, 0), (6, 0), (0, 2), (4, 2), (8, 2), (2, 4), (6, 4)]),
    PAWN: _mask([(x, y) for x in (0, 2, 4, 6, 8) for y in (3, 4)] + [(x, y) for x in range(9) for y in range(5, 10)]),
    ROOK: np.ones(90, dtype=bool),
    KNIGHT: np.ones(90, dtype=bool),
    CANNON: np.ones(90, dtype=bool),
}
# placement order (each type for both sides in turn): the types with the fewest squares first, so that no rook takes the last
# palace square before the king is there
ORDER = (KING, ADVISOR, ELEPHANT, PAWN, ROOK, KNIGHT, CANNON)
REAL_COUNTS = {ADVISOR: 2, ELEPHANT: 2, PAWN: 5, ROOK: 2, KNIGHT: 2, CANNON: 2}
OVERFULL_COUNTS = {ADVISOR: 5, ELEPHANT: 7, PAWN: 30, ROOK: 14, KNIGHT: 14, CANNON: 14}


def placement_legal(boards):
    """bool [n]: every piece of every board on a square its type can stand on"""
    boards = np.asarray(boards, dtype=np.int8).reshape(-1, 90)
    ok = np.ones(len(boards), dtype=bool)
    for t, m in ALLOWED.items():
        ok &= ~((boards == t) & ~m).any(axis=1)
        ok &= ~((boards == -t) & ~m[::-1]).any(axis=1)
    return ok


def raw_counts(boards):
    """int32 [n]: the oracle's move count of each board, counted past 128 (legal_moves_board asserts there)"""
    boards = np.ascontiguousarray(boards, dtype=np.int8).reshape(-1, 90)
    L = xo.lib()
    buf = np.zeros(MAXMOVES, dtype=np.uint16)
    bp = buf.ctypes.data_as(C.POINTER(C.c_uint16))
    out = np.zeros(len(boards), dtype=np.int32)
    for i, b in enumerate(boards):
        out[i] = L.xqo_legal_moves(b.ctypes.data_as(C.POINTER(C.c_int8)), bp)
    return out


def flipped(boards):
    """fliped_state on arrays: out[89 - s] = -in[s]"""
    return np.ascontiguousarray(-np.asarray(boards, dtype=np.int8).reshape(-1, 90)[:, ::-1])


def in_domain(boards):
    """bool [n]: placement-legal and at most 128 moves for the mover and for the flipped board"""
    return placement_legal(boards) & (raw_counts(boards) <= MAXMOVES) & (raw_counts(flipped(boards)) <= MAXMOVES)


def _place(rng, boards, allowed, piece, k):
    """put k[i] pieces on random free allowed squares of board i (fewer where the squares run out)"""
    n = len(boards)
    keys = rng.random((n, 90))
    keys[~(allowed[None, :] & (boards == 0))] = 2.0
    order = np.argsort(keys, axis=1, kind="stable")
    rows = np.arange(n)
    for j in range(int(k.max(initial=0))):
        sq = order[:, j]
        ok = (j < k) & (keys[rows, sq] < 2.0)
        boards[rows[ok], sq[ok]] = piece
    return boards


@functools.lru_cache(maxsize=None)
def _family(seed, n, overfull_):
    rng = np.random.default_rng(seed)
    caps = OVERFULL_COUNTS if overfull_ else REAL_COUNTS
    boards = np.zeros((n, 90), dtype=np.int8)
    for t in ORDER:
        for sign in (1, -1):
            k = np.ones(n, dtype=np.int64) if t == KING else rng.integers(0, caps[t] + 1, size=n)
            if not overfull_ and t in (ROOK, KNIGHT, CANNON):      # the larger of two draws: more boards with long lists
                k = np.maximum(k, rng.integers(0, caps[t] + 1, size=n))
            _place(rng, boards, ALLOWED[t] if sign > 0 else ALLOWED[t][::-1], sign * t, k)
    keep = in_domain(boards)
    out = np.ascontiguousarray(boards[keep])
    out.setflags(write=False)
    return out, int(n - keep.sum())


def legal_placement(seed, n):
    """n placement-legal boards with the piece counts of a game (one king per side; at most 2 advisors, 2 elephants, 5 pawns,
    2 rooks, 2 knights, 2 cannons), less those with more than 128 moves for either side"""
    return _family(int(seed), int(n), False)[0]


def overfull(seed, n):
    """the same squares with up to 5 advisors, 7 elephants, 30 pawns and 14 rooks, knights and cannons per side: more than 24
    pieces of the mover or more than 9 of one type take the lane form's generic generator (xq_tpb.h::tpb_movegen)"""
    return _family(int(seed), int(n), True)[0]


def dropped(family, seed, n):
    """how many of the n generated boards of legal_placement / overfull had more than 128 moves for either side"""
    return _family(int(seed), int(n), family is overfull)[1]


def takes_generic_path(boards):
    """bool [n]: the mover has more than 24 pieces or more than 9 of one type (the fallback condition of tpb_movegen)"""
    boards = np.asarray(boards).reshape(-1, 90)
    many = (boards > 0).sum(axis=1) > 24
    of_one = np.stack([(boards == t).sum(axis=1) for t in range(1, 8)]).max(axis=0) > 9
    return many, of_one


def with_move_count(boards, counts=(63, 64, 65, 66)):
    """{count: the boards of the family with exactly that many oracle moves, in the family's order}"""
    boards = np.asarray(boards).reshape(-1, 90)
    c = raw_counts(boards)
    return {k: boards[c == k] for k in counts}


# ---- written-out boards --------------------------------------------------------------------------------------------------
def _board(*pieces):
    """pieces: (type, x, y), type > 0 the mover's"""
    b = np.zeros(90, dtype=np.int8)
    for t, x, y in pieces:
        assert b[_sq(x, y)] == 0
        b[_sq(x, y)] = t
    return b


LONG_STATES = ('3s5/9/9/2K3K2/R7R/1C5C1/P1P1P1P1P/9/9/4S4', '4s4/9/4P4/R7R/1C2K2C1/2K6/P1P3P1P/9/9/4S4')
_K, _k = (KING, 4, 0), (-KING, 5, 9)          # kings on different files: nothing is decided by them


@functools.lru_cache(maxsize=None)
def _directed():
    named = [
        ("empty", _board()),
        ("mover without a king", _board((-KING, 4, 9), (ROOK, 0, 0), (-PAWN, 4, 3))),
        ("opponent without a king", _board((KING, 4, 0), (-ROOK, 0, 9), (CANNON, 1, 2))),
        ("neither king", _board((ROOK, 0, 0), (-ROOK, 8, 9))),
        ("bare king of the mover", _board((KING, 4, 1))),
        ("kings facing, 0 blockers", _board((KING, 4, 0), (-KING, 4, 9))),
        ("kings facing, 1 blocker", _board((KING, 4, 0), (-KING, 4, 9), (PAWN, 4, 5))),
        ("kings facing, 2 blockers", _board((KING, 4, 0), (-KING, 4, 9), (PAWN, 4, 5), (-PAWN, 4, 4))),
        ("kings facing, the only blocker beside the opponent's king", _board((KING, 4, 0), (-KING, 4, 9), (-ADVISOR, 4, 8))),
        ("kings facing, the only blocker beside the mover's king", _board((KING, 4, 0), (-KING, 4, 9), (ADVISOR, 4, 1))),
        ("kings facing on file 3, a rook behind", _board((KING, 3, 2), (-KING, 3, 7), (-ROOK, 3, 8))),
        ("kings facing, blocker beside the file only", _board((KING, 5, 1), (-KING, 5, 8), (ROOK, 4, 4), (-ROOK, 6, 5))),
        ("kings on different files", _board((KING, 3, 0), (-KING, 5, 9))),
        ("cannon over a screen on file 0", _board(_K, _k, (CANNON, 0, 0), (PAWN, 0, 3), (-ROOK, 0, 7))),
        ("cannon over a screen on file 8", _board(_K, _k, (CANNON, 8, 2), (-KNIGHT, 8, 5), (-ROOK, 8, 9))),
        ("cannon with its screens on the edge files", _board(_K, _k, (CANNON, 4, 5), (ROOK, 0, 5), (-ROOK, 8, 5))),
        ("cannon with its screens on the edge ranks", _board(_K, _k, (CANNON, 1, 4), (KNIGHT, 1, 0), (-KNIGHT, 1, 9))),
        ("knight, leg (4,3) blocked", _board(_K, _k, (KNIGHT, 4, 4), (PAWN, 4, 3))),
        ("knight, leg (5,4) blocked", _board(_K, _k, (KNIGHT, 4, 4), (-PAWN, 5, 4))),
        ("knight, leg (4,5) blocked", _board(_K, _k, (KNIGHT, 4, 4), (-CANNON, 4, 5))),
        ("knight, leg (3,4) blocked", _board(_K, _k, (KNIGHT, 4, 4), (ROOK, 3, 4))),
        ("knight in the corner", _board(_K, _k, (KNIGHT, 0, 0), (KNIGHT, 8, 9))),
        ("elephant, one eye blocked", _board(_K, _k, (ELEPHANT, 2, 0), (ROOK, 3, 1))),
        ("elephant at the river", _board(_K, _k, (ELEPHANT, 2, 4), (ELEPHANT, 6, 4), (-PAWN, 5, 3))),
        ("pawn on the last rank, x = 0", _board(_K, _k, (PAWN, 0, 9))),
        ("pawn on the last rank, x = 4: takes the king sideways", _board(_K, _k, (PAWN, 4, 9))),
        ("pawn on the last rank, x = 8", _board(_K, _k, (PAWN, 8, 9), (-ROOK, 7, 9))),
        ("pawn before and after the river", _board(_K, _k, (PAWN, 2, 4), (PAWN, 6, 5), (-PAWN, 2, 5), (-PAWN, 6, 4))),
        # two pieces take the king: the knight on the lower square is first in the list, the rook is generated first by the
        # lane form (one loop per type, rooks before knights)
        ("king taken by the later type first", _board(_K, (-KING, 4, 9), (PAWN, 4, 3), (KNIGHT, 3, 7), (ROOK, 4, 8))),
        # the rook on (4,8) comes first in the opponent's list and stops at its own cannon; the only move that lands on the
        # king's square is the cannon's, over the pawn
        ("in check by the cannon in front of a blocked rook", _board(_K, _k, (-ROOK, 4, 8), (-CANNON, 4, 6), (PAWN, 4, 3))),
        ("not in check: two screens before the cannon", _board(_K, _k, (-CANNON, 4, 8), (PAWN, 4, 3), (PAWN, 4, 5))),
        ("in check by a pawn beside the king", _board((KING, 4, 1), _k, (-PAWN, 3, 1))),
    ]
    named += [("long list %d" % i, xo.state_to_board(s)) for i, s in enumerate(LONG_STATES)]
    boards = np.stack([b for _, b in named])
    assert in_domain(boards).all(), [n for (n, _), ok in zip(named, in_domain(boards)) if not ok]
    boards.setflags(write=False)
    return tuple(n for n, _ in named), boards


def directed():
    """the written-out boards (directed_names() names them in the same order)"""
    return _directed()[1]


def directed_names():
    return _directed()[0]
