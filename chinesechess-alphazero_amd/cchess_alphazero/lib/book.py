"""Start-position books: self-play (``run.py self --book FILE``) and arena (``run.py eval --book FILE``) games that start
from given positions instead of the opening position.

A book file holds one position per line; blank lines and ``#`` comments are ignored.  A line is either the package's
state string (the side to move at the bottom, in upper case -- environment/static_env.py) or a FEN with its side to move
(``... w`` / ``... b``; further FEN fields are ignored).  A position with black to move is turned into the mover's frame
(``fliped_state``), exactly as ``uci.py`` does for ``position fen ... b``: every game of the engine is played -- and
recorded -- in the frame of the side that moves first, which takes the part of "red".

``load_book`` checks every position before anything is used: ten rows of nine files, known piece letters, exactly one
king per side, elephants and advisors on squares they can reach (a move from any other has no action label), and, with
the package's own rule functions, that the game is not already over (``done``) and that a side can still attack
(``has_attack_chessman``).  Those two run on the GPU like every rule of the package; ``rules`` takes any other object
with the two functions (the tests pass the C oracle, a tool may pass ``None`` to check the form alone).
"""
import numpy as np

from cchess_alphazero.environment.static_env import array_to_state, fen_to_state, fliped_state, state_to_array

BOOK_MAX = (1 << 24) - 2          # include/czero.h CZ_BOOK_MAX: what the record's 24-bit start-position field can name
_STATE_LETTERS = "pcrkemsPCRKEMS"
_FEN_LETTERS = "pcrnbakPCRNBAK"


class _PackageRules:
    """done / has_attack_chessman of environment/static_env.py, one launch each for the whole book."""

    @staticmethod
    def check(states):
        from cchess_alphazero.environment import static_env as senv
        over = [d[0] for d in senv.done_batch(states)]
        from cchess_alphazero import _native
        attack = _native.has_attack(senv._to_device(states)).cpu().numpy()
        return over, [bool(a) for a in attack]


def _check_form(text, letters):
    """Ten rows of nine files in known letters; returns an error text or None."""
    rows = text.split("/")
    if len(rows) != 10:
        return f"{len(rows)} rows, expected 10"
    for r, row in enumerate(rows):
        width = 0
        for ch in row:
            if "1" <= ch <= "9":
                width += int(ch)
            elif ch in letters:
                width += 1
            else:
                return f"unknown piece letter {ch!r} in row {r + 1}"
        if width != 9:
            return f"row {r + 1} has {width} files, expected 9"
    return None


def parse_position(line):
    """One book line (comment already removed) -> state string in the mover's frame.  ValueError on a malformed line."""
    parts = line.split()
    if len(parts) == 1:
        err = _check_form(parts[0], _STATE_LETTERS)
        if err:
            raise ValueError(err)
        state = parts[0]
    else:
        if parts[1] not in ("w", "b"):
            raise ValueError(f"side to move {parts[1]!r}, expected 'w' or 'b'")
        err = _check_form(parts[0], _FEN_LETTERS)
        if err:
            raise ValueError(err)
        state = fen_to_state(parts[0])
        if parts[1] == "b":
            state = fliped_state(state)
    for king, side in (("S", "the side to move"), ("s", "the other side")):
        if state.count(king) != 1:
            raise ValueError(f"{state.count(king)} kings of {side}, expected exactly one")
    err = _check_squares(state)
    if err:
        raise ValueError(err)
    return array_to_state(state_to_array(state))          # (canonical form: digits merged)


# (file, rank) from the owner's own back rank: the only squares an elephant / an advisor ever stands on.  Their moves
# from anywhere else have no action label, which the search indexes the policy with.
_ELEPHANT_SQUARES = {(2, 0), (6, 0), (0, 2), (4, 2), (8, 2), (2, 4), (6, 4)}
_ADVISOR_SQUARES = {(3, 0), (5, 0), (4, 1), (3, 2), (5, 2)}


def _check_squares(state):
    """Elephants and advisors stand on squares of their own; returns an error text or None."""
    for r, row in enumerate(state.split("/")):
        x = 0
        for ch in row:
            if ch.isdigit():
                x += int(ch)
                continue
            squares = {"e": _ELEPHANT_SQUARES, "m": _ADVISOR_SQUARES}.get(ch.lower())
            rank = 9 - r if ch.isupper() else r           # (row 1 of the string is the other side's back rank)
            if squares is not None and (x, rank) not in squares:
                name = "elephant" if ch.lower() == "e" else "advisor"
                return f"{name} {ch!r} in row {r + 1}, file {x + 1}: no {name} can reach that square"
            x += 1
    return None


def load_book(path, rules=_PackageRules):
    """The positions of the book file `path`, as state strings in the mover's frame, in file order.  Any invalid line
    raises ValueError naming file and line; nothing is returned then.  rules: object with done(state) and
    has_attack_chessman(state) (default: the package's rule kernels, batched), or None to skip those two checks."""
    states, lines = [], []
    with open(path) as f:
        for no, raw in enumerate(f, 1):
            line = raw.split("#", 1)[0].strip()
            if not line:
                continue
            try:
                states.append(parse_position(line))
            except ValueError as e:
                raise ValueError(f"{path}:{no}: {e}") from None
            lines.append(no)
    if not states:
        raise ValueError(f"{path}: no position in the book")
    if len(states) > BOOK_MAX:
        raise ValueError(f"{path}: {len(states)} positions, a book holds at most {BOOK_MAX}")
    if rules is not None:
        if hasattr(rules, "check"):
            over, attack = rules.check(states)
        else:
            over = [rules.done(s)[0] for s in states]
            attack = [rules.has_attack_chessman(s) for s in states]
        for s, no, o, a in zip(states, lines, over, attack):
            if o:
                raise ValueError(f"{path}:{no}: the game is already over in this position (done): {s}")
            if not a:
                raise ValueError(f"{path}:{no}: neither side has a piece that can attack (has_attack_chessman): {s}")
    return states


def book_boards(states):
    """States in the mover's frame -> int8 [n, 90] boards (what cz_search_set_book takes)."""
    return np.ascontiguousarray(np.stack([state_to_array(s) for s in states]), dtype=np.int8)
