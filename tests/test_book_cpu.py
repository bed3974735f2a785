"""Start-position books on the host: the parser of cchess_alphazero/lib/book.py (both notations, every rejection class
with its line number), tools/make_book.py on the golden engine records, the command-line flags, the arena's per-position
table.  The rule checks of load_book run here on the C oracle (`rules=`: same names and semantics as the package's rule
kernels, which need the GPU -- tests/test_gpu_book.py runs load_book on those)."""
import importlib.util
import json
import os

import numpy as np
import pytest

from cchess_alphazero.environment.static_env import INIT_STATE, fen_to_state, fliped_state, state_to_array
from cchess_alphazero.lib import book as bk
from oracle import xq_oracle as xo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
MID = 'r1e1s1e1r/4m4/2k1c1k2/p1p1p1p1p/9/2P6/P3P1P1P/1CK1C1K2/9/R1EMSME1R'
FEN_B = 'rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C2C4/9/RNBAKABNR b - - 0 1'
FEN_W = 'r1bakabnr/9/1cn4c1/p1p1p1p1p/9/9/P1P1P1P1P/1C2C4/9/RNBAKABNR w - - 2 2'


def _write(tmp_path, text, name="book.txt"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def test_parser_reads_both_notations_and_comments(tmp_path):
    path = _write(tmp_path, f"# a book\n\n{MID}\n   {FEN_B}   # black to move\n{FEN_W}\n\n{INIT_STATE} # trailing\n")
    book = bk.load_book(path, rules=xo)
    assert book == [MID, fliped_state(fen_to_state(FEN_B)), fen_to_state(FEN_W), INIT_STATE]
    # the flipped position is in the mover's frame: black's pieces at the bottom, in upper case, one cannon centralised above
    assert book[1] == 'rkemsmekr/9/4c2c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9/RKEMSMEKR'
    assert book[1] == xo.fliped_state(fen_to_state(FEN_B))
    boards = bk.book_boards(book)
    assert boards.dtype == np.int8 and boards.shape == (4, 90)
    assert all(np.array_equal(boards[i], xo.state_to_board(s)) for i, s in enumerate(book))


def test_golden_book_file_is_the_book_of_the_golden_games():
    with open(os.path.join(GOLDEN, "book_games.json")) as f:
        gold = json.load(f)
    assert bk.load_book(os.path.join(GOLDEN, "book.txt"), rules=xo) == gold["book"]


ROW9 = "9/9/9/9/9/9/9/9"
REJECTS = [
    ("rows", "4s4/9/9/4S4", "rows"),
    ("short row", f"4s3/{ROW9}/4S4", "files"),
    ("long row", f"4s4/{ROW9}/4S5", "files"),
    ("letter", f"4s4/{ROW9[:-1]}x8/4S4", "unknown piece letter 'x'"),
    ("fen letter in a state string", f"4s4/{ROW9[:-1]}n8/4S4", "unknown piece letter 'n'"),
    ("state letter in a FEN", f"4k4/{ROW9[:-1]}m8/4K4 w", "unknown piece letter 'm'"),
    ("side", f"4k4/{ROW9[:-1]}r8/4K4 x", "side to move"),
    ("no king of the mover", f"4s4/{ROW9[:-1]}R8/9", "kings of the side to move"),
    ("two kings of the other side", f"3ss4/{ROW9[:-1]}R8/4S4", "kings of the other side"),
    ("no king in a FEN", f"9/{ROW9[:-1]}R8/4K4 b", "kings"),
    ("already over: the mover takes the king", f"4s4/{ROW9[:-1]}R8/4S4".replace("R8", "4R4"), "already over"),
    ("nothing can attack", f"3s5/4m4/{ROW9[2:]}/4S4", "attack"),
]


@pytest.mark.parametrize("name,line,needle", REJECTS, ids=[r[0] for r in REJECTS])
def test_every_rejection_names_file_and_line(tmp_path, name, line, needle):
    path = _write(tmp_path, f"# comment\n{MID}\n\n{line}\n{INIT_STATE}\n")
    with pytest.raises(ValueError) as e:
        bk.load_book(path, rules=xo)
    msg = str(e.value)
    assert msg.startswith(f"{path}:4: "), msg
    assert needle in msg, msg


MISPLACED = [
    # an elephant on a square no elephant reaches: its moves have no action label (the oracle's player dies on it)
    ("black elephant", "3s1e3/4m4/4e4/9/r8/6K2/9/4E3R/4M4/2E1S4", "elephant 'e' in row 1, file 6"),
    ("red elephant", "3s5/4m4/4e4/9/r8/6K2/9/3E4R/4M4/2E1S4", "elephant 'E' in row 8, file 4"),
    ("elephant across the river", "3s5/4m4/9/9/2E6/9/9/8R/4M4/4S4", "elephant 'E' in row 5, file 3"),
    ("red advisor", "3s5/4m4/9/9/9/9/9/8R/9/3SM4", "advisor 'M' in row 10, file 5"),
    ("black advisor", "3s5/3m5/9/9/9/9/9/8R/4M4/4S4", "advisor 'm' in row 2, file 4"),
    ("in a FEN", "3k1b3/9/9/9/9/9/9/8R/9/4K4 w", "elephant 'e' in row 1, file 6"),
]


@pytest.mark.parametrize("name,line,needle", MISPLACED, ids=[r[0] for r in MISPLACED])
def test_elephants_and_advisors_off_their_squares_are_refused(tmp_path, name, line, needle):
    """Refused by the parser, before any rule function sees the position."""
    path = _write(tmp_path, f"{MID}\n{line}\n")
    with pytest.raises(ValueError) as e:
        bk.load_book(path, rules=None)
    assert str(e.value).startswith(f"{path}:2: ") and needle in str(e.value), str(e.value)


def test_every_elephant_and_advisor_square_is_accepted(tmp_path):
    """All seven elephant squares and five advisor squares of both sides, and every position of the golden books."""
    lines = ["3s5/9/9/9/R8/2E3E2/9/E3E3E/9/2E1S1E2", "3s5/9/9/9/R8/9/9/3M1M3/4M4/3MSM3"]
    lines += [fliped_state(s) for s in lines]               # ... the same squares seen from the other side
    path = _write(tmp_path, "\n".join(lines) + "\n")
    assert bk.load_book(path, rules=None) == lines
    for name in ("book.txt", "endgame_book.txt"):
        assert bk.load_book(os.path.join(GOLDEN, name), rules=xo)


def test_empty_book_is_rejected(tmp_path):
    path = _write(tmp_path, "# nothing\n\n")
    with pytest.raises(ValueError, match="no position"):
        bk.load_book(path, rules=xo)


def _make_book_module():
    spec = importlib.util.spec_from_file_location("make_book", os.path.join(ROOT, "tools", "make_book.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("ply", [0, 3, 6])
def test_make_book_on_the_golden_engine_records(tmp_path, ply):
    mb = _make_book_module()
    with open(os.path.join(GOLDEN, "engine_records.json")) as f:
        games = [g["data"] for g in json.load(f)["games"]]
    # two record files as the worker writes them: games flat-concatenated
    files = []
    for k, part in enumerate((games[::2], games[1::2])):
        p = tmp_path / f"play_{k}.json"
        p.write_text(json.dumps([item for g in part for item in g]))
        files.append(str(p))
    out = str(tmp_path / "book.txt")
    mb.main(["--ply", str(ply), "--out", out] + files)
    book = bk.load_book(out, rules=xo)                     # valid, the rule checks included
    assert len(book) == len(set(book))
    # the oracle's replay of the records: the position after `ply` moves of every game that went on from it
    expect = []
    for g in games[::2] + games[1::2]:
        moves = [it[0] for it in g[1:]]
        if ply >= len(moves):
            continue
        state = g[0]
        for m in moves[:ply]:
            state = xo.step(state, m)
        if xo.done(state)[0]:
            continue                                        # (only the appended king capture follows)
        if state not in expect:
            expect.append(state)
    assert book == expect and (ply > 0 or book == [INIT_STATE])
    assert ply == 0 or len(book) > 1


def test_make_book_host_step_equals_the_oracle():
    mb = _make_book_module()
    rng = np.random.default_rng(3)
    state = INIT_STATE
    for _ in range(60):
        moves = xo.get_legal_moves(state)
        if xo.done(state)[0] or not moves:
            break
        mv = moves[int(rng.integers(len(moves)))]
        nxt, took = mb.host_step(state_to_array(state), mv)
        state = xo.step(state, mv)
        assert np.array_equal(nxt, xo.state_to_board(state)) and not took


def test_command_line_flags():
    from cchess_alphazero import manager
    p = manager.create_parser()
    cfg = manager.build_config(p.parse_args(["self", "--book", "b.txt", "--book-rate", "0.25"]))
    assert cfg.engine.book_path == "b.txt" and cfg.engine.book_rate == 0.25
    cfg = manager.build_config(p.parse_args(["eval", "--book", "openings.txt"]))
    assert cfg.engine.book_path == "openings.txt" and cfg.engine.book_rate == 1.0
    cfg = manager.build_config(p.parse_args(["self"]))
    assert cfg.engine.book_path is None and cfg.engine.book_rate == 1.0
    with pytest.raises(SystemExit):
        manager.build_config(p.parse_args(["self", "--book", "b.txt", "--book-rate", "1.5"]))


def test_arena_book_order_and_position_table():
    from cchess_alphazero.worker import evaluator as ev
    book = ["a", "b", "c"]
    assert ev.book_states(book, range(8)) == ["a", "a", "b", "b", "c", "c", "a", "a"]
    rng = np.random.default_rng(1)
    results = [(int(v), 10) for v in rng.integers(-1, 2, size=23)]
    rows = ev.position_table(results, 3)
    assert sum(r["games"] for r in rows) == 23
    total = ev.score_table(results)
    assert tuple(sum(r["table"][i] for r in rows) for i in range(7)) == total
    assert sum(r["score"] for r in rows) == total[0]
    for p, r in enumerate(rows):                            # each row is the score table of that position's games alone
        mine = [results[i] if (i // 2) % 3 == p else None for i in range(23)]
        t = [0.0, 0, 0, 0, 0, 0, 0]
        for i, g in enumerate(mine):
            if g is not None:
                one = ev.score_table([(0, 0)] * i + [g])
                pad = ev.score_table([(0, 0)] * i)
                t = [a + b - c for a, b, c in zip(t, one, pad)]
        assert tuple(t) == r["table"]
