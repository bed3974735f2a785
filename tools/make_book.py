#!/usr/bin/env python3
"""Writes a start-position book (run.py self / eval --book FILE) from play-record files: the position after ply N of
every stored game, in the mover's frame, deduplicated, in first-seen order.

    python tools/make_book.py --ply 8 --out book.txt data/play_data/play_*.json

A record is ``[first state, [move, value(, pi)], ...]`` (a file may hold several games flat-concatenated); its moves and
states are in the frame of the side to move, so replaying is a host-side board update and a flip per ply -- no GPU is
needed.  Only positions that the game itself went on from are taken: a game shorter than N + 1 plies gives none, and
neither does the position before an appended king capture (there the game was already over).  Such positions passed the
engine's own `done` / `has_attack_chessman` tests when they were played, so the book is valid under
cchess_alphazero.lib.book.load_book.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "chinesechess-alphazero_amd"))

from cchess_alphazero.environment.static_env import array_to_state, state_to_array  # noqa: E402
from cchess_alphazero.lib.book import parse_position  # noqa: E402
from cchess_alphazero.lib.record_decoder import split_games  # noqa: E402

KING = 7


def host_step(board, move):
    """One ply on the int8[90] board (square y * 9 + x, mover at the bottom): move 'x0y0x1y1', then the flip into the
    next mover's frame (static_env.step).  Returns (next board, the move took a king)."""
    f = int(move[1]) * 9 + int(move[0])
    t = int(move[3]) * 9 + int(move[2])
    if board[f] <= 0:
        raise ValueError(f"no piece of the mover on the source square of {move}")
    took_king = board[t] == -KING
    nxt = board.copy()
    nxt[t] = nxt[f]
    nxt[f] = 0
    return -nxt[::-1], took_king


def position_after(game, ply):
    """The state after `ply` moves of the record `game`, or None when the game did not go on from there."""
    moves = [item[0] for item in game[1:]]
    if ply >= len(moves):
        return None
    board = state_to_array(game[0])
    for i in range(ply):
        board, _ = host_step(board, moves[i])
    _, took_king = host_step(board, moves[ply])
    if took_king:                     # the appended king capture: the game was over in this position
        return None
    return array_to_state(board)


def make_book(paths, ply):
    seen, book = set(), []
    for path in paths:
        with open(path) as f:
            data = json.load(f)
        for game in split_games(data):
            state = position_after(game, ply)
            if state is not None and state not in seen:
                parse_position(state)                     # form and kings, as load_book checks them
                seen.add(state)
                book.append(state)
    return book


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("records", nargs="+", help="play-record JSON files")
    ap.add_argument("--ply", type=int, default=8, help="take the position after this many plies (default 8)")
    ap.add_argument("--out", required=True, help="book file to write")
    args = ap.parse_args(argv)
    if args.ply < 0:
        ap.error("--ply must be >= 0")
    book = make_book(args.records, args.ply)
    if not book:
        raise SystemExit(f"no game of {len(args.records)} file(s) goes on after ply {args.ply}: no book written")
    with open(args.out, "w") as f:
        f.write(f"# positions after ply {args.ply} of {len(args.records)} play-record file(s), side to move at the bottom\n")
        f.write("\n".join(book) + "\n")
    print(f"{args.out}: {len(book)} positions")


if __name__ == "__main__":
    main()
