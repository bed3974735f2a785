"""Stored games as scripts for the search (``run.py reanalyse``, worker/reanalyse.py): MuZero's Reanalyse.  No torch, no
device.

A record file is what lib/data_helper.py describes: one flat JSON list, a game at every string item, its items from
``[move, value]`` (the reference's own records, and everything written before ``--record-visits``) up to
``[move, value, pi, weight, q, s]``.  Whatever the form, a game reduces to its start position, its moves and its result z:
that is a SCRIPT.  ``pack_scripts`` lays scripts out as ``cz_replay_games`` takes games (init_boards [n, 90], labels flat,
offsets [n + 1]) plus z [n], which is what ``Search.set_script`` / ``SelfPlayEngine(script=...)`` take; the engine walks
script i as game id i and ``rewrite_game`` puts the targets of that walk (pi, weight, q, s) beside the source's own moves
and values."""
from collections import namedtuple

import numpy as np

from cchess_alphazero.environment.lookup_tables import label_index
from cchess_alphazero.environment.static_env import state_to_array
from cchess_alphazero.lib.data_helper import read_game_data_from_file
from cchess_alphazero.lib.record_decoder import split_games

# what set_script takes, in its order: int8 [n, 90], uint16 [offsets[n]], int32 [n + 1], int8 [n]
Scripts = namedtuple("Scripts", "init_boards labels offsets z")
# where a packed script came from: index into the list of files (or whatever the caller numbers), game index in that file
Source = namedtuple("Source", "file game")


def load_games(path):
    """The games of one record file, each ``[init_state, item, ...]``."""
    return split_games(read_game_data_from_file(path))


def game_z(game):
    """The game's result from its first mover's view, -1 / 0 / 1: the sign of the first item's value (the values alternate
    from there, lib/data_helper.py).  0 for a game without items."""
    if len(game) < 2:
        return 0
    v = float(game[1][1])
    return (v > 0) - (v < 0)


def game_labels(game):
    """The game's moves as label indices, whatever form its items have."""
    return [label_index(item[0]) for item in game[1:]]


def pack_scripts(games, max_len, sources=None):
    """games: record games; max_len: the longest script the engine's record holds, its max_plies + 1.  Returns (scripts,
    kept, aside): `scripts` the Scripts of the games that are neither empty nor longer than max_len and start with one king a
    side, in order; `kept` their
    sources (sources[i] of game i; default Source(0, i)); `aside` [(source, reason)] of the others."""
    if sources is None:
        sources = [Source(0, i) for i in range(len(games))]
    kept, aside, boards, labels, offsets, z = [], [], [], [], [0], []
    for game, src in zip(games, sources):
        n = len(game) - 1
        if n < 1 or n > max_len:
            aside.append((src, "empty" if n < 1 else f"{n} plies, more than {max_len}"))
            continue
        if game[0].count("S") != 1 or game[0].count("s") != 1:      # (the search vouches for nothing on such a board)
            aside.append((src, "a start position without one king a side"))
            continue
        kept.append(src)
        boards.append(state_to_array(game[0]))
        labels += game_labels(game)
        offsets.append(len(labels))
        z.append(game_z(game))
    scripts = Scripts(np.ascontiguousarray(np.stack(boards), dtype=np.int8) if boards else np.zeros((0, 90), np.int8),
                      np.asarray(labels, dtype=np.uint16), np.asarray(offsets, dtype=np.int32), np.asarray(z, dtype=np.int8))
    return scripts, kept, aside


def script_of(scripts, i):
    """(init board int8 [90], labels uint16 [plies], z) of packed script i."""
    return scripts.init_boards[i], scripts.labels[scripts.offsets[i]:scripts.offsets[i + 1]], int(scripts.z[i])


def rewrite_game(source, data):
    """source: the record game that was the script; data: the drained game's record list (engine.py drain: element 0, then one
    item per move).  Returns the output game: the source's start position, and per move the source's own move and value
    followed by what this walk recorded for the ply (pi, weight, q, s: the tail of the drained item, lib/data_helper.py
    record_item).  ValueError when the two do not hold the same moves."""
    if len(data) != len(source) or any(a[0] != b[0] for a, b in zip(source[1:], data[1:])):
        raise ValueError("the drained game does not hold the script's moves")
    return [source[0]] + [[s[0], s[1]] + list(d[2:]) for s, d in zip(source[1:], data[1:])]


def batches(plies_per_file, ply_budget):
    """Consecutive files into batches: as many whole files as fit `ply_budget` plies, at least one.  plies_per_file: the
    plies of each file, in order.  Returns [(first, last + 1), ...]."""
    out, first, used = [], 0, 0
    for i, n in enumerate(plies_per_file):
        if i > first and used + n > ply_budget:
            out.append((first, i))
            first, used = i, 0
        used += n
    if first < len(plies_per_file):
        out.append((first, len(plies_per_file)))
    return out
