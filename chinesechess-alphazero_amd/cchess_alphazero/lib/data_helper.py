"""Play-record files (reference: cchess_alphazero/lib/data_helper.py and SelfPlayWorker.save_play_data,
worker/self_play.py:214-251).  The format is what the reference's ``opt`` trainer reads:
one JSON list ``[init_state, [move, value], [move, value], ...]`` per file (``nb_game_in_file`` games are
concatenated into one flat list, as the reference does).

With ``engine.record_visits`` on, a searched move's item is ``[move, value, pi]``: pi = ``[[move, count], ...]``, the
root's visit counts when the move was chosen (see ``pi_from_visits``).  The reference's trainer reads only ``item[0]``
and ``item[1]`` (worker/optimize.py:245-246), so such files feed it unchanged.

With a playout cap the item of a fast ply is ``[move, value, pi or None, 0]``; with ``engine.record_q`` on every searched
ply's item is ``[move, value, pi or None, weight, q]``, with ``engine.record_surprise`` on
``[move, value, pi or None, weight, q or None, s]`` (``record_item``)."""
import json
import os
from datetime import datetime, timedelta, timezone
from glob import glob
from logging import getLogger

logger = getLogger(__name__)


def pi_from_visits(moves, n, banned, labels):
    """One searched ply's root (edge order: label indices, visit counts, banned flags) -> the record's pi, a list of
    ``[move, count]`` in edge order without banned edges and edges that have no visit.  count / sum(counts) is the
    policy calc_policy returns (agent/player.py:375-406: banned edges zeroed, then normalised).  labels: label index ->
    move string (ActionLabelsRed; the moves are in the mover's frame, like the record's moves)."""
    return [[labels[int(m)], int(c)] for m, c, b in zip(moves, n, banned) if not b and int(c) > 0]


def record_item(move, value, entry=None, fast=False, record_q=False, labels=None, record_surprise=False):
    """One ply's record item (engine.py drain).  entry: the ply's VisitEntry, or None where the ply has none to show (the
    appended king capture, a resignation, a game whose visit record is incomplete).
      [move, value]                          no entry, a full ply
      [move, value, pi]                      an entry (pi_from_visits)
      [move, value, pi or None, 0]           a fast ply of the playout cap: training weight 0
      [move, value, pi or None, weight, q]   record_q on and an entry: weight 1 on a full ply, 0 on a fast one;
                                             q = round(entry.q, 6), None where the root had no value
      [move, value, pi or None, weight, q or None, s]
                                             record_surprise on and an entry: weight as above, q None with record_q off,
                                             s = round(entry.s, 6), None where the root had no surprise
    Without an entry neither option changes anything, and with both off the items are what they were."""
    item = [move, value]
    if entry is not None:
        item.append(pi_from_visits(entry.moves, entry.n, entry.banned, labels))
    if fast:
        item += [None] * (3 - len(item)) + [0]
    if (record_q or record_surprise) and entry is not None:
        if not fast:
            item.append(1)
        item.append(None if not record_q or entry.q is None else round(float(entry.q), 6))
        if record_surprise:
            item.append(None if entry.s is None else round(float(entry.s), 6))
    return item


def mean_abs_q_minus_z(data):
    """(sum of |q - z|, count) over the items of one game's record list that carry a q (self-play's log line)."""
    d = [abs(it[4] - it[1]) for it in data[1:] if len(it) >= 5 and it[4] is not None]
    return sum(d), len(d)


def surprise_sums(data):
    """(sum of s over full plies, their count, sum over fast plies, their count) over the items of one game's record list
    that carry a policy surprise (self-play's log line); a fast ply is one with training weight 0."""
    full = [it[5] for it in data[1:] if len(it) >= 6 and it[5] is not None and it[3] != 0]
    fast = [it[5] for it in data[1:] if len(it) >= 6 and it[5] is not None and it[3] == 0]
    return sum(full), len(full), sum(fast), len(fast)


def get_game_data_filenames(rc):
    pattern = os.path.join(rc.play_data_dir, rc.play_data_filename_tmpl % "*")
    return list(sorted(glob(pattern)))


def write_game_data_to_file(path, data):
    with open(path, "wt") as f:
        json.dump(data, f)


def read_game_data_from_file(path):
    with open(path, "rt") as f:
        return json.load(f)


class PlayDataWriter:
    """Buffers finished games and writes ``play_<Beijing time>.json`` files (self_play.py:214-232);
    keeps at most ``play_data.max_file_num`` files (self_play.py:243-251)."""

    def __init__(self, config, rank=0, world=1):
        self.config = config
        self.rank, self.world = rank, world
        self.buffer = []
        self.idx = 1
        self._last_stamp = None
        self.files_written = 0
        os.makedirs(config.resource.play_data_dir, exist_ok=True)

    def _game_id(self):
        bj = datetime.utcnow().replace(tzinfo=timezone.utc).astimezone(timezone(timedelta(hours=8)))
        if self._last_stamp is not None and bj <= self._last_stamp:
            bj = self._last_stamp + timedelta(microseconds=1)
        self._last_stamp = bj
        s = bj.strftime("%Y%m%d-%H%M%S.%f")
        return s if self.world == 1 else f"{s}-r{self.rank}"

    def add_game(self, data):
        """data: [init_state, [move, value], ...] of one stored game (items may carry pi: [move, value, pi])."""
        self.buffer += data
        idx, self.idx = self.idx, self.idx + 1
        if idx % self.config.play_data.nb_game_in_file != 0:
            return None
        rc = self.config.resource
        path = os.path.join(rc.play_data_dir, rc.play_data_filename_tmpl % self._game_id())
        write_game_data_to_file(path, self.buffer)
        self.buffer = []
        self.files_written += 1
        self.remove_play_data()
        return path

    def remove_play_data(self):
        files = get_game_data_filenames(self.config.resource)
        extra = len(files) - self.config.play_data.max_file_num
        for f in files[:max(0, extra)]:
            try:
                os.remove(f)
            except OSError:
                pass
