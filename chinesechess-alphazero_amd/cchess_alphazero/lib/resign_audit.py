"""Resignation audit (run.py self --resign-audit; NumPy only, no device).

Self-play resigns when the root's best edge value max q falls below ``resign_threshold`` (strictly, after
``min_resign_turn``), and keeps a share of the games playing on without resignation.  Those games show what a threshold
would have cost: for each threshold T of a grid, whether the game WOULD have been resigned -- at the first searched ply
with ``ply > min_resign_turn`` and ``maxq < T`` -- and whether that resignation would have been a FALSE POSITIVE: the
mover who would have resigned went on to win or draw.  AlphaGo Zero keeps the false-positive share below 5 %.

The inputs are the max-q record of the search (Search.record_maxq: VisitEntry.maxq and VisitEntry.no_resign) and the
game's value from the first mover's view.  The first mover is on even plies.
"""
import json
import math

import numpy as np


def check_options(resign_audit, fp_target, record_visits, cmd="self", min_events=None):
    """The one check of the audit's options, for the command line and the worker alike: raises ValueError with the
    sentence the caller reports.  resign_audit needs record_visits (the numbers ride beside the visit entries); fp_target is
    0 (off) or 0 < P < 1 and needs resign_audit; both are options of `run.py self`."""
    fp_target = float(fp_target or 0.0)
    if cmd != "self" and (resign_audit or fp_target != 0.0):
        raise ValueError("--resign-audit and --resign-fp-target are options of `run.py self`")
    if fp_target != 0.0 and not 0.0 < fp_target < 1.0:
        raise ValueError(f"--resign-fp-target {fp_target:g}: expected 0 < P < 1")
    if fp_target != 0.0 and not resign_audit:
        raise ValueError("--resign-fp-target needs --resign-audit: the threshold follows the audit's histogram")
    if resign_audit and not record_visits:
        raise ValueError("--resign-audit needs --record-visits: the max q rides beside the visit entries")
    if min_events is not None and int(min_events) < 1:
        raise ValueError(f"resign_audit_min_events {min_events}: expected an integer >= 1")


def default_grid():
    """T_k = (k - 100) / 100.0, k = 0 .. 100: -1.00, -0.99, ... 0.00."""
    return np.array([(k - 100) / 100.0 for k in range(101)], dtype=np.float64)


def audit_game(trace, value, min_resign_turn, grid=None):
    """trace: the (ply, maxq) of a finished game's searched plies; value: the game's value from the first mover's view
    (> 0 win, < 0 loss, 0 draw).  Returns (would, fp), two boolean vectors over the grid: would[k], the game would have
    been resigned at threshold grid[k]; fp[k], that resignation would have been a false positive."""
    grid = default_grid() if grid is None else np.asarray(grid, dtype=np.float64)
    would = np.zeros(len(grid), dtype=bool)
    fp = np.zeros(len(grid), dtype=bool)
    for ply, maxq in sorted(trace, key=lambda e: e[0]):
        if not ply > min_resign_turn or maxq is None:
            continue
        new = (float(maxq) < grid) & ~would          # strict, as in the kernel; NaN crosses nothing
        if new.any():
            result = value if ply % 2 == 0 else -value      # the game's result for the mover of this ply
            would |= new
            if result >= 0:
                fp |= new
        if would.all():
            break
    return would, fp


class ResignAudit:
    """The histogram over the audited games: would[k], fp[k] (int64) and the number of games, per threshold of the grid."""

    def __init__(self, min_resign_turn, grid=None):
        self.grid = default_grid() if grid is None else np.asarray(grid, dtype=np.float64).copy()
        self.min_resign_turn = int(min_resign_turn)
        self.reset()

    def reset(self):
        self.would = np.zeros(len(self.grid), dtype=np.int64)
        self.fp = np.zeros(len(self.grid), dtype=np.int64)
        self.games = 0
        self.skipped = 0

    def add_trace(self, trace, value):
        would, fp = audit_game(trace, value, self.min_resign_turn, self.grid)
        self.would += would
        self.fp += fp
        self.games += 1

    def add_game(self, visits, value):
        """visits: the game's VisitEntry list as drain_records(with_visits=True) hands it out -- None when the game's record
        is flagged GAME_VISITS_LOST or incomplete.  The game counts only if every entry carries CZ_VISIT_NO_RESIGN
        (no_resign) and a max q; otherwise it is skipped, and counted as skipped.  Returns True when it counted."""
        if visits is None or not all(e.no_resign and e.maxq is not None for e in visits):
            self.skipped += 1
            return False
        self.add_trace([(e.ply, e.maxq) for e in visits], value)
        return True

    def rates(self):
        """fp / would per threshold, NaN where no game would have resigned."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.would > 0, self.fp / np.maximum(self.would, 1), np.nan)

    def choose_threshold(self, target, min_events=None):
        """The largest grid[k] with would[k] >= min_events and fp[k] <= target * would[k]; None when there is none.
        min_events defaults to ceil(5 / target): the target then corresponds to at least five games."""
        if not 0.0 < target < 1.0:
            raise ValueError(f"resign audit: target {target}: expected 0 < P < 1")
        if min_events is None:
            min_events = int(math.ceil(5.0 / target))
        ok = (self.would >= min_events) & (self.fp <= target * self.would)
        return float(self.grid[ok].max()) if ok.any() else None

    def at(self, threshold):
        """(would, fp) at the grid point closest to `threshold`, and that grid point."""
        k = int(np.abs(self.grid - float(threshold)).argmin())
        return int(self.would[k]), int(self.fp[k]), float(self.grid[k])

    # ---- the all-reduce message and the JSON file ----
    def message(self):
        """int64[2 * len(grid) + 2]: would, fp, games, skipped."""
        return np.concatenate([self.would, self.fp, [self.games, self.skipped]]).astype(np.int64)

    def with_message(self, msg):
        """A ResignAudit of the same grid holding the counts of `msg`."""
        msg = np.asarray(msg, dtype=np.int64)
        n = len(self.grid)
        if msg.shape != (2 * n + 2,):
            raise ValueError(f"resign audit: message of {msg.shape}, expected ({2 * n + 2},)")
        out = ResignAudit(self.min_resign_turn, self.grid)
        out.would, out.fp = msg[:n].copy(), msg[n:2 * n].copy()
        out.games, out.skipped = int(msg[2 * n]), int(msg[2 * n + 1])
        return out

    def to_json(self, threshold=None):
        return dict(grid=self.grid.tolist(), would=self.would.tolist(), fp=self.fp.tolist(), games=int(self.games),
                    skipped=int(self.skipped), threshold=threshold, min_resign_turn=self.min_resign_turn)

    @classmethod
    def from_json(cls, d):
        out = cls(d.get("min_resign_turn", 0), d["grid"])
        if len(d["would"]) != len(out.grid) or len(d["fp"]) != len(out.grid):
            raise ValueError("resign audit: would / fp do not match the grid")
        out.would = np.asarray(d["would"], dtype=np.int64)
        out.fp = np.asarray(d["fp"], dtype=np.int64)
        out.games, out.skipped = int(d["games"]), int(d["skipped"])
        return out

    def merge(self, other):
        """Add another histogram of the same grid."""
        if self.grid.tobytes() != other.grid.tobytes():
            raise ValueError("resign audit: the grids differ")
        self.would += other.would
        self.fp += other.fp
        self.games += other.games
        self.skipped += other.skipped
        return self

    def write(self, path, threshold=None):
        with open(path, "wt") as f:
            json.dump(self.to_json(threshold), f)


def reduce_resign_audit(audit, group=None):
    """All-reduce (SUM) the histogram over the ranks: one int64[2 * len(grid) + 2] message.  Returns a new ResignAudit with
    the global counts; `audit` keeps the local ones.  Without a process group: a copy."""
    import torch
    import torch.distributed as dist
    msg = audit.message()
    if not (dist.is_available() and dist.is_initialized()):
        return audit.with_message(msg)
    dev = "cuda" if dist.get_backend(group) == "nccl" else "cpu"
    t = torch.from_numpy(msg).to(dev)
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return audit.with_message(t.cpu().numpy())
