"""The trainer's replay window on the device (run.py opt, worker/optimize.py).

The reference keeps its window as dense float32 arrays, 14 x 90 planes plus 2086 policy values per position
(worker/optimize.py:261-281, about 13.4 KB a position).  Here a position costs its 90-byte board, the index of the
position two plies back, the played label, the value, the root's search value q and the ply's policy surprise s
(float32 each, NaN where the record has none) and its visit counts in CSR form (about 104 B plus 6 B per visited edge); the minibatch's planes are built when it is drawn (``cz_gather_planes``) and the loss reads the sparse targets
directly (``cz_policy_value_loss``), so neither planes nor dense targets exist for the whole window.

Record files are replayed on the device, one wavefront per game (``cz_replay_games``): the boards are those of
``record_decoder.expand_records`` bit for bit, and the positions are kept in the order ``expanding_data`` produces.

Positions and visit entries are indexed with int32: a window holds at most 2^31 - 1 of each.  At `distribute`'s 90 M
positions the visit entries reach that limit at about 24 visited edges per position (not measured on real records); a
load beyond it raises ValueError instead of wrapping.
"""
from logging import getLogger

import numpy as np
import torch

from cchess_alphazero import _native
from cchess_alphazero.environment.lookup_tables import ActionLabelsRed
from cchess_alphazero.environment.static_env import state_to_array
from cchess_alphazero.lib.record_decoder import split_games

logger = getLogger(__name__)

_LABEL = {m: i for i, m in enumerate(ActionLabelsRed)}
MODES = {"played": 0, "visits": 1}
INT32_MAX = 2 ** 31 - 1         # positions and visit entries are indexed with int32 (prev, row_ptr, the kernels' counts)
Q_BOUND = 2.0                   # |q| of a record item: every value the search backs up is a network value in [-1, 1] or a
                                # terminal one, done.v * 2 = +-2 (csrc/xq_search_tree.h backup), so every edge's w / n and their
                                # weighted mean lie in [-2, 2]
S_BOUND = 70.0                  # a record item's policy surprise lies in [0, ln 1e30] (include/czero.h CZ_SURPRISE_BOUND)


def surprise_weights(s, trainable, game_offsets, alpha):
    """Per-row training weights from the records' policy surprise (KataGo's policy surprise weighting; run.py opt
    --surprise-weight A).  s: the rows' surprise, NaN = none; trainable: 0 marks a weight-0 row; game_offsets: [G + 1]
    row offsets of the games; alpha = A.  Per game, F = the rows with trainable = 1 and a finite s, S = the sum of s over
    F: with S > 0 a row of F gets (1 - A) + A |F| s / S, so the weights over F sum to |F| -- a game's total is what it
    was, A of it handed out in proportion to the surprise.  Every other trainable row gets 1, a weight-0 row 0.  Float64
    arithmetic, float32 result."""
    s = np.asarray(s, dtype=np.float64)
    tr = np.asarray(trainable) != 0
    a = float(alpha)
    w = tr.astype(np.float64)
    offs = np.asarray(game_offsets, dtype=np.int64)
    for lo, hi in zip(offs[:-1], offs[1:]):
        f = tr[lo:hi] & np.isfinite(s[lo:hi])
        nf = int(f.sum())
        if nf == 0:
            continue
        sf = s[lo:hi][f]
        total = float(sf.sum())
        if total > 0:
            w[lo:hi][f] = (1.0 - a) + a * nf * sf / total
    return w.astype(np.float32)


def mix_targets(z, q, q_ratio):
    """The value targets of cz_policy_value_loss_q on the host: t = z + L * (q - z) in float32, a rounded difference, a
    rounded product and a rounded sum; t = z where q is NaN.  z, q: float32 arrays."""
    z = np.asarray(z, dtype=np.float32)
    q = np.asarray(q, dtype=np.float32)
    lam = np.float32(q_ratio)
    if lam == 0:
        return z.copy()
    with np.errstate(invalid="ignore"):
        t = z + lam * (q - z)
    return np.where(np.isnan(q), z, t).astype(np.float32)


def moves_left_targets(lens):
    """The moves-left targets of whole games (run.py opt --moves-left), game after game: lens[g] = the record items of
    game g, and the position before item t (t = 0 .. L - 1) gets L - t, the number of items from its own to the end of its
    game, inclusive -- the last recorded position has 1, whatever ended the game (king capture, resignation, the length
    limit).  A record does not say that it was cut short: the games `run.py reanalyse --reanalyse-plies` truncates carry
    targets that are too small, and nothing here or in the trainer can tell.  -> int32 [sum(lens)]."""
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    if (lens < 0).any():
        raise ValueError("moves_left_targets: a negative game length")
    if lens.sum() == 0:
        return np.zeros(0, dtype=np.int32)
    return np.concatenate([np.arange(n, 0, -1, dtype=np.int32) for n in lens])


class ReplayWindow:
    """Positions of whole record files, appended in load order.  ``capacity`` is ``trainer.dataset_size``: ``full`` turns
    true once it is reached, and the file that reaches it is kept whole (the reference's fill_queue checks the size before
    each file).  depth 28 = ``has_history`` networks (state_history_to_planes)."""

    def __init__(self, capacity, depth=14, device="cuda", surprise_weight=0.0, moves_left=False):
        """surprise_weight A > 0: the window also holds ``w``, every position's training weight from the records' policy
        surprise (surprise_weights), on the device for ``loss(..., surprise=True)``; at 0 no such array exists.
        moves_left=True: the window also holds ``left`` (int32, on the device), every position's moves-left target
        (moves_left_targets; weight-0 rows get theirs like every row), for ``loss(..., moves_left=...)``; with False no such
        array exists."""
        if depth not in (14, 28):
            raise ValueError(f"depth={depth}: expected 14 or 28")
        if isinstance(surprise_weight, bool) or not 0.0 <= float(surprise_weight) <= 1.0:
            raise ValueError(f"surprise_weight={surprise_weight!r}: expected 0 <= A <= 1")
        self.surprise_weight = float(surprise_weight)
        self.w = None
        self.moves_left = bool(moves_left)
        self.left = None
        _native.require_gpu()
        self.capacity, self.depth = int(capacity), depth
        self.device = torch.device(device)
        self.n = 0                      # positions
        self.nnz = 0                    # visit entries
        self.n_games = 0
        self.files = []                 # the files loaded, in load order
        self._trainable = np.zeros(0, dtype=np.uint8)   # host, grown with the device arrays (_reserve)
        self._alloc(0, 0)

    def _alloc(self, n, nnz):
        d = self.device
        self.boards = torch.empty((n, 90), dtype=torch.int8, device=d)
        self.prev = torch.empty((n,), dtype=torch.int32, device=d)
        self.played = torch.empty((n,), dtype=torch.uint16, device=d)
        self.z = torch.empty((n,), dtype=torch.float32, device=d)
        self.q = torch.empty((n,), dtype=torch.float32, device=d)
        self.s = torch.empty((n,), dtype=torch.float32, device=d)
        if self.surprise_weight:
            self.w = torch.empty((n,), dtype=torch.float32, device=d)
        if self.moves_left:
            self.left = torch.empty((n,), dtype=torch.int32, device=d)
        self.row_ptr = torch.zeros((n + 1,), dtype=torch.int32, device=d)
        self.vis_label = torch.empty((nnz,), dtype=torch.uint16, device=d)
        self.vis_count = torch.empty((nnz,), dtype=torch.int32, device=d)

    def _reserve(self, n, nnz):
        """Grow the device arrays to hold n positions and nnz entries: positions double up to the capacity and no further
        (the file that crosses the capacity gets exactly the room it needs), visit entries double up to INT32_MAX."""
        if n > self.boards.shape[0]:
            cap = min(self.capacity, max(n, 1 << 16, 2 * self.boards.shape[0])) if n <= self.capacity else n
            for name in (("boards", "prev", "played", "z", "q", "s") + (("w",) if self.w is not None else ()) +
                         (("left",) if self.left is not None else ())):
                old = getattr(self, name)
                new = torch.empty((cap,) + tuple(old.shape[1:]), dtype=old.dtype, device=self.device)
                new[:self.n] = old[:self.n]
                setattr(self, name, new)
            tr = np.empty(cap, dtype=np.uint8)
            tr[:self.n] = self._trainable[:self.n]
            self._trainable = tr
            rp = torch.zeros((cap + 1,), dtype=torch.int32, device=self.device)
            rp[:self.n + 1] = self.row_ptr[:self.n + 1]
            self.row_ptr = rp
        if nnz > self.vis_label.shape[0]:
            cap = min(INT32_MAX, max(nnz, 2 * self.vis_label.shape[0], 1 << 16))
            for name in ("vis_label", "vis_count"):
                old = getattr(self, name)
                new = torch.empty((cap,), dtype=old.dtype, device=self.device)
                new[:self.nnz] = old[:self.nnz]
                setattr(self, name, new)

    @property
    def full(self):
        return self.n >= self.capacity

    def __len__(self):
        return self.n

    @property
    def trainable(self):
        """uint8 per position: 0 = a weight-0 row (a fast ply of the playout cap), kept for the history planes and the
        prev links, never drawn by the trainer."""
        return self._trainable[:self.n]

    def load_file(self, path):
        """Append the games of one record file.  Returns the number of positions added."""
        from cchess_alphazero.lib.data_helper import read_game_data_from_file
        data = read_game_data_from_file(path)
        if not isinstance(data, list) or (data and not isinstance(data[0], str)):
            raise ValueError(f"{path}: not a play record (a list that starts with a state string)")
        n = self.add_games(split_games(data), source=path)
        self.files.append(path)
        return n

    def add_games(self, games, source=None):
        """games: ``[init_state, [move, value(, pi)], ...]`` lists; an item may also be ``[move, value, pi or None, weight]``
        with weight 0 or 1 (engine.py drain: 0 = a fast ply of the playout cap): the position is kept like every other --
        history planes and ``prev`` links run through it -- and ``trainable`` is 0 for it.  Raises ValueError (naming the
        game and the ply) for a move that is not a label or whose from-square is empty, for a weight other than 0 or 1,
        and for items that are not of these forms; the window is unchanged then.  A fifth element is the root's search
        value q of the ply (engine.py drain with record_q): None or a finite number in [-Q_BOUND, Q_BOUND], anything else
        raises the same ValueError; ``q`` holds NaN for None, for shorter items and so for every older record.  A sixth element
        is the ply's policy surprise s (engine.py drain with record_surprise): None or a finite number in [0, S_BOUND],
        anything else raises the same ValueError; ``s`` holds NaN for None and for shorter items, and with surprise_weight
        > 0 ``w`` gets the new games' weights (surprise_weights).  The window holds at most INT32_MAX
        positions and INT32_MAX visit entries (int32 indices: about 24 visited edges per position at `distribute`'s 90 M
        positions); a load beyond either raises ValueError."""
        where = f" in {source}" if source else ""
        for gi, g in enumerate(games):
            if not isinstance(g[0], str) or g[0].split(" ")[0].count("/") != 9:
                raise ValueError(f"Game {gi} does not start with a state string{where}")
        lens = [len(g) - 1 for g in games]
        P = int(sum(lens))
        if P == 0:
            self.n_games += len(games)
            return 0
        labels = np.empty(P, dtype=np.uint16)
        vals = np.empty(P, dtype=np.float32)
        nvis = np.zeros(P, dtype=np.int64)
        train = np.ones(P, dtype=np.uint8)
        qs = np.full(P, np.nan, dtype=np.float32)
        ss = np.full(P, np.nan, dtype=np.float32)
        vl, vc = [], []
        k = 0
        lookup = _LABEL
        for gi, g in enumerate(games):
            if not isinstance(g[0], str):
                raise ValueError(f"Game {gi} does not start with a state string{where}")
            for t, item in enumerate(g[1:]):
                try:
                    lab = lookup.get(item[0])
                    if lab is None:
                        raise ValueError(f"Invalid move {item[0]!r} (game {gi}, ply {t}){where}")
                    labels[k] = lab
                    vals[k] = float(item[1])
                    if len(item) >= 4:
                        w = item[3]
                        if isinstance(w, bool) or not isinstance(w, (int, float)) or w not in (0, 1):
                            raise ValueError(f"Training weight {w!r}: expected 0 or 1 (game {gi}, ply {t}){where}")
                        train[k] = int(w)
                    if len(item) >= 5 and item[4] is not None:
                        q = item[4]
                        if isinstance(q, bool) or not isinstance(q, (int, float)) or not -Q_BOUND <= q <= Q_BOUND:
                            raise ValueError(f"Search value {q!r}: expected None or a finite number in "
                                             f"[-{Q_BOUND:g}, {Q_BOUND:g}] (game {gi}, ply {t}){where}")
                        qs[k] = q
                    if len(item) >= 6 and item[5] is not None:
                        sp = item[5]
                        if isinstance(sp, bool) or not isinstance(sp, (int, float)) or not 0.0 <= sp <= S_BOUND:
                            raise ValueError(f"Policy surprise {sp!r}: expected None or a finite number in "
                                             f"[0, {S_BOUND:g}] (game {gi}, ply {t}){where}")
                        ss[k] = sp
                    if len(item) >= 3 and not (len(item) >= 4 and item[2] is None):
                        pi = item[2]
                        for mv, c in pi:
                            lb = lookup.get(mv)
                            if lb is None:
                                raise ValueError(f"Invalid visit move {mv!r} (game {gi}, ply {t}){where}")
                            c = int(c)
                            if c < 0:
                                raise ValueError(f"Negative visit count (game {gi}, ply {t}){where}")
                            vl.append(lb)
                            vc.append(c)
                        if len(pi) != len({mv for mv, _ in pi}):
                            raise ValueError(f"Repeated visit move (game {gi}, ply {t}){where}")
                        nvis[k] = len(pi)
                except (TypeError, IndexError, KeyError) as e:
                    raise ValueError(f"Malformed item {item!r} (game {gi}, ply {t}){where}: {e}") from None
                k += 1
        if self.n + P > INT32_MAX or self.nnz + len(vl) > INT32_MAX:
            raise ValueError(f"the window would hold more than {INT32_MAX} positions or visit entries (int32 indices){where}")
        dev = self.device
        init = torch.from_numpy(np.stack([state_to_array(g[0]) for g in games])).to(dev)
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        boards, prev, bad = _native.replay_games(init, torch.from_numpy(labels).to(dev), torch.from_numpy(offsets).to(dev))
        bad = bad.cpu().numpy()
        if (bad != -1).any():
            gi = int(np.flatnonzero(bad != -1)[0])
            t = int(bad[gi])
            raise ValueError(f"No chessman in {games[gi][1 + t][0]} (game {gi}, ply {t}){where}")
        nnz = len(vl)
        n0, z0 = self.n, self.nnz
        self._reserve(n0 + P, z0 + nnz)
        self.boards[n0:n0 + P] = boards
        self.prev[n0:n0 + P] = torch.where(prev >= 0, prev + n0, prev)
        self.played[n0:n0 + P] = torch.from_numpy(labels).to(dev)
        self.z[n0:n0 + P] = torch.from_numpy(vals).to(dev)
        self.q[n0:n0 + P] = torch.from_numpy(qs).to(dev)
        self.s[n0:n0 + P] = torch.from_numpy(ss).to(dev)
        if self.w is not None:                  # a game's weights depend on that game's rows alone
            self.w[n0:n0 + P] = torch.from_numpy(surprise_weights(ss, train, offsets, self.surprise_weight)).to(dev)
        if self.left is not None:
            self.left[n0:n0 + P] = torch.from_numpy(moves_left_targets(lens)).to(dev)
        rp = (z0 + np.cumsum(nvis)).astype(np.int32)
        self.row_ptr[n0 + 1:n0 + P + 1] = torch.from_numpy(rp).to(dev)
        if nnz:
            self.vis_label[z0:z0 + nnz] = torch.from_numpy(np.asarray(vl, dtype=np.uint16)).to(dev)
            self.vis_count[z0:z0 + nnz] = torch.from_numpy(np.asarray(vc, dtype=np.int32)).to(dev)
        self._trainable[n0:n0 + P] = train
        self.n, self.nnz = n0 + P, z0 + nnz
        self.n_games += len(games)
        return P

    def training_rows(self):
        """The window positions a trainer may draw, ascending (int64): all but the weight-0 rows."""
        return np.flatnonzero(self.trainable)

    def planes(self, idx, mirror=None):
        """float32 planes [B, depth, 10, 9] of the window positions idx (int32 [B] on the device).  mirror: uint8 [B] on the
        device, or None: a row with a nonzero flag is the left-right mirrored position (cz_gather_planes_m)."""
        return _native.gather_planes(self.boards[:self.n], self.prev[:self.n], idx, self.depth, mirror=mirror)

    def loss(self, logits, v, idx, targets="played", weights=(1.0, 1.0), mirror=None, q_ratio=0.0, surprise=False,
             moves_left=None, legal_mask=False, mask_stats=None):
        """-> (w_p * mean policy loss + w_v * mean value loss, mean policy loss, mean value loss); the first is
        differentiable in logits [B, 2086] and v [B] (gradients from cz_policy_value_loss).  mirror: the flags given to
        ``planes``: a flagged row's target is the mirrored move's (cz_policy_value_loss_m).  q_ratio L > 0: the value
        target is z + L (q - z) where the position has a q (cz_policy_value_loss_q), and the value loss is against it.
        surprise=True (a window with surprise_weight > 0): row r counts with the weight w[idx[r]] in the gradients
        (cz_policy_value_loss_w) and in the returned means, mean(w[idx] * loss) -- still divided by B.
        v of shape [B, 3] -- the value logits of a win / draw / loss network (CChessNet(value_outputs=3)): the value loss is
        the cross-entropy against the class of z (cz_policy_wdl_loss), and a fourth entry follows, the mean squared error
        of P(win) - P(loss) against z: the number a scalar run reports.  q_ratio must be 0 then.
        moves_left=(x, W) (a window built with moves_left=True): x [B] is the network's raw moves-left output and W >= 0 the
        loss weight.  W * mean Huber loss (cz_moves_left_loss; the mean formed as the others are, surprise included) is added
        to the first entry, differentiable in x, and the mean Huber loss follows as one more entry at the end.  Without the
        argument the result is what it is above, from the same launches.
        legal_mask=True (run.py opt --policy-mask legal): the policy softmax, loss and gradient run over each row's legal
        moves and its target's support, the distribution the search reads (cz_policy_value_loss_l / cz_policy_wdl_loss_l: the
        mask is generated in the loss kernel from the window's boards, mirrored with a flagged row); everything else above
        holds as it is.  mask_stats: a dict that receives per-row tensors of the masked kernel: off_mask (int32: the row's
        target labels outside its legal moves, 0 for a valid record), illegal_mass (the share of the full softmax outside
        the row's index set) and illegal_margin (the best logit outside it minus the best inside).  An empty dict receives
        all three; a dict that holds some of these keys receives those alone, and the kernel computes the last two only
        when asked.  Without legal_mask nothing more is passed on than without these arguments."""
        if surprise and self.w is None:
            raise ValueError("loss(surprise=True) needs a window built with surprise_weight > 0")
        if mask_stats is not None and not legal_mask:
            raise ValueError("loss(mask_stats=...) needs legal_mask=True")
        mk = dict(legal_mask=True, mask_stats=mask_stats) if legal_mask else {}
        if moves_left is not None:
            if self.left is None:
                raise ValueError("loss(moves_left=...) needs a window built with moves_left=True")
            x_ml, w_m = moves_left
            res = self.loss(logits, v, idx, targets, weights, mirror=mirror, q_ratio=q_ratio, surprise=surprise, **mk)
            ml_total, ml_mean = _MovesLeftLoss.apply(x_ml, idx, self, float(w_m), bool(surprise))
            return (res[0] + ml_total,) + tuple(res[1:]) + (ml_mean,)
        if v.dim() == 2:
            if v.shape[1] != 3:
                raise ValueError(f"value of shape {tuple(v.shape)}: [B] (scalar head) or [B, 3] (win / draw / loss logits)")
            if q_ratio:
                raise ValueError("q_ratio > 0 with a win / draw / loss value head: a scalar q does not determine a "
                                 "distribution over win / draw / loss")
            return _PolicyWdlLoss.apply(logits, v, idx, self, MODES[targets], float(weights[0]), float(weights[1]), mirror,
                                        bool(surprise), *mk.values())
        return _PolicyValueLoss.apply(logits, v, idx, self, MODES[targets], float(weights[0]), float(weights[1]), mirror,
                                      float(q_ratio), bool(surprise), *mk.values())

    def value_targets(self, idx, q_ratio=0.0):
        """Host float32 [B] value targets of the positions idx as the loss kernel forms them (tests, tools): mix_targets."""
        idx = np.asarray(idx.cpu() if hasattr(idx, "cpu") else idx).astype(np.int64)
        return mix_targets(self.z[:self.n].cpu().numpy()[idx], self.q[:self.n].cpu().numpy()[idx], q_ratio)

    def dense_targets(self, idx, targets="visits", mirror=None):
        """Host float32 [B, 2086] policy targets of the positions idx as the loss kernel forms them (tests, tools); mirror:
        per-row flags (anything np.asarray takes, or a tensor), a flagged row's labels go through _native.label_mirror()."""
        if mirror is None:
            flags, M = np.zeros(len(idx), dtype=bool), None
        else:
            flags, M = np.asarray(mirror.cpu() if hasattr(mirror, "cpu") else mirror) != 0, _native.label_mirror()
        rp = self.row_ptr[:self.n + 1].cpu().numpy()
        lab = self.vis_label[:self.nnz].cpu().numpy()
        cnt = self.vis_count[:self.nnz].cpu().numpy()
        played = self.played[:self.n].cpu().numpy()
        idx = np.asarray(idx.cpu() if hasattr(idx, "cpu") else idx)
        out = np.zeros((len(idx), _native.NLABELS), dtype=np.float32)
        for r, i in enumerate(idx):
            lo, hi = rp[i], rp[i + 1]
            total = int(cnt[lo:hi].sum())
            if targets == "visits" and total > 0:
                for k in range(lo, hi):
                    out[r, M[lab[k]] if flags[r] else lab[k]] = np.float32(int(cnt[k]) / total)
            else:
                out[r, M[played[i]] if flags[r] else played[i]] = 1.0
        return out

    def legal_labels(self, idx, mirror=None):
        """Host bool [B, 2086]: the legal labels of the positions idx (tests, tools), from the rules the package's host code
        uses (environment/static_env.py: cz_movegen on the state strings), not from the loss kernel; mirror: per-row flags
        as in dense_targets, a flagged row's set is that of the mirrored board."""
        from cchess_alphazero.environment.static_env import array_to_state, get_legal_moves_batch
        idx = np.asarray(idx.cpu() if hasattr(idx, "cpu") else idx).astype(np.int64)
        flags = np.zeros(len(idx), dtype=bool) if mirror is None else \
            np.asarray(mirror.cpu() if hasattr(mirror, "cpu") else mirror) != 0
        boards = self.boards[:self.n].cpu().numpy()[idx].reshape(-1, 10, 9)
        boards = np.where(flags[:, None, None], boards[:, :, ::-1], boards).reshape(-1, 90)
        out = np.zeros((len(idx), _native.NLABELS), dtype=bool)
        if len(idx):
            for r, moves in enumerate(get_legal_moves_batch([array_to_state(b) for b in boards])):
                out[r, [_LABEL[m] for m in moves]] = True
        return out


MASK_STATS = ("off_mask", "illegal_mass", "illegal_margin")


def _mask_args(win, legal_mask, mask_stats):
    """The keywords of _native's loss functions for loss(legal_mask=..., mask_stats=...): nothing without the mask."""
    if not legal_mask:
        return {}
    want = () if mask_stats is None else (tuple(mask_stats) or MASK_STATS)
    unknown = [k for k in want if k not in MASK_STATS]
    if unknown:
        raise ValueError(f"mask_stats: unknown keys {unknown}: expected some of {MASK_STATS}")
    return dict(boards=win.boards[:win.n], off_mask="off_mask" in want,
                mask_diag="illegal_mass" in want or "illegal_margin" in want)


def _mask_results(mask_stats, kw, more):
    """Hand the outputs that followed the gradients (off_mask, then illegal_mass and illegal_margin) to the caller's dict."""
    if mask_stats is None:
        return
    more = list(more)
    if kw["off_mask"]:
        mask_stats["off_mask"] = more.pop(0)
    if kw["mask_diag"]:
        mask_stats["illegal_mass"], mask_stats["illegal_margin"] = more


class _PolicyValueLoss(torch.autograd.Function):
    """w_p * mean(policy loss) + w_v * mean(value loss) of a minibatch; backward hands out the kernel's gradients."""

    @staticmethod
    def forward(ctx, logits, v, idx, win, mode, w_p, w_v, mirror=None, q_ratio=0.0, surprise=False, legal_mask=False,
                mask_stats=None):
        n = win.n
        mk = _mask_args(win, legal_mask, mask_stats)
        if surprise:
            pl, se, gl, gv, *more = _native.policy_value_loss(
                logits.detach(), v.detach().contiguous(), idx, win.played[:n], win.z[:n], win.row_ptr[:n + 1],
                win.vis_label[:win.nnz], win.vis_count[:win.nnz], mode, w_p, w_v, mirror=mirror,
                q=win.q[:n] if q_ratio else None, q_ratio=q_ratio, row_w=win.w[:n], **mk)
            ctx.save_for_backward(gl, gv)
            wr = win.w[:n][idx.long()]
            pm, vm = (wr * pl).mean(), (wr * se).mean()     # the loss whose gradients the kernel returned
        else:
            pl, se, gl, gv, *more = _native.policy_value_loss(
                logits.detach(), v.detach().contiguous(), idx, win.played[:n], win.z[:n], win.row_ptr[:n + 1],
                win.vis_label[:win.nnz], win.vis_count[:win.nnz], mode, w_p, w_v, mirror=mirror,
                q=win.q[:n] if q_ratio else None, q_ratio=q_ratio, **mk)
            ctx.save_for_backward(gl, gv)
            pm, vm = pl.mean(), se.mean()
        if mk:
            _mask_results(mask_stats, mk, more)
        ctx.mark_non_differentiable(pm, vm)
        return w_p * pm + w_v * vm, pm, vm

    @staticmethod
    def backward(ctx, g_total, _g_pm, _g_vm):
        gl, gv = ctx.saved_tensors
        return (g_total * gl, g_total * gv) + (None,) * 10


class _PolicyWdlLoss(torch.autograd.Function):
    """_PolicyValueLoss for the three value logits of a win / draw / loss head (cz_policy_wdl_loss): the value loss is the
    cross-entropy; the fourth result is the mean squared error of P(win) - P(loss) against z."""

    @staticmethod
    def forward(ctx, logits, vlogits, idx, win, mode, w_p, w_v, mirror=None, surprise=False, legal_mask=False, mask_stats=None):
        n = win.n
        mk = _mask_args(win, legal_mask, mask_stats)
        pl, ce, se, gl, gv, *more = _native.policy_wdl_loss(
            logits.detach(), vlogits.detach().contiguous(), idx, win.played[:n], win.z[:n], win.row_ptr[:n + 1],
            win.vis_label[:win.nnz], win.vis_count[:win.nnz], mode, w_p, w_v, mirror=mirror,
            row_w=win.w[:n] if surprise else None, **mk)
        if mk:
            _mask_results(mask_stats, mk, more)
        ctx.save_for_backward(gl, gv)
        if surprise:
            wr = win.w[:n][idx.long()]
            pm, vm, sm = (wr * pl).mean(), (wr * ce).mean(), (wr * se).mean()
        else:
            pm, vm, sm = pl.mean(), ce.mean(), se.mean()
        ctx.mark_non_differentiable(pm, vm, sm)
        return w_p * pm + w_v * vm, pm, vm, sm

    @staticmethod
    def backward(ctx, g_total, _g_pm, _g_vm, _g_sm):
        gl, gv = ctx.saved_tensors
        return (g_total * gl, g_total * gv) + (None,) * 9


class _MovesLeftLoss(torch.autograd.Function):
    """W * mean(Huber loss of the moves-left output) of a minibatch and that mean (cz_moves_left_loss); backward hands out
    the kernel's gradient.  surprise: the rows count with their weights, as in the other losses."""

    @staticmethod
    def forward(ctx, x, idx, win, w_m, surprise=False):
        from cchess_alphazero.agent.model import MOVES_LEFT_DELTA, MOVES_LEFT_UNIT
        n = win.n
        hl, gx = _native.moves_left_loss(x.detach().contiguous(), idx, win.left[:n], MOVES_LEFT_UNIT, MOVES_LEFT_DELTA,
                                         row_w=win.w[:n] if surprise else None, w_m=w_m)
        ctx.save_for_backward(gx)
        mm = (win.w[:n][idx.long()] * hl).mean() if surprise else hl.mean()
        ctx.mark_non_differentiable(mm)
        return w_m * mm, mm

    @staticmethod
    def backward(ctx, g_total, _g_mm):
        gx, = ctx.saved_tensors
        return g_total * gx, None, None, None, None
