"""``run.py opt`` worker (reference: cchess_alphazero/worker/optimize.py, OptimizeWorker :38-232): trains the best model
on the play records of ``run.py self`` and hands the result to ``run.py eval`` as the next generation.

File selection, the window size, the learning-rate schedule, the epochs, the validation split, the step count and the
saving follow the reference.  The data path runs on the device: record files are replayed into a ``ReplayWindow``
(lib/replay_window.py: boards, previous-position indices, labels, values and sparse visit counts, no dense planes), each
minibatch's planes are gathered and encoded by ``cz_gather_planes`` and the loss and its gradients with respect to the
logits and the value come from ``cz_policy_value_loss``.  The network's forward and backward passes are fp32 torch
autograd.

Deliberate deviations from the reference:
  - record files are split into games with ``split_games``: the reference flat-parses a file with several games
    (nb_game_in_file > 1) as one game;
  - only the files actually loaded into the window are moved to ``data_dir/trained`` (the reference also moves files
    whose loading futures it dropped, so their positions are never trained on); an unreadable file is skipped and left
    where it is (the reference deletes it);
  - ``--policy-targets visits`` trains the policy on the records' root visit counts (items [move, value, pi]); the
    default, ``played``, is the reference's one-hot of the played move;
  - ``--augment mirror`` (default ``none``: the reference, no augmentation) shows every training row of every epoch as
    its left-right mirror image with probability 1/2 -- Xiangqi's rules do not tell the two wings apart, so the image
    is a position the same game could have reached.  ``cz_gather_planes_m`` mirrors the 90-byte board and
    ``cz_policy_value_loss_m`` the sparse target labels; no dense tensor is flipped.  The flags come from a generator of
    their own, so the shuffles are those of a run without the option; validation rows are never mirrored, and the
    epoch also reports the validation losses of the all-mirrored rows (``val_mirror``): its gap to ``val`` shows how
    unevenly the network treats the two wings;
  - ``--q-ratio L`` (default 0: the reference, the game result z alone) trains the value head towards z + L (q - z)
    where a record item carries the root's search value q (``run.py self --record-q``; rows without one keep z).  The
    target is formed in ``cz_policy_value_loss_q``; with L > 0 the logged value losses are against the mixed target and
    every epoch also reports ``val_value_z``, the validation value loss against z alone, so that runs with different L
    stay comparable (with L = 0 that is ``val``'s own value loss and nothing is added);
  - ``--surprise-weight A`` (default 0: every trainable row counts alike, the reference) weights the training rows by the
    records' policy surprise s (``run.py self --record-surprise``), KataGo's policy surprise weighting: within a game a
    row with an s gets (1 - A) + A |F| s / S (lib/replay_window.py ``surprise_weights``), so a game's total weight is
    unchanged and rows without an s keep 1.  The weight scales the row's gradients in ``cz_policy_value_loss_w`` and the
    logged training losses are the weighted means, still divided by the batch size; KataGo replicates rows in proportion
    to their weight instead, which this matches in expectation.  Validation is never weighted, so ``val`` stays
    comparable between runs with different A.  Fast plies keep the weight 0 (KataGo gives them a surprise-based one);
  - ``--value-head wdl`` (default: the head the best model has; a new model gets the reference's scalar head) trains a
    network whose value head ends in Dense(3) + softmax over (win, draw, loss) for the side to move
    (``CChessNet(value_outputs=3)``).  Its value loss is the cross-entropy of the three logits against the class of the
    game result z (``cz_policy_wdl_loss``), which is what ``value`` / ``val_value`` then report; every epoch adds
    ``val_value_z``, the squared error of P(win) - P(loss) against z (the number a scalar run reports), and the mean
    predicted draw probability on the validation rows beside their share of drawn results.  ``--q-ratio`` is refused
    with such a model: a scalar q does not determine a distribution.  The flag is refused when it contradicts the best
    model's head;
  - ``--moves-left W`` (default 0: off) trains the moves-left output, lc0's moves-left head reduced to one more Dense(1)
    on the value head's hidden layer (``CChessNet(moves_left=True)``): its raw output x means 32 softplus(x) plies until
    the game ends.  A position's target is the number of record items from its own to the end of its game, inclusive
    (lib/replay_window.py ``moves_left_targets``), and W times the mean Huber loss of softplus(x) - target / 32, threshold
    0.5 (``cz_moves_left_loss``), is added to the loss; the row weights of ``--surprise-weight`` apply, the mirror leaves
    the target as it is.  A new model (``--new``, or none there) is built with the output; a best model without it is
    refused.  Every epoch reports ``moves_left`` / ``val_moves_left`` (the mean Huber loss) and ``val_moves_left_mae``,
    the mean |32 softplus(x) - target| in plies on the validation rows.  With W = 0 a model that has the output trains
    as one without it: the output gets no gradient beyond L2.  A record does not say that it was cut short, so the games
    of ``run.py reanalyse --reanalyse-plies`` carry targets that are too small, and ``opt`` cannot tell;
  - ``--policy-mask legal`` (default ``none``: the reference, the softmax over all 2086 labels) takes the policy softmax,
    its loss and its gradient over each row's legal moves, which is the distribution the search reads: it forms a node's
    priors from the legal moves' logits alone, so no gradient goes into pushing some 2000 illegal labels down.  The mask is
    generated in the loss kernel (``cz_policy_value_loss_l`` / ``cz_policy_wdl_loss_l``) from the window's 90-byte board,
    mirrored with a flagged row; there is no dense mask and no host rule code in a step.  ``val`` and ``val_mirror`` are
    then masked losses, and every epoch adds ``val_policy_full`` (the unmasked policy loss of the same rows, which keeps
    runs with and without the mask comparable), ``val_illegal_mass`` (the mean share of the full softmax on illegal labels),
    ``val_illegal_margin`` (the largest best-illegal minus best-legal logit) and ``off_mask_targets`` (target labels outside
    the legal moves among the epoch's training and validation rows: 0 for valid records, an error in the log otherwise).
    Nothing pushes the illegal logits of such a model down: `run.py eval`, the UCI engine and CChessPlayer hand the search
    a full fp32 softmax, in which the best legal move's probability leaves the normal range once the margin nears
    87 = -ln(FLT_MIN); the trainer warns from there on.  A masked model is an ordinary model file;
  - Keras' SGD folds the learning rate into its velocity, torch's does not: the two differ only in the first steps
    after a learning-rate change;
  - a model loaded from Keras HDF5 is saved back as this package's JSON + ``.pt`` (there is no HDF5 writer);
  - a missing ``trainer.load_step`` (the ``normal`` configuration) means no limit, where the reference raises
    AttributeError; the next generation is saved only after at least one training pass;
  - one device: with several in ``--gpu`` the first one trains (no multi-GPU data parallelism).
"""
import os
import shutil
import time
from logging import getLogger

import numpy as np

from cchess_alphazero.lib.data_helper import get_game_data_filenames

logger = getLogger(__name__)

VALIDATION_SPLIT = 0.02          # Keras fit(validation_split=0.02), optimize.py:120-133
FULL_SOFTMAX_MARGIN = 87.0       # -ln(FLT_MIN) = 87.3: a logit this far below the row's maximum has a subnormal fp32 softmax


def select_files(files, last_file, tc):
    """The files of the next training pass, or None when there is not enough new data (training() :60-89).
    files: the play-data files, sorted; last_file: the last file of the previous pass (None at the start)."""
    offset = tc.min_games_to_begin_learn
    if len(files) < offset or (last_file is not None and last_file in files
                               and files.index(last_file) + 1 + offset > len(files)):
        return None
    load_step = getattr(tc, "load_step", None)                  # missing (normal): no limit
    if last_file is not None and last_file in files:
        idx = files.index(last_file) + 1
        return files[idx:] if load_step is None else files[idx:idx + load_step]
    if load_step is not None and len(files) > load_step:
        return files[:load_step]
    return list(files)


def decide_learning_rate(lr_schedules, total_steps):
    ret = None
    for step, lr in lr_schedules:
        if total_steps >= step:
            ret = lr
    return ret


def validation_split(n):
    """(training indices, validation indices) of a window of n positions: the last 2 % in load order validate
    (Keras: split_at = int(n * (1 - validation_split)))."""
    split_at = int(n * (1. - VALIDATION_SPLIT))
    return np.arange(split_at), np.arange(split_at, n)


def steps_of_pass(n, batch_size, epochs):
    """The reference's step count of one pass (train_epoch :134): full batches of the whole window, times the epochs."""
    return (n // batch_size) * epochs


def l2_parameters(net):
    """The weights under Keras' kernel_regularizer=l2: every convolution's and dense layer's kernel (no biases, no
    BatchNorm parameters), agent/model.py:37-78 of the reference."""
    import torch.nn as nn
    return [m.weight for m in net.modules() if isinstance(m, (nn.Conv2d, nn.Linear))]


def input_depth(config):
    return 28 if (config.opts.has_history or getattr(config.model, "input_depth", 14) == 28) else 14


def start(config):
    """Entry point of ``run.py opt`` (reference :32-34)."""
    import torch
    devices = str(config.opts.device_list).split(",")
    if len(devices) > 1:
        logger.info(f"multi-GPU training is not supported: training on device {devices[0]} only")
    torch.cuda.set_device(int(devices[0]))
    return OptimizeWorker(config).start()


class OptimizeWorker:
    def __init__(self, config):
        self.config = config
        self.model = None
        self.opt = None
        self.window = None
        self.count = 0                  # training passes
        self.total_steps = config.trainer.start_total_steps
        self.depth = input_depth(config)
        self.targets = getattr(config.trainer, "policy_targets", "played")
        self.augment = getattr(config.trainer, "augment", "none")
        if self.augment not in ("none", "mirror"):
            raise ValueError(f"trainer.augment={self.augment!r}: expected none or mirror")
        self.q_ratio = float(getattr(config.trainer, "q_ratio", 0.0))
        if not 0.0 <= self.q_ratio <= 1.0:
            raise ValueError(f"trainer.q_ratio={self.q_ratio!r}: expected 0 <= L <= 1")
        self.surprise_weight = float(getattr(config.trainer, "surprise_weight", 0.0))
        if not 0.0 <= self.surprise_weight <= 1.0:
            raise ValueError(f"trainer.surprise_weight={self.surprise_weight!r}: expected 0 <= A <= 1")
        self.value_head = getattr(config.trainer, "value_head", None)          # None: what the best model has
        if self.value_head not in (None, "scalar", "wdl"):
            raise ValueError(f"trainer.value_head={self.value_head!r}: expected scalar or wdl")
        self.wdl = False                # set by load_model: the model has the win / draw / loss head
        self.moves_left_weight = float(getattr(config.trainer, "moves_left", 0.0))
        if not 0.0 <= self.moves_left_weight < float("inf"):
            raise ValueError(f"trainer.moves_left={self.moves_left_weight!r}: expected a finite W >= 0")
        self.policy_mask = getattr(config.trainer, "policy_mask", "none")
        if self.policy_mask not in ("none", "legal"):
            raise ValueError(f"trainer.policy_mask={self.policy_mask!r}: expected none or legal")
        self.legal_mask = self.policy_mask == "legal"
        self.off_mask_sum = None        # legal mask: target labels outside the legal moves in the steps since the last epoch
        self.rng = np.random.default_rng(config.engine.base_seed)
        # the mirror flags have their own stream: self.rng draws what it draws without the option
        self.aug_rng = np.random.default_rng([config.engine.base_seed, 1]) if self.augment == "mirror" else None
        self.history = []               # per epoch: the logged losses

    def start(self):
        self.model = self.load_model()
        return self.training()

    # ---- the model ---------------------------------------------------------------------------------------------------
    def load_model(self):
        """The best model, or (``--new`` / none there) a freshly built one saved as best (reference :185-190)."""
        from cchess_alphazero.agent.model import CChessModel
        from cchess_alphazero.lib.model_helper import load_best_model_weight, save_as_best_model
        model = CChessModel(self.config)
        if self.config.opts.new or not load_best_model_weight(model):
            self.config.model.input_depth = self.depth
            self.config.model.value_outputs = 3 if self.value_head == "wdl" else 1
            self.config.model.moves_left = bool(self.moves_left_weight)
            model.build(seed=self.config.engine.base_seed)
            save_as_best_model(model)
        if self.moves_left_weight and not model.model.moves_left_head:
            raise ValueError(f"--moves-left {self.moves_left_weight:g}: the best model has no moves-left output; train it "
                             f"without the option, or start a new model with --new")
        if model.model.moves_left_head and not self.moves_left_weight:
            logger.info("the model has a moves-left output and --moves-left is 0: the output is not trained (it gets no "
                        "gradient beyond L2)")
        has = "wdl" if model.model.wdl_head else "scalar"
        if self.value_head is not None and self.value_head != has:
            raise ValueError(f"--value-head {self.value_head}: the best model has the {has} value head (scalar: Dense(1) + "
                             f"tanh, wdl: Dense(3) + softmax); train it as it is, or start a new model with --new")
        self.wdl = has == "wdl"
        if self.wdl and self.q_ratio:
            raise ValueError(f"--q-ratio {self.q_ratio:g} with a win / draw / loss value head: a scalar q does not "
                             "determine a distribution over win / draw / loss (train on z: --q-ratio 0)")
        if model.model.cfg["input_depth"] != self.depth:
            raise ValueError(f"the best model takes {model.model.cfg['input_depth']} input planes, the trainer makes "
                             f"{self.depth} (opts.has_history / model.input_depth)")
        model.model.cuda().train()
        return model

    def compile_model(self):
        """One SGD optimiser for the whole process (reference :136-146: lr 0.02, momentum, no Nesterov)."""
        import torch
        self.opt = torch.optim.SGD(self.model.model.parameters(), lr=0.02, momentum=self.config.trainer.momentum,
                                   nesterov=False)
        self.l2 = l2_parameters(self.model.model)

    def update_learning_rate(self, total_steps):
        lr = decide_learning_rate(self.config.trainer.lr_schedules, total_steps)
        if lr:
            for g in self.opt.param_groups:
                g["lr"] = lr
            logger.debug(f"total step={total_steps}, set learning rate to {lr}")

    def save_current_model(self, send=False):
        from cchess_alphazero.lib.model_helper import save_as_best_model, save_as_next_generation_model
        logger.info("Save as ng model" if send else "Save as best model")
        (save_as_next_generation_model if send else save_as_best_model)(self.model)

    # ---- the loop ----------------------------------------------------------------------------------------------------
    def new_window(self):
        from cchess_alphazero.lib.replay_window import ReplayWindow
        # (nothing is passed at 0: the window is built as it was without the option)
        extra = dict(surprise_weight=self.surprise_weight) if self.surprise_weight else {}
        if self.moves_left_weight:
            extra["moves_left"] = True
        return ReplayWindow(self.config.trainer.dataset_size, depth=self.depth, **extra)

    def training(self):
        """The reference's loop (:55-104): take the next files, fill the window, train epoch_to_checkpoint epochs when it
        holds more than a batch, save as best, move the files to `trained`; when the data runs out, save the next
        generation (after at least one pass) and return the total step count."""
        self.compile_model()
        tc = self.config.trainer
        total_steps = self.total_steps
        last_file = None
        self.window = self.new_window()
        while True:
            files = select_files(get_game_data_filenames(self.config.resource), last_file, tc)
            if files is None:
                if self.count > 0:
                    self.save_current_model(send=True)
                else:
                    logger.info("not enough play data to train on")
                break
            last_file = files[-1]
            logger.info(f"Last file = {last_file}")
            order = list(files)
            self.rng.shuffle(order)
            self.fill_window(order)
            self.update_learning_rate(total_steps)
            # (positions, like the reference's len(dataset[0]) -- those a step may draw: weight-0 rows do not count.
            #  This loop asks a window for nothing but its length, its files and load_file -- tests/test_trainer_cpu.py
            #  drives it with such a stand-in -- so a window that has no weights counts every position)
            rows = getattr(self.window, "training_rows", None)
            if (len(rows()) if rows is not None else len(self.window)) > tc.batch_size:
                total_steps += self.train_epoch(tc.epoch_to_checkpoint)
                self.save_current_model(send=False)
                self.update_learning_rate(total_steps)
                self.count += 1
                loaded = list(self.window.files)
                self.window = self.new_window()
                self.backup_play_data(loaded)
        self.total_steps = total_steps
        return total_steps

    def fill_window(self, order):
        """Load files from the end of the shuffled list until the window holds dataset_size positions; the file that
        reaches it is loaded whole (fill_queue :148-171)."""
        n0, t0 = len(self.window), time.time()
        while order and not self.window.full:
            path = order.pop()
            try:
                self.window.load_file(path)
            except (OSError, ValueError, TypeError, IndexError, KeyError, AttributeError) as e:   # one bad file: skip it
                logger.error(f"Error when loading data {path}: {e}")
        logger.info(f"window: {len(self.window)} positions (+{len(self.window) - n0} in {time.time() - t0:.2f} s) from "
                     f"{len(self.window.files)} files")

    def train_epoch(self, epochs):
        """epochs passes over the window's first 98 % in a fresh order each, the last 2 % validating; returns the
        reference's step count (:106-134).  Weight-0 rows (fast plies of a playout cap, lib/replay_window.py `trainable`)
        are dropped from both sides AFTER the split, which is taken over all positions; the step count is that of the
        rows left.  A window without such rows gives the indices, draws and steps it always gave."""
        import torch
        tc = self.config.trainer
        win, net = self.window, self.model.model
        n = len(win)
        tr, va = validation_split(n)
        skipped = n - len(win.training_rows())
        if skipped:
            keep = win.trainable[:n] != 0
            tr, va = tr[keep[tr]], va[keep[va]]
            logger.info(f"window: {skipped} of {n} positions carry the training weight 0 (fast plies) and are skipped: "
                        f"{len(tr)} training and {len(va)} validation rows")
        self.skipped_rows = skipped
        if self.surprise_weight:
            wt = win.w[:n].cpu().numpy()[tr]
            with_s = int(np.isfinite(win.s[:n].cpu().numpy()[tr]).sum())
            logger.info(f"window: training rows weighted by policy surprise, A = {self.surprise_weight:g}: {with_s} of "
                        f"{len(tr)} carry an s; weights min {wt.min() if len(wt) else 1.0:.4f} mean "
                        f"{wt.mean() if len(wt) else 1.0:.4f} max {wt.max() if len(wt) else 1.0:.4f}")
        dev = win.device
        va_d = torch.from_numpy(va.astype(np.int32)).to(dev)
        bs = tc.batch_size
        for ep in range(epochs):
            perm = torch.from_numpy(self.rng.permutation(tr).astype(np.int32)).to(dev)
            flags = self.mirror_flags(len(tr))
            flags_d = torch.from_numpy(flags).to(dev) if flags is not None else None
            net.train()
            ml = bool(self.moves_left_weight)        # a step then returns a fourth figure, the mean moves-left loss
            sums = torch.zeros(4 if ml else 3, dtype=torch.float64, device=dev)
            t0 = time.time()
            for b in range(0, len(tr), bs):
                idx = perm[b:b + bs]
                res = self.step(idx, None if flags_d is None else flags_d[b:b + bs])
                sums += torch.stack([res[0].detach(), *res[1:]]).double() * len(idx)
            tr_loss = (sums / max(1, len(tr))).tolist()
            # (a win / draw / loss model's and the moves-left output's further validation figures; nothing is asked otherwise)
            extra = {}
            mask = {}                                # (--policy-mask legal: the masked kernel's validation figures)
            va_loss = (self.evaluate(va_d, **(dict(extra=extra) if self.wdl or ml else {}),
                                     **(dict(mask_out=mask) if self.legal_mask else {}))) if len(va) else [float("nan")] * 3
            entry = dict(train=tr_loss[:3], val=va_loss, **extra)
            if ml:
                entry["moves_left"] = tr_loss[3]
                for k in ("val_moves_left", "val_moves_left_mae"):      # (`extra` keeps the win / draw / loss figures only)
                    entry[k] = extra.pop(k, float("nan"))
            logger.info(f"epoch {ep + 1}/{epochs}: {len(tr)} positions in {time.time() - t0:.1f} s; "
                        f"loss {tr_loss[0]:.4f} policy {tr_loss[1]:.4f} value {tr_loss[2]:.4f} - "
                        f"val_loss {va_loss[0]:.4f} val_policy {va_loss[1]:.4f} val_value {va_loss[2]:.4f}")
            if flags is not None:
                vm_loss = self.evaluate(va_d, mirror=True) if len(va) else [float("nan")] * 3
                entry["val_mirror"] = vm_loss
                logger.info(f"epoch {ep + 1}/{epochs}: {int(flags.sum())} of {len(tr)} training rows mirrored; all "
                            f"validation rows mirrored: val_loss {vm_loss[0]:.4f} val_policy {vm_loss[1]:.4f} "
                            f"val_value {vm_loss[2]:.4f}")
            if extra:
                logger.info(f"epoch {ep + 1}/{epochs}: win / draw / loss head, value = cross-entropy; P(win) - P(loss) "
                            f"against z: val_value_z {extra['val_value_z']:.4f}; validation rows: mean P(draw) "
                            f"{extra['val_draw_pred']:.4f}, drawn results {extra['val_draw_share']:.4f}")
            if ml:
                logger.info(f"epoch {ep + 1}/{epochs}: moves-left output, weight {self.moves_left_weight:g}: moves_left "
                            f"{entry['moves_left']:.4f} - val_moves_left {entry['val_moves_left']:.4f} val_moves_left_mae "
                            f"{entry['val_moves_left_mae']:.2f} plies")
            if self.q_ratio:
                entry["val_value_z"] = self.evaluate(va_d, q_ratio=0.0)[2] if len(va) else float("nan")
                logger.info(f"epoch {ep + 1}/{epochs}: value targets z + {self.q_ratio:g} (q - z); against z alone: "
                            f"val_value_z {entry['val_value_z']:.4f}")
            if self.legal_mask:
                off = (int(self.off_mask_sum) if self.off_mask_sum is not None else 0) + mask.get("off_mask_targets", 0)
                self.off_mask_sum = None
                entry.update(val_illegal_mass=mask.get("val_illegal_mass", float("nan")),
                             val_illegal_margin=mask.get("val_illegal_margin", float("nan")), off_mask_targets=off,
                             val_policy_full=self.evaluate(va_d, legal_mask=False)[1] if len(va) else float("nan"))
                logger.info(f"epoch {ep + 1}/{epochs}: policy over the legal moves; over all labels: val_policy_full "
                            f"{entry['val_policy_full']:.4f}; validation rows: mean illegal share of the full softmax "
                            f"val_illegal_mass {entry['val_illegal_mass']:.4f}, largest best-illegal minus best-legal logit "
                            f"val_illegal_margin {entry['val_illegal_margin']:.2f}; off_mask_targets {off}")
                if off:
                    logger.error(f"epoch {ep + 1}/{epochs}: {off} target labels are no legal move of their position: the "
                                 f"records and the rules disagree (such a label stays in its row's softmax)")
                if entry["val_illegal_margin"] >= FULL_SOFTMAX_MARGIN:
                    logger.warning(f"epoch {ep + 1}/{epochs}: val_illegal_margin {entry['val_illegal_margin']:.1f} >= "
                                   f"{FULL_SOFTMAX_MARGIN:g}: a full fp32 softmax (run.py eval, the UCI engine, CChessPlayer) "
                                   f"no longer holds the best legal move's probability as a normal number")
            self.history.append(entry)
        return steps_of_pass(n - skipped, bs, epochs)

    def mirror_flags(self, n):
        """uint8 [n]: one fair coin per training row of an epoch from the flags' own generator; None without
        ``--augment mirror`` (nothing is drawn then)."""
        if self.aug_rng is None:
            return None
        return self.aug_rng.integers(0, 2, size=n, dtype=np.uint8)

    def l2_term(self):
        return self.config.model.l2_reg * sum((w * w).sum() for w in self.l2)

    def step(self, idx, mirror=None):
        """One SGD step on the window positions idx; returns (total loss incl. L2, policy loss, value loss).  mirror:
        uint8 [B] on the device, the rows to train on as their mirror image (planes and targets alike), or None.
        With --moves-left W > 0 the total includes W times the mean moves-left loss, which follows as a fourth entry."""
        tc = self.config.trainer
        planes = self.window.planes(idx, mirror=mirror)
        stats = dict(off_mask=None)                  # --policy-mask legal: the one per-row figure a training step asks for
        if self.moves_left_weight:
            logits, v, x_ml = self.model.model(planes, logits=True, moves_left=True)
            res = self.window.loss(logits, v, idx, self.targets, tc.loss_weights, mirror=mirror,
                                   **self._q_args(self.q_ratio), **self._s_args(self.surprise_weight),
                                   moves_left=(x_ml, self.moves_left_weight), **self._m_args(self.legal_mask, stats))
            total, more = res[0], (res[1], res[2], res[-1])
        else:
            logits, v = self.model.model(planes, logits=True)
            # (a win / draw / loss model returns its three value logits: the window's loss takes them as they are)
            total, pm, vm = self.window.loss(logits, v, idx, self.targets, tc.loss_weights, mirror=mirror,
                                             **self._q_args(self.q_ratio), **self._s_args(self.surprise_weight),
                                             **self._m_args(self.legal_mask, stats))[:3]
            more = (pm, vm)
        if stats["off_mask"] is not None:
            off = stats["off_mask"].sum()
            self.off_mask_sum = off if self.off_mask_sum is None else self.off_mask_sum + off
        loss = total + self.l2_term()
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()
        return (loss,) + more

    @staticmethod
    def _q_args(q_ratio):
        # (nothing is passed at 0: the loop asks no more of a window's loss() than it did without the option)
        return dict(q_ratio=q_ratio) if q_ratio else {}

    @staticmethod
    def _s_args(surprise_weight):
        # (likewise; only training steps are weighted, evaluate() never passes it)
        return dict(surprise=True) if surprise_weight else {}

    @staticmethod
    def _m_args(legal_mask, stats):
        # (likewise: without --policy-mask legal a window's loss() is asked nothing new)
        return dict(legal_mask=True, mask_stats=stats) if legal_mask else {}

    def evaluate(self, idx_all, mirror=False, q_ratio=None, extra=None, legal_mask=None, mask_out=None):
        """Validation losses (inference-mode BatchNorm, as Keras): [total incl. L2, policy, value]; mirror=True: of the
        mirror images of all rows.  q_ratio: the value targets' mix, None = the trainer's own.  extra: a dict that, for a
        win / draw / loss model, receives val_value_z (the squared error of P(win) - P(loss) against z), val_draw_pred
        (the mean predicted draw probability) and val_draw_share (the share of rows with z == 0); with --moves-left W > 0 it
        receives val_moves_left (the mean Huber loss, unweighted) and val_moves_left_mae (the mean |32 softplus(x) - target|
        in plies), and the total includes W times the former.
        legal_mask: whether the policy loss is the masked one, None = the trainer's own (--policy-mask); mask_out: a dict
        that, with the mask on, receives val_illegal_mass (the mean over the rows), val_illegal_margin (the maximum over
        them) and off_mask_targets (the sum over them)."""
        import torch
        from cchess_alphazero.agent.model import moves_left_plies
        tc = self.config.trainer
        net = self.model.model
        net.eval()
        masked = self.legal_mask if legal_mask is None else bool(legal_mask)
        if masked:
            mass_sum = torch.zeros((), dtype=torch.float64, device=idx_all.device)
            margin_max = torch.full((), float("-inf"), dtype=torch.float32, device=idx_all.device)
            off_sum = torch.zeros((), dtype=torch.int64, device=idx_all.device)
        sums = torch.zeros(2, dtype=torch.float64, device=idx_all.device)
        wdl_sums = torch.zeros(3, dtype=torch.float64, device=idx_all.device)
        ml_sums = torch.zeros(2, dtype=torch.float64, device=idx_all.device)
        ml_args = {}
        with torch.no_grad():
            for b in range(0, idx_all.shape[0], tc.batch_size):
                idx = idx_all[b:b + tc.batch_size]
                flags = torch.ones(idx.shape[0], dtype=torch.uint8, device=idx.device) if mirror else None
                if self.moves_left_weight:
                    logits, v, x_ml = net(self.window.planes(idx, mirror=flags), logits=True, moves_left=True)
                    ml_args = dict(moves_left=(x_ml, self.moves_left_weight))
                else:
                    logits, v = net(self.window.planes(idx, mirror=flags), logits=True)
                stats = {}                           # the masked kernel's three per-row figures
                res = self.window.loss(logits, v, idx, self.targets, tc.loss_weights, mirror=flags,
                                       **self._q_args(self.q_ratio if q_ratio is None else q_ratio), **ml_args,
                                       **self._m_args(masked, stats))
                pm, vm = res[1], res[2]
                if stats:
                    mass_sum += stats["illegal_mass"].double().sum()
                    margin_max = torch.maximum(margin_max, stats["illegal_margin"].max())
                    off_sum += stats["off_mask"].sum()
                if ml_args:
                    err = (moves_left_plies(x_ml.double()) - self.window.left[idx.long()].double()).abs().sum()
                    ml_sums += torch.stack([res[-1].double() * len(idx), err])
                sums += torch.stack([pm, vm]).double() * len(idx)
                if v.dim() == 2:
                    draws = (self.window.z[idx.long()] == 0).double().sum()
                    wdl_sums += torch.stack([res[3].double() * len(idx), torch.softmax(v, dim=1)[:, 1].double().sum(), draws])
            p, v = (sums / idx_all.shape[0]).tolist()
            if extra is not None and self.wdl:
                sq, dp, ds = (wdl_sums / idx_all.shape[0]).tolist()
                extra.update(val_value_z=sq, val_draw_pred=dp, val_draw_share=ds)
            if mask_out is not None and masked:
                mask_out.update(val_illegal_mass=float(mass_sum) / idx_all.shape[0], val_illegal_margin=float(margin_max),
                                off_mask_targets=int(off_sum))
            l2 = float(self.l2_term())
        net.train()
        w = tc.loss_weights
        if self.moves_left_weight:
            mh, mae = (ml_sums / idx_all.shape[0]).tolist()
            if extra is not None:
                extra.update(val_moves_left=mh, val_moves_left_mae=mae)
            return [w[0] * p + w[1] * v + self.moves_left_weight * mh + l2, p, v]
        return [w[0] * p + w[1] * v + l2, p, v]

    def backup_play_data(self, files):
        """Move the files of the pass to data_dir/trained (:212-224)."""
        backup_folder = os.path.join(self.config.resource.data_dir, "trained")
        os.makedirs(backup_folder, exist_ok=True)
        cnt = 0
        for f in files:
            try:
                shutil.move(f, backup_folder)
            except OSError:
                cnt += 1
        logger.info(f"backup {len(files)} files, {cnt} failed")
