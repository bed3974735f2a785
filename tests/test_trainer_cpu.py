"""run.py opt without a GPU: the trainer's host logic (worker/optimize.py) against the reference's OptimizeWorker
(worker/optimize.py:38-232) -- file selection, learning-rate schedule, the weights under L2, validation split and step
count, which files are backed up -- and the command line reaching OptimizeWorker.  The device parts are stubbed."""
import os
import sys
import types

import numpy as np
import pytest


def tc(**kw):
    base = dict(min_games_to_begin_learn=1, load_step=6)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_select_files_follows_the_reference():
    from cchess_alphazero.worker.optimize import select_files
    files = [f"f{i:02d}" for i in range(20)]
    assert select_files(files, None, tc()) == files[:6]
    assert select_files(files[:4], None, tc()) == files[:4]
    assert select_files(files, "f05", tc()) == files[6:12]
    assert select_files(files, "f17", tc()) == files[18:]
    assert select_files(files, "f18", tc()) == ["f19"]
    assert select_files(files, "f19", tc()) is None                      # nothing after the last file
    assert select_files(files, "f17", tc(min_games_to_begin_learn=3)) is None
    assert select_files(files[:2], None, tc(min_games_to_begin_learn=3)) is None
    assert select_files([], None, tc()) is None
    assert select_files(files, "gone", tc()) == files[:6]                # last file moved away: from the start
    no_step = types.SimpleNamespace(min_games_to_begin_learn=1)          # normal: no load_step -> no limit
    assert select_files(files, None, no_step) == files
    assert select_files(files, "f09", no_step) == files[10:]


def test_learning_rate_schedule():
    from cchess_alphazero.config import Config
    from cchess_alphazero.worker.optimize import decide_learning_rate
    sched = Config("normal").trainer.lr_schedules
    assert [decide_learning_rate(sched, s) for s in (0, 149999, 150000, 399999, 400000, 10 ** 7)] == \
        [0.01, 0.01, 0.003, 0.003, 0.0001, 0.0001]
    assert decide_learning_rate([(100, 0.1)], 5) is None


def test_l2_covers_the_kernels_only():
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.worker.optimize import l2_parameters
    net = CChessNet(cnn_filter_num=8, res_layer_num=2)
    ids = {id(p) for p in l2_parameters(net)}
    names = {n for n, p in net.named_parameters() if id(p) in ids}
    want = {"input_conv.weight", "policy_conv.weight", "policy_out.weight", "value_conv.weight", "value_dense.weight",
            "value_out.weight"} | {f"res.{i}.conv{j}.weight" for i in range(2) for j in (1, 2)}
    assert names == want


def test_validation_split_and_steps():
    from cchess_alphazero.worker.optimize import steps_of_pass, validation_split
    tr, va = validation_split(1000)
    assert (tr == np.arange(980)).all() and (va == np.arange(980, 1000)).all()
    tr, va = validation_split(49)                                          # int(49 * 0.98) = 48
    assert len(tr) == 48 and list(va) == [48]
    tr, va = validation_split(10)
    assert len(tr) == 9 and list(va) == [9]
    assert steps_of_pass(1000, 512, 3) == 3 and steps_of_pass(1023, 512, 1) == 1 and steps_of_pass(100, 512, 3) == 0


class FakeWindow:
    """Stands in for ReplayWindow: every file holds `per_file` positions."""
    per_file = 4

    def __init__(self, capacity):
        self.capacity, self.n, self.files = capacity, 0, []

    @property
    def full(self):
        return self.n >= self.capacity

    def __len__(self):
        return self.n

    def load_file(self, path):
        self.n += self.per_file
        self.files.append(path)


def stub_worker(monkeypatch, tmp_path, n_files, **trainer):
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    from cchess_alphazero.config import Config
    from cchess_alphazero.worker import optimize
    cfg = Config("mini")
    for k, v in trainer.items():
        setattr(cfg.trainer, k, v)
    cfg.resource.create_directories()
    for i in range(n_files):
        with open(os.path.join(cfg.resource.play_data_dir, f"play_{i:03d}.json"), "w") as f:
            f.write("[]")
    w = optimize.OptimizeWorker(cfg)
    w.saved, w.passes, w.lrs = [], [], []
    monkeypatch.setattr(w, "new_window", lambda: FakeWindow(cfg.trainer.dataset_size))
    monkeypatch.setattr(w, "compile_model", lambda: setattr(w, "opt", types.SimpleNamespace(param_groups=[{}])))
    monkeypatch.setattr(w, "save_current_model", lambda send=False: w.saved.append(send))

    def train_epoch(epochs):
        w.passes.append(sorted(w.window.files))
        return 1000 * epochs
    monkeypatch.setattr(w, "train_epoch", train_epoch)
    orig = w.update_learning_rate

    def lr(total):
        orig(total)
        w.lrs.append(w.opt.param_groups[0].get("lr"))
    monkeypatch.setattr(w, "update_learning_rate", lr)
    return cfg, w


def test_loop_moves_only_the_loaded_files(monkeypatch, tmp_path):
    """dataset_size = 2 files: of the first pass's 6 files two are loaded, trained on and moved; the loop goes on with the
    files after the pass's last one, and stops when too few are left; the next generation is saved at the end."""
    cfg, w = stub_worker(monkeypatch, tmp_path, 10, dataset_size=8, batch_size=2, epoch_to_checkpoint=2)
    total = w.training()
    rc = cfg.resource
    trained = sorted(os.listdir(os.path.join(rc.data_dir, "trained")))
    left = sorted(os.listdir(rc.play_data_dir))
    assert w.count == len(w.passes) >= 2
    assert trained == sorted(os.path.basename(p) for ps in w.passes for p in ps)
    assert set(trained).isdisjoint(left) and len(trained) + len(left) == 10
    assert all(1 <= len(ps) <= 2 for ps in w.passes) and len(w.passes[0]) == 2
    assert w.saved == [False] * w.count + [True]
    assert total == cfg.trainer.start_total_steps + 2000 * w.count
    assert w.lrs[0] == 0.01


def test_loop_without_data_trains_nothing(monkeypatch, tmp_path):
    cfg, w = stub_worker(monkeypatch, tmp_path, 0)
    assert w.training() == cfg.trainer.start_total_steps
    assert w.count == 0 and w.saved == [] and w.passes == []


def test_small_window_is_not_trained(monkeypatch, tmp_path):
    """A window of no more than batch_size positions is not trained on and its files stay (reference :91)."""
    cfg, w = stub_worker(monkeypatch, tmp_path, 1, batch_size=4)
    w.training()
    assert w.count == 0 and w.saved == [] and os.listdir(cfg.resource.play_data_dir) == ["play_000.json"]


def test_opt_dispatch_reaches_optimize_worker(monkeypatch, tmp_path):
    import logging
    from cchess_alphazero import manager
    from cchess_alphazero.worker import optimize
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    cfg = manager.build_config(manager.create_parser().parse_args(["opt", "--policy-targets", "visits", "--new"]))
    assert cfg.trainer.policy_targets == "visits" and cfg.opts.new
    assert manager.build_config(manager.create_parser().parse_args(["opt"])).trainer.policy_targets == "played"
    with pytest.raises(SystemExit):
        manager.create_parser().parse_args(["opt", "--policy-targets", "dense"])
    seen = {}

    class Stub:
        def __init__(self, config):
            seen["config"] = config

        def start(self):
            seen["started"] = True
            return 7

    monkeypatch.setattr(optimize, "OptimizeWorker", Stub)
    monkeypatch.setattr(sys, "argv", ["run.py", "opt", "--type", "mini", "--gpu", "0,1", "--policy-targets", "visits"])
    import torch
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: seen.setdefault("device", d))
    root = logging.getLogger()
    handlers = list(root.handlers)
    try:
        assert manager.start() == 7
    finally:
        for h in root.handlers[len(handlers):]:
            root.removeHandler(h)
            h.close()
    assert seen["started"] and seen["device"] == 0 and seen["config"].trainer.policy_targets == "visits"
    assert os.path.exists(os.path.join(str(tmp_path), "logs", "opt.log"))
    # the other refused sub-commands stay refused
    monkeypatch.setattr(sys, "argv", ["run.py", "sl"])
    try:
        with pytest.raises(SystemExit):
            manager.start()
    finally:
        for h in root.handlers[len(handlers):]:
            root.removeHandler(h)
            h.close()
