"""-m gpu: run.py opt --augment mirror -- the per-row mirror flag of the trainer's two per-step kernels
(cz_gather_planes_m / cz_policy_value_loss_m through lib/replay_window.py) and the worker's use of it.

The feature is a permutation of inputs and targets, so the kernel comparisons are exact: a flagged row against the
x-reversed planes, and against the unflagged kernels on a second window built from the HOST-mirrored games (mirror_state
of the initial state, mirror_move of every move and every pi entry).  The float64, pure-torch and overfit checks repeat
tests/test_gpu_trainer.py's with flags, under that file's own tolerances and criterion."""
import copy
import logging
import os
import re
import sys

import numpy as np
import pytest

from test_gpu_trainer import EPS, HI, loss_case, random_games, small_config, window_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    from cchess_alphazero import _native
    _native.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def mirror_games(games):
    """The records of the same games played on the left-right mirrored board."""
    from cchess_alphazero.environment.lookup_tables import mirror_move
    from cchess_alphazero.environment.static_env import mirror_state
    out = []
    for g in games:
        data = [mirror_state(g[0])]
        for it in g[1:]:
            item = [mirror_move(it[0]), it[1]]
            if len(it) >= 3:
                item.append([[mirror_move(str(m)), c] for m, c in it[2]])
            data.append(item)
        out.append(data)
    return out


def flags_of(rng, n, dev):
    import torch
    f = rng.integers(0, 2, size=n).astype(np.uint8)
    return f, torch.from_numpy(f).to(dev)


def ones(n, dev):
    import torch
    return torch.ones(n, dtype=torch.uint8, device=dev)


# ---- a. the gather against the x-reversed planes ---------------------------------------------------------------------
@pytest.mark.parametrize("depth", [14, 28])
@pytest.mark.parametrize("pi", [False, True])
def test_gather_flagged_rows_are_the_reversed_planes(dev, depth, pi):
    import torch
    w = window_of(random_games(41 + depth + pi, 10, pi=pi), depth=depth)
    n = len(w)
    rng = np.random.default_rng(depth + pi)
    idx = np.concatenate([rng.integers(0, n, size=150), [3, 3, 3, 0, n - 1, n - 1],          # repeated indices
                          [-1, n, n + 7, -2 ** 31, 2 ** 31 - 1]]).astype(np.int32)            # out of range: zero planes
    rng.shuffle(idx)
    idx_d = torch.from_numpy(idx).to(dev)
    f = rng.integers(0, 2, size=len(idx)).astype(np.uint8)
    out = np.flatnonzero((idx < 0) | (idx >= n))
    f[out[0]], f[out[1]] = 1, 0                          # an out-of-range row with and without the flag
    f_d = torch.from_numpy(f).to(dev)
    assert f.any() and not f.all()
    plain = w.planes(idx_d)
    got = w.planes(idx_d, mirror=f_d)
    want = torch.where(f_d.bool()[:, None, None, None], plain.flip(-1), plain)
    assert got.shape == (len(idx), depth, 10, 9) and torch.equal(got, want)
    assert not torch.equal(got, plain)
    assert torch.equal(w.planes(idx_d, mirror=None), plain)
    assert torch.equal(w.planes(idx_d, mirror=torch.zeros_like(f_d)), plain)
    assert torch.equal(w.planes(idx_d, mirror=ones(len(idx), dev)), plain.flip(-1))
    oob = torch.from_numpy((idx < 0) | (idx >= n)).to(dev)
    assert not got[oob].any()
    if depth == 28:                                      # a missing history position stays zero, a present one is mirrored
        first = (w.prev[:n] < 0)[idx_d[~oob].long()]
        assert first.any() and not first.all()
        assert not got[~oob][first][:, 14:].any() and got[~oob][~first][:, 14:].any()


# ---- b. the same positions as a window of the host-mirrored games -----------------------------------------------------
@pytest.mark.parametrize("depth", [14, 28])
def test_flagged_window_equals_the_window_of_the_mirrored_games(dev, depth):
    import torch
    games = random_games(52, 12, pi=True)
    w, wm = window_of(games, depth=depth), window_of(mirror_games(games), depth=depth)
    n = len(w)
    assert len(wm) == n and wm.nnz == w.nnz
    idx = torch.arange(n, dtype=torch.int32, device=dev)
    assert not torch.equal(wm.planes(idx), w.planes(idx))
    assert torch.equal(wm.planes(idx), w.planes(idx, mirror=ones(n, dev)))
    for targets in ("played", "visits"):
        a, b = wm.dense_targets(idx, targets), w.dense_targets(idx, targets, mirror=np.ones(n, dtype=np.uint8))
        assert a.tobytes() == b.tobytes()
        assert a.tobytes() != w.dense_targets(idx, targets).tobytes()
        assert w.dense_targets(idx, targets, mirror=np.zeros(n)).tobytes() == w.dense_targets(idx, targets).tobytes()
    M = _native_mirror()
    assert (wm.played[:n].cpu().numpy() == M[w.played[:n].cpu().numpy()]).all()
    assert (wm.vis_label[:w.nnz].cpu().numpy() == M[w.vis_label[:w.nnz].cpu().numpy()]).all()      # the same CSR order


def _native_mirror():
    from cchess_alphazero import _native
    return _native.label_mirror()


# ---- c. the loss: bit-identical to the unflagged kernel on the mirrored window ----------------------------------------
def mirrored_loss_case(dev, seed, B=48):
    """loss_case's kind of rows (one-hot, visit counts, zero-sum visits; peaked logits that drive targets into the clip),
    with the window of the mirrored games beside it."""
    import torch
    games = random_games(seed, 8, max_plies=30, pi=True)
    w, wm = window_of(games), window_of(mirror_games(games))
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(w), size=B).astype(np.int32)
    logits = rng.normal(0, 2, size=(B, 2086)).astype(np.float32)
    for r in range(0, B, 3):
        logits[r, rng.integers(2086)] += 40.0
    v = np.tanh(rng.normal(size=B)).astype(np.float32)
    f, f_d = flags_of(rng, B, dev)
    return w, wm, torch.from_numpy(idx).to(dev), torch.from_numpy(logits).to(dev), torch.from_numpy(v).to(dev), f, f_d


def raw_loss(w, logits, v, idx, mode, wp, wv, mirror=None):
    from cchess_alphazero import _native
    n = len(w)
    return _native.policy_value_loss(logits, v, idx, w.played[:n], w.z[:n], w.row_ptr[:n + 1], w.vis_label[:w.nnz],
                                     w.vis_count[:w.nnz], mode, wp, wv, mirror=mirror)


@pytest.mark.parametrize("targets", ["played", "visits"])
def test_loss_flagged_rows_are_the_mirrored_windows_rows_bit_for_bit(dev, targets):
    import torch
    from cchess_alphazero.lib.replay_window import MODES
    w, wm, idx, logits, v, f, f_d = mirrored_loss_case(dev, seed=61 if targets == "visits" else 62)
    mode, wp, wv = MODES[targets], 1.25, 0.75
    got = raw_loss(w, logits, v, idx, mode, wp, wv, mirror=f_d)
    plain = raw_loss(w, logits, v, idx, mode, wp, wv)                    # the existing entry point, same n_rows
    mirrored = raw_loss(wm, logits, v, idx, mode, wp, wv)
    fb = f_d.bool()
    assert fb.any() and not fb.all()
    for g, p, m in zip(got, plain, mirrored):
        assert torch.equal(g[fb], m[fb]) and torch.equal(g[~fb], p[~fb])
    assert not torch.equal(got[2], plain[2])                              # the flags did something
    for a, b in zip(raw_loss(w, logits, v, idx, mode, wp, wv, mirror=torch.zeros_like(f_d)), plain):
        assert torch.equal(a, b)
    # the case holds what it is meant to: flagged rows on the one-hot fallback of a zero visit total and on real visit
    # counts, and flagged rows with a target entry in the clip
    rp = w.row_ptr[:len(w) + 1].cpu().numpy()
    cnt = w.vis_count[:w.nnz].cpu().numpy()
    i = idx.cpu().numpy()
    tot = np.array([cnt[rp[k]:rp[k + 1]].sum() for k in i])
    has = np.array([rp[k + 1] > rp[k] for k in i])
    assert (f.astype(bool) & has & (tot == 0)).any() and (f.astype(bool) & (tot > 0)).any() and (f.astype(bool) & ~has).any()
    p = torch.softmax(logits.double(), 1).cpu().numpy()
    t = w.dense_targets(idx, targets, mirror=f)
    assert ((t > 0) & ~((p > EPS) & (p < HI)))[f.astype(bool)].any()


# ---- d. the mirrored loss against float64 ----------------------------------------------------------------------------
@pytest.mark.parametrize("targets", ["played", "visits"])
def test_mirrored_loss_matches_float64_and_autograd(dev, targets):
    """test_loss_kernel_matches_float64_and_autograd with flags: the reference is dense_targets(mirror=f), the tolerances
    are that test's."""
    import torch
    from cchess_alphazero.lib.replay_window import MODES
    w, idx, logits, v = loss_case(dev, seed=1 if targets == "visits" else 2)
    B = idx.shape[0]
    f, f_d = flags_of(np.random.default_rng(70), B, dev)
    wp, wv = 1.25, 0.75
    n = len(w)
    pl, se, gl, gv = raw_loss(w, logits, v, idx, MODES[targets], wp, wv, mirror=f_d)
    t = w.dense_targets(idx, targets, mirror=f)
    assert t.tobytes() != w.dense_targets(idx, targets).tobytes()
    z = w.z[:n].cpu().numpy()[idx.cpu().numpy()]
    x = logits.cpu().numpy().astype(np.float64)
    p = np.exp(x - x.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    pc = np.clip(p, np.float64(EPS), np.float64(HI))
    lo_ref = -(t * np.log(pc)).sum(1)
    assert np.allclose(pl.cpu().numpy(), lo_ref, rtol=1e-6, atol=1e-7)
    vv = v.cpu().numpy().astype(np.float64)
    assert np.allclose(se.cpu().numpy(), (vv - z) ** 2, rtol=1e-6, atol=1e-9)
    m = (p > EPS) & (p < HI)
    assert ((t > 0) & ~m).any(), "no target entry with a clipped probability in the case"
    S = (t * m).sum(1, keepdims=True)
    g_ref = wp / B * (p * S - t * m)
    assert np.abs(gl.cpu().numpy() - g_ref).max() < 1e-6
    assert np.abs(gv.cpu().numpy() - wv * 2 * (vv - z) / B).max() < 1e-6
    lg = logits.clone().requires_grad_(True)
    vg = v.clone().requires_grad_(True)
    tt = torch.from_numpy(t).to(dev)
    pr = torch.softmax(lg, 1)
    prc = torch.where((pr > float(EPS)) & (pr < float(HI)), pr, pr.clamp(float(EPS), float(HI)).detach())
    loss = wp * (-(tt * torch.log(prc)).sum(1)).mean() + wv * ((vg - torch.from_numpy(z).to(dev)) ** 2).mean()
    loss.backward()
    assert (lg.grad - gl).abs().max().item() < 1e-6 and (vg.grad - gv).abs().max().item() < 1e-6
    lg2 = logits.clone().requires_grad_(True)
    vg2 = v.clone().requires_grad_(True)
    tot, pm, vm = w.loss(lg2, vg2, idx, targets, (wp, wv), mirror=f_d)
    tot.backward()
    assert abs(tot.item() - loss.item()) <= 1e-6 * abs(loss.item())
    assert torch.equal(lg2.grad, gl) and torch.equal(vg2.grad, gv)


# ---- e. SGD steps against pure torch on the mirrored games' records --------------------------------------------------
def test_mirrored_sgd_steps_match_pure_torch(dev, tmp_path, monkeypatch):
    """test_sgd_steps_match_pure_torch with flags: the torch trainer gets, for a flagged row, the dense planes and targets
    expand_records gives for the host-mirrored games.  rtol / atol are that test's."""
    import torch
    from cchess_alphazero.agent.model import CChessModel
    from cchess_alphazero.lib.record_decoder import expand_records
    from cchess_alphazero.worker.optimize import OptimizeWorker, l2_parameters
    cfg = small_config(tmp_path, monkeypatch, batch_size=32, policy_targets="visits", loss_weights=[1.25, 1.0])
    games = random_games(21, 10, pi=True)
    ow = OptimizeWorker(cfg)
    ow.model = CChessModel(cfg)
    ow.model.build(seed=3)
    ow.model.model.cuda().train()
    ref = copy.deepcopy(ow.model.model)
    ow.compile_model()
    ow.update_learning_rate(0)
    ow.window = window_of(games)
    planes, pol, vals, _ = expand_records(games, targets="visits")
    planes_m, pol_m, vals_m, _ = expand_records(mirror_games(games), targets="visits")
    assert torch.equal(vals, vals_m)
    opt = torch.optim.SGD(ref.parameters(), lr=0.01, momentum=0.9)
    rng = np.random.default_rng(0)
    wp, wv = cfg.trainer.loss_weights
    for _ in range(3):
        idx = rng.permutation(len(ow.window))[:32].astype(np.int32)
        f, f_d = flags_of(rng, 32, dev)
        assert f.any() and not f.all()
        ow.step(torch.from_numpy(idx).to(dev), mirror=f_d)
        it = torch.from_numpy(idx.astype(np.int64)).to(dev)
        fb = f_d.bool()
        x = torch.where(fb[:, None, None, None], planes_m[it], planes[it])
        tgt = torch.where(fb[:, None], pol_m[it], pol[it])
        logits, v = ref(x, logits=True)
        p = torch.softmax(logits, 1)
        pc = torch.where((p > float(EPS)) & (p < float(HI)), p, p.clamp(float(EPS), float(HI)).detach())
        loss = wp * (-(tgt * torch.log(pc)).sum(1)).mean() + wv * ((v - vals[it]) ** 2).mean()
        loss = loss + cfg.model.l2_reg * sum((x * x).sum() for x in l2_parameters(ref))
        opt.zero_grad()
        loss.backward()
        opt.step()
    for (name, a), b in zip(ow.model.model.state_dict().items(), ref.state_dict().values()):
        if a.dtype.is_floating_point:
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), name
        else:
            assert torch.equal(a, b), name


# ---- f. the seeded overfit, half of its rows mirrored ----------------------------------------------------------------
def test_overfit_128_half_mirrored_positions(dev, tmp_path, monkeypatch):
    """test_overfit_128_positions with one fixed random flag vector: its own criterion."""
    import torch
    from cchess_alphazero.agent.model import CChessModel
    from cchess_alphazero.worker.optimize import OptimizeWorker
    cfg = small_config(tmp_path, monkeypatch, batch_size=128)
    ow = OptimizeWorker(cfg)
    ow.model = CChessModel(cfg)
    ow.model.build(seed=7)
    ow.model.model.cuda().train()
    ow.compile_model()
    ow.update_learning_rate(0)
    ow.window = window_of(random_games(9, 12, max_plies=60))
    assert len(ow.window) >= 128
    idx = torch.arange(128, dtype=torch.int32, device=dev)
    f, f_d = flags_of(np.random.default_rng(80), 128, dev)
    assert 32 <= int(f.sum()) <= 96
    first = None
    for s in range(300):
        _, pm, _ = ow.step(idx, mirror=f_d)
        if first is None:
            first = pm.item()
    last = pm.item()
    assert last < 0.5 * first, (first, last)


# ---- g. an epoch of the worker ---------------------------------------------------------------------------------------
def test_train_epoch_with_augment_mirror(dev, tmp_path, monkeypatch, caplog):
    import torch
    from cchess_alphazero.agent.model import CChessModel
    from cchess_alphazero.worker.optimize import OptimizeWorker, validation_split
    games = random_games(90, 16, max_plies=40, pi=True)
    cfg = small_config(tmp_path, monkeypatch, batch_size=32, policy_targets="visits", augment="mirror")
    ow = OptimizeWorker(cfg)
    ow.model = CChessModel(cfg)
    ow.model.build(seed=5)
    ow.model.model.cuda().train()
    ow.compile_model()
    ow.update_learning_rate(0)
    ow.window = window_of(games)
    n = len(ow.window)
    tr, va = validation_split(n)
    assert len(va) >= 2 and len(tr) > 64
    with caplog.at_level(logging.INFO, logger="cchess_alphazero.worker.optimize"):
        steps = ow.train_epoch(2)
    assert steps == (n // 32) * 2 and len(ow.history) == 2
    for h in ow.history:
        assert set(h) == {"train", "val", "val_mirror"}
        assert all(np.isfinite(h[k]).all() and len(h[k]) == 3 for k in h)
    # the log line counts the mirrored rows: the flags' own generator, replayed
    replay = np.random.default_rng([cfg.engine.base_seed, 1])
    want = [int(replay.integers(0, 2, size=len(tr), dtype=np.uint8).sum()) for _ in range(2)]
    seen = [int(m.group(1)) for r in caplog.records
            for m in [re.search(r"(\d+) of (\d+) training rows mirrored", r.getMessage())] if m and int(m.group(2)) == len(tr)]
    assert seen == want and all(0 < k < len(tr) for k in want)
    # validation is never mirrored: the same weights give the same numbers with the option off
    va_d = torch.from_numpy(va.astype(np.int32)).to(dev)
    cfg_off = small_config(tmp_path, monkeypatch, batch_size=32, policy_targets="visits")
    off = OptimizeWorker(cfg_off)
    assert off.augment == "none" and off.aug_rng is None
    off.model, off.window = ow.model, ow.window
    off.l2 = ow.l2
    off.window = window_of(mirror_games(games))
    e1, e2 = off.evaluate(va_d), off.evaluate(va_d)      # evaluate()'s run-to-run spread: twice on one window
    spread = max(abs(a - b) for a, b in zip(e1, e2))
    off.window = ow.window
    e_on, e_off = ow.evaluate(va_d), off.evaluate(va_d)
    got = ow.history[-1]["val_mirror"]
    print("val", ow.history[-1]["val"], e_on, e_off, "val_mirror", got, "mirrored window", e1, e2, "spread", spread)
    assert all(abs(a - b) <= spread for a, b in zip(e_on, e_off))
    assert all(abs(a - b) <= spread for a, b in zip(e_on, ow.history[-1]["val"]))
    # val_mirror is evaluate() of the window of the host-mirrored games
    assert all(abs(a - b) <= spread for a, b in zip(got, e1))
    assert abs(got[1] - e_on[1]) > spread                 # a network not trained for it does tell the wings apart


# ---- h. through the command line -------------------------------------------------------------------------------------
def test_run_opt_augment_mirror_from_the_command_line(dev, tmp_path, monkeypatch):
    from cchess_alphazero import manager
    from cchess_alphazero.agent.model import CChessModel
    from cchess_alphazero.lib.data_helper import get_game_data_filenames, write_game_data_to_file
    from cchess_alphazero.worker import optimize
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    build = manager.build_config
    seen = {}

    def small(args):                                      # the command line's config at test size (as the cycle test sets it)
        cfg = build(args)
        cfg.model.cnn_filter_num, cfg.model.res_layer_num = 32, 2
        cfg.trainer.batch_size = 16
        seen["cfg"] = cfg
        return cfg
    monkeypatch.setattr(manager, "build_config", small)
    cfg = small(manager.create_parser().parse_args(["opt"]))
    cfg.resource.create_directories()
    rc = cfg.resource
    model = CChessModel(cfg)
    model.build(seed=0)
    model.save(rc.model_best_config_path, rc.model_best_weight_path)
    digest0 = model.digest
    games = [g for g in random_games(95, 12, max_plies=40, pi=True) if len(g) > 4][:5]
    assert len(games) == 5
    for i, g in enumerate(games):
        write_game_data_to_file(os.path.join(rc.play_data_dir, rc.play_data_filename_tmpl % f"{i:03d}"), g)
    files = get_game_data_filenames(rc)
    workers = []
    orig = optimize.OptimizeWorker

    class Keep(orig):
        def __init__(self, config):
            super().__init__(config)
            workers.append(self)
    monkeypatch.setattr(optimize, "OptimizeWorker", Keep)
    monkeypatch.setattr(sys, "argv", ["run.py", "opt", "--type", "mini", "--augment", "mirror", "--policy-targets", "visits"])
    root = logging.getLogger()
    handlers, level = list(root.handlers), root.level
    try:
        total = manager.start()
    finally:
        root.setLevel(level)
        for h in root.handlers[len(handlers):]:
            root.removeHandler(h)
            h.close()
    ow = workers[0]
    assert seen["cfg"].trainer.augment == "mirror" and ow.augment == "mirror"
    assert ow.count >= 1 and total == ow.total_steps > 0
    assert ow.history and all(np.isfinite(h[k]).all() for h in ow.history for k in ("train", "val", "val_mirror"))
    best = CChessModel(cfg)
    assert best.load(rc.model_best_config_path, rc.model_best_weight_path) and best.digest != digest0
    assert os.path.exists(best._pt(rc.next_generation_weight_path))
    assert sorted(os.listdir(os.path.join(rc.data_dir, "trained"))) == sorted(os.path.basename(p) for p in files)
    with open(rc.opt_log_path) as f:
        assert re.search(r"\d+ of \d+ training rows mirrored", f.read())
