"""-m gpu: the win / draw / loss value head above the dense tail: the loss kernel (cz_policy_wdl_loss) against float64 NumPy,
cz_policy_value_loss_w and torch autograd; a whole 128-filter network on the default arithmetic against the guard's float64
reference; and the loop -- self-play, hot reload between a scalar and a WDL net, the trainer, save and reload."""
import json
import os

import numpy as np
import pytest

from oracle import xq_oracle as xo
from test_gpu_trainer import EPS, HI, random_games, small_config, window_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    from cchess_alphazero import _native
    _native.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def games_with_draws(seed, n_games, max_plies=30, pi=True):
    """test_gpu_trainer.random_games with every third game drawn (all its items carry the value 0)."""
    games = random_games(seed, n_games, max_plies=max_plies, pi=pi)
    for g in games[::3]:
        for item in g[1:]:
            item[1] = 0
    return games


# ---- 4. the loss kernel ------------------------------------------------------------------------------------------------------
def wdl_loss_case(dev, seed, B=40):
    import torch
    w = window_of(games_with_draws(seed, 9))
    n = len(w)
    rng = np.random.default_rng(seed)
    z_all = w.z[:n].cpu().numpy()
    # at least a quarter of the rows from each result, the rest at random; one index out of range
    pick = [rng.choice(np.flatnonzero(z_all == t), size=B // 4) for t in (1.0, 0.0, -1.0)]
    idx = np.concatenate(pick + [rng.integers(0, n, size=B - 3 * (B // 4))]).astype(np.int32)
    rng.shuffle(idx)
    idx[7] = n + 3
    logits = rng.normal(0, 2, size=(B, 2086)).astype(np.float32)
    for r in range(0, B, 3):
        logits[r, rng.integers(2086)] += 40.0
    vl = rng.normal(0, 1.5, size=(B, 3)).astype(np.float32)
    # planted value logits: the target class at p < 1e-7 (rows 1, 5, 9, ...) and at p > 1 - 1e-7 (rows 3, 11, ...)
    tc = np.where(z_all[np.clip(idx, 0, n - 1)] > 0, 0, np.where(z_all[np.clip(idx, 0, n - 1)] < 0, 2, 1))
    for r in range(1, B, 4):
        vl[r, tc[r]] -= 30.0
    for r in range(3, B, 8):
        vl[r, tc[r]] += 30.0
    mirror = (rng.random(B) < 0.4).astype(np.uint8)
    return w, idx, torch.from_numpy(idx).to(dev), torch.from_numpy(logits).to(dev), torch.from_numpy(vl).to(dev), \
        torch.from_numpy(mirror).to(dev)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("targets", ["played", "visits"])
def test_wdl_loss_kernel_matches_float64_and_the_scalar_kernels_policy_half(dev, targets, weighted):
    """cz_policy_wdl_loss on 40 rows (a quarter or more from each of z = 1 / 0 / -1, one index out of range, mirrored rows,
    value logits that put the target class below 1e-7 and above 1 - 1e-7) against a float64 restatement: losses rtol 1e-6 /
    atol 1e-7, gradients 1e-6 absolute (test_gpu_trainer's tolerances for the policy half).  Its policy outputs are
    cz_policy_value_loss_w's bit for bit, and autograd through ReplayWindow.loss hands out the kernel's gradients."""
    import torch
    from cchess_alphazero import _native
    from cchess_alphazero.lib.replay_window import MODES
    w, idx_h, idx, logits, vl, mirror = wdl_loss_case(dev, seed=3 if targets == "visits" else 4)
    B, n = idx.shape[0], len(w)
    wp, wv = 1.25, 0.75
    rw = None
    if weighted:
        rw = torch.from_numpy(np.random.default_rng(8).uniform(0.25, 2.0, size=n).astype(np.float32)).to(dev)
    args = (idx, w.played[:n], w.z[:n], w.row_ptr[:n + 1], w.vis_label[:w.nnz], w.vis_count[:w.nnz], MODES[targets], wp, wv)
    pl, ce, se, gl, gv = _native.policy_wdl_loss(logits, vl, *args, mirror=mirror, row_w=rw)
    ok = idx_h < n
    assert (~ok).sum() == 1
    # the policy half: the scalar kernel's bits
    v_any = torch.zeros(B, device=dev)
    pl_s, _, gl_s, _ = _native.policy_value_loss(logits, v_any, *args, mirror=mirror, row_w=rw)
    assert torch.equal(pl, pl_s) and torch.equal(gl, gl_s)
    # the value half in float64
    iz = np.clip(idx_h, 0, n - 1)
    z = w.z[:n].cpu().numpy().astype(np.float64)[iz]
    assert all((z[ok] == t).sum() >= B // 4 - 1 for t in (1.0, 0.0, -1.0))
    tc = np.where(z > 0, 0, np.where(z < 0, 2, 1))
    x = vl.cpu().numpy().astype(np.float64)
    p = np.exp(x - x.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    pt = p[np.arange(B), tc]
    m = ((pt > EPS) & (pt < HI)).astype(np.float64)
    assert (pt[ok] <= EPS).any() and (pt[ok] >= HI).any() and ((m == 1) & ok).sum() >= B // 2, "the case misses the clip"
    ce_ref = np.where(ok, -np.log(np.clip(pt, np.float64(EPS), np.float64(HI))), 0.0)
    se_ref = np.where(ok, ((p[:, 0] - p[:, 2]) - z) ** 2, 0.0)
    t = np.zeros((B, 3))
    t[np.arange(B), tc] = 1.0
    scale = wv / B * (rw.cpu().numpy().astype(np.float64)[iz] if weighted else 1.0)
    g_ref = np.where(ok[:, None], np.reshape(scale, (-1, 1)) * (p * m[:, None] - t * m[:, None]), 0.0)
    assert np.allclose(ce.cpu().numpy(), ce_ref, rtol=1e-6, atol=1e-7)
    assert np.allclose(se.cpu().numpy(), se_ref, rtol=1e-6, atol=1e-7)
    assert np.abs(gv.cpu().numpy() - g_ref).max() < 1e-6
    assert pl[~torch.from_numpy(ok).to(dev)].abs().max().item() == 0.0
    # the policy half in float64 as well (test_gpu_trainer's restatement), on the rows in range
    tp = w.dense_targets(iz, targets, mirror=mirror.cpu().numpy())
    xl = logits.cpu().numpy().astype(np.float64)
    q = np.exp(xl - xl.max(1, keepdims=True))
    q /= q.sum(1, keepdims=True)
    lo_ref = np.where(ok, -(tp * np.log(np.clip(q, np.float64(EPS), np.float64(HI)))).sum(1), 0.0)
    assert np.allclose(pl.cpu().numpy(), lo_ref, rtol=1e-6, atol=1e-7)
    if not weighted:
        # the autograd.Function of the window hands out the kernel's gradients
        lg, vg = logits.clone().requires_grad_(True), vl.clone().requires_grad_(True)
        tot, pm, vm, sm = w.loss(lg, vg, idx, targets, (wp, wv), mirror=mirror)
        tot.backward()
        assert torch.equal(lg.grad, gl) and torch.equal(vg.grad, gv)
        assert torch.equal(pm, pl.mean()) and torch.equal(vm, ce.mean()) and torch.equal(sm, se.mean())
        assert abs(tot.item() - (wp * lo_ref.mean() + wv * ce_ref.mean())) <= 1e-5 * abs(tot.item())
        # and torch autograd of the dense formula agrees on the value logits
        vg2 = vl.clone().requires_grad_(True)
        pr = torch.softmax(vg2, 1)
        prc = torch.where((pr > float(EPS)) & (pr < float(HI)), pr, pr.clamp(float(EPS), float(HI)).detach())
        tt = torch.from_numpy(t * ok[:, None]).float().to(dev)
        (wv * (-(tt * torch.log(prc)).sum(1)).sum() / B).backward()
        assert (vg2.grad - gv).abs().max().item() < 1e-6
        with pytest.raises(ValueError, match="scalar q does not determine a distribution"):
            w.loss(lg, vg, idx, targets, (wp, wv), q_ratio=0.5)


# ---- 5. the whole network ----------------------------------------------------------------------------------------------------
def _wdl_net(seed=0, blocks=2):
    import torch
    from cchess_alphazero.agent.model import CChessNet
    torch.manual_seed(seed)
    return CChessNet(cnn_filter_num=128, res_layer_num=blocks, value_outputs=3).eval()


def test_whole_wdl_network_stays_within_the_guards_tolerances(dev):
    """A 128-filter, 2-block WDL net on the default arithmetic, ~70 positions of the rule kernels: v, the legal priors and wdl
    within GUARD_TOL of reference_forward_f64, the logits within LOGIT_TOL; the compact-queue form writes the same bits.
    Measured on an MI355X (bf16x3): value 3.3e-8, wdl 3.5e-8, legal priors 7.3e-9, logits 3.3e-7."""
    import torch
    from cchess_alphazero.agent.model import (GUARD_TOL, LOGIT_TOL, calibration_planes, guarded_inference_net,
                                              measure_against_reference, reference_forward_f64, within_guard)
    raw = _wdl_net()
    planes, legal = calibration_planes(70, 14, dev, seed=5, with_legal=True)
    inf = guarded_inference_net(raw, torch.float32, trunk="mfma", device=dev)
    assert inf.wdl_head and inf.trunk == "mfma" and inf.supports_logits(), inf.arith_effective
    ref = reference_forward_f64(raw, planes, with_wdl=True)
    assert tuple(ref[-1].shape) == (70, 3) and torch.equal(ref[1], ref[-1][:, 0] - ref[-1][:, 2])
    m = measure_against_reference(inf, ref, planes, legal)
    wdl = torch.full((70, 3), 7.0, device=dev)
    p, v = inf(planes, wdl=wdl)
    m["wdl_max_abs"] = float((wdl.double() - ref[-1]).abs().max())
    print("\nwhole WDL net (%s): %s" % (inf.arith_effective, {k: (f"{x:.3g}" if isinstance(x, float) else x) for k, x in m.items()}))
    assert within_guard(m, GUARD_TOL, LOGIT_TOL), m
    assert m["wdl_max_abs"] <= GUARD_TOL and (v.double() - ref[1]).abs().max().item() <= GUARD_TOL
    assert (wdl.double().sum(1) - 1).abs().max().item() < 1e-6
    assert float(ref[-1][:, 1].max()) > 0.05, "the draw class carries no mass on these positions: the comparison is empty"
    # the compact queue: rows / count, results indexed by queue position
    assert inf.supports_compact_queue()
    n, cnt = planes.shape[0], 41
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(1)).int().to(dev)
    out = (torch.full((n, 2086), 7.0, device=dev), torch.full((n,), 7.0, device=dev))
    w2 = torch.full((n, 3), 7.0, device=dev)
    inf(planes, rows=rows, count=torch.tensor([cnt], dtype=torch.int32, device=dev), out=out, wdl=w2)
    sel = rows[:cnt].long()
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(out[1][:cnt]), bits(v[sel])) and torch.equal(bits(w2[:cnt]), bits(wdl[sel]))
    assert torch.equal(bits(out[0][:cnt]), bits(p[sel]))
    assert (out[1][cnt:] == 7.0).all() and (w2[cnt:] == 7.0).all()
    # the torch tail (CZ_FUSED_TAIL=0) and the fp32 library floor of the guard compute the same quantity
    from cchess_alphazero.agent.model import InferenceNet
    inf.fused_tail = False
    w3 = torch.empty((n, 3), device=dev)
    p3, v3 = inf(planes, wdl=w3)
    inf.fused_tail = True
    lib = InferenceNet(raw, torch.float32, trunk="library").to(dev)
    w4 = torch.empty((n, 3), device=dev)
    p4, v4 = lib(planes.float(), wdl=w4)
    for vv, ww in ((v3, w3), (v4, w4)):
        assert (vv.double() - ref[1]).abs().max().item() <= GUARD_TOL
        assert (ww.double() - ref[-1]).abs().max().item() <= GUARD_TOL


# ---- 6. the loop ---------------------------------------------------------------------------------------------------------------
def test_selfplay_engine_plays_on_a_wdl_net_and_reloads_between_heads(dev):
    """8 games x 16 simulations on the WDL net: per round q_count == the rise of expansions; hot reload WDL -> scalar -> WDL
    mid-run; the records replay move by move."""
    import torch as t
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.config import Config
    from cchess_alphazero.engine import SelfPlayEngine
    G = 8
    cfg = Config("mini")
    cfg.model.cnn_filter_num, cfg.model.res_layer_num = 128, 2
    cfg.play.simulation_num_per_move, cfg.play.search_threads, cfg.play.noise_eps = 16, 8, 0.0
    cfg.play.max_game_length = 8
    eng = SelfPlayEngine(cfg, G, net=_wdl_net(2), dtype=t.float32, seed=13)
    try:
        assert eng.compact and eng.net.wdl_head
        eng.start()
        games, before = [], 0

        def rounds(k):
            nonlocal before
            for _ in range(k):
                eng.step()
                now = eng.counters()["expansions"]
                assert int(eng.search.q_count.item()) == now - before
                before = now
            games.extend(eng.drain())
        rounds(16)
        v = eng.search.value[:int(eng.search.q_count.item())]
        assert t.isfinite(v).all() and (v.abs() <= 1).all()
        t.manual_seed(4)
        eng.set_network(CChessNet(cnn_filter_num=128, res_layer_num=2).eval())
        assert not eng.net.wdl_head
        rounds(16)
        eng.set_network(_wdl_net(3))
        assert eng.net.wdl_head
        rounds(32)
        c = eng.counters()
        assert c["overflow_sims"] == 0 and c["ring_dropped"] == 0
    finally:
        eng.close()
    assert len(games) >= G
    for g in games:
        state = g["data"][0]
        assert state == xo.INIT_STATE and len(g["data"]) - 1 == g["turns"]
        for i, item in enumerate(g["data"][1:]):
            assert item[0] in xo.get_legal_moves(state), (g["game_id"], i)
            state = xo.step(state, item[0])


def test_trainer_overfits_a_wdl_model_and_the_next_generation_reloads(dev, tmp_path, monkeypatch):
    """OptimizeWorker with --value-head wdl on a window of <= 64 positions, a third of them from drawn games: the value loss
    (cross-entropy) falls below half of its first value (test_gpu_trainer's overfit criterion; measured on an MI355X: 1.099
    -> 0.093 in 300 steps); an epoch reports the WDL figures; the saved next generation reloads as a WDL net that reproduces its own outputs."""
    import torch
    from cchess_alphazero.agent.model import CChessModel
    from cchess_alphazero.lib.model_helper import save_as_next_generation_model
    from cchess_alphazero.worker.optimize import OptimizeWorker
    cfg = small_config(tmp_path, monkeypatch, batch_size=16, value_head="wdl", policy_targets="visits", augment="mirror",
                       surprise_weight=0.0)
    cfg.opts.new = True
    cfg.resource.create_directories()
    ow = OptimizeWorker(cfg)
    ow.model = ow.load_model()
    assert ow.wdl and ow.model.model.wdl_head and ow.model.model.cfg["value_outputs"] == 3
    ow.compile_model()
    ow.update_learning_rate(0)
    games = random_games(9, 9, max_plies=12, pi=True)
    total, drawn = sum(len(g) - 1 for g in games), 0
    for g in games:                                             # whole games drawn until they hold a third of the positions
        if 3 * drawn < total:
            drawn += len(g) - 1
            for item in g[1:]:
                item[1] = 0
    ow.window = window_of(games)
    n = len(ow.window)
    assert 32 <= n <= 64, n
    z = ow.window.z[:n].cpu().numpy()
    assert 1 / 3 <= (z == 0).mean() <= 0.5 and (z == 1).any() and (z == -1).any()
    idx = torch.arange(n, dtype=torch.int32, device=dev)
    first = None
    for s in range(300):
        _, pm, vm = ow.step(idx)
        if first is None:
            first = vm.item()
    last = vm.item()
    assert last < 0.5 * first, (first, last)
    extra = {}
    va = ow.evaluate(idx, extra=extra)
    assert set(extra) == {"val_value_z", "val_draw_pred", "val_draw_share"} and np.isfinite(va).all()
    assert abs(extra["val_draw_share"] - (z == 0).mean()) < 1e-9 and 0.0 <= extra["val_draw_pred"] <= 1.0
    # (va[2] is the cross-entropy under inference-mode BatchNorm, whose running statistics -- momentum 0.01 -- lag 300
    #  steps behind: measured 0.76 against a training-mode 0.09, first 1.10; it is reported, not compared)
    # one epoch of the loop logs the same figures into history
    ow.train_epoch(1)
    h = ow.history[-1]
    assert {"val_value_z", "val_draw_pred", "val_draw_share", "val_mirror"} <= set(h) and np.isfinite(h["train"]).all()
    # the next generation: saved, reloaded as a WDL net, the same outputs
    save_as_next_generation_model(ow.model)
    rc = cfg.resource
    assert json.load(open(rc.next_generation_config_path))["value_outputs"] == 3
    back = CChessModel(cfg)
    assert back.load(rc.next_generation_config_path, rc.next_generation_weight_path) and back.model.wdl_head
    x = ow.window.planes(idx[:8])
    a, b = ow.model.model.eval(), back.model.cuda().eval()
    with torch.no_grad():
        for u, w in zip(a(x, logits=True), b(x, logits=True)):
            assert torch.equal(u, w)
        assert torch.equal(a.wdl(x), b.wdl(x))
    # the scalar flag against this best model is refused, and so is a q mix
    cfg.opts.new = False
    cfg.trainer.value_head = "scalar"
    with pytest.raises(ValueError, match="the best model has the wdl value head"):
        OptimizeWorker(cfg).load_model()
    cfg.trainer.value_head, cfg.trainer.q_ratio = None, 0.5
    with pytest.raises(ValueError, match="scalar q does not determine a distribution"):
        OptimizeWorker(cfg).load_model()
