"""-m gpu: the moves-left output in the trainer: the loss kernel (cz_moves_left_loss) against the float64 model and the bound
of tests/moves_left_check.py, the library terms it rests on, autograd through ReplayWindow.loss, the window's targets, one SGD
step against a pure-torch step, and a seeded overfit with save and reload."""
import copy
import json

import numpy as np
import pytest

import f16_pairs as fp
import moves_left_check as mc
from test_gpu_trainer import EPS, HI, random_games, small_config

pytestmark = pytest.mark.gpu
U = fp.U


@pytest.fixture(scope="module")
def dev():
    import torch
    from cchess_alphazero import _native
    _native.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def ml_window(games, **kw):
    from cchess_alphazero.lib.replay_window import ReplayWindow
    w = ReplayWindow(10 ** 6, moves_left=True, **kw)
    w.add_games(games)
    return w


# ---- the library terms -------------------------------------------------------------------------------------------------------
def test_library_terms_through_the_loss_kernel(dev):
    """moves_left_check's SOFTPLUS_REL = EXPF_REL + LOG1P_REL, held through cz_moves_left_loss itself: with left = 0 and unit =
    1, d = y = log1pf(expf(x)) for x <= 0, and with delta a power of two below half an ulp of every y the linear branch
    returns delta (y - delta / 2) = delta y exactly, so y is read back bit for bit.  Every fp16 value x in [-10, -2^-10]
    (delta = 2^-45) and in [-25, -10) (delta = 2^-70).  Measured on an MI355X: worst |y - log1p(exp(x))| / (SOFTPLUS_REL y)
    0.383 and 0.381 (1.92 U and 1.91 U relative)."""
    import torch
    from cchess_alphazero import _native
    neg = torch.arange(0x1400, 0x4E41, dtype=torch.int16).view(torch.float16).float()           # 2^-10 ... 25
    assert neg[0].item() == 2.0 ** -10 and neg[-1].item() == 25.0
    left = torch.zeros(1, dtype=torch.int32, device=dev)
    worst = []
    for sel, delta in ((neg <= 10.0, 2.0 ** -45), (neg > 10.0, 2.0 ** -70)):
        x = (-neg[sel]).to(dev)
        idx = torch.zeros(x.shape[0], dtype=torch.int32, device=dev)
        loss, _ = _native.moves_left_loss(x, idx, left, 1.0, delta)
        y = loss.double() / delta
        ref = torch.log1p(torch.exp(x.double()))
        assert (ref > 2.0 ** 26 * delta).all() and (loss > 2.0 ** -120).all()        # the read-back is exact
        worst.append(((y - ref).abs() / (mc.SOFTPLUS_REL * ref)).max().item())
    print(f"\nlog1pf(expf(x)) / SOFTPLUS_REL: {worst[0]:.3f} on [-10, -2^-10], {worst[1]:.3f} on [-25, -10)")
    assert max(worst) <= 1.0, worst


# ---- the loss kernel ---------------------------------------------------------------------------------------------------------
def loss_inputs(B, seed):
    """x spanning -100 ... +100, targets 1 ... 500 in a 600-position table, idx with repeats.  Half of the rows draw x
    uniformly from [-100, 100] (far out on the linear branch), the other half put softplus(x) within N(0, 0.6) units of the
    row's target (both branches); the first rows are planted: |d| = delta exactly from above and below (x = 16: softplus(16)
    = 16 in fp32), and both ends of x."""
    rng = np.random.default_rng(seed)
    n_pos = 600
    left = rng.integers(1, 501, size=n_pos).astype(np.int32)
    left[:4] = (496, 528, 1, 500)
    idx = rng.integers(0, n_pos, size=B).astype(np.int32)
    near = np.maximum(left[idx] / mc.UNIT + rng.normal(0, 0.6, size=B), 0.01)
    x = np.where(rng.random(B) < 0.5, rng.uniform(-100, 100, size=B), np.log(np.expm1(near))).astype(np.float32)
    idx[B // 2:], x[B // 2:] = idx[:B - B // 2], x[:B - B // 2][::-1]          # repeated targets under other outputs
    plant = [(16.0, 0), (16.0, 1), (-100.0, 2), (100.0, 3)][:B]
    for r, (xv, i) in enumerate(plant):
        x[r], idx[r] = xv, i
    w = rng.uniform(0.25, 2.0, size=n_pos).astype(np.float32)
    w[rng.random(n_pos) < 0.2] = 0.0
    return x, idx, left, w


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_loss_kernel_matches_float64(dev, B, weighted):
    """Per-row loss and gradient within moves_left_check.loss_check's bounds, finite everywhere, both Huber branches and
    |d| = delta hit, weight-0 rows with a zero gradient, two launches bit-identical (rows are independent: the kernel's
    contract permits it), an index out of range gives zeros.  Measured on an MI355X, worst error / bound over the ten cases:
    loss 0.391, gradient 0.369 (B = 257; B = 1: 0.058 and 0.011)."""
    import torch
    from cchess_alphazero import _native
    x, idx, left, w = loss_inputs(B, 11 + B)
    w_m = 0.75
    dx, di, dl = (torch.from_numpy(a).to(dev) for a in (x, idx, left))
    dw = torch.from_numpy(w).to(dev) if weighted else None
    loss, grad = _native.moves_left_loss(dx, di, dl, mc.UNIT, mc.DELTA, row_w=dw, w_m=w_m)
    loss2, grad2 = _native.moves_left_loss(dx, di, dl, mc.UNIT, mc.DELTA, row_w=dw, w_m=w_m)
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(grad.view(torch.int32), grad2.view(torch.int32))
    assert torch.isfinite(loss).all() and torch.isfinite(grad).all() and (loss >= 0).all()
    r = mc.loss_check(x, left[idx], w[idx] if weighted else None, w_m=w_m)
    if B >= 63:
        ad = np.abs(r["d"])
        assert (ad < 0.5).sum() >= 3 and (ad > 0.5).sum() >= 3 and (r["d"] > 0.5).any() and (r["d"] < -0.5).any()
        assert np.abs(x).max() == 100.0 and len(set(idx.tolist())) < B
        # |d| = delta exactly, from either side, in the kernel's own arithmetic: the loss is delta^2 / 2, the clamp is at its edge
        assert loss[0].item() == 0.125 and loss[1].item() == 0.125
        if weighted:
            assert (w[idx] == 0).any() and (grad[torch.from_numpy(w[idx] == 0).to(dev)] == 0).all()
    rl = (np.abs(loss.cpu().numpy().astype(np.float64) - r["loss"]) / r["e_loss"]).max()
    rg = (np.abs(grad.cpu().numpy().astype(np.float64) - r["grad"]) / r["e_grad"]).max()
    print(f"\nmoves-left loss B={B} weighted={weighted}: loss {rl:.3f}, gradient {rg:.3f} of their bounds")
    assert rl <= 1.0 and rg <= 1.0, (rl, rg)
    # an index outside the table: zeros, nothing read
    bad = di.clone()
    bad[0] = left.shape[0] + 5
    lb, gb = _native.moves_left_loss(dx, bad, dl, mc.UNIT, mc.DELTA, row_w=dw, w_m=w_m)
    assert lb[0].item() == 0.0 and gb[0].item() == 0.0 and torch.equal(lb[1:], loss[1:]) and torch.equal(gb[1:], grad[1:])


# ---- the window --------------------------------------------------------------------------------------------------------------
def games_with_weights(seed, n_games=7):
    """random_games with 4-, 5- and 6-element items mixed in: weight-0 rows, a q, a surprise."""
    games = random_games(seed, n_games, max_plies=14, pi=True)
    rng = np.random.default_rng(seed)
    for g in games:
        for t, item in enumerate(g[1:]):
            kind = int(rng.integers(4))
            if kind == 0:
                continue
            while len(item) < 3:
                item.append(None)
            item.append(0 if (t % 3 == 1) else 1)
            if kind >= 2:
                item.append(float(np.round(rng.uniform(-1, 1), 3)))
            if kind == 3:
                item.append(float(np.round(rng.uniform(0, 3), 3)))
    return games


def test_window_holds_the_targets_of_every_row(dev):
    import torch
    from cchess_alphazero.lib.replay_window import ReplayWindow, moves_left_targets
    games = games_with_weights(5) + [[games_with_weights(5)[0][0]]]          # and a game without items
    assert {len(it) for g in games for it in g[1:]} >= {4, 5, 6}
    w = ml_window(games, surprise_weight=0.5)
    n = len(w)
    lens = [len(g) - 1 for g in games]
    want = np.concatenate([np.arange(L, 0, -1) for L in lens if L])
    assert w.left.dtype == torch.int32 and w.left.is_cuda
    assert n == sum(lens) and (w.left[:n].cpu().numpy() == want).all() and (want == moves_left_targets(lens)).all()
    assert (w.trainable == 0).any(), "the case has no weight-0 rows"
    ends = np.cumsum([L for L in lens if L]) - 1
    assert (w.left[:n].cpu().numpy()[ends] == 1).all()
    # a second file goes behind the first, and growing the arrays keeps what they held
    w.add_games(random_games(6, 3, max_plies=9))
    assert (w.left[:n].cpu().numpy() == want).all() and len(w) > n and w.left[len(w) - 1].item() == 1
    plain = ReplayWindow(10 ** 6)
    plain.add_games(games)
    assert plain.left is None
    with pytest.raises(ValueError, match="moves_left=True"):
        plain.loss(torch.zeros((2, 2086), device=dev), torch.zeros(2, device=dev), torch.zeros(2, dtype=torch.int32, device=dev),
                   moves_left=(torch.zeros(2, device=dev), 1.0))


# ---- autograd ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("surprise", [False, True])
@pytest.mark.parametrize("outputs", [1, 3])
def test_window_loss_adds_the_weighted_mean_and_hands_out_the_kernels_gradient(dev, outputs, surprise):
    import torch
    from cchess_alphazero import _native
    w = ml_window(games_with_weights(8), surprise_weight=0.5)
    n, B, W = len(w), 40, 0.3
    g = torch.Generator().manual_seed(outputs)
    idx = torch.randint(0, n, (B,), generator=g).int().to(dev)
    logits = torch.randn((B, 2086), generator=g).to(dev)
    v = (torch.randn((B, 3), generator=g) if outputs == 3 else torch.tanh(torch.randn(B, generator=g))).to(dev)
    x = (torch.randn(B, generator=g) * 2 + 1).to(dev)
    mirror = (torch.rand(B, generator=g) < 0.4).to(torch.uint8).to(dev)
    kw = dict(mirror=mirror, surprise=True) if surprise else dict(mirror=mirror)
    lg, vg = logits.clone().requires_grad_(True), v.clone().requires_grad_(True)
    base = w.loss(lg, vg, idx, "visits", (1.25, 0.75), **kw)
    base[0].backward()
    assert len(base) == (4 if outputs == 3 else 3)
    lg2, vg2, xg = logits.clone().requires_grad_(True), v.clone().requires_grad_(True), x.clone().requires_grad_(True)
    res = w.loss(lg2, vg2, idx, "visits", (1.25, 0.75), moves_left=(xg, W), **kw)
    res[0].backward()
    hl, gx = _native.moves_left_loss(x, idx, w.left[:n], mc.UNIT, mc.DELTA, row_w=w.w[:n] if surprise else None, w_m=W)
    mean = (w.w[:n][idx.long()] * hl).mean() if surprise else hl.mean()
    bits = lambda t: t.contiguous().view(torch.int32)
    assert len(res) == len(base) + 1
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(res[1:-1], base[1:]))            # today's entries, today's bits
    assert torch.equal(bits(res[-1]), bits(mean)) and torch.equal(bits(res[0]), bits(base[0] + W * mean))
    assert torch.equal(bits(xg.grad), bits(gx)) and torch.equal(bits(lg2.grad), bits(lg.grad)) and torch.equal(bits(vg2.grad), bits(vg.grad))
    # and torch autograd of the formula agrees with the kernel's gradient
    x2 = x.clone().requires_grad_(True)
    t = w.left[:n][idx.long()].float() / mc.UNIT
    per_row = torch.nn.functional.huber_loss(torch.nn.functional.softplus(x2), t, reduction="none", delta=mc.DELTA)
    (W * ((w.w[:n][idx.long()] * per_row) if surprise else per_row).mean()).backward()
    assert (x2.grad - gx).abs().max().item() < 1e-7 and (per_row.detach() - hl).abs().max().item() < 1e-5


# ---- one SGD step against pure torch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", [1, 3])
def test_sgd_steps_with_the_output_match_pure_torch(dev, tmp_path, monkeypatch, outputs):
    """test_gpu_trainer.test_sgd_steps_match_pure_torch with --moves-left 0.4 (and either value head): three steps of
    OptimizeWorker.step against the same steps written out in torch, at that test's tolerance."""
    import torch
    import torch.nn.functional as F
    from cchess_alphazero.agent.model import CChessModel
    from cchess_alphazero.lib.record_decoder import expand_records
    from cchess_alphazero.worker.optimize import OptimizeWorker, l2_parameters
    W = 0.4
    cfg = small_config(tmp_path, monkeypatch, batch_size=32, policy_targets="visits", loss_weights=[1.25, 1.0], moves_left=W)
    cfg.model.value_outputs, cfg.model.moves_left = outputs, True
    games = random_games(21, 10, pi=True)
    ow = OptimizeWorker(cfg)
    ow.model = CChessModel(cfg)
    ow.model.build(seed=3)
    assert ow.model.model.moves_left_head and ow.model.model.wdl_head == (outputs == 3)
    ow.model.model.cuda().train()
    ref = copy.deepcopy(ow.model.model)
    ow.compile_model()
    ow.update_learning_rate(0)
    ow.window = ow.new_window()
    assert ow.window.left is not None
    ow.window.add_games(games)
    planes, pol, vals, _ = expand_records(games, targets="visits")
    left = torch.from_numpy(np.concatenate([np.arange(len(g) - 1, 0, -1) for g in games if len(g) > 1])).float().to(dev)
    opt = torch.optim.SGD(ref.parameters(), lr=0.01, momentum=0.9)
    rng = np.random.default_rng(0)
    wp, wv = cfg.trainer.loss_weights
    for _ in range(3):
        idx = rng.permutation(len(ow.window))[:32].astype(np.int32)
        out = ow.step(torch.from_numpy(idx).to(dev))
        assert len(out) == 4
        it = torch.from_numpy(idx.astype(np.int64)).to(dev)
        logits, v, x = ref(planes[it], logits=True, moves_left=True)
        p = torch.softmax(logits, 1)
        pc = torch.where((p > float(EPS)) & (p < float(HI)), p, p.clamp(float(EPS), float(HI)).detach())
        if outputs == 3:
            pv = torch.softmax(v, 1)
            cls = torch.where(vals[it] > 0, 0, torch.where(vals[it] < 0, 2, 1))
            value_loss = -torch.log(pv[torch.arange(32), cls].clamp(float(EPS), float(HI))).mean()
        else:
            value_loss = ((v - vals[it]) ** 2).mean()
        ml = F.huber_loss(F.softplus(x), left[it] / 32.0, delta=0.5)
        assert abs(ml.item() - out[3].item()) < 1e-5
        loss = wp * (-(pol[it] * torch.log(pc)).sum(1)).mean() + wv * value_loss + W * ml
        loss = loss + cfg.model.l2_reg * sum((t * t).sum() for t in l2_parameters(ref))
        opt.zero_grad()
        loss.backward()
        opt.step()
    for (name, a), b in zip(ow.model.model.state_dict().items(), ref.state_dict().values()):
        if a.dtype.is_floating_point:
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), name
        else:
            assert torch.equal(a, b), name


# ---- overfit, save, reload ---------------------------------------------------------------------------------------------------
def test_trainer_overfits_the_output_and_the_next_generation_reloads(dev, tmp_path, monkeypatch, caplog):
    """OptimizeWorker with --moves-left 1 (with the mirror and the surprise weights) on a window of 32-64 positions from a few
    short games: the moves-left loss falls below half of its first value (test_gpu_trainer's overfit criterion; measured
    on an MI355X: 0.8174 -> 0.0007 in 300 steps); an epoch reports the three figures; the saved next generation carries
    "moves_left": 1 and reloads with equal outputs.  With W = 0 the same model trains as one without the output."""
    import logging
    import torch
    from cchess_alphazero.agent.model import CChessModel
    from cchess_alphazero.lib.model_helper import save_as_next_generation_model
    from cchess_alphazero.worker.optimize import OptimizeWorker
    cfg = small_config(tmp_path, monkeypatch, batch_size=16, policy_targets="visits", augment="mirror", surprise_weight=0.5,
                       moves_left=1.0)
    cfg.opts.new = True
    cfg.resource.create_directories()
    ow = OptimizeWorker(cfg)
    ow.model = ow.load_model()
    assert ow.model.model.moves_left_head and ow.model.model.cfg["moves_left"] == 1
    ow.compile_model()
    ow.update_learning_rate(0)
    ow.window = ow.new_window()
    ow.window.add_games(random_games(9, 9, max_plies=12, pi=True))
    n = len(ow.window)
    assert 32 <= n <= 64 and ow.window.left is not None and ow.window.w is not None, n
    idx = torch.arange(n, dtype=torch.int32, device=dev)
    first = None
    for s in range(300):
        out = ow.step(idx)
        if first is None:
            first = out[3].item()
    last = out[3].item()
    print(f"\nmoves-left overfit: {first:.4f} -> {last:.4f}")
    assert last < 0.5 * first, (first, last)
    extra = {}
    va = ow.evaluate(idx, extra=extra)
    assert set(extra) == {"val_moves_left", "val_moves_left_mae"} and np.isfinite(va).all()
    assert np.isfinite(list(extra.values())).all() and extra["val_moves_left_mae"] >= 0.0
    ow.train_epoch(1)
    h = ow.history[-1]
    assert {"moves_left", "val_moves_left", "val_moves_left_mae", "val_mirror"} <= set(h) and len(h["train"]) == 3
    assert np.isfinite([h["moves_left"], h["val_moves_left"], h["val_moves_left_mae"]]).all() and np.isfinite(h["train"]).all()
    save_as_next_generation_model(ow.model)
    rc = cfg.resource
    assert json.load(open(rc.next_generation_config_path))["moves_left"] == 1
    back = CChessModel(cfg)
    assert back.load(rc.next_generation_config_path, rc.next_generation_weight_path) and back.model.moves_left_head
    x = ow.window.planes(idx[:8])
    a, b = ow.model.model.eval(), back.model.cuda().eval()
    with torch.no_grad():
        for u, w in zip(a(x, logits=True, moves_left=True), b(x, logits=True, moves_left=True)):
            assert torch.equal(u, w)
    # W = 0 on this best model: it trains as today, says so once, and the output's bias does not move
    cfg.opts.new = False
    cfg.trainer.moves_left = 0.0
    ow0 = OptimizeWorker(cfg)
    with caplog.at_level(logging.INFO, logger="cchess_alphazero.worker.optimize"):
        ow0.model = ow0.load_model()
    assert sum("the output is not trained" in r.getMessage() for r in caplog.records) == 1
    ow0.compile_model()
    ow0.update_learning_rate(0)
    ow0.window = ow0.new_window()
    assert ow0.window.left is None
    ow0.window.add_games(random_games(9, 9, max_plies=12, pi=True))
    bias = ow0.model.model.moves_left_out.bias.detach().clone()
    out = ow0.step(idx)
    assert len(out) == 3 and torch.equal(ow0.model.model.moves_left_out.bias.detach(), bias)
    # and a best model without the output is refused with W > 0
    cfg.opts.new, cfg.trainer.moves_left = True, 0.0
    OptimizeWorker(cfg).load_model()
    cfg.opts.new, cfg.trainer.moves_left = False, 0.5
    with pytest.raises(ValueError, match="the best model has no moves-left output.*--new"):
        OptimizeWorker(cfg).load_model()
