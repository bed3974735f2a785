"""-m gpu: the moves-left output through InferenceNet and the engine, on the small network of tests/test_gpu_wdl_loop.py
(128 filters, 2 blocks, the default arithmetic), for both value heads: forward(moves_left=) against a forward without it,
against a direct cz_heads_tail_ml launch on the same value features and against the float64 module; the compact queue; a
net without the output; hot reload between a net with the output and one without."""
import copy

import pytest

from oracle import xq_oracle as xo

pytestmark = pytest.mark.gpu
N = 70


@pytest.fixture(scope="module")
def dev():
    import torch
    from cchess_alphazero import _native
    _native.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _net(seed=0, outputs=1, moves_left=True):
    import torch
    from cchess_alphazero.agent.model import CChessNet
    torch.manual_seed(seed)
    return CChessNet(cnn_filter_num=128, res_layer_num=2, value_outputs=outputs, moves_left=moves_left).eval()


@pytest.fixture(scope="module")
def positions(dev):
    """Positions from the rule kernels, as the load-time guard's calibration set is (computed once, only read)."""
    from cchess_alphazero.agent.model import calibration_planes
    return calibration_planes(N, 14, dev, seed=5, with_legal=True)[0]


@pytest.mark.parametrize("outputs", [1, 3])
def test_inference_net_serves_the_output_beside_unchanged_policy_and_value(dev, positions, outputs):
    """forward(moves_left=out): policy and value (and wdl) bit for bit those of a forward without it; x bit for bit a direct
    heads_tail_ml launch on the same value features; x within LOGIT_TOL -- the guard's own tolerance for a linear output --
    of the float64 evaluation of the module; the compact queue's count is honoured.  Measured on an MI355X (bf16x3, the
    guard's choice): max |x - float64| 7.8e-8 (scalar head) and 2.8e-7 (win / draw / loss) against LOGIT_TOL = 2e-4."""
    import torch
    from cchess_alphazero import _native
    from cchess_alphazero.agent.model import LOGIT_TOL, guarded_inference_net
    raw = _net(outputs, outputs)
    inf = guarded_inference_net(raw, torch.float32, trunk="mfma", device=dev)
    assert inf.moves_left_head and inf.wdl_head == (outputs == 3) and inf.trunk == "mfma" and inf.supports_logits()
    planes = positions
    bits = lambda t: t.contiguous().view(torch.int32)
    p0, v0 = inf(planes)
    x = torch.full((N,), 7.0, device=dev)
    p1, v1 = inf(planes, moves_left=x)
    assert torch.equal(bits(p0), bits(p1)) and torch.equal(bits(v0), bits(v1))
    assert torch.isfinite(x).all() and (x != 7.0).all()
    l0, _ = inf(planes, logits=True)
    l1, _ = inf(planes, logits=True, moves_left=torch.empty_like(x))
    assert torch.equal(bits(l0), bits(l1))
    if outputs == 3:
        w0, w1 = torch.empty((N, 3), device=dev), torch.empty((N, 3), device=dev)
        inf(planes, wdl=w0)
        x_w = torch.empty_like(x)
        inf(planes, wdl=w1, moves_left=x_w)
        assert torch.equal(bits(w0), bits(w1)) and torch.equal(bits(x_w), bits(x))
    # against the float64 module (BatchNorm in inference mode), on the CPU
    with torch.no_grad():
        ref = copy.deepcopy(raw).double().cpu().eval()(planes.cpu().double(), moves_left=True)[2]
    err = (x.double().cpu() - ref).abs().max().item()
    print(f"\nmoves-left output through InferenceNet ({inf.arith_effective}, head {outputs}): max |x - float64| {err:.3g}, "
          f"LOGIT_TOL {LOGIT_TOL:g}; x in [{x.min().item():.3f}, {x.max().item():.3f}]")
    assert err <= LOGIT_TOL, err
    # the compact queue: rows / count, results indexed by queue position; rows past the count keep what they held
    assert inf.supports_compact_queue()
    cnt = 41
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(1)).int().to(dev)
    out = (torch.full((N, 2086), 7.0, device=dev), torch.full((N,), 7.0, device=dev))
    xq = torch.full((N,), 7.0, device=dev)
    count = torch.tensor([cnt], dtype=torch.int32, device=dev)
    inf(planes, rows=rows, count=count, out=out, moves_left=xq)
    sel = rows[:cnt].long()
    assert torch.equal(bits(xq[:cnt]), bits(x[sel])) and torch.equal(bits(out[1][:cnt]), bits(v0[sel]))
    assert torch.equal(bits(out[0][:cnt]), bits(p0[sel]))
    assert (xq[cnt:] == 7.0).all() and (out[1][cnt:] == 7.0).all() and (out[0][cnt:] == 7.0).all()
    # a direct launch on the value features that forward left in the queue's persistent buffers
    npol = inf.policy_conv.out_channels
    pf, vf = inf._head_feats(N, npol, dev)
    pol, val, xd = torch.full((N, 2086), 7.0, device=dev), torch.full((N,), 7.0, device=dev), torch.full((N,), 7.0, device=dev)
    assert tuple(inf.tail_w2_ml.shape) == (outputs + 1, 256) and len(inf._tail_b2_ml) == outputs + 1
    _native.heads_tail_ml(pf, vf, inf.tail_wp.view(inf._tail_dtype), inf.tail_bp, inf.tail_w1.view(inf._tail_dtype), inf.tail_b1,
                          inf.tail_w2_ml, inf._tail_b2_ml, pol, val, torch.empty((N, 2), device=dev), xd, count=count)
    assert torch.equal(bits(xd), bits(xq)) and torch.equal(bits(val), bits(out[1])) and torch.equal(bits(pol), bits(out[0]))
    # the torch tail (CZ_FUSED_TAIL=0) computes the same quantity
    inf.fused_tail = False
    x3 = torch.empty_like(x)
    inf(planes, moves_left=x3)
    inf.fused_tail = True
    assert (x3.double().cpu() - ref).abs().max().item() <= LOGIT_TOL


def test_a_net_without_the_output_raises_on_the_keyword(dev, positions):
    import torch
    from cchess_alphazero.agent.model import InferenceNet
    inf = InferenceNet(_net(1, 1, moves_left=False), torch.float32, trunk="mfma").to(dev)
    assert not inf.moves_left_head and not hasattr(inf, "tail_w2_ml")
    with pytest.raises(RuntimeError, match="no moves-left output"):
        inf(positions, moves_left=torch.empty((N,), device=dev))
    p, v = inf(positions)
    assert torch.isfinite(p).all() and torch.isfinite(v).all()


def test_selfplay_engine_reloads_between_a_net_with_the_output_and_one_without(dev):
    """8 games x 16 simulations: per round q_count == the rise of expansions; hot reload with -> without -> with (the second
    time beside the win / draw / loss head) mid-run; the records replay move by move."""
    import torch as t
    from cchess_alphazero.config import Config
    from cchess_alphazero.engine import SelfPlayEngine
    G = 8
    cfg = Config("mini")
    cfg.model.cnn_filter_num, cfg.model.res_layer_num = 128, 2
    cfg.play.simulation_num_per_move, cfg.play.search_threads, cfg.play.noise_eps = 16, 8, 0.0
    cfg.play.max_game_length = 8
    eng = SelfPlayEngine(cfg, G, net=_net(2, 1), dtype=t.float32, seed=13)
    try:
        assert eng.compact and eng.net.moves_left_head
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
        eng.set_network(_net(4, 1, moves_left=False))
        assert not eng.net.moves_left_head
        rounds(16)
        eng.set_network(_net(3, 3))
        assert eng.net.moves_left_head and eng.net.wdl_head
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
