"""-m gpu: the load-time guard of the tower arithmetics (agent/model.py guarded_inference_net) and the tolerance
north_star states -- policy / value within 1e-4 of the reference network (agent/model.py:32-83 as api.py:63-74 evaluates
it) -- on networks with a PEAKED policy, where the trunk's relative error is amplified by the logit scale.

Every number is against a float64 evaluation of the same network (reference_forward_f64, itself pinned to the PyTorch
module on the CPU).  Tolerances, stated here as the contract asks:
  * the arithmetic the guard selects: policy and value within 5e-5 on the calibration positions (GUARD_TOL) and within
    1e-4 with a factor-of-two margin on FRESH positions of other playouts;
  * f16x3 (the fallback the guard reaches for peaked networks): within 2.5e-5, a factor of four inside the tolerance;
  * bf16x3 and the unguarded c8 are reported with their margins, not asserted: at max p ~ 0.9 they sit AT the
    tolerance -- which is what the guard exists for.
"""
import pytest

pytestmark = pytest.mark.gpu


def peaked_net(policy_scale, blocks=7, filters=128, seed=11):
    """7 x 128 with perturbed BatchNorm statistics and the policy layer scaled so that the softmax is peaked (a trained
    network's policy puts most of its mass on a few moves; random-init gives 1 / 2086 everywhere)."""
    import torch
    import torch.nn.functional as F
    from cchess_alphazero.agent.model import CChessNet
    torch.manual_seed(seed)
    net = CChessNet(cnn_filter_num=filters, res_layer_num=blocks)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.3)
            m.running_var.uniform_(0.5, 2.0)
            m.weight.data.normal_(1, 0.2)
            m.bias.data.normal_(0, 0.2)
    net.policy_out.weight.data.mul_(policy_scale)
    # a live value head whose output spreads over (-1, 1) (with the perturbed statistics alone the head's ReLUs are dead and
    # the value is one constant): positive BatchNorm shifts, then the last layer centred and stretched on probe planes
    net.value_bn.bias.data.fill_(0.5)
    net.value_bn.weight.data.fill_(1.0)
    net.value_dense.bias.data.uniform_(0.0, 0.3)
    net.eval()
    with torch.no_grad():
        probe = (torch.rand((48, net.cfg["input_depth"], 10, 9)) < 0.07).float()
        x = net.trunk(probe)
        h = F.relu(net.value_dense(F.relu(net.value_bn(net.value_conv(x))).flatten(1)))
        pre = (h @ net.value_out.weight.data.T).squeeze(1)
        k = 1.2 / float(pre.std())
        net.value_out.weight.data.mul_(k)
        net.value_out.bias.data.fill_(-k * float(pre.mean()))
    return net


def test_calibration_positions_are_positions():
    import torch
    from cchess_alphazero.agent.model import calibration_planes
    for depth in (14, 28):
        p = calibration_planes(200, depth)
        assert p.shape == (200, depth, 10, 9) and p.dtype == torch.uint8 and p.is_cuda
        cur = p[:, :14].long()
        assert int(cur.max()) == 1 and int(cur.sum((1,)).max()) == 1              # one piece per square at most
        assert torch.all(cur[:, 6].sum((1, 2)) == 1) and torch.all(cur[:, 13].sum((1, 2)) == 1)      # both kings
        pieces = cur.sum((1, 2, 3))
        assert int(pieces.max()) == 32 and int(pieces.min()) < 32                  # openings and positions after captures
        assert len({bytes(x.cpu().numpy().tobytes()) for x in p}) > 150            # not 200 copies of the opening


def test_reference_forward_matches_the_module_in_float64():
    import copy
    import torch
    from cchess_alphazero.agent.model import calibration_planes, reference_forward_f64
    net = peaked_net(20.0, blocks=2)
    planes = calibration_planes(16, 14)
    p, v, lg, acts, quants = reference_forward_f64(net, planes, with_activations=True)
    with torch.no_grad():
        pr, vr = copy.deepcopy(net).double()(planes.double().cpu())
    # (float64 on the device: rocBLAS GEMMs, 1e-9-class agreement with the CPU module on a peaked policy -- four orders below
    #  anything it is used to measure; the CPU evaluation of the same function agrees to 1e-16, tests/test_host_logic.py)
    assert (p.cpu() - pr).abs().max().item() < 2e-8 and (v.cpu() - vr).abs().max().item() < 2e-8
    assert len(acts) == 1 + 2 * 2 and all(a > 0 for a in acts)


@pytest.mark.parametrize("policy_scale,min_peak", [(60.0, 0.6), (150.0, 0.85)])
def test_peaked_policy_networks_stay_within_tolerance(policy_scale, min_peak):
    import torch
    from cchess_alphazero.agent.model import (InferenceNet, calibration_planes, guarded_inference_net,
                                              measure_against_reference, reference_forward_f64)
    net = peaked_net(policy_scale)
    fresh = calibration_planes(192, 14, seed=777)                  # not the guard's calibration set
    ref = reference_forward_f64(net, fresh)
    peak = float(ref[0].max())
    assert peak >= min_peak, peak
    rows = {}
    for arith in ("bf16x3", "f16x3", "c8"):
        m = measure_against_reference(InferenceNet(net, torch.float32, trunk="mfma", arith=arith).cuda(), ref, fresh)
        rows[arith] = m
        print(f"policy x{policy_scale:g} (max p {peak:.3f}) {arith:7s}: policy {m['policy_max_abs']:.2e} "
              f"(margin {1e-4 / max(m['policy_max_abs'], 1e-30):.1f}x)  value {m['value_max_abs']:.2e}  logit {m['logit_max_abs']:.2e}")
    assert rows["f16x3"]["policy_max_abs"] < 2.5e-5 and rows["f16x3"]["value_max_abs"] < 2.5e-5, rows["f16x3"]
    g = guarded_inference_net(net, torch.float32, trunk="mfma", arith="c8")
    m = measure_against_reference(g, ref, fresh)
    print(f"guard: requested c8 -> {g.arith_effective}: policy {m['policy_max_abs']:.2e} "
          f"(margin {1e-4 / max(m['policy_max_abs'], 1e-30):.1f}x), candidates {g.calibration['candidates']}")
    assert g.arith_requested == "c8" and g.calibration["max_policy_probability"] >= min_peak
    assert m["policy_max_abs"] < 5e-5 and m["value_max_abs"] < 5e-5, (g.arith_effective, m)
    last = g.calibration["chosen"]
    assert g.arith_effective == "fp32-library" or \
        (g.arith_effective == last["arith"] and last["policy_max_abs"] <= g.calibration["tol"])
    assert [r["arith"] for r in g.calibration["candidates"]] == [n for n in g.calibration["tried"] if n != "fp32-library"]


def test_guard_keeps_the_requested_arithmetic_where_it_is_exact_enough():
    """The benchmark's network (random init, near-uniform policy): c8 stays, and the report says why."""
    import torch
    from cchess_alphazero.agent.model import CChessNet, guarded_inference_net
    torch.manual_seed(0)
    net = CChessNet(cnn_filter_num=128, res_layer_num=7).eval()
    g = guarded_inference_net(net, torch.float32, trunk="mfma", arith="c8")
    assert g.arith_effective == "c8" and g.arith == "c8" and g.c8_blocks == 7
    c = g.calibration["candidates"]
    assert len(c) == 1 and c[0]["policy_max_abs"] < 5e-5 and c[0]["value_max_abs"] < 5e-5
    assert g.calibration["c8_saturating_layers"] == [] and len(g.calibration["activation_max"]) == 15
    # guard off: exactly what was asked for, nothing measured
    g0 = guarded_inference_net(net, torch.float32, trunk="mfma", arith="c8", guard=False)
    assert g0.arith_effective == "c8" and g0.calibration is None
    # 256 filters have no c8: the request degrades to the fp16 pairs (192 filters: c8 since round 4)
    g1 = guarded_inference_net(CChessNet(cnn_filter_num=256, res_layer_num=2).eval(), torch.float32, trunk="mfma", arith="c8")
    assert g1.arith_effective == "f16x3"
    g2 = guarded_inference_net(CChessNet(cnn_filter_num=192, res_layer_num=2).eval(), torch.float32, trunk="mfma", arith="c8")
    assert g2.arith_effective == "c8"


def test_guard_moves_out_of_range_activations_into_the_operand_formats():
    """Activations above e4m3's 448 would lose the w_lo x correction silently in the kernels (xq_nn_common.h cf8::sat), tiny
    ones fall into its subnormals.  The guard sees every tower tensor's range in the float64 pass and applies exact
    power-of-two scales (InferenceNet act_shift: a reparametrisation of the folded network, outputs unchanged) before it
    measures the candidates; the report carries the ranges before and after."""
    import torch
    from cchess_alphazero.agent.model import (InferenceNet, calibration_planes, guarded_inference_net,
                                              measure_against_reference, reference_forward_f64)
    for factor in (3000.0, 40000.0):
        net = peaked_net(1.0, blocks=3)
        net.input_bn.weight.data.mul_(factor)
        net.input_bn.bias.data.mul_(factor)
        g = guarded_inference_net(net, torch.float32, trunk="mfma", arith="c8")
        cal = g.calibration
        assert cal["act_shift"]["stream"] < 0 and all(v < 0 for v in cal["act_shift"]["mid"])
        assert max(cal["activation_max"]) > 448.0 and cal["c8_saturating_layers"]
        assert max(cal["activation_max_scaled"]) <= 448.0 and not cal["c8_saturating_layers_after_scaling"]
        assert cal["candidates"][0]["arith"] == "c8"                 # tried, now that its image holds the tensors
        fresh = calibration_planes(64, 14, seed=5)
        ref = reference_forward_f64(net, fresh)
        m = measure_against_reference(g, ref, fresh)
        assert m["policy_max_abs"] < 1e-4 and m["value_max_abs"] < 1e-4, (factor, g.arith_effective, m)
        # the scales are an exact reparametrisation: the same network, shifted and unshifted, on the range-free bf16 pairs
        a = InferenceNet(net, torch.float32, trunk="mfma", arith="bf16x3").cuda()(fresh)
        b = InferenceNet(net, torch.float32, trunk="mfma", arith="bf16x3", act_shift=g.act_shift).cuda()(fresh)
        assert (a[0] - b[0]).abs().max().item() < 2e-6 and (a[1] - b[1]).abs().max().item() < 2e-6
    # a network in the usual range is left alone
    g = guarded_inference_net(peaked_net(1.0, blocks=2), torch.float32, trunk="mfma", arith="c8")
    assert g.act_shift is None and g.calibration["act_shift"] == {"stream": 0, "mid": [0, 0]}


@pytest.mark.parametrize("n8", [0, 3, 5, 7])
def test_hybrid_tower_runs_its_first_blocks_on_c8(n8):
    """arith "c8>N": N = all blocks is the c8 network bit for bit, N = 0 the f16x3 network; in between the error against
    float64 lies between the two (c8 blocks add ~sqrt(N) of a block's error)."""
    import torch
    from cchess_alphazero.agent.model import (InferenceNet, calibration_planes, measure_against_reference,
                                              reference_forward_f64)
    net = peaked_net(60.0)
    planes = calibration_planes(96, 14, seed=9)
    ref = reference_forward_f64(net, planes)
    h = InferenceNet(net, torch.float32, trunk="mfma", arith=f"c8>{n8}").cuda()
    assert h.arith_name == ("c8" if n8 == 7 else ("f16x3" if n8 == 0 else f"c8>{n8}"))
    p, v = h(planes)
    if n8 in (0, 7):
        q, w = InferenceNet(net, torch.float32, trunk="mfma", arith="c8" if n8 else "f16x3").cuda()(planes)
        assert torch.equal(p, q) and torch.equal(v, w)
    e = {a: measure_against_reference(InferenceNet(net, torch.float32, trunk="mfma", arith=a).cuda(), ref, planes)["logit_max_abs"]
         for a in ("f16x3", "c8")}
    mine = measure_against_reference(h, ref, planes)["logit_max_abs"]
    print(f"c8>{n8}: logit error {mine:.2e} (f16x3 {e['f16x3']:.2e}, c8 {e['c8']:.2e})")
    assert mine <= 1.5 * e["c8"] + 1e-9 and mine >= 0.5 * e["f16x3"]
    # the compact queue (device-side count) goes through the hybrid hand-over too
    rows = torch.arange(planes.shape[0] - 1, -1, -1, dtype=torch.int32, device="cuda")
    cnt = torch.tensor([40], dtype=torch.int32, device="cuda")
    pc, vc = h(planes, rows=rows, count=cnt)
    assert torch.equal(pc[:40], p.flip(0)[:40]) and torch.equal(vc[:40], v.flip(0)[:40])


def test_hybrid_and_guard_on_the_192_filter_tower():
    """The reference's deployed topology (10 x 192, configs/distribute.py:84-87) through the same machinery: c8 on
    k_resblock_ip_c8, the hybrid hand-over (fp32 out of the last c8 block, re-split into fp16 pairs for k_resblock_ip), the
    guard's choice on a peaked policy."""
    import torch
    from cchess_alphazero.agent.model import (InferenceNet, calibration_planes, guarded_inference_net,
                                              measure_against_reference, reference_forward_f64)
    net = peaked_net(60.0, blocks=4, filters=192)
    planes = calibration_planes(64, 14, seed=21)
    ref = reference_forward_f64(net, planes)
    errs = {}
    for arith in ("f16x3", "c8>2", "c8"):
        inf = InferenceNet(net, torch.float32, trunk="mfma", arith=arith).cuda()
        assert inf.arith_name == arith
        errs[arith] = measure_against_reference(inf, ref, planes)["logit_max_abs"]
    # (round 6) c6 at 192 filters, and its hybrids: a c6 block writing the c8 image the c8 blocks behind it read
    for arith in ("c6", "c6>2", "c6>1"):
        inf = guarded_inference_net(net, torch.float32, trunk="mfma", arith=arith, guard=False, planes=planes)
        assert inf.arith_name == arith and inf.c6
        errs[arith] = measure_against_reference(inf, ref, planes)["logit_max_abs"]
    print("192 filters, logit error:", errs)
    assert errs["f16x3"] < errs["c8>2"] * 1.5 + 1e-9 and errs["c8>2"] < errs["c8"] * 1.5 + 1e-9 and errs["f16x3"] < 0.3 * errs["c8"]
    assert errs["c8"] * 0.5 < errs["c6>2"] < errs["c6"] * 1.5 + 1e-9 and errs["c6"] < 6.0 * errs["c8"], errs
    g = guarded_inference_net(net, torch.float32, trunk="mfma", arith="c8")
    m = measure_against_reference(g, ref, planes)
    print("guard on 192:", g.arith_effective, m)
    assert m["policy_max_abs"] < 1e-4 and m["value_max_abs"] < 1e-4


@pytest.mark.parametrize("n6", [1, 3, 5, 7])
def test_hybrid_tower_runs_its_first_blocks_on_c6(n6):
    """arith "c6>N" (round 5): the first N blocks on c6, the rest on c8; block N - 1 writes a c8 image (cz_conv3x3_c6_pack_weights
    y_exp = 127).  N = all blocks is the c6 network bit for bit; in between the error against float64 lies between c8's and
    c6's; the compact queue goes through the hand-over too."""
    import torch
    from cchess_alphazero.agent.model import (calibration_planes, guarded_inference_net, measure_against_reference,
                                              reference_forward_f64)
    net = peaked_net(60.0)
    planes = calibration_planes(96, 14, seed=9)
    ref = reference_forward_f64(net, planes)
    build = lambda a: guarded_inference_net(net, torch.float32, trunk="mfma", arith=a, guard=False, planes=planes)
    h = build(f"c6>{n6}")
    assert h.arith_name == ("c6" if n6 == 7 else f"c6>{n6}") and h.c6 and h.c6_blocks == n6
    p, v = h(planes)
    if n6 == 7:
        q, w = build("c6")(planes)
        assert torch.equal(p, q) and torch.equal(v, w)
    e = {a: measure_against_reference(build(a), ref, planes)["logit_max_abs"] for a in ("c8", "c6")}
    mine = measure_against_reference(h, ref, planes)["logit_max_abs"]
    print(f"c6>{n6}: logit error {mine:.2e} (c8 {e['c8']:.2e}, c6 {e['c6']:.2e})")
    assert mine <= 1.5 * e["c6"] + 1e-9 and mine >= 0.5 * e["c8"]
    rows = torch.arange(planes.shape[0] - 1, -1, -1, dtype=torch.int32, device="cuda")
    cnt = torch.tensor([40], dtype=torch.int32, device="cuda")
    pc, vc = h(planes, rows=rows, count=cnt)
    assert torch.equal(pc[:40], p.flip(0)[:40]) and torch.equal(vc[:40], v.flip(0)[:40])


def test_guard_sees_an_error_that_hides_behind_an_illegal_peak():
    """the search consumes priors renormalised over the LEGAL moves (reference player.py:272-283), so a
    label that is never legal can hold almost all of the 2086-way softmax's mass and shrink every absolute softmax error below
    any tolerance while the priors the search sees are off.  Such a network: a peaked policy plus a large bias on a label that
    no calibration position can play.  The full-softmax criterion of round 4 accepts c6 there; the guard (logit deviation
    <= 2e-4, legal-renormalised priors <= 5e-5) does not, and what it selects keeps the legal priors within north_star's 1e-4
    on fresh positions."""
    import torch
    from cchess_alphazero.agent.model import (GUARD_TOL, LOGIT_TOL, calibration_planes, guarded_inference_net,
                                              measure_against_reference, reference_forward_f64, within_guard)
    from cchess_alphazero.agent.model import CChessNet
    torch.manual_seed(0)
    net = CChessNet(cnn_filter_num=128, res_layer_num=7).eval()    # the benchmark's weights, policy layer x 480 (value head: exact)
    net.policy_out.weight.data.mul_(480.0)
    planes, legal = calibration_planes(256, 14, with_legal=True)
    never = (~legal.any(0)).nonzero().flatten()
    assert never.numel() > 0                                       # labels no calibration position can play
    with torch.no_grad():
        top = float(reference_forward_f64(net, planes)[2].max())
        net.policy_out.bias.data[int(never[0])] = top + 25.0       # e^-25 of the mass is left for every other label
    ref = reference_forward_f64(net, planes)
    assert float(ref[0][:, int(never[0])].min()) > 1.0 - 1e-9      # the illegal label holds the softmax
    raw = guarded_inference_net(net, torch.float32, trunk="mfma", arith="c6", guard=False, planes=planes)
    m = measure_against_reference(raw, ref, planes, legal)
    print("c6, unguarded:", m)
    assert m["policy_max_abs"] <= GUARD_TOL and m["value_max_abs"] <= GUARD_TOL          # round 4's test: passes
    assert m["logit_max_abs"] > LOGIT_TOL and m["legal_prior_max_abs"] > GUARD_TOL       # the search's priors: off
    assert not within_guard(m)
    g = guarded_inference_net(net, torch.float32, trunk="mfma", arith="c6")
    assert g.arith_effective != "c6" and g.calibration["candidates"][0]["arith"] == "c6"
    last = g.calibration["chosen"]
    assert g.arith_effective == "fp32-library" or (last["arith"] == g.arith_effective and within_guard(last))
    fresh, fresh_legal = calibration_planes(192, 14, seed=4242, with_legal=True)
    mf = measure_against_reference(g, reference_forward_f64(net, fresh), fresh, fresh_legal)
    print(f"guard: c6 -> {g.arith_effective}; fresh positions: {mf}")
    assert mf["legal_prior_max_abs"] <= 1e-4 and mf["value_max_abs"] <= 1e-4
