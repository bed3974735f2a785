"""-m gpu: the fp16-pair ("f16x3") tower arithmetic -- (hi, lo) fp16 operands, w_hi x_hi + w_lo x_hi + w_hi x_lo in fp32 --
kernel by kernel against float64, with the per-element bounds derived in tests/f16_pairs.py (and shown to catch dropped
terms, flushed fp16 subnormals and hi-only arithmetic in tests/test_f16x3_bounds_cpu.py):
  (a) against float64 on the same operands: fp32 accumulation, epilogue additions, the output pair's 22 bits;
  (b) against float64 on the exact fp32 operands: (a) plus the dropped w_lo x_lo and the pairs' representation errors
      e(v) <= 2^-22 |v| + 2^-25 summed over the dot product.
Fused kernels are pinned bit for bit to the single convolution, and the 192- and 256-filter f16x3 networks to the float64
network at the 128-filter network's bar (tests/test_gpu_guard.py)."""
import numpy as np
import pytest

import f16_pairs as fp

pytestmark = pytest.mark.gpu

EPILOGUES = ((False, True, False), (True, True, False), (True, False, True), (False, False, False))   # skip, relu, out_f32


def _pair(t):
    import torch
    hi = t.to(torch.float16)
    return hi, (t - hi.float()).to(torch.float16)


def _f64(pair):
    return tuple(t.double() for t in pair)


def _weights(w):
    """The (hi, lo) pair of an fp32 filter as float64 values, split as the weight packers split it (nearest even)."""
    return _f64(_pair(w.float()))


def _bits(t):
    import torch
    return t.view(torch.int16)


def _run_conv(xs, wp, b, skip, relu, f32):
    import torch
    from cchess_alphazero import _native
    n, c = xs[0].shape[0], xs[0].shape[-1]
    if f32:
        of = torch.full((n, 90, c), 7.0, device="cuda")
        _native.conv3x3(xs, wp, b, skip=skip, out_f32=of, relu=relu)
        return of
    out = tuple(torch.full((n, 90, c), 7.0, device="cuda", dtype=torch.float16) for _ in range(2))
    _native.conv3x3(xs, wp, b, skip=skip, out=out, relu=relu)
    return out


@pytest.mark.parametrize("c", [32, 128, 192, 256])
@pytest.mark.parametrize("n", [1, 2, 7, 64, 257])
def test_conv3x3_f16_pairs_against_float64(c, n):
    """cz_conv3x3 on fp16 pairs, every epilogue (skip or not, ReLU or not, pair or fp32 output), bound (a) per element;
    a pair output is the round-to-nearest-even split of the fp32 output of the same launch configuration, bit for bit
    (both epilogues compute the same fp32 value v = acc + b + s_hi + s_lo, then ReLU)."""
    import torch
    from cchess_alphazero import _native
    g = torch.Generator(device="cuda").manual_seed(3000 * c + n)
    x = torch.randn((n, 90, c), device="cuda", generator=g).relu()
    sk = torch.randn((n, 90, c), device="cuda", generator=g)
    w = torch.randn((c, c, 3, 3), device="cuda", generator=g) / (3.0 * c ** 0.5)
    b = torch.randn((c,), device="cuda", generator=g)
    wp = _native.pack_conv3x3_weights(w, torch.float16, 2).cuda()
    xs, ss = _pair(x), _pair(sk)
    check = fp.ConvCheck(_f64(xs), _weights(w), x.double(), w.double())
    worst = 0.0
    for skip, relu, f32 in EPILOGUES:
        sp = ss if skip else None
        got = _run_conv(xs, wp, b, sp, relu, f32)
        if not f32:
            ref = _run_conv(xs, wp, b, sp, relu, True)
            want = _pair(ref)
            assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1])), (skip, relu)
            got = got[0].double() + got[1].double()
        else:
            got = got.double()
        ra, rb = check.ratios(got, b.double(), skip=_f64(ss) + (sk.double(),) if skip else None, relu=relu, pair_out=not f32)
        assert ra <= 1.0, (skip, relu, f32, ra)
        worst = max(worst, ra)
    print(f"conv3x3 f16x3 C={c} n={n}: worst error / bound (a) {worst:.3g}")


@pytest.mark.parametrize("c", [32, 128, 192, 256])
def test_conv3x3_f16_pairs_range_against_exact_operands(c):
    """The range the guard admits f16x3 for: activations mixed per element over zeros, exact fp16 values, subnormal hi,
    subnormal lo, O(1) and large values up to the admission cap 3.0e4 (f16_pairs.mixed_activations), filters at the usual
    1 / (3 sqrt C) scale and scaled by 2^-3 (the factor choose_act_shift may move into filters); bound (b) against the
    exact fp32 operands, (a) as well.  Then O(1) activations with usual-scale filters: f16x3's error against the exact
    operands is at most a quarter of bf16x3's on the same data up to 128 filters (measured 1 / 12 at 32, 1 / 5.4 at 128).
    At 192 and 256 filters the taps (~1 / (3 sqrt C) = 0.024 / 0.021) have their lo parts deep in fp16's subnormals,
    whose step 2^-24 leaves a tap ~19.5 bits instead of 22 -- the format, not the kernel (bound (b) holds) --, and the
    measured ratio is 1 / 4.0 and 1 / 3.2: asserted <= 0.4 there.  Flushed lo parts would cost every product 2^-12 of its
    size, some 30x bf16x3's error."""
    import torch
    from cchess_alphazero import _native
    rng = np.random.default_rng(c)
    n = 6
    x = torch.from_numpy(fp.mixed_activations((n, 90, c), rng)).cuda()
    g = torch.Generator(device="cuda").manual_seed(c + 1)
    sk = torch.randn((n, 90, c), device="cuda", generator=g) * 4.0
    b = torch.randn((c,), device="cuda", generator=g)
    xs, ss = _pair(x), _pair(sk)
    for scale in (1.0, 2.0 ** -3):
        w = torch.randn((c, c, 3, 3), device="cuda", generator=g) / (3.0 * c ** 0.5) * scale
        wp = _native.pack_conv3x3_weights(w, torch.float16, 2).cuda()
        check = fp.ConvCheck(_f64(xs), _weights(w), x.double(), w.double())
        for skip, relu, f32 in EPILOGUES:
            got = _run_conv(xs, wp, b, ss if skip else None, relu, f32)
            got = got.double() if f32 else got[0].double() + got[1].double()
            assert got.abs().max().item() < fp.CAP
            ra, rb = check.ratios(got, b.double(), skip=_f64(ss) + (sk.double(),) if skip else None, relu=relu,
                                  pair_out=not f32)
            print(f"conv3x3 f16x3 range C={c} w x{scale:g} skip={skip} relu={relu} f32={f32}: (a) {ra:.3g} (b) {rb:.3g}")
            assert ra <= 1.0 and rb <= 1.0, (scale, skip, relu, f32, ra, rb)
    # f16x3 against bf16x3 on O(1) activations
    x = (torch.randn((n, 90, c), device="cuda", generator=g) * 1.5).relu()
    w = torch.randn((c, c, 3, 3), device="cuda", generator=g) / (3.0 * c ** 0.5)
    check = fp.ConvCheck(_f64(_pair(x)), _weights(w), x.double(), w.double())
    errs = {}
    for dt in (torch.float16, torch.bfloat16):
        y = torch.empty((n, 90, c), device="cuda")
        xh = x.to(dt)
        _native.conv3x3((xh, (x - xh.float()).to(dt)), _native.pack_conv3x3_weights(w, dt, 2).cuda(), b, out_f32=y, relu=False)
        errs[str(dt)] = check.error(y.double(), b.double())
    print(f"conv3x3 C={c}, O(1) activations: max error vs exact operands f16x3 {errs['torch.float16']:.3g}, "
          f"bf16x3 {errs['torch.bfloat16']:.3g}")
    assert errs["torch.float16"] <= (0.25 if c <= 128 else 0.4) * errs["torch.bfloat16"], errs


def test_split_bias_act_f16_pairs_is_the_nearest_even_split():
    """cz_split_bias_act with fp16 pairs = hi = fp16(y), lo = fp16(y - hi) for y = x + b in fp32 (ReLU optional), bit for
    bit: bias None without ReLU (the hand-over of a c8>N tower to its f16x3 blocks, agent/model.py _trunk_mfma) and bias
    with ReLU; inputs over +-0, negative values, exact fp16 values, subnormal hi and lo, and up to 3.0e4."""
    import torch
    from cchess_alphazero import _native
    rng = np.random.default_rng(9)
    n, c = 13, 128
    mag = fp.mixed_activations((n, 90, c), rng).astype(np.float64)
    sign = np.where(rng.random((n, 90, c)) < 0.5, -1.0, 1.0)
    x = torch.from_numpy((sign * mag).astype(np.float32)).cuda()
    x[0, 0, :4] = torch.tensor([0.0, -0.0, 3.0e4, -3.0e4])
    x[0, 1, :4] = torch.tensor([2.0 ** -24, -(2.0 ** -24), 2.0 ** -25, 3.0 * 2.0 ** -26])     # tiny: ties / the smallest step
    b = torch.from_numpy((rng.standard_normal(c) * 0.01).astype(np.float32)).cuda()
    for bias, relu in ((None, False), (b, True), (b, False)):
        out = tuple(torch.full((n, 90, c), 7.0, device="cuda", dtype=torch.float16) for _ in range(2))
        _native.split_bias_act(x, bias, out, relu=relu)
        y = x if bias is None else x + bias
        if relu:
            y = torch.where(y > 0, y, torch.zeros_like(y))
        hi = y.to(torch.float16)
        lo = (y - hi.float()).to(torch.float16)
        assert torch.equal(_bits(out[0]), _bits(hi)) and torch.equal(_bits(out[1]), _bits(lo)), (bias is None, relu)
        err = (out[0].double() + out[1].double() - y.double()).abs()
        assert (err <= fp.pair_err(y.double())).all()


@pytest.mark.parametrize("pipelined", [True, False])
def test_resblock_f16_pairs_128_equals_two_convolutions(pipelined):
    """cz_resblock on fp16 pairs at 128 filters (k_resblock_pipe / k_resblock, both schedules) = two cz_conv3x3 launches
    bit for bit: pair output, fp32 output, in place, a device-side count; the pair output is the nearest-even split of the
    fp32 output."""
    import torch
    from cchess_alphazero import _native
    c = 128
    g = torch.Generator(device="cuda").manual_seed(41)
    ws = [torch.randn((c, c, 3, 3), device="cuda", generator=g) / (3.0 * c ** 0.5) for _ in range(2)]
    bs = [torch.randn((c,), device="cuda", generator=g) for _ in range(2)]
    ps = [_native.pack_conv3x3_weights(w, torch.float16, 2).cuda() for w in ws]
    old = _native.resblock_pipelined(pipelined)
    try:
        for n in (1, 3, 257, 700):
            xs = _pair(torch.randn((n, 90, c), device="cuda", generator=g).relu())
            t = tuple(torch.empty_like(xs[0]) for _ in range(2))
            want = tuple(torch.empty_like(xs[0]) for _ in range(2))
            _native.conv3x3(xs, ps[0], bs[0], out=t)
            _native.conv3x3(t, ps[1], bs[1], skip=xs, out=want)
            got = tuple(torch.full_like(xs[0], 7.0) for _ in range(2))
            _native.resblock(xs, ps[0], bs[0], ps[1], bs[1], out=got)
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want)), n
            want_f = torch.empty((n, 90, c), device="cuda")
            _native.conv3x3(t, ps[1], bs[1], skip=xs, out_f32=want_f)
            got_f = torch.full((n, 90, c), 7.0, device="cuda")
            _native.resblock(xs, ps[0], bs[0], ps[1], bs[1], out_f32=got_f)
            assert torch.equal(got_f, want_f), n
            split = _pair(got_f)
            assert torch.equal(_bits(got[0]), _bits(split[0])) and torch.equal(_bits(got[1]), _bits(split[1])), n
            xi = tuple(a.clone() for a in xs)
            _native.resblock(xi, ps[0], bs[0], ps[1], bs[1], out=xi)
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(xi, want)), n
            if n > 3:
                cnt = n // 2 + 1
                y = tuple(torch.full_like(xs[0], 7.0) for _ in range(2))
                _native.resblock(xs, ps[0], bs[0], ps[1], bs[1], out=y,
                                 count=torch.tensor([cnt], dtype=torch.int32, device="cuda"))
                for part in range(2):
                    assert torch.equal(_bits(y[part][:cnt]), _bits(want[part][:cnt])) and (y[part][cnt:] == 7.0).all()
    finally:
        _native.resblock_pipelined(old)


@pytest.mark.parametrize("c,in_planes", [(128, 14), (128, 28), (192, 14), (256, 14), (256, 28)])
@pytest.mark.parametrize("pdt", ["float32", "uint8"])
def test_input_conv_f16_pairs_against_float64(c, in_planes, pdt):
    """cz_input_conv with fp16-pair filters on 0 / 1 feature planes: bounds (a) and (b) per element (the planes are exact
    in fp16: x_lo = 0, e(x) = 0; 25 taps of 16-channel K-steps)."""
    import torch
    from cchess_alphazero import _native
    n = 9
    g = torch.Generator(device="cuda").manual_seed(7 * c + in_planes)
    planes = (torch.rand((n, in_planes, 10, 9), device="cuda", generator=g) < 0.15).float()
    w = torch.randn((c, in_planes, 5, 5), device="cuda", generator=g) / (5.0 * in_planes ** 0.5)
    b = torch.randn((c,), device="cuda", generator=g)
    wp = _native.pack_input_conv_weights(w, torch.float16, 2).cuda()
    out = tuple(torch.full((n, 90, c), 7.0, device="cuda", dtype=torch.float16) for _ in range(2))
    _native.input_conv(planes.to(getattr(torch, pdt)), wp, b, out)
    x = planes.permute(0, 2, 3, 1).reshape(n, 90, in_planes).double()
    check = fp.ConvCheck((x, torch.zeros_like(x)), _weights(w), x, w.double())
    ra, rb = check.ratios(out[0].double() + out[1].double(), b.double(), relu=True, pair_out=True)
    print(f"input_conv f16x3 C={c} planes={in_planes} {pdt}: (a) {ra:.3g} (b) {rb:.3g}")
    assert ra <= 1.0 and rb <= 1.0, (ra, rb)


@pytest.mark.parametrize("n,npol", [(1, 4), (5, 2), (300, 4)])
def test_resblock_heads_f16_pairs_equals_resblock_then_head_convs(n, npol):
    """cz_resblock_heads on fp16 pairs (CZ_F16) = cz_resblock (fp32 out) followed by cz_head_convs.  Both head sums are
    the same 128 products + bias in fp32 in different orders: each of their <= 2 * 128 + 1 roundings is <= u S,
    S = sum |x_c w_c| + |b|; independent zero-mean errors, 8 standard deviations: |d| <= 8 u sqrt(2 (2 * 128 + 1) / 3) S
    per element."""
    import torch
    from cchess_alphazero import _native
    c = 128
    g = torch.Generator(device="cuda").manual_seed(n + 50)
    x = torch.randn((n, 90, c), device="cuda", generator=g).relu()
    ws = [torch.randn((c, c, 3, 3), device="cuda", generator=g) / (3.0 * c ** 0.5) for _ in range(2)]
    bs = [torch.randn((c,), device="cuda", generator=g) for _ in range(2)]
    ps = [_native.pack_conv3x3_weights(w, torch.float16, 2).cuda() for w in ws]
    hw = torch.randn((6, c), device="cuda", generator=g) / c ** 0.5
    hb = torch.randn((6,), device="cuda", generator=g)
    xs = _pair(x)
    mid = torch.empty((n, 90, c), device="cuda")
    _native.resblock(xs, ps[0], bs[0], ps[1], bs[1], out_f32=mid)
    pf0 = torch.empty((n, npol * 90), device="cuda")
    vf0 = torch.empty((n, (6 - npol) * 90), device="cuda")
    _native.head_convs(mid, hw, hb, npol, pf0, vf0)
    pf, vf = torch.full_like(pf0, 7.0), torch.full_like(vf0, 7.0)
    _native.resblock_heads(xs, ps[0], bs[0], ps[1], bs[1], hw, hb, npol, pf, vf)
    s = (mid.double().abs() @ hw.double().abs().t() + hb.double().abs()).permute(0, 2, 1)        # [n, 6, 90]
    bound = fp.LAMBDA * fp.U * (2.0 * (2 * c + 1) / 3.0) ** 0.5 * s
    d = torch.cat([(pf - pf0).double().view(n, npol, 90), (vf - vf0).double().view(n, 6 - npol, 90)], dim=1)
    ratio = (d.abs() / bound).max().item()
    print(f"resblock_heads f16x3 n={n}: worst difference / bound {ratio:.3g}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("filters,blocks", [(256, 2), (192, 3)])
def test_f16x3_network_against_float64(filters, blocks):
    """The whole peaked-policy network on f16x3 (256 filters: cz_input_conv + cz_conv3x3 launches; 192: the fused pair
    blocks) against the float64 network on fresh positions: policy and value within 2.5e-5, the 128-filter network's
    bar (tests/test_gpu_guard.py) -- except the value at 256 filters.  That network's value head amplifies the trunk's
    error about 3x more than the 128-filter one's: bf16x3 is off by 3.5e-4 there (1.2e-4 at 2 x 128), f16x3 by 3.0e-5
    (1.4e-5), the same ~1 / 10 of bf16x3 at both widths, with every 256-filter kernel inside its per-element bound above.
    So at 256 filters the value is held to the guard's own tolerance (GUARD_TOL) and to a quarter of bf16x3's error on the
    same positions.  The guard asked for c8 (which 256 filters do not have) ends on f16x3 itself, not on bf16x3 or the
    fp32 library trunk."""
    import torch
    from cchess_alphazero.agent.model import (GUARD_TOL, InferenceNet, calibration_planes, guarded_inference_net,
                                              measure_against_reference, reference_forward_f64)
    from test_gpu_guard import peaked_net
    net = peaked_net(60.0, blocks=blocks, filters=filters)
    fresh = calibration_planes(128, 14, seed=4000 + filters)
    ref = reference_forward_f64(net, fresh)
    inf = InferenceNet(net, torch.float32, trunk="mfma", arith="f16x3").cuda()
    assert inf.arith_name == "f16x3"
    m = measure_against_reference(inf, ref, fresh)
    print(f"f16x3 {blocks} x {filters} (max p {float(ref[0].max()):.3f}): policy {m['policy_max_abs']:.2e} "
          f"value {m['value_max_abs']:.2e} logit {m['logit_max_abs']:.2e}")
    assert m["policy_max_abs"] < 2.5e-5, m
    if filters != 256:
        assert m["value_max_abs"] < 2.5e-5, m
    else:
        mb = measure_against_reference(InferenceNet(net, torch.float32, trunk="mfma", arith="bf16x3").cuda(), ref, fresh)
        print(f"bf16x3 {blocks} x {filters}: policy {mb['policy_max_abs']:.2e} value {mb['value_max_abs']:.2e}")
        assert m["value_max_abs"] < GUARD_TOL and m["value_max_abs"] <= 0.25 * mb["value_max_abs"], (m, mb)
    if filters == 256:
        gd = guarded_inference_net(net, torch.float32, trunk="mfma", arith="c8")
        print(f"guard at 256 filters: c8 -> {gd.arith_effective}, candidates {gd.calibration['candidates']}")
        assert gd.arith_effective == "f16x3", gd.calibration["candidates"]
