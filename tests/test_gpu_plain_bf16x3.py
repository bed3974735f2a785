"""-m gpu: the convolutions on plain 2-byte operands (parts = 1, fp16 or bf16: one matrix instruction per K-step) and on bf16
pairs ("bf16x3": w_hi x_hi + w_lo x_hi + w_hi x_lo) against float64, element by element, with the bounds derived in
tests/f16_pairs.py (part BF16 PAIRS AND PLAIN OPERANDS) and shown to catch dropped terms, flushed fp16 subnormals, a skipped
K-step and a truncating store in tests/test_pair_bounds_cpu.py:
  (a) against float64 on the same operands: fp32 accumulation and the epilogue's additions (plus, for cz_input_conv's plain
      2-byte output, half a unit of the last place of the output format);
  (b) bf16 pairs only, against float64 on the exact fp32 operands: (a) plus the dropped w_lo x_lo and the pairs' representation
      errors e(v) <= 2^-16 |v| summed over the dot product.
cz_conv3x3 and cz_input_conv are the roots every fused kernel on these operands hangs off by bit-identity tests
(tests/test_gpu_conv.py, tests/test_gpu_tower.py); the last test here adds the link from cz_tower_plain to cz_resblock.

  a. cz_conv3x3 on N(0, 1) data, four epilogues, every (filters, mode) instantiation, board counts that leave a workgroup half
     empty and quarter full: fp32 output inside (a); the 2-byte output = the nearest-even cast of it, bit for bit;
  b. range data (zeros, subnormals, exact values, O(1), large; output rows scaled by 0.004 and 50): (a), (b) for pairs, and one
     fp32 result above 65504 whose fp16 store is torch's cast of it (+inf: the hardware conversion overflows as IEEE does);
  c. w = 0: the epilogue's fp32 sum (0 + b) + s_hi + s_lo and its cast on planted +-0, ties, near-ties, subnormals, negatives;
  d. each of the 9 taps as a one-hot filter: the shifted, channel-rotated board exactly;
  e. cz_input_conv per element;  f. cz_split_bias_act bit for bit;  g. cz_tower_plain = a loop of cz_resblock, bit for bit.

Measured on an MI355X, worst error / bound per kernel and mode over all widths and board counts (the limit is 1.0, from the
derivation; a later change to the K loop is judged against these figures, which test_z_report_gpu_seconds prints again):
  cz_conv3x3, N(0, 1) data, (a):   plain bf16 0.206 (32 filters; 0.162 / 0.134 / 0.175 at 128 / 192 / 256), plain fp16 0.193
                                   (0.174 / 0.181 / 0.166), bf16 pairs 0.154 (0.133 / 0.133 / 0.148);
  cz_conv3x3, range data:          plain bf16 (a) 0.713, plain fp16 (a) 0.712, bf16 pairs (a) 0.466 (b) 0.508 -- where the products
                                   are tiny the error is the one rounding of acc + b, which reaches U |v| when v lies just above
                                   a power of two, against a bound of U (|y| + |b|);
  cz_input_conv:                   bf16 pairs (a) 0.472 (b) 0.358; plain bf16 0.99978, plain fp16 0.99899 -- the 2-byte cast's own
                                   half unit of the last place is all but the whole bound there, and some element always comes
                                   within 1e-3 of a tie; no element differed from the cast of the float64 value itself.
156 tests, 6.3 - 6.7 s on the GPU since import (tests/test_gpu_f16x3.py: 42 tests, 5.0 s)."""
import functools
import time

import numpy as np
import pytest

import f16_pairs as fp
from test_gpu_f16x3 import EPILOGUES             # (skip, relu, out_f32) x 4

pytestmark = pytest.mark.gpu

T0 = time.time()
COUNTS = (1, 2, 3, 5, 7, 257)
WIDTHS = (32, 128, 192, 256)
MODES = {"bf16": ("bfloat16", 1), "f16": ("float16", 1), "bf16x3": ("bfloat16", 2)}
OUT_FMT = {"bf16": fp.BF16_PLAIN, "f16": fp.F16_PLAIN}
WORST = {}                      # (kernel, mode) -> worst error / bound (a), (b), printed by test_z_report_gpu_seconds


def _note(kernel, mode, ra, rb=None):
    a, b = WORST.get((kernel, mode), (0.0, 0.0))
    WORST[(kernel, mode)] = (max(a, ra), max(b, rb or 0.0))


def _mode(mode):
    import torch
    dt, parts = MODES[mode]
    return getattr(torch, dt), parts


def _split(t, dtype, parts):
    """The operand tuple of fp32 values: torch's casts (round to nearest even), hi and the remainder's."""
    hi = t.to(dtype)
    return (hi,) if parts == 1 else (hi, (t - hi.float()).to(dtype))


def _f64(ts):
    return tuple(t.double() for t in ts)


def _same_bits(got, want):
    """Tuples of 2-byte tensors equal as int16 (so that -0 and +0 differ), or two fp32 tensors as int32."""
    import torch
    if not isinstance(got, tuple):
        return torch.equal(got.view(torch.int32), want.view(torch.int32))
    return len(got) == len(want) and all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(got, want))


def _run(xs, wp, b, skip, relu, f32):
    """cz_conv3x3 into tensors pre-filled with 7.0: the fp32 output, or the 2-byte operand tuple."""
    import torch
    from cchess_alphazero import _native
    n, c = xs[0].shape[0], xs[0].shape[-1]
    if f32:
        of = torch.full((n, 90, c), 7.0, device="cuda")
        _native.conv3x3(xs, wp, b, skip=skip, out_f32=of, relu=relu)
        return of
    out = tuple(torch.full((n, 90, c), 7.0, device="cuda", dtype=xs[0].dtype) for _ in xs)
    _native.conv3x3(xs, wp, b, skip=skip, out=out, relu=relu)
    return out


def _check(xs, ws, x, w, **kw):
    """ConvCheck for the operand tuples xs / ws (plain: their values are the operands; pairs: x, w the fp32 values they split)."""
    if len(xs) == 1:
        return fp.ConvCheck(_f64(xs), _f64(ws), plain=True)
    return fp.ConvCheck(_f64(xs), _f64(ws), x.double(), w.double(), fmt=fp.BF16_PAIR, **kw)


def _skip64(ss, sk):
    return _f64(ss) if len(ss) == 1 else _f64(ss) + (sk.double(),)


def _row_scales(t):
    """Output rows (or biases) of very different magnitude, as folded BatchNorm scales give them."""
    t[::3] *= 0.004
    t[1::7] *= 50.0
    return t


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("c", WIDTHS)
def test_conv3x3_per_element_against_float64(c, mode, n):
    """cz_conv3x3, every epilogue (skip or not, ReLU or not, 2-byte or fp32 output): the fp32 output of each of the four launch
    configurations inside bound (a) per element, and the 2-byte output the nearest-even cast (for pairs: the nearest-even
    (hi, lo) split) of the fp32 output of the same configuration, bit for bit -- both stores take the same fp32 value
    v = acc + b (+ s_hi (+ s_lo)), then ReLU."""
    import torch
    from cchess_alphazero import _native
    dtype, parts = _mode(mode)
    g = torch.Generator(device="cuda").manual_seed(5000 * c + 10 * n + parts)
    x = torch.randn((n, 90, c), device="cuda", generator=g).relu()
    sk = torch.randn((n, 90, c), device="cuda", generator=g)
    w = torch.randn((c, c, 3, 3), device="cuda", generator=g) / (3.0 * c ** 0.5)
    b = torch.randn((c,), device="cuda", generator=g)
    wp = _native.pack_conv3x3_weights(w, dtype, parts).cuda()
    xs, ss = _split(x, dtype, parts), _split(sk, dtype, parts)
    check = _check(xs, _split(w, dtype, parts), x, w)
    worst = 0.0
    for skip, relu, f32 in EPILOGUES:
        sp = ss if skip else None
        ref = _run(xs, wp, b, sp, relu, True)
        if not f32:
            got = _run(xs, wp, b, sp, relu, False)
            assert _same_bits(got, _split(ref, dtype, parts)), (skip, relu)
        ra = check.ratios(ref.double(), b.double(), skip=_skip64(ss, sk) if skip else None, relu=relu)[0]
        assert ra <= 1.0, (skip, relu, f32, ra)
        worst = max(worst, ra)
    _note("conv3x3", mode, worst)
    print(f"conv3x3 {mode} C={c} n={n}: worst error / bound (a) {worst:.3g}")


@functools.lru_cache(maxsize=None)
def _mixed(c, cap):
    """f16_pairs.mixed_activations for the largest board count, drawn once per width (a slice keeps each board's regime)."""
    return fp.mixed_activations((max(COUNTS), 90, c), np.random.default_rng(int(c + cap)), cap=cap)


F16_CAP = 500.0         # plain fp16: with rows scaled by 50 no exact result reaches 6e4 (asserted), so only the planted one overflows


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("c", WIDTHS)
def test_conv3x3_range_data(c, mode):
    """Activations mixed per element over zeros, exact fp16 values, values below 2^-14 (fp16 subnormals), 2^-14 .. 2^-3, O(1) and
    large ones (up to 3.0e4; 500 for fp16 operands), board regime 2 holding only the small kinds; filters at the usual
    1 / (3 sqrt C) scale with output rows scaled by 0.004 and by 50, biases alike.  Bound (a) for every mode, (b) for pairs; the
    2-byte output again the cast of the fp32 one.  Plain fp16: one skip value of 65504 sits on the largest conv + bias value of
    board 0, so that fp32 result exceeds 65504 (asserted): its 2-byte store has the bits of torch's cast (+inf)."""
    import torch
    from cchess_alphazero import _native
    dtype, parts = _mode(mode)
    g = torch.Generator(device="cuda").manual_seed(77 * c + parts)
    w = _row_scales(torch.randn((c, c, 3, 3), device="cuda", generator=g) / (3.0 * c ** 0.5))
    b = _row_scales(torch.randn((c,), device="cuda", generator=g))
    wp = _native.pack_conv3x3_weights(w, dtype, parts).cuda()
    ws = _split(w, dtype, parts)
    worst_a = worst_b = 0.0
    for n in COUNTS:
        x = torch.from_numpy(_mixed(c, F16_CAP if mode == "f16" else fp.CAP)[:n]).cuda()
        sk = torch.randn((n, 90, c), device="cuda", generator=g) * 4.0
        xs = _split(x, dtype, parts)
        check = _check(xs, ws, x, w)
        planted = None
        if mode == "f16":
            assert (check.y3 + b.double()).abs().max().item() + sk.abs().max().item() < 6.0e4
            planted = np.unravel_index(int((check.y3[0] + b.double()).argmax()), (90, c))
            sk[0, planted[0], planted[1]] = 65504.0
        ss = _split(sk, dtype, parts)
        for skip, relu, f32 in EPILOGUES:
            sp = ss if skip else None
            ref = _run(xs, wp, b, sp, relu, True)
            if not f32:
                got = _run(xs, wp, b, sp, relu, False)
                assert _same_bits(got, _split(ref, dtype, parts)), (n, skip, relu)
                if planted is not None and skip:
                    v, h = ref[0, planted[0], planted[1]], got[0][0, planted[0], planted[1]]
                    assert v.item() > 65520.0 and torch.isinf(h) and h > 0, (v.item(), h.item())
                    assert int(torch.isinf(got[0]).sum()) == 1
            ra, rb = check.ratios(ref.double(), b.double(), skip=_skip64(ss, sk) if skip else None, relu=relu)
            assert ra <= 1.0 and (rb is None or rb <= 1.0), (n, skip, relu, f32, ra, rb)
            worst_a, worst_b = max(worst_a, ra), max(worst_b, rb or 0.0)
    _note("conv3x3 range", mode, worst_a, worst_b)
    print(f"conv3x3 range {mode} C={c}: worst error / bound (a) {worst_a:.3g}" + (f" (b) {worst_b:.3g}" if parts == 2 else ""))


# the zero-filter test's biases (one per channel, cycled) and skip values (one per pixel, cycled): their fp32 sums, and the
# biases on their own, are +-0, exact ties of bf16 (1 + 2^-8, 3 + 2^-7) and of fp16 (1 + 2^-11) in both parities, values
# just above and below such ties, fp16 subnormals and their ties, values that round to -0, and negative values
B_VALUES = (0.0, -0.0, 2.0 ** -8, -(2.0 ** -8), 2.0 ** -8 + 2.0 ** -20, 2.0 ** -8 - 2.0 ** -20, 2.0 ** -7, 2.0 ** -11, -(2.0 ** -11),
            2.0 ** -11 + 2.0 ** -23, 2.0 ** -11 - 2.0 ** -23, 2.0 ** -20, 3.0 * 2.0 ** -26, -(2.0 ** -26), 2.0 ** -24, 2.0 ** -25,
            3.0 * 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, -1.5, 0.3, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 3.0 + 2.0 ** -7,
            3.0 + 2.0 ** -6 + 2.0 ** -7, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10 + 2.0 ** -11, 1.0 + 2.0 ** -8 + 2.0 ** -20,
            1.0 + 2.0 ** -8 - 2.0 ** -20, -(1.0 + 2.0 ** -8), -(2.0 ** -140))
S_VALUES = (0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -7, 3.0, 3.0 + 2.0 ** -6, -3.0, 2.0 ** -14, 1.0 + 2.0 ** -10, -2.5, 1.0 + 2.0 ** -12,
            100.0, -(2.0 ** -8))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("c", [128, 256])
def test_conv3x3_zero_filter_gives_the_epilogue_sum_exactly(c, mode):
    """w = 0 (activations random, both signs): the result is the kernel's own fp32 sum (0 + b), then + s_hi, then + s_lo,
    emulated with torch in fp32, then ReLU; the fp32 output has its bits, the 2-byte output those of its nearest-even cast /
    split.  Every combination of B_VALUES (per channel) and S_VALUES (per pixel), skip on and off, ReLU on and off."""
    import torch
    from cchess_alphazero import _native
    dtype, parts = _mode(mode)
    n = 3
    g = torch.Generator(device="cuda").manual_seed(c)
    xs = _split(torch.randn((n, 90, c), device="cuda", generator=g) * 3.0, dtype, parts)
    wp = _native.pack_conv3x3_weights(torch.zeros((c, c, 3, 3)), dtype, parts).cuda()
    b = torch.tensor(B_VALUES, dtype=torch.float64).to(torch.float32).repeat(c // len(B_VALUES) + 1)[:c].cuda()
    assert c >= len(B_VALUES) and n * 90 >= len(B_VALUES) * len(S_VALUES) // 2
    s_pix = torch.tensor(S_VALUES, dtype=torch.float32).repeat(n * 90 // len(S_VALUES) + 1)[:n * 90].cuda()
    ss = _split(s_pix.view(n, 90, 1).expand(n, 90, c).contiguous(), dtype, parts)
    neg_zero = False
    for skip in (False, True):
        v = torch.zeros((n, 90, c), device="cuda") + b
        if skip:
            for part in ss:
                v = v + part.float()
        for relu in (False, True):
            want = torch.where(v > 0, v, torch.zeros_like(v)) if relu else v
            assert _same_bits(_run(xs, wp, b, ss if skip else None, relu, True), want), (skip, relu, "fp32")
            want2 = _split(want, dtype, parts)
            assert _same_bits(_run(xs, wp, b, ss if skip else None, relu, False), want2), (skip, relu, "2-byte")
            neg_zero |= bool((want2[0].view(torch.int16) == -32768).any())
    assert neg_zero                      # (the planted values do reach -0 in this format)


@functools.lru_cache(maxsize=None)
def _one_hot_pack(c, mode, tap):
    import torch
    from cchess_alphazero import _native
    dtype, parts = _mode(mode)
    w = torch.zeros((c, c, 3, 3))
    w[torch.arange(c), (torch.arange(c) + 1) % c, tap // 3, tap % 3] = 1.0
    return _native.pack_conv3x3_weights(w, dtype, parts).cuda()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("c", WIDTHS)
def test_conv3x3_every_tap_is_a_shift(c, mode):
    """For each of the 9 taps the one-hot filter w[o, (o + 1) % C, ky, kx] = 1: the output is exactly the board shifted by the
    tap and rotated by one channel, with (+)zeros where the tap leaves the board; integer activations in [-125, 125] are exact in
    both formats (the lo part of a pair is zero, and so is the output's)."""
    import torch
    dtype, parts = _mode(mode)
    zero_b = torch.zeros(c, device="cuda")
    for n in COUNTS:
        x = (torch.arange(n * 90 * c, device="cuda") % 251 - 125).float().reshape(n, 90, c)
        xs = _split(x, dtype, parts)
        src = x.view(n, 10, 9, c).roll(-1, dims=3)
        for tap in range(9):
            dy, dx = tap // 3 - 1, tap % 3 - 1
            out = _run(xs, _one_hot_pack(c, mode, tap), zero_b, None, False, False)
            want = torch.zeros((n, 10, 9, c), device="cuda")
            y0, y1, x0, x1 = max(0, -dy), 10 - max(0, dy), max(0, -dx), 9 - max(0, dx)
            want[:, y0:y1, x0:x1] = src[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            assert _same_bits(out, _split(want.view(n, 90, c), dtype, parts)), (n, tap)


@pytest.mark.parametrize("pdt", ["float32", "uint8"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("in_planes", [14, 28])
@pytest.mark.parametrize("c", WIDTHS)
def test_input_conv_per_element_against_float64(c, in_planes, mode, pdt):
    """cz_input_conv on 0 / 1 feature planes (exact in either format: x_lo = 0, e(x) = 0), filters the packer's nearest-even
    values, 25 taps of 16-channel K-steps, bias and ReLU.  Pairs: bounds (a) and (b).  Plain: the 2-byte output -- this entry
    point has no fp32 one -- within ACC + EPI + half a unit of its last place of the float64 value, which is where the nearest-
    even cast of a value inside (a) must lie; the share of elements that differ from the cast of the float64 value itself
    (those within ACC + EPI of a tie) is printed.  (With 28 planes the kernel runs both 16-channel groups of a tap against
    w_hi before w_lo; the accumulation model takes the groups in turn, as tests/test_gpu_f16x3.py does.)"""
    import torch
    from cchess_alphazero import _native
    dtype, parts = _mode(mode)
    n = 9
    g = torch.Generator(device="cuda").manual_seed(11 * c + in_planes + parts)
    planes = (torch.rand((n, in_planes, 10, 9), device="cuda", generator=g) < 0.15).float()
    w = torch.randn((c, in_planes, 5, 5), device="cuda", generator=g) / (5.0 * in_planes ** 0.5)
    b = torch.randn((c,), device="cuda", generator=g)
    wp = _native.pack_input_conv_weights(w, dtype, parts).cuda()
    out = tuple(torch.full((n, 90, c), 7.0, device="cuda", dtype=dtype) for _ in range(parts))
    _native.input_conv(planes.to(getattr(torch, pdt)), wp, b, out)
    x = planes.permute(0, 2, 3, 1).reshape(n, 90, in_planes)
    xs = (x,) if parts == 1 else (x, torch.zeros_like(x))
    check = _check(xs, _split(w, dtype, parts), x, w, x_exact=True)
    got = sum(o.double() for o in out)
    if parts == 1:
        ra, rb = check.ratios(got, b.double(), relu=True, out_fmt=OUT_FMT[mode])
        cast = torch.relu(check.y3 + b.double()).to(dtype)
        print(f"input_conv {mode} C={c} planes={in_planes} {pdt}: (a) {ra:.5g}; "
              f"{float((cast.view(torch.int16) != out[0].view(torch.int16)).float().mean()):.2%} differ from the float64 value's cast")
    else:
        ra, rb = check.ratios(got, b.double(), relu=True, pair_out=True)
        print(f"input_conv {mode} C={c} planes={in_planes} {pdt}: (a) {ra:.3g} (b) {rb:.3g}")
    _note("input_conv", mode, ra, rb)
    assert ra <= 1.0 and (rb is None or rb <= 1.0), (ra, rb)


@pytest.mark.parametrize("mode", list(MODES))
def test_split_bias_act_is_the_nearest_even_cast(mode):
    """cz_split_bias_act with bf16 pairs and with parts = 1 in both dtypes (the entry point accepts it): the torch casts of
    y = x + b in fp32 (ReLU optional), bit for bit, for bias None or given and ReLU on or off; inputs over +-0, negative
    values, exact values, ties of either format in both parities, tiny and large values (beyond fp16's range for parts = 1
    as well: +-inf, as torch's cast gives); a pair stands for y to pair_err(y, BF16_PAIR)."""
    import torch
    from cchess_alphazero import _native
    dtype, parts = _mode(mode)
    rng = np.random.default_rng(9)
    n, c = 13, 128
    mag = fp.mixed_activations((n, 90, c), rng).astype(np.float64)
    sign = np.where(rng.random((n, 90, c)) < 0.5, -1.0, 1.0)
    x = torch.from_numpy((sign * mag).astype(np.float32)).cuda()
    x[0, 0, :6] = torch.tensor([0.0, -0.0, 3.0e4, -3.0e4, 7.0e4, -7.0e4])
    x[0, 1, :4] = torch.tensor([2.0 ** -24, -(2.0 ** -24), 2.0 ** -25, 3.0 * 2.0 ** -26])     # tiny: ties / the smallest step
    x[0, 2, :6] = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 3.0 + 2.0 ** -7, 1.0 + 2.0 ** -11,
                                1.0 + 2.0 ** -10 + 2.0 ** -11, -(1.0 + 2.0 ** -8)])
    b = torch.from_numpy((rng.standard_normal(c) * 0.01).astype(np.float32)).cuda()
    b[:6] = 0.0                                              # (the planted values stay what they are)
    for bias in (None, b):
        for relu in (False, True):
            out = tuple(torch.full((n, 90, c), 7.0, device="cuda", dtype=dtype) for _ in range(parts))
            _native.split_bias_act(x, bias, out, relu=relu)
            y = x if bias is None else x + bias
            if relu:
                y = torch.where(y > 0, y, torch.zeros_like(y))
            assert _same_bits(out, _split(y, dtype, parts)), (bias is None, relu)
            if parts == 2:
                err = (out[0].double() + out[1].double() - y.double()).abs()
                assert (err <= fp.pair_err(y.double(), fp.BF16_PAIR)).all()


@pytest.mark.parametrize("dt", ["float16", "bfloat16"])
def test_tower_plain_equals_a_loop_of_resblocks(dt):
    """cz_tower_plain over 1, 2 and 3 blocks = as many cz_resblock launches on plain operands, bit for bit, on range data
    (mixed activations up to 30, filter rows and biases scaled by 0.004 and by 4) for a lone board, a half-empty pair of
    boards, an odd count and many workgroups."""
    import torch
    from cchess_alphazero import _native
    dtype, c = getattr(torch, dt), 256
    g = torch.Generator(device="cuda").manual_seed(23)
    blocks = []
    for _ in range(3):
        blk = []
        for _ in range(2):
            w = torch.randn((c, c, 3, 3), device="cuda", generator=g) / (3.0 * c ** 0.5)
            bias = torch.randn((c,), device="cuda", generator=g)
            for t in (w, bias):
                t[::3] *= 0.004
                t[1::7] *= 4.0
            blk += [_native.pack_conv3x3_weights(w, dtype, 1).cuda(), bias]
        blocks.append(tuple(blk))
    for n in (1, 2, 3, 257):
        x = torch.from_numpy(_mixed(c, 30.0)[:n]).cuda().to(dtype)
        want = x
        for nb in (1, 2, 3):
            y = torch.full_like(x, 7.0)
            _native.resblock((want,), *blocks[nb - 1], out=(y,))
            want = y
            got = _native.tower_plain(x, blocks[:nb], torch.full_like(x, 7.0))
            assert torch.isfinite(got.float()).all() and got.float().abs().max().item() > 1.0, (n, nb)
            assert _same_bits((got,), (want,)), (n, nb)


def test_z_report_gpu_seconds():
    """Not a check: prints the worst ratios this file measured and what it cost."""
    import torch
    torch.cuda.synchronize()
    for (kernel, mode), (ra, rb) in sorted(WORST.items()):
        print(f"\n{kernel} {mode}: worst error / bound (a) {ra:.5g}" + (f" (b) {rb:.3g}" if rb else ""), end="")
    print(f"\ntests/test_gpu_plain_bf16x3.py: {time.time() - T0:.1f} s since import")
