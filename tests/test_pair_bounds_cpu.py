"""The per-element bounds of tests/f16_pairs.py for the convolution on bf16 pairs ("bf16x3") and on plain fp16 / bf16 operands
(which tests/test_gpu_plain_bf16x3.py holds the kernels to) must tell the correct arithmetic from subtly wrong arithmetic.  No
GPU, the method of tests/test_f16x3_bounds_cpu.py: a numpy model of the kernel -- 2-byte operands, an fp32 accumulator rounded
after EVERY product in the kernel's order (tap, 16-channel step, term), the fp32 epilogue (bias, then the skip parts), the
output cast -- is fed to the very check the GPU tests use, correct and with faults:
  bf16x3:      w_lo x_hi dropped;  w_hi x_lo dropped;  hi parts only;
  plain fp16:  operands below 2^-14 (fp16 subnormals) flushed to zero, in the activations or in the filters;  one K-step skipped;
  plain bf16:  the output truncated instead of rounded to nearest even.
The correct model must pass every bound (error / bound <= 1), every fault must exceed one of them by 4x or more; the output
rounding fault must change output bits, which is what the GPU tests compare.

Data: O(1) activations, and f16_pairs.mixed_activations (board regime 2 holds only zeros and values below 2^-3, so small
operands are not buried under a large neighbour's rounding); filters at the usual 1 / (3 sqrt C) scale with every fifth output
row scaled by 2^-10 (all of its taps are fp16 subnormals).

Measured, error / bound over C = 32 and 128 and both kinds of data: the correct model 0.47 - 0.48 (a) and 0.38 - 0.44 (b) on
bf16 pairs, 0.47 - 0.61 on plain fp16; a dropped cross term 380 - 940 (a) and 10 - 67 (b), hi parts only 630 - 1400 and 18 - 91;
flushed filters and a skipped K-step above 1e5, flushed activations 108 and 122; a truncated bf16 output differs from the
rounded one in 24.8 % of the elements."""
import numpy as np
import pytest

import f16_pairs as fp

SUB = 2.0 ** -14
FORMATS = {"bf16": (fp.BF16_PAIR, fp.BF16_PLAIN), "f16": (fp.F16_PAIR, fp.F16_PLAIN)}


def cast(v, dt, nearest=True):
    """fp32 -> the 2-byte format dt ("bf16" / "f16") and back, as float32."""
    if dt == "bf16":
        return fp.bf16_round(v, nearest)
    assert nearest
    return np.asarray(v, dtype=np.float32).astype(np.float16).astype(np.float32)


def split(v, dt, parts):
    """The operand tuple (hi,) or (hi, lo) of fp32 values, as float64 arrays."""
    hi = cast(v, dt)
    return (hi.astype(np.float64),) if parts == 1 else (hi.astype(np.float64), cast(v - hi, dt).astype(np.float64))


def kernel_fp32(xs, ws, bias, ss, relu, terms, skip_step=None, per_product=True):
    """The fp32 value a convolution kernel computes before its output cast: xs / ws / ss the operand tuples (float64 values
    of 2-byte numbers), terms a sequence of (w part, x part) index pairs, one matrix instruction each per K-step.
    per_product=False rounds the accumulator once per instruction (16 products) instead of after every product."""
    n, c_in, c_out = xs[0].shape[0], xs[0].shape[-1], ws[0].shape[0]
    acc = np.zeros((n * 90, c_out), dtype=np.float32)
    part_taps = list(zip(*[list(fp.taps(x, w)) for x, w in zip(xs, ws)]))          # [tap][part] -> (x rows, w slice)
    step = 0
    for tap in part_taps:
        for c0 in range(0, c_in, 16):
            k = slice(c0, c0 + 16)
            step += 1
            if step - 1 == skip_step:
                continue
            ops = [(tap[xp][0][:, k], tap[wp][1][k]) for wp, xp in terms]
            if per_product:         # (products of 2-byte values are exact in fp32; cumsum adds in order, rounding each sum)
                seq = [acc[:, None, :]] + [(a[:, :, None] * b[None, :, :]).astype(np.float32) for a, b in ops]
                acc = np.cumsum(np.concatenate(seq, axis=1), axis=1, dtype=np.float32)[:, -1, :]
            else:
                for a, b in ops:
                    acc = (acc + a @ b).astype(np.float32)
    v = (acc.reshape(n, 90, c_out) + bias.astype(np.float32)).astype(np.float32)
    for s in ss:
        v = (v + s.astype(np.float32)).astype(np.float32)
    return np.where(v > 0, v, np.float32(0.0)) if relu else v


def data(c, kind, rng, n=3):
    if kind == "mixed":
        x = fp.mixed_activations((n, 90, c), rng, cap=1000.0)
    else:
        x = np.abs(rng.standard_normal((n, 90, c))).astype(np.float32)
    w = (rng.standard_normal((c, c, 3, 3)) / (3.0 * c ** 0.5)).astype(np.float32)
    w[::5] *= np.float32(2.0 ** -10)
    bias = rng.standard_normal(c).astype(np.float32)
    bias[::5] *= np.float32(2.0 ** -10)
    skip = (rng.standard_normal((n, 90, c)) * 2.0).astype(np.float32)
    return x, w, bias, skip


PAIR_TERMS = ((0, 0), (1, 0), (0, 1))           # w_hi x_hi, w_lo x_hi, w_hi x_lo: the kernel's order within a K-step
PAIR_FAULTS = {"correct": PAIR_TERMS, "drop w_lo*x_hi": ((0, 0), (0, 1)), "drop w_hi*x_lo": ((0, 0), (1, 0)),
               "hi only": ((0, 0),)}


@pytest.mark.parametrize("kind", ["O(1)", "mixed"])
@pytest.mark.parametrize("c", [32, 128])
def test_bf16x3_bounds_pass_the_arithmetic_and_catch_its_faults(c, kind):
    rng = np.random.default_rng(10 * c + (kind == "mixed"))
    x, w, bias, skip = data(c, kind, rng)
    xs, ws, ss = split(x, "bf16", 2), split(w, "bf16", 2), split(skip, "bf16", 2)
    check = fp.ConvCheck(xs, ws, x.astype(np.float64), w.astype(np.float64), fmt=fp.BF16_PAIR)
    ratios = {}
    for name, terms in PAIR_FAULTS.items():
        v = kernel_fp32(xs, ws, bias, ss, True, terms, per_product=name == "correct")
        hi = cast(v, "bf16")
        got = hi.astype(np.float64) + cast(v - hi, "bf16").astype(np.float64)
        ratios[name] = check.ratios(got, bias.astype(np.float64), skip=ss + (skip.astype(np.float64),), relu=True, pair_out=True)
    print("bf16x3", c, kind, {k: tuple(f"{r:.3g}" for r in v) for k, v in ratios.items()})
    assert max(ratios["correct"]) <= 1.0, ratios["correct"]
    for name, r in ratios.items():
        if name != "correct":
            assert max(r) >= 4.0, (name, r)


@pytest.mark.parametrize("kind", ["O(1)", "mixed"])
@pytest.mark.parametrize("c", [32, 128])
def test_plain_f16_bound_passes_the_arithmetic_and_catches_its_faults(c, kind):
    """fp32 output against bound (a); the 2-byte output is then a cast of it (next test).  Flushed activations can only show
    where there are fp16 subnormals among them: the mixed data (its worst element lies on the regime-2 board, which holds nothing
    larger than 2^-3 beside them)."""
    rng = np.random.default_rng(20 * c + (kind == "mixed"))
    x, w, bias, skip = data(c, kind, rng)
    xs, ws, ss = split(x, "f16", 1), split(w, "f16", 1), split(skip, "f16", 1)
    check = fp.ConvCheck(xs, ws, plain=True)
    flush = lambda t: np.where(np.abs(t) < SUB, 0.0, t)
    faults = {"correct": {}, "flush filters < 2^-14": {"ws": (flush(ws[0]),)}, "skip one K-step": {"skip_step": 4 * (c // 16) + 1}}
    if kind == "mixed":
        faults["flush activations < 2^-14"] = {"xs": (flush(xs[0]),)}
    ratios = {}
    for name, fault in faults.items():
        args = {"xs": xs, "ws": ws, **fault}
        v = kernel_fp32(args["xs"], args["ws"], bias, ss, True, ((0, 0),), skip_step=args.get("skip_step"),
                        per_product=name == "correct").astype(np.float64)
        b64 = bias.astype(np.float64)
        ratios[name] = check.ratios(v, b64, skip=ss, relu=True)[0]
    print("plain f16", c, kind, {k: f"{r:.3g}" for k, r in ratios.items()})
    assert ratios["correct"] <= 1.0, ratios["correct"]
    for name, r in ratios.items():
        if name != "correct":
            assert r >= 4.0, (name, r)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_plain_two_byte_output_bound_and_its_rounding(dt):
    """The 2-byte output of a kernel without an fp32 one (cz_input_conv) is held to ACC + EPI + ulp / 2: the correct cast passes,
    a bf16 store that truncated is off by up to twice that and changes the bits of a large share of the elements (the GPU tests
    compare the bits with torch's cast, which is this file's cast bit for bit)."""
    import torch
    c = 32
    rng = np.random.default_rng(5)
    x, w, bias, skip = data(c, "O(1)", rng)
    xs, ws = split(x, dt, 1), split(w, dt, 1)
    check = fp.ConvCheck(xs, ws, plain=True)
    v = kernel_fp32(xs, ws, bias, (), True, ((0, 0),))
    near = cast(v, dt)
    tdt = torch.bfloat16 if dt == "bf16" else torch.float16
    assert np.array_equal(torch.from_numpy(v).to(tdt).view(torch.int16).numpy(),
                          torch.from_numpy(near).to(tdt).view(torch.int16).numpy())           # = torch's cast
    assert np.array_equal(torch.from_numpy(v).to(tdt).float().numpy().view(np.uint32), near.view(np.uint32))
    r = check.ratios(near.astype(np.float64), bias.astype(np.float64), relu=True, out_fmt=FORMATS[dt][1])[0]
    print(f"plain {dt} 2-byte output: correct {r:.3g}")
    assert r <= 1.0, r
    if dt == "bf16":
        cut = cast(v, dt, nearest=False)
        share = float((cut.view(np.uint32) != near.view(np.uint32)).mean())
        rc = check.ratios(cut.astype(np.float64), bias.astype(np.float64), relu=True, out_fmt=FORMATS[dt][1])[0]
        print(f"plain bf16 truncated output: {share:.1%} of the elements differ in bits, error / bound {rc:.3g}")
        assert share >= 0.1, share
        assert rc >= 1.5, rc                    # (up to one ulp against a bound of half an ulp: below 2 by construction)


def test_half_ulp_is_the_formats_half_spacing():
    """half_ulp against the spacing numpy / torch report, on numpy arrays and torch tensors alike: normal values, powers of two,
    subnormals and zero."""
    import torch
    g = np.array([0.0, 1.0, 1.5, 2.0, 0.75, 2.0 ** -14, 2.0 ** -15, 3.0 * 2.0 ** -24, 40000.0, -3.0, 2.0 ** -24])
    want = np.spacing(np.abs(g).astype(np.float16)).astype(np.float64) / 2.0
    assert np.array_equal(fp.half_ulp(g, fp.F16_PLAIN), want)
    assert np.array_equal(fp.half_ulp(torch.from_numpy(g), fp.F16_PLAIN).numpy(), want)
    gb = np.array([1.0, 1.5, 3.0, 2.0 ** -100, 3.0e4, 0.0])
    wantb = np.array([2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -108, 2.0 ** 6, 2.0 ** -134])
    assert np.array_equal(fp.half_ulp(gb, fp.BF16_PLAIN), wantb)
    assert np.array_equal(fp.half_ulp(torch.from_numpy(gb), fp.BF16_PLAIN).numpy(), wantb)
