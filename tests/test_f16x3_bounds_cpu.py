"""The per-element bounds of tests/f16_pairs.py (which tests/test_gpu_f16x3.py holds the fp16-pair kernels to) must tell
correct f16x3 arithmetic from subtly wrong arithmetic.  No GPU: a numpy model of the kernels' arithmetic -- (hi, lo) fp16
operands, the three products, an fp32 accumulator rounded after EVERY product in the kernels' order (tap, 16-channel
step, term), the fp32 epilogue, the re-split into a pair -- is fed to the same check as the kernels' results, correct
and with three kinds of fault:
  * one cross term dropped (w_lo x_hi, or w_hi x_lo);
  * lo parts below 2^-14 (fp16 subnormals) flushed to zero, in the filters or in the activations -- what a matrix unit
    or a conversion that flushed fp16 subnormals would do;
  * hi parts only (plain fp16 arithmetic).
The correct model must pass both bounds, every fault must exceed one of them by 4x or more -- the bounds are tight
enough to catch these faults on data like the GPU tests'."""
import numpy as np
import pytest

import f16_pairs as fp

TERMS = ("hh", "lh", "hl")          # w_hi x_hi, w_lo x_hi, w_hi x_lo: the kernels' order within a K-step
SUB = 2.0 ** -14


def kernel_model(x, w, bias, skip, relu, terms=TERMS, flush_w=False, flush_x=False, per_product=True):
    """What an f16x3 convolution kernel computes, in numpy: the pair output hi + lo as float64 (module docstring).
    per_product=False rounds the accumulator once per matrix instruction (16 products) instead."""
    n, c_in, c_out = x.shape[0], x.shape[-1], w.shape[0]
    xh, xl = (t.astype(np.float64) for t in fp.split16(x))
    wh, wl = (t.astype(np.float64) for t in fp.split16(w))
    if flush_w:
        wl = np.where(np.abs(wl) < SUB, 0.0, wl)
    if flush_x:
        xl = np.where(np.abs(xl) < SUB, 0.0, xl)
    acc = np.zeros((n * 90, c_out), dtype=np.float32)
    for (xh_t, wh_t), (xl_t, wl_t) in zip(fp.taps(xh, wh), fp.taps(xl, wl)):
        ops = {"hh": (xh_t, wh_t), "lh": (xh_t, wl_t), "hl": (xl_t, wh_t)}
        for c0 in range(0, c_in, 16):
            k = slice(c0, c0 + 16)
            if per_product:         # (products of fp16 values are exact in fp32; cumsum adds in order, rounding each sum)
                seq = [acc[:, None, :]] + [(ops[t][0][:, k, None] * ops[t][1][None, k, :]).astype(np.float32) for t in terms]
                acc = np.cumsum(np.concatenate(seq, axis=1), axis=1, dtype=np.float32)[:, -1, :]
            else:
                for t in terms:
                    acc = (acc + ops[t][0][:, k] @ ops[t][1][k]).astype(np.float32)
    v = (acc.reshape(n, 90, c_out) + bias.astype(np.float32)).astype(np.float32)
    sh, sl = fp.split16(skip)
    v = (v + sh.astype(np.float32)).astype(np.float32)
    v = (v + sl.astype(np.float32)).astype(np.float32)
    if relu:
        v = np.where(v > 0, v, np.float32(0.0))
    hi, lo = fp.split16(v)
    return hi.astype(np.float64) + lo.astype(np.float64)


FAULTS = {"correct": {}, "drop w_lo*x_hi": {"terms": ("hh", "hl")}, "drop w_hi*x_lo": {"terms": ("hh", "lh")},
          "flush filter lo < 2^-14": {"flush_w": True}, "flush activation lo < 2^-14": {"flush_x": True},
          "hi only": {"terms": ("hh",)}}


@pytest.mark.parametrize("data", ["O(1)", "mixed"])
@pytest.mark.parametrize("c", [128, 256])
def test_bounds_pass_the_arithmetic_and_catch_its_faults(c, data):
    rng = np.random.default_rng(c + (data == "mixed"))
    n = 3
    if data == "mixed":
        x = fp.mixed_activations((n, 90, c), rng)
    else:
        x = np.abs(rng.standard_normal((n, 90, c))).astype(np.float32)
    w = (rng.standard_normal((c, c, 3, 3)) / (3.0 * c ** 0.5)).astype(np.float32)
    bias = rng.standard_normal(c).astype(np.float32)
    skip = (rng.standard_normal((n, 90, c)) * 2.0).astype(np.float32)
    xp = tuple(t.astype(np.float64) for t in fp.split16(x))
    wp = tuple(t.astype(np.float64) for t in fp.split16(w))
    sp = tuple(t.astype(np.float64) for t in fp.split16(skip))
    check = fp.ConvCheck(xp, wp, x.astype(np.float64), w.astype(np.float64))
    ratios = {}
    for name, fault in FAULTS.items():
        got = kernel_model(x, w, bias, skip, relu=True, per_product=name == "correct", **fault)
        ratios[name] = check.ratios(got, bias.astype(np.float64), skip=sp + (skip.astype(np.float64),), relu=True,
                                    pair_out=True)
    print(c, data, {k: tuple(f"{r:.3g}" for r in v) for k, v in ratios.items()})
    assert max(ratios["correct"]) <= 1.0, ratios["correct"]
    for name, r in ratios.items():
        if name != "correct":
            assert max(r) >= 4.0, (name, r)
