"""The per-element dense-layer bounds of tests/f16_pairs.py (DenseCheck, which tests/test_gpu_heads.py holds k_fc_tile to) must
tell the correct fp16-pair arithmetic from subtly wrong arithmetic.  No GPU: a numpy model of the kernel -- (hi, lo) fp16
features and weights, the three products of a K-step of 16 features in the kernel's order (w_hi x_hi, w_lo x_hi, w_hi x_lo), an
fp32 accumulator rounded after EVERY product (the most pessimistic reading of a matrix instruction), one fp32 addition for the
bias -- is fed to the same check as the kernel's logits, on the data generators of the GPU test (f16_pairs.dense_features, the
GPU test's weight scale), correct and with four faults:
  * lo parts of the weights below 2^-14 (fp16 subnormals) flushed to zero -- what a packer or a matrix unit that flushed them would do;
  * the same for the lo parts of the features (the kernel's staging conversion, or the matrix unit);
  * w_lo x_hi dropped in a single K-step (a wrong ring slot for one step's lo weights);
  * hi-only features (w_hi x_lo dropped throughout).
The correct model must stay within both bounds; every fault must exceed bound (a) on both data sets.
The correct model runs twice: rounded after every product (per_product=True, the figures 0.17-0.38 of (a)) and rounded once
per matrix instruction (per_product=False).  The four faults run with per_product=False only: that is the conservative choice,
since less rounding noise leaves less beside the fault to push the error over the bound (8x-350x of (a) as recorded in
EXPERIMENTS.md are those runs)."""
import numpy as np
import pytest

import f16_pairs as fp

SUB = 2.0 ** -14


def kernel_model(x, w, bias, flush_w=False, flush_x=False, drop_lh_step=None, hi_only_x=False, per_product=True):
    """What k_fc_tile computes for fp16 pairs, in numpy: logits [n, n_out] as float64."""
    f = x.shape[1]
    xh, xl = (t.astype(np.float64) for t in fp.split16(x))
    wh, wl = (t.astype(np.float64) for t in fp.split16(w))
    if flush_w:
        wl = np.where(np.abs(wl) < SUB, 0.0, wl)
    if flush_x:
        xl = np.where(np.abs(xl) < SUB, 0.0, xl)
    acc = np.zeros((x.shape[0], w.shape[0]), dtype=np.float32)
    for s, k0 in enumerate(range(0, f, 16)):
        k = slice(k0, k0 + 16)
        terms = [(xh, wh)] + ([] if drop_lh_step == s else [(xh, wl)]) + ([] if hi_only_x else [(xl, wh)])
        if per_product:            # (a product of two fp16 values is exact in fp32; cumsum adds in order, rounding each sum)
            seq = [acc[:, None, :]] + [(a[:, k, None] * b.T[None, k, :]).astype(np.float32) for a, b in terms]
            acc = np.cumsum(np.concatenate(seq, axis=1), axis=1, dtype=np.float32)[:, -1, :]
        else:
            for a, b in terms:
                acc = (acc + a[:, k] @ b[:, k].T).astype(np.float32)
    return (acc + bias.astype(np.float32)).astype(np.float64)


FAULTS = {"correct": {}, "flush weight lo < 2^-14": {"flush_w": True}, "flush feature lo < 2^-14": {"flush_x": True},
          "drop w_lo*x_hi in K-step 3": {"drop_lh_step": 3}, "hi-only features": {"hi_only_x": True}}


@pytest.mark.parametrize("data", ["O(1)", "mixed"])
@pytest.mark.parametrize("f", [180, 360])
def test_dense_bounds_pass_the_arithmetic_and_catch_its_faults(f, data):
    rng = np.random.default_rng(f + (data == "mixed"))
    n, n_out = 48, 70
    x = fp.dense_features(data, n, f, rng)
    w = (rng.standard_normal((n_out, f)) * 0.08).astype(np.float32)
    bias = (rng.standard_normal(n_out) * 0.5).astype(np.float32)
    xp = tuple(t.astype(np.float64) for t in fp.split16(x))
    wp = tuple(t.astype(np.float64) for t in fp.split16(w))
    check = fp.DenseCheck(xp, wp, x.astype(np.float64), w.astype(np.float64))
    ratios = {name: check.ratios(kernel_model(x, w, bias, per_product=name == "correct", **fault), bias.astype(np.float64))
              for name, fault in FAULTS.items()}
    print(f, data, {k: tuple(f"{r:.3g}" for r in v) for k, v in ratios.items()})
    assert max(ratios["correct"]) <= 1.0, ratios["correct"]
    # the instruction-wise rounding (16 products added before a rounding) is correct arithmetic too
    assert max(check.ratios(kernel_model(x, w, bias, per_product=False), bias.astype(np.float64))) <= 1.0
    for name, r in ratios.items():
        if name != "correct":
            assert r[0] > 1.0, (name, r)


def test_bf16_pair_format_bound():
    """e(v) of a bf16 pair as derived in f16_pairs (2^-16 |v| + 2^-134), on values over the whole fp32 range of the tests."""
    rng = np.random.default_rng(7)
    v = (rng.standard_normal(1 << 16) * np.exp2(rng.uniform(-40, 15, 1 << 16))).astype(np.float32)
    hi, lo = fp.split_pair(v, fp.BF16_PAIR)
    assert ((hi.view(np.uint32) | lo.view(np.uint32)) & 0xFFFF == 0).all()        # both parts are bf16 values
    err = np.abs(v.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64))
    assert (err <= fp.pair_err(v.astype(np.float64), fp.BF16_PAIR)).all()
    assert (err / np.abs(v)).max() > 2.0 ** -18                                   # and the bound is not slack by more than 4x
    import torch
    t = torch.from_numpy(v)
    th = t.to(torch.bfloat16)
    assert np.array_equal(hi, th.float().numpy()) and np.array_equal(lo, (t - th.float()).to(torch.bfloat16).float().numpy())
