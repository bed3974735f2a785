"""The check tests/c6_model.py builds can tell right from wrong (numpy, no GPU): a correct emulation of a c6 residual block
-- operands decoded from the bytes, products in float64, accumulation in fp32 step by step in the K loop's order, the
intermediate image re-encoded from that fp32 value -- stays under the per-element bound, and every listed fault of a reader,
a converter or the sum exceeds it at least twofold somewhere.  Also: the image codec round trip and the fact the skip path
and the identity-filter test of tests/test_gpu_c6_elements.py rest on (hi + lo6 2^(k - 11) is an fp32 number)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "chinesechess-alphazero_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import c6_model as m  # noqa: E402

f32 = lambda a: a.astype(np.float32).astype(np.float64)


def emulate_conv(xv, wv, start):
    """A kernel's convolution: fp32 accumulators, one rounding per K-loop step (the step's products summed in float64)."""
    n, C, O = xv[0].shape[0], xv[0].shape[-1], wv[0].shape[0]
    xt = [m._taps(v) for v in xv]
    acc = f32(np.zeros((n * 90, O)) + np.asarray(start).reshape(-1, O))
    for tap, op, c0, k in m.kloop_steps(C):
        acc = f32(acc + xt[op][tap][:, c0:c0 + k] @ wv[op][:, c0:c0 + k, tap].T)
    return acc.reshape(n, 90, O)


def bf6_trunc(v):
    a = np.minimum(np.abs(v), m.BF6_MAX)
    step = m.bf6_step(a)
    return np.sign(v) * np.floor(a / step) * step


def bf6_wrap(v):
    """Nearest even without the clamp: the exponent field of a value that rounds to 32 or more wraps around (3 bits)."""
    a = np.abs(v)
    step = m.bf6_step(a)
    q = np.rint(a / step) * step
    mant, e = np.frexp(q)
    field = (e + 2) & 7
    wrapped = np.where(field == 0, (mant * 8 - 4) / 16.0, mant * 2 * 2.0 ** (field - 3))
    return np.sign(v) * np.where(q >= 32.0, wrapped, q)


def emulate_block(case, fault=None):
    """The block of `case` as a kernel computes it, with one thing wrong if `fault` names it."""
    C, kx, kmid = case["C"], m.K_X, m.K_MID
    reader, k_lo, k_val = {}, kx, kx
    if fault == "elements swapped":                            # odd / even elements of every piece
        reader["elem_ch"] = m.ELEM_CH[np.arange(32) ^ 1]
    if fault == "tail from the wrong chunk":                   # lo piece of block 1: its tail read where block 0's tail sits
        off = m.piece_offsets(C)
        offsets = np.stack([off, off + 16], -1)
        offsets[0, 1, 1] = offsets[0, 0, 1]
        reader["offsets"] = offsets
    if fault == "value exponent + 1":
        k_val = kx + 1
    if fault == "lo exponent - 1":
        k_lo = kx - 1
    xv = m.image_values(case["x_hi"], case["x_img"], k_lo, k_val=k_val, **reader)
    d1, d2 = dict(case["d1"]), dict(case["d2"])
    if fault == "shifts per 32-row tile":
        for d in (d1, d2):
            d["sh"], d["sl"] = d["sh"][np.arange(C) & ~31], d["sl"][np.arange(C) & ~31]
    wv1, wv2 = m.filter_values(d1), m.filter_values(d2)
    if fault == "w_lo x dropped":
        wv1, wv2 = wv1[:2] + (wv1[2] * 0,), wv2[:2] + (wv2[2] * 0,)
    t = m.relu(emulate_conv(xv, wv1, case["b1"]))
    rnd = {"truncation": bf6_trunc, "no saturation": bf6_wrap}.get(fault, m.bf6_round)
    hi = m.to_f16(t)
    mid = (hi, rnd((t - hi) * 2.0 ** (m.LO_SHIFT - kmid)) * 2.0 ** (kmid - m.LO_SHIFT), rnd(t * 2.0 ** -kmid) * 2.0 ** kmid)
    skip = xv[0] + xv[1]
    return m.relu(emulate_conv(mid, wv2, f32(case["b2"] + skip)))


FAULTS = ["elements swapped", "tail from the wrong chunk", "value exponent + 1", "lo exponent - 1", "w_lo x dropped",
          "truncation", "shifts per 32-row tile", "no saturation"]


CONFIGS = {"second convolution on exact operands": ("identity", "random", True),      # tests/test_gpu_c6_elements.py (c)
           "first convolution": ("random", "identity", False),                          # (d), w2 = the centre-tap identity
           "general block": ("random", "random", False)}                                # (d), both filters random


@pytest.fixture(scope="module")
def cases():
    import torch
    from cchess_alphazero import _native
    C, n = 128, 3
    out = {}
    for name, (f1, f2, exact_mid) in CONFIGS.items():
        rng = np.random.default_rng(61)
        x = m.activations(n, C, m.K_X, rng)
        (w1, b1), (w2, b2) = m.filters(C, rng, identity=f1 == "identity"), m.filters(C, rng, identity=f2 == "identity")
        x_hi, x_img = m.encode_c6_image(x, m.K_X)
        d1 = m.decode_c6_pack(_native.pack_conv3x3_c6_weights(torch.from_numpy(w1), m.K_X, m.K_MID), C)
        d2 = m.decode_c6_pack(_native.pack_conv3x3_c6_weights(torch.from_numpy(w2), m.K_MID, m.K_OUT), C)
        assert len(set(d1["sh"].tolist())) >= 3 or f1 == "identity"
        assert len(set(d2["sh"].tolist())) >= 3 or f2 == "identity"
        xv = m.image_values(x_hi, x_img, m.K_X)
        model = m.c6_block(xv, xv[0] + xv[1], m.filter_values(d1), b1.astype(np.float64), m.filter_values(d2),
                           b2.astype(np.float64), m.K_MID, exact_mid=exact_mid)
        out[name] = {"C": C, "x_hi": x_hi, "x_img": x_img, "d1": d1, "d2": d2, "b1": b1.astype(np.float64),
                     "b2": b2.astype(np.float64), "model": model}
    return out


def test_correct_emulation_is_inside_the_bound_and_every_fault_is_twice_outside(cases):
    """On the three configurations of the GPU tests (3 boards, 128 filters, their inputs), largest element each.
    Observed, correct emulation / each fault as a multiple of the bound ("inf": an element whose bound is 0 -- all its terms
    are zero -- became non-zero):
                                      second conv. on exact operands   first convolution   general block
      correct emulation                          0.076                      0.950              0.058
      elements swapped                           3.1e4                      inf                193
      tail from the wrong chunk                  1.3e4                      inf                39
      value exponent + 1                         (0.076)                    5.4e3              3.6
      lo exponent - 1                            148                        1.3e3              11.7
      w_lo x dropped                             180                        5.4e3              4.8
      truncation                                 33                         43                 (0.63)
      shifts per 32-row tile                     2.1e6                      inf                4.4e4
      no saturation                              108                        34                 5.1
    (In parentheses: not caught there.  An identity first filter has no w_lo, so the value piece of ITS input is never used;
    the first-convolution figure of the correct emulation is near 1 by construction: an element whose rounding fell the other
    way uses its whole allowance.)
    A fault of a reader shows best where the convolution that reads is checked alone; the general block's bound has to pay for
    every rounding of the intermediate image that may fall the other way (about 12 % of its lo pieces lie within A1 of a
    boundary), which is why truncation -- one step of the lo piece on half the elements -- hides there and is caught by the two
    configurations with an identity filter."""
    worst = {name: 0.0 for name in FAULTS}
    for cname, case in cases.items():
        model = case["model"]
        r = m.ratio(emulate_block(case), model["y"], model["bound"])
        print(f"{cname}: correct emulation {r:.3f} of the bound")
        assert r <= 1.0, (cname, r)
        for name in FAULTS:
            rf = m.ratio(emulate_block(case, name), model["y"], model["bound"])
            print(f"    {name}: {min(rf, 1e9):.3g} x the bound")
            worst[name] = max(worst[name], rf)
    for name in FAULTS:
        assert worst[name] >= 2.0, (name, worst[name])


def test_value_piece_follows_the_pair_except_near_ties(cases):
    """The check tests/test_gpu_c6_elements.py applies to cz_input_resblock's image (the only output that entry point has on
    c6), on the correct emulation's output: the value piece equals bf6 of the pair's value except near a tie, and at most 1 % of
    the elements are near one (observed: 0.1 - 0.2 % near a tie, under 0.01 % differ)."""
    out = emulate_block(cases["general block"])
    for k in (m.K_OUT, m.K_OUT - 2, m.K_OUT + 3):
        h, lo6, hi6 = m.decode_c6_image(*m.encode_c6_image(out, k))
        near, differ, outside = m.value_piece_check(h + lo6 * 2.0 ** (k - m.LO_SHIFT), hi6, k)
        print(f"k = {k}: {100 * near:.3f} % near a tie, {100 * differ:.4f} % differ, {outside} away from a tie")
        assert outside == 0 and near <= 0.01


def test_the_bound_is_of_the_size_of_fp32_accumulation(cases):
    """The accumulation bound against the c8 test's figure for the same instructions, 1e-5 of an output's sum of |main
    terms|: several times tighter at the median (on exact operands, where nothing but accumulation enters)."""
    case = cases["second convolution on exact operands"]
    model = case["model"]
    mag = m.conv(abs(model["mid"][0]), abs(case["d2"]["w_hi"])) + abs(case["b2"]) + abs(model["mid"][0])
    rel = model["bound"] / mag
    print(f"bound / sum |terms|: median {np.median(rel):.2e}, 99 % {np.quantile(rel, 0.99):.2e}, max {rel.max():.2e}")
    assert np.median(rel) < 3e-6 and np.quantile(rel, 0.99) < 3e-5


@pytest.mark.parametrize("k", [-3, 0, 2, 5])
def test_image_round_trip_and_the_pair_is_an_fp32_number(k):
    """decode(encode(x)) gives f16(x), bf6((x - f16(x)) 2^(11 - k)) and bf6(x 2^-k) for both filter counts, on a sweep with 0,
    lo parts in bf6's subnormals, exact ties and values up to 1.5 * 28 * 2^k; the pair  hi + lo6 2^(k - 11)  is exactly an fp32
    number (the kernels form it in fp32 for the skip connection), and stands for x to 2^-14 relative for every x between
    1/64 of the image's range and its saturation point (half a step of the lo piece)."""
    from test_c6_pack_cpu import bf6_round as grid_round         # (the brute-force rounding: nearest grid point, ties to even)
    rng = np.random.default_rng(100 + k)
    s = 2.0 ** k
    for C in (128, 192):
        n = 5
        x = np.exp2(rng.uniform(-14.0, np.log2(42.0), (n, 90, C))) * s
        x[0] = np.abs(rng.standard_normal((90, C))) * 7 * s
        grid = np.array([m.bf6_value(c) for c in range(32)])
        ties = np.concatenate([grid, (grid[1:] + grid[:-1]) / 2, [29.0, 30.0, 31.0, 42.0]]) * s
        x[1, 0, :ties.size] = ties
        x[1, 1, :14] = m.planted(k)
        h16 = np.abs(rng.standard_normal(C)).astype(np.float16).astype(np.float64) * s          # f16 values + a tiny / tie lo part
        x[1, 2] = h16 + 2.0 ** np.floor(np.log2(h16 + 1e-30)) * 2.0 ** -11
        x[1, 3] = h16 + 2.0 ** (k - 11) * rng.choice(np.concatenate([grid[:8], (grid[1:8] + grid[:7]) / 2]), C)
        x = x.astype(np.float32)
        hi, img = m.encode_c6_image(x, k)
        assert hi.dtype == np.float16 and img.dtype == np.int8 and img.shape == (n, 90, 2 * C)
        assert not img.view(np.uint8)[..., ~m.image_mask(C)].any()
        h, lo6, hi6 = m.decode_c6_image(hi, img)
        x64 = x.astype(np.float64)
        assert np.array_equal(h, x.astype(np.float16).astype(np.float64))
        assert np.array_equal(lo6, grid_round((x64 - h) * 2.0 ** (11 - k))) and np.array_equal(hi6, grid_round(x64 / s))
        assert hi6.max() == 28.0 and (lo6 == 0.0625).any() and (hi6 == 0.0625).any()
        pair = h + lo6 * 2.0 ** (k - 11)
        assert np.array_equal(pair, f32(pair))
        inside = (x64 >= 28.0 * s / 64) & (x64 <= 28.0 * s)
        rel = np.abs(pair - x64)[inside] / x64[inside]
        print(f"k = {k}, {C} filters: |pair - x| / x <= 2^{np.log2(rel.max()):.2f} on {inside.sum()} values")
        assert rel.max() <= 2.0 ** -14
        # the values the kernels' products use
        v = m.image_values(hi, img, k)
        e = m.encode_values(x64, k)
        assert all(np.array_equal(a, b) for a, b in zip(v, e))


def test_model_agrees_with_the_operand_emulator():
    """One convolution of c6_model against tools/emulate_fp8_corrections.py's "c6k" model (which the network-level test of
    tests/test_gpu_c6.py uses) on the same fp32 tensor: the same operand values, so equal to float64 rounding of the sums.
    (The emulator's network run hands its convolutions the STORED value hi + lo6 2^(k - 11) and derives the value piece from
    that; the kernels convert the fp32 value itself, as encode_c6_image does -- tests/test_gpu_c6_elements.py (a) holds them to
    it bit for bit.  The two differ where the value lies within 2^-14 of a bf6 tie: 2e-7 of an output's sum of |terms| at the
    median, far inside the network test's tolerance.)"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import emulate_fp8_corrections as emu
    from cchess_alphazero import _native
    C, n, k = 128, 2, m.K_X
    rng = np.random.default_rng(7)
    x = m.activations(n, C, k, rng)
    w, b = m.filters(C, rng)
    xv = m.image_values(*m.encode_c6_image(x, k), k)
    wv = m.filter_values(m.decode_c6_pack(_native.pack_conv3x3_c6_weights(torch.from_numpy(w), k, 0), C))
    mine, _ = m.c6_conv(xv, wv, b.astype(np.float64))
    d = torch.float64
    xi = torch.from_numpy(x).to(d).view(n, 10, 9, C).permute(0, 3, 1, 2)
    theirs = emu.conv_model(xi, torch.from_numpy(w).to(d), torch.from_numpy(b).to(d), f"c6k:{k}", 1)
    theirs = theirs.permute(0, 2, 3, 1).reshape(n, 90, C).numpy()
    mag = m.conv(abs(xv[0]), abs(wv[0])) + np.abs(b)
    assert (np.abs(mine - theirs) / mag).max() < 1e-13
