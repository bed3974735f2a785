"""-m gpu: the dense tail of a win / draw / loss value head, cz_heads_tail_wdl (k_fc_tile<WDL>; csrc/xq_heads.hip), against
float64 element by element with the bounds derived in tests/wdl_check.py.

  a. per element: every wdl probability and every value P(win) - P(loss) within its bound on the pairs' own operands (a) and
     on the exact fp32 operands (b), rows of wdl summing to 1, for fp16 and bf16 pairs, both feature splits, n_hidden 256 / 100
     / 33 (an even count of 32-wide tiles; a count not divisible by four with a partial tile; a partial tile only), 1 / 63 /
     64 / 65 / 130 rows, O(1) and mixed data.  Planted rows: two gate features (the last two of the value features: 1.0 on the
     rows r % 5 == 1 resp. r % 5 == 3 that are not all zero, 0.0 elsewhere) drive two hidden units of their own (a one-hot
     weight row of 1.0, bias 0: 1.0 exactly on those rows in either pair format), whose w2 entries are +60 / 0 / -60 resp.
     -60 / 0 / +60 -- the class biases of those rows.  There p runs from ~1 to exp(-120), below fp32's range, v sits at +-1
     and nothing is NaN.
  b. the exact sign symmetry: rows 0 and 2 of w2 / b2 swapped negate v and swap wdl's outer columns bit for bit.
  c. batch position and device-side counts: test_gpu_heads' 193-row scheme; wdl = NULL gives the same value bits.
  d. the launch's memory footprint (tests/footprint.py through test_gpu_footprint's driver)."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import f16_pairs as fp  # noqa: E402
import wdl_check as wc  # noqa: E402
from test_gpu_heads import _cus, _pairs64  # noqa: E402

B2 = (float(np.float32(0.13)), float(np.float32(-0.21)), float(np.float32(0.05)))
N_LAB = 70                    # the policy half is cz_heads_tail's launch (tests/test_gpu_heads.py): a small one rides along


@functools.lru_cache(maxsize=2)
def _case(pair, f_pol, f_val, n_hid, data, rows):
    """One set of operands on the device with every float64 reference and bound, computed once and only read afterwards."""
    import torch
    from cchess_alphazero import _native
    pdt = getattr(torch, pair)
    fmt = fp.F16_PAIR if pair == "float16" else fp.BF16_PAIR
    rng = np.random.default_rng([f_val, n_hid, int(data == "mixed"), int(pair == "float16"), 3])
    pf, vf = fp.dense_features(data, rows, f_pol, rng), fp.dense_features(data, rows, f_val, rng)
    wp = (rng.standard_normal((N_LAB, f_pol)) * 0.08).astype(np.float32)
    bp = (rng.standard_normal(N_LAB) * 0.5).astype(np.float32)
    w1 = (rng.standard_normal((n_hid, f_val)) * 0.1).astype(np.float32)
    b1 = (rng.standard_normal(n_hid) * 0.2).astype(np.float32)
    w2 = (rng.standard_normal((3, n_hid)) * 0.2).astype(np.float32)
    # the gates: hidden unit ja is 1.0 on the rows r % 5 == 1, unit jb on the rows r % 5 == 3 (all-zero rows stay all zero)
    live = vf.any(axis=1)
    ga, gb = (np.arange(rows) % 5 == 1) & live, (np.arange(rows) % 5 == 3) & live
    vf[:, -1], vf[:, -2] = ga, gb
    ja, jb = 1, n_hid - 1
    for j, k in ((ja, -1), (jb, -2)):
        w1[j] = 0.0
        w1[j, k] = 1.0
        b1[j] = 0.0
    c = dict(pair=pair, n_hid=n_hid, rows=rows, ga=torch.from_numpy(ga).cuda(), gb=torch.from_numpy(gb).cuda())
    dev = lambda a: torch.from_numpy(a).cuda()
    pf, vf, wp, bp, w1, b1, w2 = (dev(a) for a in (pf, vf, wp, bp, w1, b1, w2))
    xp, x = _pairs64(vf, pdt)
    w1p, w = _pairs64(w1, pdt)
    h_a, hb_a, h_b, hb_b = fp.DenseCheck(xp, w1p, x, w, fmt).bounds(b1.double())
    # keep the softmax of the ordinary rows out of saturation on either data set: |logit - bias| <= 1.8 at the 93 % quantile
    q = torch.quantile((torch.relu(h_b) @ w2.double().T).abs().flatten(), 0.93).item()
    if q > 1.8:
        w2 = (w2.double() * (1.8 / q)).float()
    w2[:, ja] = torch.tensor([60.0, 0.0, -60.0], device="cuda")
    w2[:, jb] = torch.tensor([-60.0, 0.0, 60.0], device="cuda")
    w2 = w2.contiguous()
    c["a"] = wc.wdl_check(h_a, hb_a, w2.double(), B2)
    c["b"] = wc.wdl_check(h_b, hb_b, w2.double(), B2)
    c.update(pf=pf, vf=vf, bp=bp, b1=b1, w2=w2, pk_p=_native.pack_fc_weights(wp, pdt).cuda(),
             pk_1=_native.pack_fc_weights(w1, pdt).cuda())
    return c


def _run(c, pf, vf, count=None, with_wdl=True, swap=False):
    import torch
    from cchess_alphazero import _native
    n = pf.shape[0]
    pol = torch.full((n, N_LAB), 7.0, device="cuda")
    val = torch.full((n,), 7.0, device="cuda")
    wdl = torch.full((n, 3), 7.0, device="cuda") if with_wdl else None
    stats = torch.empty((n, 2), device="cuda")
    w2, b2 = (c["w2"][[2, 1, 0]].contiguous(), B2[::-1]) if swap else (c["w2"], B2)
    _native.heads_tail_wdl(pf, vf, c["pk_p"], c["bp"], c["pk_1"], c["b1"], w2, b2, pol, val, stats, wdl=wdl, count=count,
                           normalize=True)
    return pol, val, wdl


def _ratios(c, n):
    """Worst error / bound of the first n rows' probabilities, values and row sums, against (a) and (b)."""
    import torch
    _, val, wdl = _run(c, c["pf"][:n].contiguous(), c["vf"][:n].contiguous())
    assert torch.isfinite(val).all() and torch.isfinite(wdl).all()
    out = {}
    for k in "ab":
        r = c[k]
        out["p " + k] = ((wdl.double() - r["p"][:n]).abs() / r["bp"][:n]).max().item()
        out["v " + k] = ((val.double() - r["v"][:n]).abs() / r["bv"][:n]).max().item()
    out["row sum"] = ((wdl.double().sum(1) - 1.0).abs() / wc.ROWSUM_TOL).max().item()
    # the exact symmetry: win and loss swapped
    _, val_s, wdl_s = _run(c, c["pf"][:n].contiguous(), c["vf"][:n].contiguous(), swap=True)
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(-val_s), bits(val)), n
    assert torch.equal(bits(wdl_s[:, [2, 1, 0]]), bits(wdl)), n
    return out


def _assert_case_is_sharp(c, data):
    """The data does what the docstring says: both kinds of planted rows at p ~ (1, e^-60, e^-120) and back, the ordinary
    rows' softmax unsaturated."""
    import torch
    r = c["b"]
    plant = torch.tensor([60.0, 0.0, -60.0], dtype=torch.float64, device="cuda")
    for gate, top, low, sign in ((c["ga"], 0, 2, 1.0), (c["gb"], 2, 0, -1.0)):
        # (the gate rows whose other hidden units add an ordinary amount: mixed data has rows of large features)
        calm = gate & ((r["l"] - sign * plant).abs().amax(1) <= 2.0)
        p = r["p"][calm]
        assert p.shape[0] >= 3 and (p[:, top] > 0.99).all(), p[:2]
        assert (p[:, 1] < 1e-20).all() and (p[:, 1] > 1e-32).all()                 # exp(-60) or so
        assert (p[:, low] < 2.0 ** -149).all()                                     # exp(-120): below fp32's subnormals
        assert ((r["v"][calm] - sign).abs() < 1e-12).all()
    plain = ~(c["ga"] | c["gb"])
    assert ((r["l"][plain].abs() <= 2.0).all(1)).double().mean().item() >= 0.75
    if data == "mixed":
        assert (~c["vf"].any(1)).sum().item() >= 1                                 # all-zero rows


@pytest.mark.parametrize("data", ["O(1)", "mixed"])
@pytest.mark.parametrize("n_hid", [256, 100, 33])
@pytest.mark.parametrize("f_pol,f_val", [(360, 180), (180, 360)])
@pytest.mark.parametrize("pair", ["float16", "bfloat16"])
def test_wdl_tail_per_element(pair, f_pol, f_val, n_hid, data):
    """Every probability and value within wdl_check's bounds, rows summing to 1, the W / L swap exact.
    Measured on an MI355X, worst error / bound over the row counts, range over the 12 cases of a pair type:
      fp16 pairs: p (a) 0.016-0.048, (b) 0.012-0.043, value (a) 0.001-0.003, (b) 0.001-0.004, row sum 0.25-0.54 of 4 U;
      bf16 pairs: p (a) 0.012-0.052, (b) 0.001-0.024, value (a) 0.001-0.004, (b) 0.001-0.012, row sum 0.31-0.47.
    The bounds on p and v are worst cases over the hidden units (sum_j B_j |w2_kj| and gamma_n A_k, as in value_check, whose
    O(1) cases sit at 0.002-0.010 for the same reason): 33 ... 256 independent errors add like a random walk.  That they still
    tell right from wrong arithmetic is shown on the CPU (tests/test_wdl_cpu.py: a dropped w_lo x_hi term 3.4-6.1 x the
    bound, win and loss swapped > 1e7 x, the clean model 0.02-0.03); the exact parts -- the W / L symmetry, the row sums, the
    batch-position bits -- carry no slack."""
    c = _case(pair, f_pol, f_val, n_hid, data, 130)
    _assert_case_is_sharp(c, data)
    worst = {}
    for n in (1, 63, 64, 65, 130):
        r = _ratios(c, n)
        assert all(v <= 1.0 for v in r.values()), (n, r)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
    print(f"\nwdl tail {pair} F={f_pol}/{f_val} hidden {n_hid} {data}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("pair,n_hid", [("float16", 256), ("bfloat16", 33)])
def test_wdl_tail_rows_do_not_depend_on_their_place_in_the_batch(pair, n_hid):
    """The 193-row scheme of test_gpu_heads: 193 distinct rows tiled to P + 65 and 2 P + 65 rows (P = 2 CUs x 64, one pass of
    k_fc_tile's workgroups), without a count and with device-side counts that end mid-tile in the first pass's last tile, in a
    second tile, inside the second pass and in its last tile.  value and wdl of every counted row equal the 193-row launch's
    bit for bit, rows past the count keep their 7.0 in both, and wdl = NULL gives the same value bits.  Measured on an MI355X
    (256 CUs: n = 32 833 and 65 601): identical in all twelve launches per case; the 193 rows' own ratios: p 0.039 (a) / 0.035
    (b), value 0.003 for fp16 pairs at 256 hidden units; 0.022 / 0.019, 0.004 / 0.005 for bf16 at 33."""
    import torch
    r = 193
    c = _case(pair, 360, 180, n_hid, "mixed", r)
    ratios = _ratios(c, r)
    print(f"\nwdl tail {pair} hidden {n_hid}, {r} rows: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    per_pass = 2 * _cus() * 64
    bits = lambda t: t.view(torch.int32)
    _, small_v, small_w = _run(c, c["pf"], c["vf"])
    for n, counts in ((per_pass + 65, (None, per_pass - 5, per_pass + 25)),
                      (2 * per_pass + 65, (None, per_pass + 64 * 37 + 25, 2 * per_pass - 5))):
        assert all(cnt % 64 and cnt < n for cnt in counts[1:]) and per_pass < counts[2] < 2 * per_pass
        src = torch.arange(n, device="cuda") % r
        pf, vf = c["pf"][src].contiguous(), c["vf"][src].contiguous()
        for cnt in counts:
            count = None if cnt is None else torch.tensor([cnt], dtype=torch.int32, device="cuda")
            _, big_v, big_w = _run(c, pf, vf, count=count)
            m = n if cnt is None else cnt
            assert torch.equal(bits(big_v[:m]), bits(small_v[src[:m]])), (n, cnt)
            assert torch.equal(bits(big_w[:m]), bits(small_w[src[:m]])), (n, cnt)
            assert torch.all(big_v[m:] == 7.0) and torch.all(big_w[m:] == 7.0), (n, cnt)
            _, null_v, _ = _run(c, pf, vf, count=count, with_wdl=False)
            assert torch.equal(bits(null_v), bits(big_v)), (n, cnt)
            del big_v, big_w, null_v
        del pf, vf, src


@pytest.mark.parametrize("key", ["f16", "bf16"])
def test_wdl_tail_footprint(key):
    """Every operand of cz_heads_tail_wdl carved with guard bytes and poisoned padding (tests/footprint.py, the driver and the
    shapes of test_gpu_footprint): no guard byte changes, nothing is written past the count or into an input, and no poisoned
    input reaches an owned output -- value and wdl included."""
    import torch
    import test_gpu_footprint as tf
    from cchess_alphazero import _native
    net = tf.F16 if key == "f16" else tf.BF16
    g = tf._net(*net)
    pf, vf = tf._feats(net)
    n_hid = g.tail_b1.shape[0]
    w2 = (torch.randn((3, n_hid), generator=torch.Generator().manual_seed(5)) * 0.2).cuda()
    outs = {"policy": tf.Out((g.policy_out.out_features,), torch.float32), "value": tf.Out((), torch.float32),
            "wdl": tf.Out((3,), torch.float32), "stats": tf.Out((2,), torch.float32)}

    def run(i, o, w, count, rows, masks):
        _native.heads_tail_wdl(i["pf"], i["vf"], w[0], w[1], w[2], w[3], w[4], B2, o["policy"], o["value"], o["stats"],
                               wdl=o["wdl"], count=count, normalize=True)
    L = tf.Launch({"pf": tf.In(pf), "vf": tf.In(vf)}, outs,
                  [g.tail_wp.view(g._tail_dtype), g.tail_bp, g.tail_w1.view(g._tail_dtype), g.tail_b1, w2], run)
    assert tf._check_case(L) >= 12
