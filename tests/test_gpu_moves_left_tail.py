"""-m gpu: the dense tail with a moves-left output, cz_heads_tail_ml (k_fc_tile<VALUE_ML> and <WDL_ML>; csrc/xq_heads.hip),
against float64 element by element with the bound derived in tests/moves_left_check.py.

  a. per element: every x within its bound on the pairs' own operands (a) and on the exact fp32 operands (b), for fp16 and
     bf16 pairs, both feature splits, n_hidden 256 / 100 / 33 (an even count of 32-wide tiles; a count not divisible by the
     four wave classes with a partial tile; a partial tile only), 1 / 63 / 64 / 65 / 130 rows, both value heads, O(1) and
     mixed data with all-zero rows.  Planted rows as in test_gpu_wdl_tail: two gate features (the last two of the value
     features: 1.0 on the rows r % 5 == 1 resp. r % 5 == 3 that are not all zero) drive two hidden units of their own to 1.0
     exactly, whose entries in the moves-left row are +60 resp. -60: there x sits near +-60 (m(x) from 1920 plies down to
     nothing) and nothing is NaN.
  b. value, and wdl, bit for bit those of cz_heads_tail / cz_heads_tail_wdl on the first rows of w2 and b2 -- in every launch
     of (a) and (c).
  c. batch position and device-side counts: test_gpu_heads' 193-row scheme; rows past the count keep their fill value in
     every output.
  d. the launch's memory footprint (tests/footprint.py through test_gpu_footprint's driver), moves_left an owned output.
  e. value_outputs 2, a NULL moves_left and wdl with the scalar head are refused with the entry point's message."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import f16_pairs as fp  # noqa: E402
import moves_left_check as mc  # noqa: E402
from test_gpu_heads import _cus, _pairs64  # noqa: E402

B2 = tuple(float(np.float32(b)) for b in (0.13, -0.21, 0.05))
B_ML = float(np.float32(1.8545866))       # about ln(e^2 - 1): the output's initial bias
N_LAB = 70                    # the policy half is cz_heads_tail's launch (tests/test_gpu_heads.py): a small one rides along


@functools.lru_cache(maxsize=2)
def _case(pair, f_pol, f_val, n_hid, data, rows):
    """One set of operands on the device with the float64 reference and bound of x, computed once and only read afterwards.
    w2 holds four rows, (win, draw, loss, moves left): the scalar head's launches take rows (0, 3), the others all four."""
    import torch
    from cchess_alphazero import _native
    pdt = getattr(torch, pair)
    fmt = fp.F16_PAIR if pair == "float16" else fp.BF16_PAIR
    rng = np.random.default_rng([f_val, n_hid, int(data == "mixed"), int(pair == "float16"), 4])
    pf, vf = fp.dense_features(data, rows, f_pol, rng), fp.dense_features(data, rows, f_val, rng)
    wp = (rng.standard_normal((N_LAB, f_pol)) * 0.08).astype(np.float32)
    bp = (rng.standard_normal(N_LAB) * 0.5).astype(np.float32)
    w1 = (rng.standard_normal((n_hid, f_val)) * 0.1).astype(np.float32)
    b1 = (rng.standard_normal(n_hid) * 0.2).astype(np.float32)
    w2 = (rng.standard_normal((4, n_hid)) * 0.2).astype(np.float32)
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
    # the ordinary rows' outputs stay ordinary on either data set: |x - bias| <= 1.8 at the 93 % quantile, row by row of w2
    for k in range(4):
        q = torch.quantile((torch.relu(h_b) @ w2[k].double()).abs(), 0.93).item()
        if q > 1.8:
            w2[k] = (w2[k].double() * (1.8 / q)).float()
    w2[3, ja], w2[3, jb] = 60.0, -60.0
    w2 = w2.contiguous()
    c["a"] = mc.x_check(h_a, hb_a, w2[3].double(), B_ML)
    c["b"] = mc.x_check(h_b, hb_b, w2[3].double(), B_ML)
    c.update(pf=pf, vf=vf, bp=bp, b1=b1, w2=w2, pk_p=_native.pack_fc_weights(wp, pdt).cuda(),
             pk_1=_native.pack_fc_weights(w1, pdt).cuda())
    return c


def _run(c, pf, vf, vo, count=None, with_wdl=True):
    """-> (value, wdl or None, x) of cz_heads_tail_ml, after checking value and wdl bit for bit against the entry point
    without the output on the same operands (b), and the policy too."""
    import torch
    from cchess_alphazero import _native
    n = pf.shape[0]
    bits = lambda t: t.contiguous().view(torch.int32)
    new = lambda *shape: torch.full(shape, 7.0, device="cuda")
    pol, val, x, stats = new(n, N_LAB), new(n), new(n), torch.empty((n, 2), device="cuda")
    pol0, val0 = new(n, N_LAB), new(n)
    if vo == 3:
        wdl, wdl0 = (new(n, 3), new(n, 3)) if with_wdl else (None, None)
        _native.heads_tail_ml(pf, vf, c["pk_p"], c["bp"], c["pk_1"], c["b1"], c["w2"], B2 + (B_ML,), pol, val, stats, x,
                              wdl=wdl, count=count)
        _native.heads_tail_wdl(pf, vf, c["pk_p"], c["bp"], c["pk_1"], c["b1"], c["w2"][:3].contiguous(), B2, pol0, val0,
                               stats, wdl=wdl0, count=count)
        assert wdl is None or torch.equal(bits(wdl), bits(wdl0))
    else:
        wdl = None
        _native.heads_tail_ml(pf, vf, c["pk_p"], c["bp"], c["pk_1"], c["b1"], c["w2"][[0, 3]].contiguous(), (B2[0], B_ML),
                              pol, val, stats, x, count=count)
        _native.heads_tail(pf, vf, c["pk_p"], c["bp"], c["pk_1"], c["b1"], c["w2"][0].contiguous(), B2[0], pol0, val0, stats,
                           count=count)
    assert torch.equal(bits(val), bits(val0)) and torch.equal(bits(pol), bits(pol0))
    return val, wdl, x


def _ratios(c, n, vo):
    """Worst error / bound of the first n rows' x against (a) and (b)."""
    import torch
    val, wdl, x = _run(c, c["pf"][:n].contiguous(), c["vf"][:n].contiguous(), vo)
    assert torch.isfinite(x).all() and torch.isfinite(val).all() and (wdl is None or torch.isfinite(wdl).all())
    return {"x " + k: ((x.double() - c[k][0][:n]).abs() / c[k][1][:n]).max().item() for k in "ab"}


def _assert_case_is_sharp(c, data):
    """The data does what the docstring says: the planted rows at x ~ +-60, the ordinary rows ordinary."""
    import torch
    x = c["b"][0]
    for gate, want in ((c["ga"], 60.0), (c["gb"], -60.0)):
        calm = gate & ((x - want - B_ML).abs() <= 4.0)
        assert calm.sum().item() >= 3, (want, x[gate][:4])
    plain = ~(c["ga"] | c["gb"])
    assert ((x[plain] - B_ML).abs() <= 2.0).double().mean().item() >= 0.75
    if data == "mixed":
        zero = ~c["vf"].any(1)
        assert zero.sum().item() >= 1                                              # all-zero rows


@pytest.mark.parametrize("data", ["O(1)", "mixed"])
@pytest.mark.parametrize("n_hid", [256, 100, 33])
@pytest.mark.parametrize("f_pol,f_val", [(360, 180), (180, 360)])
@pytest.mark.parametrize("pair", ["float16", "bfloat16"])
def test_moves_left_tail_per_element(pair, f_pol, f_val, n_hid, data):
    """Every x within moves_left_check.x_check's bound for both value heads; value, wdl and policy keep their bits.
    Measured on an MI355X, worst error / bound over the row counts and both heads, range over the 12 cases of a pair type:
      fp16 pairs: O(1) data x (a) 0.016-0.028, (b) 0.013-0.023, mixed data (a) 0.401-0.491, (b) 0.369-0.474;
      bf16 pairs: O(1) data x (a) 0.014-0.031, (b) 0.002-0.008, mixed data (a) 0.414-0.519, (b) 0.178-0.519.
    On O(1) data the bound is a worst case over the hidden units (sum_j B_j |w2_j| and gamma_n A, as in value_check and
    logit_check, whose cases sit as low for the same reason): 33 ... 256 independent errors add like a random walk.  On the
    mixed data's rows of large features x itself is large and the one rounding of the bias addition carries both the error and
    the bound: half an ulp against U |x|, a ratio of about a half.  That it still tells right
    from wrong arithmetic is shown on the CPU (tests/test_moves_left_cpu.py: a dropped w_lo x_hi term 6.6-10 x the bound, the
    win row read for the moves-left row > 6e4 x, the clean model 0.01-0.02); the exact parts -- value, wdl and policy bit
    for bit, the batch-position bits -- carry no slack."""
    c = _case(pair, f_pol, f_val, n_hid, data, 130)
    _assert_case_is_sharp(c, data)
    worst = {}
    for vo in (1, 3):
        for n in (1, 63, 64, 65, 130):
            r = _ratios(c, n, vo)
            assert all(v <= 1.0 for v in r.values()), (vo, n, r)
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
    print(f"\nmoves-left tail {pair} F={f_pol}/{f_val} hidden {n_hid} {data}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("pair,n_hid,vo", [("float16", 256, 1), ("bfloat16", 33, 3)])
def test_moves_left_tail_rows_do_not_depend_on_their_place_in_the_batch(pair, n_hid, vo):
    """The 193-row scheme of test_gpu_heads: 193 distinct rows tiled to P + 65 and 2 P + 65 rows (P = 2 CUs x 64, one pass of
    k_fc_tile's workgroups), without a count and with device-side counts that end mid-tile in the first pass's last tile, in a
    second tile, inside the second pass and in its last tile.  x, value and wdl of every counted row equal the 193-row
    launch's bit for bit, rows past the count keep their 7.0 in all of them; wdl = NULL gives the same bits.  Measured on an
    MI355X: identical in every launch; the 193 rows' own ratios: x 0.458 (a) / 0.422 (b) for fp16 pairs at 256 hidden units
    beside the scalar head, 0.480 / 0.351 for bf16 at 33 beside win / draw / loss."""
    import torch
    r = 193
    c = _case(pair, 360, 180, n_hid, "mixed", r)
    ratios = _ratios(c, r, vo)
    print(f"\nmoves-left tail {pair} hidden {n_hid} head {vo}, {r} rows: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    per_pass = 2 * _cus() * 64
    bits = lambda t: t.view(torch.int32)
    small_v, small_w, small_x = _run(c, c["pf"], c["vf"], vo)
    for n, counts in ((per_pass + 65, (None, per_pass - 5, per_pass + 25)),
                      (2 * per_pass + 65, (None, per_pass + 64 * 37 + 25, 2 * per_pass - 5))):
        assert all(cnt % 64 and cnt < n for cnt in counts[1:]) and per_pass < counts[2] < 2 * per_pass
        src = torch.arange(n, device="cuda") % r
        pf, vf = c["pf"][src].contiguous(), c["vf"][src].contiguous()
        for cnt in counts:
            count = None if cnt is None else torch.tensor([cnt], dtype=torch.int32, device="cuda")
            big_v, big_w, big_x = _run(c, pf, vf, vo, count=count)
            m = n if cnt is None else cnt
            assert torch.equal(bits(big_x[:m]), bits(small_x[src[:m]])), (n, cnt)
            assert torch.equal(bits(big_v[:m]), bits(small_v[src[:m]])), (n, cnt)
            assert torch.all(big_x[m:] == 7.0) and torch.all(big_v[m:] == 7.0), (n, cnt)
            if vo == 3:
                assert torch.equal(bits(big_w[:m]), bits(small_w[src[:m]])) and torch.all(big_w[m:] == 7.0), (n, cnt)
                null_v, _, null_x = _run(c, pf, vf, vo, count=count, with_wdl=False)
                assert torch.equal(bits(null_v), bits(big_v)) and torch.equal(bits(null_x), bits(big_x)), (n, cnt)
                del null_v, null_x
            del big_v, big_w, big_x
        del pf, vf, src


@pytest.mark.parametrize("key,vo", [("f16", 1), ("bf16", 3)])
def test_moves_left_tail_footprint(key, vo):
    """Every operand of cz_heads_tail_ml carved with guard bytes and poisoned padding (tests/footprint.py, the driver and the
    shapes of test_gpu_footprint): no guard byte changes, nothing is written past the count or into an input, and no poisoned
    input reaches an owned output -- value, wdl and moves_left included."""
    import torch
    import test_gpu_footprint as tf
    from cchess_alphazero import _native
    net = tf.F16 if key == "f16" else tf.BF16
    g = tf._net(*net)
    pf, vf = tf._feats(net)
    n_hid = g.tail_b1.shape[0]
    w2 = (torch.randn((vo + 1, n_hid), generator=torch.Generator().manual_seed(5)) * 0.2).cuda()
    b2 = (B2[:vo] + (B_ML,))
    outs = {"policy": tf.Out((g.policy_out.out_features,), torch.float32), "value": tf.Out((), torch.float32),
            "moves_left": tf.Out((), torch.float32), "stats": tf.Out((2,), torch.float32)}
    if vo == 3:
        outs["wdl"] = tf.Out((3,), torch.float32)

    def run(i, o, w, count, rows, masks):
        _native.heads_tail_ml(i["pf"], i["vf"], w[0], w[1], w[2], w[3], w[4], b2, o["policy"], o["value"], o["stats"],
                              o["moves_left"], wdl=o.get("wdl"), count=count, normalize=True)
    L = tf.Launch({"pf": tf.In(pf), "vf": tf.In(vf)}, outs,
                  [g.tail_wp.view(g._tail_dtype), g.tail_bp, g.tail_w1.view(g._tail_dtype), g.tail_b1, w2], run)
    assert tf._check_case(L) >= 12


def test_moves_left_tail_refuses_bad_arguments():
    """value_outputs 2, a NULL moves_left, and wdl with the scalar head: NativeError with cz_heads_tail_ml's message, and
    nothing is written."""
    import torch
    from cchess_alphazero import _native
    c = _case("float16", 360, 180, 33, "O(1)", 130)
    n = 5
    pf, vf = c["pf"][:n].contiguous(), c["vf"][:n].contiguous()
    new = lambda *shape: torch.full(shape, 7.0, device="cuda")
    pol, val, x, wdl, stats = new(n, N_LAB), new(n), new(n), new(n, 3), new(n, 2)
    args = (pf, vf, c["pk_p"], c["bp"], c["pk_1"], c["b1"])
    w2_1, b2_1 = c["w2"][[0, 3]].contiguous(), (B2[0], B_ML)
    for call in (lambda: _native.heads_tail_ml(*args, c["w2"][:3].contiguous(), B2, pol, val, stats, x, value_outputs=2),
                 lambda: _native.heads_tail_ml(*args, c["w2"], B2 + (B_ML,), pol, val, stats, None, wdl=wdl),
                 lambda: _native.heads_tail_ml(*args, w2_1, b2_1, pol, val, stats, None),
                 lambda: _native.heads_tail_ml(*args, w2_1, b2_1, pol, val, stats, x, wdl=wdl)):
        with pytest.raises(_native.NativeError, match=r"cz_heads_tail_ml: bad argument .*value_outputs 1 or 3; moves_left is "
                                                      r"required; wdl only with value_outputs 3"):
            call()
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (pol, val, x, wdl, stats))
