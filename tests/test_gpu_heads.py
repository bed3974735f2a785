"""-m gpu: the kernels every evaluated leaf passes through after the tower, against float64 element by element.

  a. cz_heads_tail (k_fc_tile<POLICY>, k_fc_tile<VALUE>, k_policy_normalize; csrc/xq_heads.hip): raw logits within
     f16_pairs.DenseCheck's bounds (a) and (b) for every element, probabilities and values within the bounds derived there
     (softmax_check, value_check), for fp16 and bf16 pairs, both feature splits, 1 / 63 / 64 / 65 / 130 rows, label counts that
     make an even, an odd and a single label tile with and without a partial last one, on O(1) and on mixed data
     (f16_pairs.dense_features).  The bias carries +40 / +80 / -80 at three labels (two when there are only two).  A bias is
     shared by the rows, so a gate feature (the last one: 1.0, with the weights -40 / -80 / +80 at those labels, all exact in
     both pair formats) cancels them on every row but r % 3 == 1 and the all-zero rows: those rows' priors run from ~1 down
     to exp(-160), below fp32's range, the others stay ordinary.
  b. batch position and later passes: 193 distinct rows tiled to 2 CUs 64 + 65 rows (two of k_fc_tile's 2 CUs workgroups walk
     a second 64-row tile, every wave of k_policy_normalize a second row) and to 4 CUs 64 + 65 rows (every workgroup walks a
     second full tile, two a third) must reproduce the 193-row launch bit for bit, also under device-side counts that end
     mid-tile inside the first pass's last tile, inside a second pass and in a second pass's last tile.
  c. cz_head_convs (k_head_convs, csrc/xq_nn_epilogue.hip) per element and with a known answer for the Flatten order.
  d. cz_bias_act (k_bias_act) value for value, and the argument checks of _native.bias_act_.

Every test prints its worst error / bound; the values measured on an MI355X (2026-10-18) stand in the tests' docstrings.
The whole file: 70 tests, 4.3 s on the GPU since import (test_z_report_gpu_seconds), 2.5 s of it the first launch."""
import functools
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import f16_pairs as fp  # noqa: E402

T0 = time.time()
U = fp.U


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _pairs64(t, pdt):
    """fp32 device tensor -> ((hi, lo) as float64, the tensor as float64): the split the kernel and the packer make."""
    hi = t.to(pdt)
    lo = (t - hi.float()).to(pdt)
    return (hi.double(), lo.double()), t.double()


@functools.lru_cache(maxsize=2)
def _case(pair, f_pol, f_val, n_lab, n_hid, data, rows):
    """One set of operands on the device with every float64 reference and bound, computed once and only read afterwards."""
    import torch
    from cchess_alphazero import _native
    pdt = getattr(torch, pair)
    fmt = fp.F16_PAIR if pair == "float16" else fp.BF16_PAIR
    rng = np.random.default_rng([f_pol, n_lab, n_hid, int(data == "mixed"), int(pair == "float16")])
    pf, vf = fp.dense_features(data, rows, f_pol, rng), fp.dense_features(data, rows, f_val, rng)
    wp = (rng.standard_normal((n_lab, f_pol)) * 0.08).astype(np.float32)
    bp = (rng.standard_normal(n_lab) * 0.5).astype(np.float32)
    w1 = (rng.standard_normal((n_hid, f_val)) * 0.1).astype(np.float32)
    b1 = (rng.standard_normal(n_hid) * 0.2).astype(np.float32)
    w2 = (rng.standard_normal(n_hid) * 0.2).astype(np.float32)
    b2 = float(np.float32(0.13))         # what the kernel is handed: value_check takes no other
    # planted bias entries, switched off by the gate feature on the rows that are neither r % 3 == 1 nor all zero
    plant = {0: 40.0, 1: 80.0} if n_lab < 64 else {1: 40.0, 33: 80.0, n_lab - 1: -80.0}
    planted = (np.arange(rows) % 3 == 1) | ~pf.any(axis=1)
    pf[:, -1] = np.where(planted, 0.0, 1.0)
    for j, v in plant.items():
        bp[j] = v
        wp[j, -1] = -v
    c = dict(pair=pair, pdt=pdt, n_lab=n_lab, n_hid=n_hid, rows=rows, b2=b2, plant=plant,
             planted=torch.from_numpy(planted & pf.any(axis=1)).cuda())
    dev = lambda a: torch.from_numpy(a).cuda()
    pf, vf, wp, bp, w1, b1, w2 = (dev(a) for a in (pf, vf, wp, bp, w1, b1, w2))
    # policy side
    xp, x = _pairs64(pf, pdt)
    wpp, w = _pairs64(wp, pdt)
    c["l_a"], c["lb_a"], c["l_b"], c["lb_b"] = fp.DenseCheck(xp, wpp, x, w, fmt).bounds(bp.double())
    c["p_a"], c["pb_a"] = fp.softmax_check(c["l_a"], c["lb_a"])
    c["p_b"], c["pb_b"] = fp.softmax_check(c["l_b"], c["lb_b"])
    # value side
    xp, x = _pairs64(vf, pdt)
    w1p, w = _pairs64(w1, pdt)
    h_a, hb_a, h_b, hb_b = fp.DenseCheck(xp, w1p, x, w, fmt).bounds(b1.double())
    # keep tanh out of saturation on either data set: |d| <= 2 on 90 % of the rows (asserted in the test)
    q = torch.quantile((torch.relu(h_b) @ w2.double()).abs(), 0.93).item()
    if q > 1.8:
        w2 = (w2.double() * (1.8 / q)).float()
    c["v_a"], c["vb_a"], c["d"] = fp.value_check(h_a, hb_a, w2.double(), b2)
    c["v_b"], c["vb_b"], _ = fp.value_check(h_b, hb_b, w2.double(), b2)
    c.update(pf=pf, vf=vf, bp=bp, b1=b1, w2=w2, pk_p=_native.pack_fc_weights(wp, pdt).cuda(),
             pk_1=_native.pack_fc_weights(w1, pdt).cuda())
    return c


def _run(c, pf, vf, normalize, count=None):
    import torch
    from cchess_alphazero import _native
    n = pf.shape[0]
    pol = torch.full((n, c["n_lab"]), 7.0, device="cuda")
    val = torch.full((n,), 7.0, device="cuda")
    stats = torch.empty((n, 2), device="cuda")
    _native.heads_tail(pf, vf, c["pk_p"], c["bp"], c["pk_1"], c["b1"], c["w2"], c["b2"], pol, val, stats, count=count,
                       normalize=normalize)
    return pol, val


def _ratios(c, n):
    """Worst error / bound of the first n rows' logits, probabilities and values, against (a) and (b)."""
    import torch
    raw, v0 = _run(c, c["pf"][:n].contiguous(), c["vf"][:n].contiguous(), False)
    pol, val = _run(c, c["pf"][:n].contiguous(), c["vf"][:n].contiguous(), True)
    assert torch.equal(v0, val)
    assert torch.isfinite(raw).all() and torch.isfinite(pol).all() and torch.isfinite(val).all()
    worst = lambda got, ref, bound: ((got.double() - ref[:n]).abs() / bound[:n]).max().item()
    return {"logit a": worst(raw, c["l_a"], c["lb_a"]), "logit b": worst(raw, c["l_b"], c["lb_b"]),
            "p a": worst(pol, c["p_a"], c["pb_a"]), "p b": worst(pol, c["p_b"], c["pb_b"]),
            "v a": worst(val, c["v_a"], c["vb_a"]), "v b": worst(val, c["v_b"], c["vb_b"])}


def _assert_case_is_sharp(c, data):
    """The data does what the docstring says: priors from ~1 to below fp32's range on the planted rows, tanh unsaturated."""
    import torch
    pr = c["p_b"][c["planted"]]
    assert pr.shape[0] >= 1 and pr.amax(1).min().item() > 0.99
    mid = pr[:, 1] if c["n_lab"] >= 64 else pr[:, 0]               # the +40 label beside the +80 one: exp(-40) or so
    assert (mid < 1e-12).all() and (mid > 1e-25).all()
    if c["n_lab"] >= 64:
        assert pr.amin(1).max().item() < 2.0 ** -149               # the -80 label: exp(-160), below fp32's subnormals
    assert (c["d"].abs() <= 2.0).double().mean().item() >= 0.9
    if data == "mixed":
        assert (~c["pf"].any(1)).sum().item() >= 1 and (~c["vf"].any(1)).sum().item() >= 1         # all-zero rows


SHAPES = [(2086, 256), (70, 100), (64, 96), (2, 33)]


@pytest.mark.parametrize("data", ["O(1)", "mixed"])
@pytest.mark.parametrize("n_lab,n_hid", SHAPES)
@pytest.mark.parametrize("f_pol,f_val", [(360, 180), (180, 360)])
@pytest.mark.parametrize("pair", ["float16", "bfloat16"])
def test_dense_tail_per_element(pair, f_pol, f_val, n_lab, n_hid, data):
    """Every logit within DenseCheck (a) and (b), every probability and value within softmax_check / value_check.
    Measured on an MI355X, worst error / bound over the row counts, range over the 16 cases of a pair type:
      fp16 pairs: logits (a) 0.23-0.47, (b) 0.13-0.91 (mixed data: the format term dominates), p 0.07-0.16, value 0.002-0.010
                  on O(1) data and 0.11-0.28 on mixed data;
      bf16 pairs: logits (a) 0.25-0.41, (b) 0.05-0.46, p 0.02-0.17, value 0.002-0.007 and 0.07-0.26.
    w2 is scaled on both data sets so that tanh stays unsaturated (|d| <= 2 on >= 90 % of the rows, asserted).  Even so the
    value results on O(1) data constrain almost nothing: the value bound is a worst case over the hidden units -- sum_j B_j
    |w2_j| and gamma_n A -- while 33 ... 256 independent errors of similar size add like a random walk, hence ratios of 0.01
    and below there.  The value path is held by the mixed cases, where a few large features carry a row's error.  (The CPU
    model's clean arithmetic sits at 0.17-0.38 of logit bound (a).)"""
    c = _case(pair, f_pol, f_val, n_lab, n_hid, data, 130)
    _assert_case_is_sharp(c, data)
    worst = {}
    for n in (1, 63, 64, 65, 130):
        r = _ratios(c, n)
        assert all(v <= 1.0 for v in r.values()), (n, r)              # per row count: a NaN ratio fails here, max() would drop it
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
    print(f"\nheads tail {pair} F={f_pol}/{f_val} {n_lab}/{n_hid} {data}: "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("pair,n_lab,n_hid", [("float16", 2086, 256), ("bfloat16", 70, 33)])
def test_dense_tail_rows_do_not_depend_on_their_place_in_the_batch(pair, n_lab, n_hid):
    """193 distinct rows (checked per element as above) tiled to two batch sizes.  k_fc_tile launches min(row tiles, 2 CUs)
    workgroups, P = 2 CUs 64 rows per pass; k_policy_normalize 16 CUs workgroups of 4 waves, one row per wave and pass (P / 2 rows).
      n = P + 65 (2 CUs + 2 tiles): workgroup 0 walks a second, full tile and workgroup 1 a second tile of one row; no other
        workgroup loops.  k_policy_normalize: every wave a second row, some a third.  Counts: none; n - 70 = P - 5, which ends
        mid-tile in the LAST TILE OF THE FIRST PASS of k_fc_tile (no workgroup loops then) and inside k_policy_normalize's second
        pass; P + 25, which ends mid-tile in workgroup 0's second tile.
      n = 2 P + 65 (4 CUs + 2 tiles): EVERY workgroup walks a second full tile (reusing the LDS feature image, `red`, the
        staging tiles and m_run / s_run / dot), workgroup 0 a third full one and workgroup 1 a third of one row.  Counts: none;
        P + 64 * 37 + 25, which ends mid-tile inside the second pass (workgroups 0 .. 36 a full second tile, 37 a partial one,
        the others none); n - 70 = 2 P - 5, mid-tile in the last tile of the second pass.
    Every row of a large batch must equal its source row bit for bit -- logits, probabilities, values -- and the rows past a
    count keep their 7.0.  Measured on an MI355X (256 CUs: n = 32 833 and 65 601): identical in all twelve large
    launches per case (0.23 s at 2086 / 256); the 193 rows' own ratios: logits 0.33 (a) / 0.86 (b), p 0.10, value 0.23 for
    fp16 pairs at 2086 / 256; 0.30 / 0.37, 0.14, 0.24 for bf16 at 70 / 33."""
    import torch
    r = 193
    c = _case(pair, 360, 180, n_lab, n_hid, "mixed", r)
    ratios = _ratios(c, r)
    print(f"\nheads tail {pair} {n_lab}/{n_hid}, {r} rows: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    per_pass = 2 * _cus() * 64                         # rows in one pass of k_fc_tile's 2 CUs workgroups
    bits = lambda t: t.view(torch.int32)
    small = {normalize: _run(c, c["pf"], c["vf"], normalize) for normalize in (False, True)}
    for n, counts in ((per_pass + 65, (None, per_pass - 5, per_pass + 25)),
                      (2 * per_pass + 65, (None, per_pass + 64 * 37 + 25, 2 * per_pass - 5))):
        assert counts[1] == n - 70 or counts[2] == n - 70
        assert all(cnt % 64 and cnt < n for cnt in counts[1:]) and per_pass < counts[2] < 2 * per_pass
        src = torch.arange(n, device="cuda") % r
        pf, vf = c["pf"][src].contiguous(), c["vf"][src].contiguous()
        for normalize in (False, True):
            small_p, small_v = small[normalize]
            for cnt in counts:
                count = None if cnt is None else torch.tensor([cnt], dtype=torch.int32, device="cuda")
                big_p, big_v = _run(c, pf, vf, normalize, count=count)
                m = n if cnt is None else cnt
                assert torch.equal(bits(big_v[:m]), bits(small_v[src[:m]])), (n, normalize, cnt)
                assert torch.all(big_v[m:] == 7.0) and torch.all(big_p[m:] == 7.0), (n, normalize, cnt)
                same = (bits(big_p[:m]) == bits(small_p)[src[:m]]).all(1)
                assert same.all(), (n, normalize, cnt, torch.nonzero(~same).flatten()[:8].tolist())
                del big_p, big_v, same
        del pf, vf, src


def test_library_terms_through_the_kernels():
    """f16_pairs' constants for tanhf, expf and v_exp_f32 were measured through PyTorch's elementwise kernels; here the same
    functions are reached through cz_heads_tail itself with arguments that arrive exactly: one-hot weights of 1.0 on feature 0,
    no bias, fp16-exact arguments a (every fp16 value in [2^-10, 87]), so that
      value = tanhf(+-a),   logits = (0, -a),   stats = (0, s') with s' = fl(1 + fexp(-a)),   p_1 = fl(expf(-a) / s').
    tanhf within TANH_REL, the quotient within EXPF_REL + U of exp(-a) / s' for the s' the kernel stored (the argument
    -a - 0 is exact), s' within one
    rounding of the sum plus fexp's own term (3 U a + EXP2_REL) exp(-a).  Measured on an MI355X, error / constant: tanhf 0.42,
    expf and the division 0.47; s' 0.999 and 1 / s' 0.994 (one correct rounding each: these approach 1 and cannot pass it)."""
    import torch
    from cchess_alphazero import _native
    a = torch.arange(0x1400, 0x5570, dtype=torch.int16).view(torch.float16).float().cuda()        # 2^-10 ... 87
    assert a[0].item() == 2.0 ** -10 and a[-1].item() < 87.34 and a[-1].item() > 86.0
    n = a.numel()
    feat = torch.zeros((n, 180), device="cuda")
    feat[:, 0] = a
    wp = torch.zeros((2, 180))
    wp[1, 0] = -1.0
    w1 = torch.zeros((1, 180))
    w1[0, 0] = 1.0
    pk_p, pk_1 = _native.pack_fc_weights(wp).cuda(), _native.pack_fc_weights(w1).cuda()
    zero2, zero1 = torch.zeros(2, device="cuda"), torch.zeros(1, device="cuda")
    ad = a.double()
    for sign in (1.0, -1.0):
        pol = torch.full((n, 2), 7.0, device="cuda")
        val = torch.full((n,), 7.0, device="cuda")
        stats = torch.full((n, 2), 7.0, device="cuda")
        _native.heads_tail(feat, feat, pk_p, zero2, pk_1, zero1, torch.full((1,), sign, device="cuda"), 0.0, pol, val, stats)
        v = torch.tanh(sign * ad)
        r_tanh = ((val.double() - v).abs() / (fp.TANH_REL * v.abs())).max().item()
        assert r_tanh <= 1.0, r_tanh
    e = torch.exp(-ad)
    assert torch.all(stats[:, 0] == 0.0)
    s = stats[:, 1].double()
    r_stat = ((s - (1.0 + e)).abs() / (U * (1.0 + e) + (3 * U * ad + fp.EXP2_REL) * e)).max().item()
    r_exp = ((pol[:, 1].double() - e / s).abs() / ((fp.EXPF_REL + U) * e / s)).max().item()
    r_one = ((pol[:, 0].double() - 1.0 / s).abs() / (U / s)).max().item()              # expf(0) = 1 and one division
    print(f"\nlibrary terms / their constants: tanhf {r_tanh:.3f}, expf and division {r_exp:.3f}, running sum {r_stat:.3f}, "
          f"1 / s {r_one:.3f}")
    assert r_stat <= 1.0 and r_exp <= 1.0 and r_one <= 1.0, (r_stat, r_exp, r_one)


# ---- c. cz_head_convs --------------------------------------------------------------------------------------------------------

def _head_inputs(kind, n, c, dt, seed):
    import torch
    rng = np.random.default_rng(seed)
    if kind == "mixed":
        x = fp.mixed_activations((n, 90, c), rng)
    else:
        x = np.maximum(rng.standard_normal((n, 90, c)), 0.0).astype(np.float32) * 1.5
    w = (rng.standard_normal((6, c)) / c ** 0.5).astype(np.float32)
    b = rng.standard_normal(6).astype(np.float32)
    return torch.from_numpy(x).cuda().to(getattr(torch, dt)), torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()


def _head_convs_ratio(x, w, b, npol):
    """Worst |error| / bound of cz_head_convs against float64 on the same (already rounded) inputs.  Bound, per element:
    (C / 8 + 5) U (sum_c |x_c w_c| + |b|) -- a lane's chain of C / 8 products, three shuffle additions and the bias (the
    deepest path of a term through the kernel's roundings is C / 32 + 8 <= C / 8 + 5 for C >= 32); ReLU is 1-Lipschitz."""
    import torch
    from cchess_alphazero import _native
    n, c = x.shape[0], x.shape[-1]
    nval = 6 - npol
    pf = torch.full((n, npol * 90), 7.0, device="cuda")
    vf = torch.full((n, nval * 90), 7.0, device="cuda")
    _native.head_convs(x, w, b, npol, pf, vf)
    xd, wd, bd = x.double(), w.double(), b.double()
    ref = torch.relu(torch.einsum("npc,oc->nop", xd, wd) + bd[None, :, None])
    bound = (c / 8 + 5) * U * (torch.einsum("npc,oc->nop", xd.abs(), wd.abs()) + bd.abs()[None, :, None])
    got = torch.cat([pf.view(n, npol, 90), vf.view(n, nval, 90)], 1).double()
    return ((got - ref).abs() / bound).max().item()


@pytest.mark.parametrize("dt", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("c", [32, 128, 192, 256])
def test_head_convs_per_element(c, dt):
    """Both filter splits (4 + 2 and 2 + 4), 1 and 37 boards, O(1) and mixed data (values from 2^-30 to 3.0e4, exact zeros).
    Measured on an MI355X, worst error / bound: C = 32: 0.39 (fp32, bf16) / 0.53 (fp16); 128: 0.21-0.23; 192: 0.14-0.16;
    256: 0.12-0.14 (the bound grows with C / 8, the deepest chain only with C / 32)."""
    worst = 0.0
    for kind in ("O(1)", "mixed"):
        for n in (1, 37):
            x, w, b = _head_inputs(kind, n, c, dt, [c, n, int(kind == "mixed")])
            for npol in (4, 2):
                worst = max(worst, _head_convs_ratio(x, w, b, npol))
    print(f"\nhead convs C={c} {dt}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("npol", [4, 2])
def test_head_convs_past_one_grid_pass(npol):
    """2913 + 7 boards at C = 32: the grid stops at 8192 workgroups of 32 pixels (2912.7 boards), the rest is a second pass.
    Measured on an MI355X: 0.33 (4 + 2) and 0.23 (2 + 4)."""
    x, w, b = _head_inputs("O(1)", 2913 + 7, 32, "float32", [2920, npol])
    r = _head_convs_ratio(x, w, b, npol)
    print(f"\nhead convs 2920 boards, {npol} policy filters: worst error / bound {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("npol", [4, 2])
@pytest.mark.parametrize("dt", ["float32", "float16"])
def test_head_convs_one_hot_filters_select_channels_in_flatten_order(dt, npol):
    """A one-hot filter per output, a different channel each, no bias: the features are the chosen input channels exactly,
    in channels-first Flatten order [n][o * 90 + q]."""
    import torch
    from cchess_alphazero import _native
    n, c = 5, 128
    chan = [3, 64, 127, 0, 33, 90]
    g = torch.Generator(device="cuda").manual_seed(11)
    x = (torch.rand((n, 90, c), device="cuda", generator=g) * 4.0).to(getattr(torch, dt))
    w = torch.zeros((6, c), device="cuda")
    for o, ch in enumerate(chan):
        w[o, ch] = 1.0
    pf = torch.full((n, npol * 90), 7.0, device="cuda")
    vf = torch.full((n, (6 - npol) * 90), 7.0, device="cuda")
    _native.head_convs(x, w, torch.zeros(6, device="cuda"), npol, pf, vf)
    for o, ch in enumerate(chan):
        feat = pf[:, o * 90:(o + 1) * 90] if o < npol else vf[:, (o - npol) * 90:(o - npol + 1) * 90]
        assert torch.equal(feat, x[:, :, ch].float()), (o, ch)


# ---- d. cz_bias_act ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("c", [8, 32, 128, 192, 256])
def test_bias_act_value_for_value(c, dt):
    """x = relu?((x + b) (+ r)) in fp32, rounded once to the element type: equal to the same expression in PyTorch.  Rows 1, 90
    and, at C = 128, one board more than a full grid of 256 * 16 * 256 16-byte vectors takes in one pass."""
    import torch
    from cchess_alphazero import _native
    dtype = getattr(torch, dt)
    g = torch.Generator(device="cuda").manual_seed(c)
    big, vec = (365 * 90, 4) if dt == "float32" else (729 * 90, 8)
    assert c != 128 or (big - 90) * c // vec <= 256 * 16 * 256 < big * c // vec
    for rows in (1, 90) + ((big,) if c == 128 else ()):
        x0 = (torch.randn((rows, c), device="cuda", generator=g) * 3).to(dtype)
        r = (torch.randn((rows, c), device="cuda", generator=g) * 3).to(dtype)
        b = torch.randn((c,), device="cuda", generator=g).to(dtype)
        for res in (None, r):
            for relu in (True, False):
                x = x0.clone()
                out = _native.bias_act_(x, b, residual=res, relu=relu)
                want = x0.float() + b.float()
                if res is not None:
                    want = want + res.float()
                if relu:
                    want = torch.relu(want)
                assert out is x and torch.equal(x, want.to(dtype)), (rows, res is not None, relu)


def test_bias_act_rejects_bad_arguments():
    import torch
    from cchess_alphazero import _native
    x = torch.zeros((5, 16), device="cuda", dtype=torch.float16)
    with pytest.raises(_native.NativeError):                     # CZ_ERR_ARG: channels % 8 != 0
        _native.bias_act_(torch.zeros((5, 12), device="cuda"), torch.zeros(12, device="cuda"))
    with pytest.raises(_native.NativeError):                     # CZ_ERR_ARG: not a whole number of rows
        _native.bias_act_(torch.zeros((5, 8), device="cuda"), torch.zeros(16, device="cuda"))
    with pytest.raises(ValueError):                              # an fp32 bias under fp16 activations
        _native.bias_act_(x, torch.zeros(16, device="cuda"))
    with pytest.raises(ValueError):
        _native.bias_act_(x, torch.zeros(16, dtype=torch.float16))                # bias on the host
    b = torch.zeros(16, device="cuda", dtype=torch.float16)
    for bad in (torch.zeros((5, 16), device="cuda"), torch.zeros((4, 16), device="cuda", dtype=torch.float16),
                torch.zeros((5, 16), dtype=torch.float16)):
        with pytest.raises(ValueError):
            _native.bias_act_(x, b, residual=bad)
    assert not x.any()                                           # a refused call leaves x alone


def test_z_report_gpu_seconds():
    """Not a check: prints what this file cost."""
    import torch
    torch.cuda.synchronize()
    print(f"\ntests/test_gpu_heads.py: {time.time() - T0:.1f} s since import")
