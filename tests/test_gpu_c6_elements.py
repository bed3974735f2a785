"""-m gpu: the c6 tower kernels against float64, element by element (tests/c6_model.py: the operand codecs, the block's value on
exactly those operands and the bound; tests/test_c6_model_cpu.py shows that check telling a correct emulation from faulty ones).

Inputs throughout (c6_model.activations / filters): activations with planted values on every board (0, a lo part in bf6's
subnormals, values just below / at / above 28 * 2^k, exact ties of the value piece and of f16, a lo part that saturates),
output rows scaled by 0.004 and by 50 so that a filter carries several row shifts (asserted), biases alike, image exponents
k_x = -3, k_mid = 0, k_out = 4.  Board counts 1, 2, 3, 257, 700: one board per workgroup, the odd-count path, and workgroups
that take several boards through the deferred epilogue.

  a. the image writer, bit for bit: the image a block writes = encode_c6_image(its fp32 output) (the c8 image with y_exp = 127 =
     split_c8 of it) -- cz_resblock 128 / 192, CZ_F16C86, cz_resblock_chain against its own fp32 exit, cz_tower against cz_resblock;
  b. the skip path, bit for bit: w2 = 0, b2 = 0 -> relu(hi + lo6 2^(k_x - 11));
  c. the second convolution on exact operands (w1 = the centre-tap identity): only accumulation differs;
  d. the first convolution (w2 = the identity) and the general block, with the re-encoding of the intermediate image bounded;
  e. cz_resblock_heads, cz_tower's heads exit (3 blocks), cz_input_resblock (image only: decoded);
  f. the arithmetic's own error against the unrounded block, beside c8 and bf16x3.
Every image comparison covers the f16 tensor and the 24 bytes of each piece; the 8 bytes behind a piece's tail belong to no
piece (kernels that stage the image in LDS copy whatever lies there)."""
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import c6_model as m  # noqa: E402

KX, KM, KO = m.K_X, m.K_MID, m.K_OUT
COUNTS = (1, 2, 3, 257, 700)
T0 = time.time()


def _t(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _vals(triple):
    return tuple(_t(v) for v in triple)


def _pack6(w, kx, ky):
    import torch
    from cchess_alphazero import _native
    return _native.pack_conv3x3_c6_weights(torch.from_numpy(w), kx, ky)


def _pack8(w):
    import torch
    from cchess_alphazero import _native
    return _native.pack_conv3x3_c8_weights(torch.from_numpy(w))


def _pair(x, k):
    """fp32 numpy [n, 90, C] -> the c6 operand pair on the device (f16, int8 image)."""
    hi, img = m.encode_c6_image(x, k)
    return _t(hi), _t(img)


def _empty_pair(n, C, c8=False):
    import torch
    return (torch.zeros((n, 90, C), dtype=torch.float16, device="cuda"),
            torch.zeros((n, 90, 2 * C), dtype=torch.uint8 if c8 else torch.int8, device="cuda"))


def _same_image(got, want_hi, want_img, C, what):
    """(f16, image) tensors against numpy (float16, int8 / uint8), bit for bit on every byte that belongs to a piece."""
    gh, gi = got[0].cpu().numpy().view(np.uint16), got[1].cpu().numpy().view(np.uint8)
    assert np.array_equal(gh, want_hi.view(np.uint16)), (what, "f16 part", int((gh != want_hi.view(np.uint16)).sum()))
    mask = m.image_mask(C)
    bad = gi[..., mask] != want_img.view(np.uint8)[..., mask]
    assert not bad.any(), (what, "image", int(bad.sum()), np.argwhere(bad)[:4].tolist())


class Setup:
    """One block's tensors for `kind` in ("c6", "c86") at C filters: x (fp32), the device operand pair, packed filters on the
    device, biases, and the float64 operand values for the model (first n_model boards)."""

    def __init__(self, C, kind, n, seed, f1="random", f2="random", k_out=KO, n_model=0):
        import torch
        from cchess_alphazero import _native
        rng = np.random.default_rng(seed)
        self.C, self.kind, self.n = C, kind, n
        if kind == "c6":
            self.x = m.activations(n, C, KX, rng)
        else:                                                     # the input layer's c8 image: usual-scale data inside e4m3's range
            self.x = m.activations(n, C, 0, rng, also=(KM, -6))
        (self.w1, self.b1) = m.filters(C, rng, identity=f1 == "identity")
        (self.w2, self.b2) = m.filters(C, rng, identity=f2 == "identity", zero=f2 == "zero")
        self.p1 = _pack6(self.w1, KX, KM) if kind == "c6" else _pack8(self.w1)
        self.p2 = _pack6(self.w2, KM, k_out)
        self.d1 = m.decode_c6_pack(self.p1, C) if kind == "c6" else m.decode_c8_pack(self.p1, C)
        self.d2 = m.decode_c6_pack(self.p2, C)
        if f1 == "random":
            assert len(set(self.d1["sh"].tolist())) >= 3 and len(set(self.d1["sl"].tolist())) >= 3
        if f2 == "random":
            assert len(set(self.d2["sh"].tolist())) >= 3 and len(set(self.d2["sl"].tolist())) >= 3
            assert (self.d2["x_exp"], self.d2["y_exp"]) == (KM, k_out)
        if kind == "c6":
            self.pair = _pair(self.x, KX)
            self.code = None
        else:
            self.pair = _native.split_c8(torch.from_numpy(self.x).cuda())
            self.code = _native.F16C86
        self.dev = (self.p1.cuda(), _t(self.b1), self.p2.cuda(), _t(self.b2))
        if n_model:
            hi, img = self.pair[0][:n_model].cpu().numpy(), self.pair[1][:n_model].cpu().numpy()
            self.xv = _vals(m.image_values(hi, img, KX) if kind == "c6" else m.c8_image_values(hi, img))
            self.wv1, self.wv2 = _vals(m.filter_values(self.d1)), _vals(m.filter_values(self.d2))

    def run(self, n, f32=True, c8_out=False):
        import torch
        from cchess_alphazero import _native
        x = (self.pair[0][:n].contiguous(), self.pair[1][:n].contiguous())
        if f32:
            out = torch.full((n, 90, self.C), 7.0, device="cuda")
            _native.resblock(x, *self.dev, out_f32=out, dtype_code=self.code)
            return out
        out = _empty_pair(n, self.C, c8=c8_out)
        _native.resblock(x, *self.dev, out=out, dtype_code=self.code if self.code is not None else _native.F16C6)
        return out

    def model(self, exact_mid=False):
        return m.c6_block(self.xv, self.xv[0] + self.xv[1], self.wv1, _t(self.b1).double(), self.wv2, _t(self.b2).double(), KM,
                          exact_mid=exact_mid)


CASES = [(128, "c6"), (192, "c6"), (192, "c86")]


@pytest.mark.parametrize("C,kind", CASES)
def test_a_image_writer_is_the_encoder_bit_for_bit(C, kind):
    """The same block with fp32 output and with the image output: image == encode_c6_image(fp32 output, k_out); with y_exp = 127
    the c8 image == split_c8(fp32 output).  No tolerance: both are formed from the same fp32 values."""
    import torch
    from cchess_alphazero import _native
    s = Setup(C, kind, max(COUNTS), 11)
    s8 = Setup(C, kind, max(COUNTS), 11, k_out=m.OUT_C8)
    for n in COUNTS:
        f = s.run(n)
        assert torch.isfinite(f).all() and (f >= 0).all()
        want_hi, want_img = m.encode_c6_image(f, KO)
        codes = m.image_codes(want_img, C)
        if n >= 257:                                               # saturated / subnormal codes occur
            assert (codes[1] == 31).any() and ((codes[1] > 0) & (codes[1] < 4)).any() and ((codes[0] & 31 > 0) & (codes[0] & 31 < 4)).any()
        _same_image(s.run(n, f32=False), want_hi, want_img, C, (C, kind, n, "c6 image"))
        f8 = s8.run(n)
        assert torch.equal(f8, f)                                  # (the output format changes nothing before the conversion)
        got = s8.run(n, f32=False, c8_out=True)
        w_hi, w_c8 = _native.split_c8(f)
        assert torch.equal(got[0], w_hi) and torch.equal(got[1], w_c8), (C, kind, n, "c8 hand-over image")


@pytest.mark.parametrize("C", [128, 192])
def test_a_chains_write_the_image_of_their_fp32_exit(C):
    """cz_resblock_chain (192 filters: CZ_F16C6 and CZ_F16C86, two blocks): the image exit == encode(the fp32 exit of the same
    chain), and the fp32 exit == block-by-block cz_resblock.  cz_tower (128 filters) has no fp32 exit on c6: its c6 image and
    its c8 hand-over image == those of block-by-block cz_resblock, which the test above pins."""
    import torch
    from cchess_alphazero import _native
    rng = np.random.default_rng(23)
    (w1, b1), (w2, b2) = m.filters(C, rng), m.filters(C, rng)
    for t in (w1, b1, w2, b2):                                    # (the large rows 8x instead of 50x: two blocks of 50x rows on end
        t[1::7] /= 6.25                                           #  leave f16's range, which is no part of this test)
    for kind in (("c6",) if C == 128 else ("c6", "c86")):
        s = Setup(C, kind, 700, 12)
        blk0 = s.dev
        for y_exp in (KO - 1, m.OUT_C8):
            blk1 = (_pack6(w1, KO, KM + 1).cuda(), _t(b1), _pack6(w2, KM + 1, y_exp).cuda(), _t(b2))
            for n in COUNTS:
                x = (s.pair[0][:n].contiguous(), s.pair[1][:n].contiguous())
                mid = _native.resblock(x, *blk0, out=_empty_pair(n, C), dtype_code=s.code if s.code is not None else _native.F16C6)
                c8 = y_exp == m.OUT_C8
                if C == 192:
                    f = torch.empty((n, 90, C), device="cuda")
                    _native.resblock_chain(x, [blk0, blk1], out_f32=f, dtype_code=s.code)
                    f1 = torch.empty((n, 90, C), device="cuda")
                    _native.resblock(mid, *blk1, out_f32=f1)
                    assert torch.equal(f, f1) and float(f.max()) < 6e4, (kind, n)
                    got = _native.resblock_chain(x, [blk0, blk1], out=_empty_pair(n, C, c8=c8), dtype_code=s.code)
                    if c8:
                        w_hi, w_c8 = _native.split_c8(f)
                        assert torch.equal(got[0], w_hi) and torch.equal(got[1], w_c8), (kind, n)
                    else:
                        _same_image(got, *m.encode_c6_image(f, y_exp), C, (kind, n, "chain image"))
                else:
                    want = _native.resblock(mid, *blk1, out=_empty_pair(n, C, c8=c8))
                    got = _native.tower(x, [blk0, blk1], _native.IMG_C8 if c8 else _native.IMG_C6, out=_empty_pair(n, C, c8=c8))
                    if c8:
                        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), n
                    else:
                        _same_image(got, want[0].cpu().numpy(), want[1].cpu().numpy(), C, (n, "tower image"))


@pytest.mark.parametrize("C,kind", CASES)
def test_b_skip_path_is_exact(C, kind):
    """w2 = 0, b2 = 0: the fp32 output is relu(hi + lo6 2^(k_x - 11)) of the input image (c8 input: hi + e4m3 2^-11), exactly, for
    every channel -- each lane's element of the lo piece (the upper lane half shifts the piece down by one element)."""
    import torch
    s = Setup(C, kind, max(COUNTS), 13, f2="zero")
    hi, img = s.pair[0].cpu().numpy(), s.pair[1].cpu().numpy()
    v = m.image_values(hi, img, KX) if kind == "c6" else m.c8_image_values(hi, img)
    want = v[0] + v[1]
    if kind == "c6":                                              # (the premise of (b) and (c): the pair's value is an fp32 number)
        assert np.array_equal(want, want.astype(np.float32).astype(np.float64))
    want = want.astype(np.float32).astype(np.float64)            # (c8 input: one fp32 rounding of hi + e4m3 2^-11)
    assert (want >= 0).all()
    assert (v[1] != 0).mean() > 0.3 and (v[1] < 0).any()
    for n in COUNTS:
        got = s.run(n).cpu().numpy().astype(np.float64)
        bad = got != want[:n]
        assert not bad.any(), (C, kind, n, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _check(s, exact_mid, what, counts=(3,)):
    worst = 0.0
    for n in counts:
        t = s if n == s.n else _setup(s.C, s.kind, n, s.seed, s.f1, s.f2)
        mod = t.model(exact_mid)
        got = t.run(n).double()
        r = m.ratio(got, mod["y"], mod["bound"])
        print(f"{what}, {t.C} filters, {t.kind}, {n} boards: {r:.3f} of the bound")
        assert r <= 1.0, (what, t.C, t.kind, n, r)
        worst = max(worst, r)
    return worst


def _setup(C, kind, n, seed, f1="random", f2="random"):
    s = Setup(C, kind, n, seed, f1=f1, f2=f2, n_model=n)
    s.seed, s.f1, s.f2 = seed, f1, f2
    return s


@pytest.mark.parametrize("C", [128, 192])
def test_c_second_convolution_on_exact_operands(C):
    """w1 = the centre-tap identity, b1 = 0, x >= 0: the intermediate value is exactly hi + lo6 2^(k_x - 11) (an fp32 number:
    tests/test_c6_model_cpu.py), so its k_mid image is known and only the second convolution's accumulation differs from the
    float64 model.  Measured on an MI355X: 0.094 / 0.132 of the bound at 128 filters (3 / 257 boards), 0.107 / 0.124 at 192."""
    _check(_setup(C, "c6", 3, 14, f1="identity"), True, "(c) second convolution", counts=(3, 257))


@pytest.mark.parametrize("C,kind", CASES)
def test_d_first_convolution_and_the_general_block(C, kind):
    """w2 = the centre-tap identity: the block's output is relu(the intermediate image's value + b2 + skip), so every element
    checks one element of the first convolution, to its accumulation bound A1 -- plus one step of the lo piece (one f16 ulp)
    where the model's value lies within A1 of a rounding boundary of the image.  Then both filters random: the same allowances
    through |w2|.  Measured on an MI355X: first convolution 0.936 (128), 0.949 (192), 0.944 (CZ_F16C86) of the bound -- an element whose rounding did fall the
    other way uses its whole allowance, so this stays close to 1 by construction; general block 0.134 / 0.267 (128 filters, 3 / 257
    boards), 0.233 (192), 0.187 (CZ_F16C86)."""
    _check(_setup(C, kind, 3, 15, f2="identity"), False, "(d) first convolution")
    _check(_setup(C, kind, 3, 16), False, "(d) general block", counts=(3, 257) if C == 128 else (3,))


def _head_filters(C, rng):
    hw = (rng.standard_normal((6, C)) / C ** 0.5).astype(np.float32)
    hb = (rng.standard_normal(6) * 0.1).astype(np.float32)
    return hw, hb


def test_e_heads_block_and_the_tower_heads_exit():
    """cz_resblock_heads on c6 filters (1 and 257 boards) and cz_tower's heads exit behind 3 blocks (3 and 257 boards): the head
    features against the float64 block model, the block's bound carried through |head filter| plus the head sum's own fp32
    rounding.  The tower's third block and heads are modelled on the image the same entry point writes behind two blocks
    (carrying the bound through three blocks' |filters| instead gives a bound thousands of times the features: no check).
    Measured on an MI355X: cz_resblock_heads 0.010 / 0.098 of the bound (1 / 257 boards), cz_tower 0.002 /
    0.059 (3 / 257 boards; the bound is 0.3 % of a feature at the median)."""
    import torch
    from cchess_alphazero import _native
    C = 128
    rng = np.random.default_rng(31)
    hw, hb = _head_filters(C, rng)
    hw_t, hb_t = _t(hw), _t(hb)
    for n in (1, 257):
        s = _setup(C, "c6", n, 17)
        mod = s.model()
        want, bound = m.heads(mod["y"], mod["bound"], hw_t.double(), hb_t.double())
        pf, vf = torch.zeros((n, 4 * 90), device="cuda"), torch.zeros((n, 2 * 90), device="cuda")
        _native.resblock_heads(s.pair, *s.dev, hw_t, hb_t, 4, pf, vf)
        got = torch.cat([pf.view(n, 4, 90), vf.view(n, 2, 90)], 1).permute(0, 2, 1).double()
        r = m.ratio(got, want, bound)
        print(f"(e) cz_resblock_heads, {n} boards: {r:.3f} of the bound")
        assert r <= 1.0, (n, r)
    # three blocks in one launch, the heads as the exit: exponents k_x -> (k_mid) -> k_out -> (k_mid + 1) -> k_out - 1 -> (k_mid) -> heads
    ks = [(KX, KM, KO), (KO, KM + 1, KO - 1), (KO - 1, KM, 0)]
    blocks_np = [(m.filters(C, rng), m.filters(C, rng)) for _ in ks]
    for (w1, _), (w2, _) in blocks_np[1:]:                        # (keep the tower's activations in range: no 50x rows twice over)
        w1[1::7] /= 50.0
        w2[1::7] /= 50.0
    packs = [(_pack6(b[0][0], kx, km), b[0][1], _pack6(b[1][0], km, ko), b[1][1]) for b, (kx, km, ko) in zip(blocks_np, ks)]
    dev = [(p1.cuda(), _t(b1), p2.cuda(), _t(b2)) for p1, b1, p2, b2 in packs]
    for n in (3, 257):
        x = m.activations(n, C, KX, np.random.default_rng(18))
        pair = _pair(x, KX)
        # the image the chain holds in LDS behind its second block = the image exit of the same entry point at two blocks
        # (which (a) pins bit for bit to block-by-block cz_resblock, and (d) pins a block to the model): decode it, model the
        # third block and the heads on exactly those operands
        img2 = _native.tower(pair, dev[:2], _native.IMG_C6, out=_empty_pair(n, C))
        by_block = _native.resblock(_native.resblock(pair, *dev[0], out=_empty_pair(n, C)), *dev[1], out=_empty_pair(n, C))
        _same_image(img2, by_block[0].cpu().numpy(), by_block[1].cpu().numpy(), C, (n, "two-block exit"))
        xv = _vals(m.image_values(img2[0].cpu().numpy(), img2[1].cpu().numpy(), ks[2][0]))
        assert float(xv[0].max()) < 6e4 and float((xv[0] > 0).double().mean()) > 0.2
        p1, b1, p2, b2 = packs[2]
        wv1, wv2 = _vals(m.filter_values(m.decode_c6_pack(p1, C))), _vals(m.filter_values(m.decode_c6_pack(p2, C)))
        mod = m.c6_block(xv, xv[0] + xv[1], wv1, _t(b1).double(), wv2, _t(b2).double(), ks[2][1])
        want, bound = m.heads(mod["y"], mod["bound"], hw_t.double(), hb_t.double())
        pf, vf = torch.zeros((n, 4 * 90), device="cuda"), torch.zeros((n, 2 * 90), device="cuda")
        _native.tower(pair, dev, _native.EXIT_HEADS, heads=(hw_t, hb_t, 4, pf, vf))
        got = torch.cat([pf.view(n, 4, 90), vf.view(n, 2, 90)], 1).permute(0, 2, 1).double()
        r = m.ratio(got, want, bound)
        pos = want > 0
        rel = float((bound[pos] / want[pos]).median())             # (the bound is a check: a small fraction of a feature)
        print(f"(e) cz_tower, 3 blocks + heads, {n} boards: {r:.3f} of the bound (median bound / feature {rel:.1e})")
        assert r <= 1.0 and rel < 1e-2, (n, r, rel)


def _planes(n, in_planes, rng):
    """uint8 [n, in_planes, 10, 9] one-hot-like planes: ~32 occupied squares, one plane each (what the search writes)."""
    p = np.zeros((n, in_planes, 90), np.uint8)
    for b in range(n):
        sq = rng.choice(90, size=32, replace=False)
        p[b, rng.integers(0, in_planes, size=32), sq] = 1
    return p.reshape(n, in_planes, 10, 9)


@pytest.mark.parametrize("in_planes", [14, 28])
def test_e_input_resblock_writes_the_image_of_the_model(in_planes):
    """cz_input_resblock on c6 (input layer in exact fp32 -> c8 image -> first filter c8-packed -> c6 block; image output only):
    the decoded pair hi + lo6 2^(k_out - 11) against the float64 model (input layer in float64, its c8 image, the block model)
    within the bound plus one encoding step of the output image; the value piece == bf6(pair value 2^-k_out) except where that
    argument lies within the lo piece's resolution of a bf6 tie (counted, at most 1 % of the image).  With and without rows /
    count / masks: identical images.  Measured on an MI355X: 0.578 (14 planes) and 0.789 (28 planes) of the bound, nothing saturated;
    0.04 % of the elements near a tie, 0.005 - 0.007 % differ, none away from a tie."""
    import torch
    from cchess_alphazero import _native
    C, n = 128, 37
    rng = np.random.default_rng(40 + in_planes)
    w_in = (rng.standard_normal((C, in_planes, 5, 5)) * 0.35).astype(np.float32)
    b_in = (rng.standard_normal(C) * 0.3).astype(np.float32)
    (w1, b1), (w2, b2) = m.filters(C, rng), m.filters(C, rng)
    k_mid, k_out = 3, 7
    p1, p2 = _pack8(w1), _pack6(w2, k_mid, k_out)
    planes = _planes(n, in_planes, rng)
    pl_t = _t(planes)
    table, bin_t = _native.input_table(torch.from_numpy(w_in)).cuda(), _t(b_in)
    dev = (p1.cuda(), _t(b1), p2.cuda(), _t(b2))
    out = _native.input_resblock(pl_t, table, bin_t, *dev, _empty_pair(n, C))
    hi, lo6, hi6 = m.decode_c6_image(out[0].cpu().numpy(), out[1].cpu().numpy())
    got = hi + lo6 * 2.0 ** (k_out - m.LO_SHIFT)
    # the model: the input layer is a sum of <= 25 * in_planes fp32 table entries + bias per output (exact fp32 gather in the
    # kernel: its rounding, (terms + 1) u sum |terms|, enters the block as a perturbation of the input value)
    import torch.nn.functional as F
    x64 = F.conv2d(pl_t.double(), _t(w_in).double(), _t(b_in).double(), padding=2)
    xmag = F.conv2d(pl_t.double(), _t(w_in).double().abs(), _t(b_in).double().abs(), padding=2)
    x64, xmag = (t.permute(0, 2, 3, 1).reshape(n, 90, C) for t in (x64, xmag))
    x_bound = 40.0 * m.U * xmag                                   # (<= 32 occupied squares + the bias: at most 33 additions)
    x32 = m.to_f32(m.relu(x64))
    h8 = m.to_f16(x32)
    e4 = lambda t: t.clamp(-448.0, 448.0).to(torch.float32).to(torch.float8_e4m3fn).double()
    xv = (h8, e4((x32 - h8) * 2.0 ** m.LO_SHIFT) * 2.0 ** -m.LO_SHIFT, e4(x32))
    # how far the kernel's c8 operands may lie from these: the interval's ends, as for a c6 image
    ends = [m.to_f32(m.relu(x64 + x_bound)), m.to_f32(m.relu(x64 - x_bound))]
    trip = lambda t: (m.to_f16(t), e4((t - m.to_f16(t)) * 2.0 ** m.LO_SHIFT) * 2.0 ** -m.LO_SHIFT, e4(t))
    up, dn = trip(ends[0]), trip(ends[1])
    dx = [torch.maximum((up[i] - xv[i]).abs(), (dn[i] - xv[i]).abs()) for i in range(3)]
    dx[1] = torch.where(dx[0] == 0, dx[1], m.f16_ulp(ends[0]) + x_bound)
    wv1, wv2 = _vals(m.filter_values(m.decode_c8_pack(p1, C))), _vals(m.filter_values(m.decode_c6_pack(p2, C)))
    mod = m.c6_block(xv, xv[0] + xv[1], wv1, _t(b1).double(), wv2, _t(b2).double(), k_mid, dx=dx)
    y = mod["y"]
    # one encoding step of the output image: half a step of the lo piece at the largest lo part an f16 rounding leaves
    # (half an f16 ulp), i.e. 2^-3 of that, and never less than half the piece's smallest step; saturated elements excluded
    half_ulp = m.f16_ulp(y + mod["bound"]) / 2
    enc = torch.maximum(half_ulp / 8, torch.full_like(y, 2.0 ** (k_out - m.LO_SHIFT - 5)))
    unsat = (y + mod["bound"] < 28.0 * 2.0 ** k_out) & (half_ulp * 2.0 ** (m.LO_SHIFT - k_out) <= 28.0)
    assert float(unsat.double().mean()) > 0.95
    r = float(((_t(got) - y).abs() / (mod["bound"] + enc))[unsat].max())
    print(f"(e) cz_input_resblock, {in_planes} planes: {r:.3f} of the bound; {100 * (1 - float(unsat.double().mean())):.2f} % saturated")
    assert r <= 1.0, r
    # the value piece from the pair's value
    near_tie, differ, outside = m.value_piece_check(got, hi6, k_out)
    print(f"    value piece: {100 * near_tie:.3f} % of the elements near a tie, {100 * differ:.4f} % differ")
    assert outside == 0 and near_tie <= 0.01, (outside, near_tie)
    # rows / count / masks: the same boards through the compact queue and with occupancy masks give the same bytes
    rows = torch.randperm(n, device="cuda").int()
    count = torch.tensor([n - 5], dtype=torch.int32, device="cuda")
    out_q = _native.input_resblock(pl_t, table, bin_t, *dev, _empty_pair(n, C), rows=rows, count=count)
    sel = rows[:n - 5].long()
    assert torch.equal(out_q[0][:n - 5], out[0][sel])
    mask = torch.from_numpy(m.image_mask(C)).cuda()
    assert torch.equal(out_q[1][:n - 5][..., mask], out[1][sel][..., mask])
    occ = np.zeros((n, 96), np.int64)
    for c in range(in_planes):
        occ[:, :90] |= planes[:, c].reshape(n, 90).astype(np.int64) << c
    masks = _t(occ.astype(np.uint32).view(np.int32))
    out_m = _native.input_resblock(pl_t, table, bin_t, *dev, _empty_pair(n, C), masks=masks)
    assert torch.equal(out_m[0], out[0]) and torch.equal(out_m[1][..., mask], out[1][..., mask])


@pytest.mark.parametrize("C", [128, 192])
def test_f_c6_block_against_the_unrounded_block(C):
    """Usual-scale data (no planted values, no scaled rows; exponents fitted to the tensors with one bit of headroom, as the
    calibration does): the c6 block's error against the float64 block on the unrounded fp32 tensors, relative to the sum of
    |terms| of the second convolution, beside the c8 block's and the bf16x3 block's on the same tensors.  include/czero.h
    claims a per-product accuracy of about 2^-15 for c6 and 2^-16 for c8.  Measured on an MI355X: relative error, max / rms over the elements -- 128 filters: c6 1.47e-5 /
    1.78e-6, c8 6.95e-6 / 8.71e-7, bf16x3 3.50e-6 / 3.90e-7; 192 filters: c6 1.51e-5 / 1.57e-6, c8 6.66e-6 / 7.68e-7, bf16x3 3.57e-6 /
    3.41e-7.  c6 / c8 = 2.04 and 2.05: the one bit the header states.  (With e rms|term| sqrt(2 * 9 C) against 9 C mean|term| the rms
    figures at 128 filters are e = 2^-15.1 for c6, 2^-16.1 for c8 and 2^-17.3 for bf16x3 per product: the header's claims hold.)."""
    import torch
    from cchess_alphazero import _native
    n = 64
    g = torch.Generator(device="cuda").manual_seed(50 + C)
    x = (torch.randn((n, 90, C), device="cuda", generator=g) * 1.5).relu()
    w1, w2 = (torch.randn((C, C, 3, 3), device="cuda", generator=g) / (3.0 * C ** 0.5) for _ in range(2))
    b1, b2 = (torch.randn((C,), device="cuda", generator=g) * 0.3 for _ in range(2))
    d = torch.float64
    w9 = lambda w: w.to(d).reshape(C, C, 9)
    t = m.relu(m.conv(x.to(d), w9(w1)) + b1.to(d))
    exact = m.relu(m.conv(t, w9(w2)) + b2.to(d) + x.to(d))
    mag = m.conv(t, w9(w2).abs()) + b2.to(d).abs() + x.to(d)
    kexp = lambda v: int(np.ceil(np.log2(float(v.max()) / 28.0))) + 1
    kx, km, ko = kexp(x), kexp(t), kexp(exact)
    err = {}
    out = torch.empty((n, 90, C), device="cuda")
    _native.resblock(_pair(x.cpu().numpy(), kx), _pack6(w1.cpu().numpy(), kx, km).cuda(), b1, _pack6(w2.cpu().numpy(), km, ko).cuda(),
                     b2, out_f32=out)
    err["c6"] = out.to(d) - exact
    _native.resblock(_native.split_c8(x), _native.pack_conv3x3_c8_weights(w1).cuda(), b1,
                     _native.pack_conv3x3_c8_weights(w2).cuda(), b2, out_f32=out)
    err["c8"] = out.to(d) - exact
    xh = x.to(torch.bfloat16)
    xp = (xh, (x - xh.float()).to(torch.bfloat16))
    pb = lambda w: _native.pack_conv3x3_weights(w, torch.bfloat16, 2).cuda()
    tp = (torch.empty_like(xh), torch.empty_like(xh))
    _native.conv3x3(xp, pb(w1), b1, out=tp, relu=True)           # (two launches: the split block kernel exists at 128 filters only)
    _native.conv3x3(tp, pb(w2), b2, skip=xp, out_f32=out, relu=True)
    err["bf16x3"] = out.to(d) - exact
    # per-product accuracy e: the block's error is a sum of ~2 * 9 C product errors of random sign, so its rms over the
    # elements is about e * rms|term| * sqrt(terms); relative to the sum of |terms| (~ terms * mean|term|):
    fig = {k: (float((v.abs() / mag).max()), float(((v / mag) ** 2).mean() ** 0.5)) for k, v in err.items()}
    print(f"(f) {C} filters, exponents {kx} {km} {ko}: " +
          ", ".join(f"{k} max {a:.2e} rms {b:.2e}" for k, (a, b) in fig.items()))
    assert fig["c6"][0] < 3e-5 and fig["c8"][0] < 3e-5            # (the c8 test's bar for one convolution, on a whole block)
    assert fig["c6"][1] < 4.0 * fig["c8"][1] + 1e-8, fig          # 2^-15 against 2^-16 per product: one bit, with as much margin
    assert fig["c6"][1] < 8.0 * fig["bf16x3"][1] + 1e-8, fig


def test_z_report_gpu_seconds():
    """Not a check: prints what this file cost."""
    import torch
    torch.cuda.synchronize()
    print(f"tests/test_gpu_c6_elements.py: {time.time() - T0:.1f} s since import")
