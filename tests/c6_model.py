"""Float64 model of the c6 tower arithmetic (csrc/xq_conv_block_c8.h k_resblock_c8<.., C6>, csrc/xq_conv_ip.h k_resblock_ip_c8,
csrc/xq_conv_ip4.h k_resblock_ip4_c8; K loop
csrc/xq_c8_kloop.h FMT = 1): the operand formats as bytes, the value of a convolution and of a residual block on exactly those
operands, and the per-element bound the kernels are held to (tests/test_gpu_c6_elements.py; the check itself is tested on
faulty arithmetic in tests/test_c6_model_cpu.py).

Operands.  bf6 = e3m2: sign, 3 exponent bits (bias 3), 2 mantissa bits, no inf / nan; grid 0, 1/16 .. 3/16 (subnormals),
1/4 .. 28; conversion rounds to nearest even and saturates at 28.
  * an activation image of exponent k stands for x (fp32) as  hi = f16(x),  lo6 = bf6((x - hi) 2^(11 - k)),  hi6 = bf6(x 2^-k):
    an f16 tensor [n, 90, C] and an image [n, 90, 2 C] of bytes.  Of a pixel's 2 C bytes the first C belong to the lo pieces,
    the last C to the value pieces; the piece of the 32-channel block w occupies 24 of the 32 bytes at 32 w (its 16-byte
    head in 16-byte chunk  kind * C / 16 + 4 (w >> 1) + 2 (w & 1),  its 8-byte tail at the start of the next chunk; the 8
    bytes behind a tail belong to nobody and are not compared).  A piece is 32 codes of 6 bits, element e at bits 6 e,
    little endian, element e = channel  8 (e >> 3) + ((e >> 1) & 3) + 4 (e & 1)  of the block.
  * a packed filter holds f16(w), W6 = bf6(w 2^sh[o]) and L6 = bf6((w - f16(w)) 2^sl[o]) with one pair of shifts per OUTPUT
    channel o, and the exponents of the image it reads and of the one its convolution writes.
A product is   f16(w) hi  +  W6 2^-sh lo6 2^(k - 11)  +  L6 2^-sl hi6 2^k.   The skip operand is  hi + lo6 2^(k - 11).
The c8 arithmetic (a c6 tower's first block reads the input layer's c8 image) is the same sum with e4m3 operands, k = 0 and
shifts that put a row's largest magnitude in [128, 256); `corr_conv` takes either as the values the operands stand for.

Accumulation (the bound).  The accumulators start at the bias (second convolution: fp32(bias + skip)); the K loop is
tap-major, and per tap and 64-channel block it issues: two fp16 matrix instructions of 16 channels, the W6 lo6 instruction
over the block's 64 channels, two more fp16 ones, the L6 hi6 instruction -- 6 steps, 192 products.  Every product is exact
(11 + 11, 3 + 3 bits), so all the error is fp32 accumulation.  As in tests/f16_pairs.py bound (a): a partial sum inside step
s is at most |P_(s-1)| + A_s (P the exact value before the step, start value included, A_s the step's sum of |term|), every
rounding is at most u (|P| + A_s) with u = 2^-24, and with one rounding per product (N_s = 16 or 64; an instruction that adds
several products before it rounds does fewer), independent and zero-mean (variance <= (u S)^2 / 3),
    ACC = 8 u sqrt(sum_s N_s / 3 (|P_(s-1)| + A_s)^2)
is 8 standard deviations of an upper model.  With 3456 roundings per output (128 filters) that is 1.6e-5 of a TYPICAL
partial sum; on the element tests' data (a partial sum is a fraction of the sum of |terms|) 1.5e-6 to 2e-6 of that sum at
the median: the c8 test's "1e-5 of the sum of |terms|" (the project's own figure for these instructions) is five times
wider, the deterministic worst case  u sum_s N_s (..)  about ten times.
Start value: at most two fp32 additions (the skip pair's value, then the bias), 2 u |bias + skip|.  ReLU and the fp32 store add nothing.

A residual block re-encodes its intermediate activation t = relu(conv1) with the exponent k_mid.  The kernel encodes ITS
fp32 t', which differs from the model's by at most A1 = ACC_1 + u |conv1| (before the ReLU), so a rounding (f16, either bf6 piece) may fall the
other way.  All three conversions are monotone: the operands of any t' in [t - A1, t + A1] lie between those of the two ends,
which the model encodes as well -- D_hi, D_hi6 = the largest distance of an end's operand from the model's (0 for nearly
all elements, one f16 ulp / one bf6 step where t sits within A1 of a rounding boundary).  The lo piece is monotone while hi
does not move: D_lo = the same distance there (at most |t' - t| plus one bf6 step of the lo piece), and one f16 ulp of the
upper end (+ A1) where hi moves.  These enter the second convolution through |f16(w)|, |W6| and |L6|:
    bound = ACC_2 + 2 u |b2 + skip| + conv(D_hi, |w_hi|) + conv(D_lo, |W6|) + conv(D_hi6, |L6|).
Nothing in a bound looks at a kernel's output.

Everything that computes works on numpy float64 arrays and on torch float64 tensors alike (the CPU test feeds the check the
very functions the GPU tests use); the byte codecs are numpy.  Activations are channels-last [n, 90, C], filters [o, c, 9]
(tap = 3 ky + kx)."""
import numpy as np

U = 2.0 ** -24                  # fp32 unit roundoff
LAMBDA = 8.0
LO_SHIFT = 11                   # lo pieces are scaled by 2^11 (csrc/xq_nn_common.h cf8::X_LO_SHIFT)
BF6_MAX = 28.0
OUT_C8 = 127                    # y_exp of a c6 filter whose block writes a c8 image (CZ_C6_OUT_C8)


# ---- bf6 ------------------------------------------------------------------------------------------------------------------
def bf6_value(code):
    s, e, m = code >> 5, (code >> 2) & 7, code & 3
    v = (1.0 + m / 4.0) * 2.0 ** (e - 3) if e else m / 16.0
    return -v if s else v


BF6_TABLE = np.array([bf6_value(c) for c in range(64)])


def channel_of(e):
    return 8 * (e >> 3) + ((e >> 1) & 3) + 4 * (e & 1)


ELEM_CH = np.array([channel_of(e) for e in range(32)])


def _is_np(t):
    return isinstance(t, np.ndarray)


def _exp2(e):
    """2^e for an integer array, EXACTLY (a device's pow / exp2 may be an ulp off, which turns an exact tie into a rounding the
    other way): the float64 whose exponent field is e + 1023."""
    if _is_np(e):
        return ((e.astype(np.int64) + 1023) << 52).view(np.float64)
    import torch
    return ((e.long() + 1023) << 52).view(torch.float64)


def _frexp_exp(a):
    if _is_np(a):
        return np.frexp(a)[1]
    import torch
    return torch.frexp(a)[1]


def _rint(a):
    return np.rint(a) if _is_np(a) else a.round()


def _min(a, b):
    return np.minimum(a, b) if _is_np(a) else a.clamp(max=b)


def _max(a, b):
    if _is_np(a):
        return np.maximum(a, b)
    import torch
    return torch.maximum(a, b)


def _where(c, a, b):
    if _is_np(c):
        return np.where(c, a, b)
    import torch
    return torch.where(c, a, b)


def _sign(a):
    return np.sign(a) if _is_np(a) else a.sign()


def bf6_step(a):
    """The grid spacing of bf6 at magnitude a (float64 >= 0): 2^(floor(log2 a) - 2), 1/16 below 1/4."""
    ex = _frexp_exp(a) - 1
    ex = np.maximum(ex, -2) if _is_np(a) else ex.clamp(min=-2)
    return _exp2(ex - 2)


def bf6_round(v):
    """float64 -> the bf6 grid value (float64): nearest, ties to the even code, saturating at +-28."""
    a = _min(abs(v), BF6_MAX)
    step = bf6_step(a)
    return _sign(v) * _min(_rint(a / step) * step, BF6_MAX)


def bf6_codes(v):
    """numpy float64 -> the 6-bit codes of bf6_round(v); the sign bit is the sign of v, also where v rounds to zero."""
    q = np.abs(bf6_round(v))
    m, e = np.frexp(q)                                           # q = m 2^e, m in [0.5, 1)
    normal = ((e + 2) << 2) | np.rint(m * 8 - 4).astype(np.int64)  # exponent field (e - 1) + 3, mantissa (2 m - 1) 4
    code = np.where(q < 0.25, np.rint(q * 16).astype(np.int64), normal)
    return (code | (np.signbit(v).astype(np.int64) << 5)).astype(np.uint8)


# ---- roundings to the kernels' storage formats, float64 in and out ----------------------------------------------------------
def to_f32(t):
    if _is_np(t):
        return t.astype(np.float32).astype(np.float64)
    import torch
    return t.to(torch.float32).double()


def to_f16(t):
    """f16(fp32(t)): the kernels convert their fp32 value."""
    if _is_np(t):
        return t.astype(np.float32).astype(np.float16).astype(np.float64)
    import torch
    return t.to(torch.float32).to(torch.float16).double()


def f16_ulp(t):
    """Spacing of f16 at magnitude t >= 0 (2^-24 in the subnormal range)."""
    ex = _frexp_exp(t) - 1
    ex = np.maximum(ex, -14) if _is_np(t) else ex.clamp(min=-14)
    return _exp2(ex - 10)


def relu(t):
    return t * (t > 0)


def encode_values(t, k):
    """The operand triple of an image of exponent k for the fp32 values t (float64 holding fp32 values), as the VALUES the
    kernels' products use:  (hi, lo6 2^(k - 11), hi6 2^k)."""
    hi = to_f16(t)
    s_lo, s_hi = 2.0 ** (k - LO_SHIFT), 2.0 ** k
    return hi, bf6_round((t - hi) / s_lo) * s_lo, bf6_round(t / s_hi) * s_hi


# ---- the activation image as bytes (numpy) ----------------------------------------------------------------------------------
def piece_offsets(C):
    """Byte offset inside a pixel's 2 C image bytes of piece (kind, 32-channel block w): int [2, C / 32].  The head's 16 bytes
    start there; the tail's 8 open the next 16-byte chunk, i.e. follow directly."""
    w = np.arange(C // 32)
    return 16 * (np.arange(2)[:, None] * (C // 16) + 4 * (w >> 1) + 2 * (w & 1))


def image_mask(C):
    """bool [2 C]: the image bytes that belong to a piece (24 of every 32)."""
    m = np.zeros(2 * C, bool)
    for off in piece_offsets(C).reshape(-1):
        m[off:off + 24] = True
    return m


def pack_pieces(codes):
    """uint8 codes [..., 32] in element order -> the 24 bytes of a piece [..., 24]."""
    bits = (codes[..., None] >> np.arange(6, dtype=np.uint8)) & 1
    return np.packbits(bits.reshape(codes.shape[:-1] + (192,)), axis=-1, bitorder="little")


def unpack_pieces(pieces):
    """[..., 24] bytes -> uint8 codes [..., 32] in element order."""
    bits = np.unpackbits(np.ascontiguousarray(pieces), axis=-1, bitorder="little").reshape(pieces.shape[:-1] + (32, 6))
    return (bits << np.arange(6, dtype=np.uint8)).sum(-1).astype(np.uint8)


def _as_numpy(t):
    return t if _is_np(t) else t.detach().cpu().numpy()


def encode_c6_image(x_f32, k):
    """fp32 [n, 90, C] (numpy, or a torch tensor on any device) -> (hi float16 [n, 90, C], img int8 [n, 90, 2 C]) numpy: the
    operand pair a c6 kernel writes for these values with the exponent k.  The 8 bytes behind each tail are zero."""
    x = _as_numpy(x_f32).astype(np.float32)
    n, _, C = x.shape
    hi = x.astype(np.float16)
    x64 = x.astype(np.float64)
    lo = x64 - hi.astype(np.float64)                             # (exact in fp32 as well)
    img = np.zeros((n, 90, 2 * C), np.uint8)
    off = piece_offsets(C)
    for kind, src in enumerate((lo * 2.0 ** (LO_SHIFT - k), x64 * 2.0 ** -k)):
        codes = bf6_codes(src).reshape(n, 90, C // 32, 32)[..., ELEM_CH]      # element e <- channel_of(e)
        pieces = pack_pieces(codes)
        for w in range(C // 32):
            img[:, :, off[kind, w]:off[kind, w] + 24] = pieces[:, :, w]
    return hi, img.view(np.int8)


def image_codes(img, C, elem_ch=ELEM_CH, offsets=None):
    """The bf6 codes of an image by channel: uint8 [2 (kind), n, 90, C].  (elem_ch / offsets: a decoder with another element
    order or other piece positions -- the faulty readers of tests/test_c6_model_cpu.py; offsets [2, C / 32, 2] = byte offsets of
    every piece's head and tail.)"""
    raw = _as_numpy(img).view(np.uint8)
    off = piece_offsets(C)
    if offsets is None:
        offsets = np.stack([off, off + 16], -1)
    out = np.zeros((2,) + raw.shape[:2] + (C,), np.uint8)
    for kind in range(2):
        for w in range(C // 32):
            h, t = offsets[kind, w]
            codes = unpack_pieces(np.concatenate([raw[:, :, h:h + 16], raw[:, :, t:t + 8]], -1))
            out[kind][:, :, w * 32 + elem_ch] = codes
    return out


def decode_c6_image(hi, img, k=None, **reader):
    """-> (hi, lo6, hi6) float64 numpy [n, 90, C]: the f16 values and the two pieces' grid values (unscaled: the image stands
    for  hi + lo6 2^(k - 11)  and carries  hi6 2^k  as its value piece; k is not needed to decode)."""
    h = _as_numpy(hi).astype(np.float64)
    codes = image_codes(img, h.shape[-1], **reader)
    return h, BF6_TABLE[codes[0]], BF6_TABLE[codes[1]]


def image_values(hi, img, k, k_val=None, **reader):
    """The operand triple of a c6 image as the values the products use: (hi, lo6 2^(k - 11), hi6 2^k), float64 numpy.
    (k_val: another exponent for the value piece -- a faulty reader.)"""
    h, lo6, hi6 = decode_c6_image(hi, img, **reader)
    return h, lo6 * 2.0 ** (k - LO_SHIFT), hi6 * 2.0 ** (k if k_val is None else k_val)


def c8_image_values(hi, img):
    """The same for a c8 image (uint8 [n, 90, 2 C]: e4m3((x - hi) 2^11) for the C channels, then e4m3(x))."""
    import torch
    h = _as_numpy(hi).astype(np.float64)
    C = h.shape[-1]
    f8 = torch.from_numpy(_as_numpy(img).view(np.uint8).copy()).view(torch.float8_e4m3fn).double().numpy()
    return h, f8[..., :C] * 2.0 ** -LO_SHIFT, f8[..., C:]


# ---- the packed filter (numpy) ------------------------------------------------------------------------------------------------
def _pack_regions(packed, C):
    kk_n, ct_n, nb = C // 16, C // 32, C // 64
    main_u4 = (9 * kk_n + 3) * ct_n * 64
    c_u4 = (9 * nb + 1) * 2 * ct_n * 2 * 64
    raw = np.ascontiguousarray(_as_numpy(packed)).view(np.uint8).reshape(-1)
    assert raw.size == (main_u4 + c_u4 + 1) * 16 + 2 * C, raw.size
    main = raw[:main_u4 * 16].view(np.float16).astype(np.float64).reshape(9 * kk_n + 3, ct_n, 64, 8)
    assert not main[9 * kk_n:].any()                             # the prefetch padding
    w_hi = np.zeros((C, C, 9))
    lane = np.arange(64)
    for tap in range(9):
        for kk in range(kk_n):
            for ct in range(ct_n):
                o = ct * 32 + (lane & 31)
                c = kk * 16 + (lane >> 5) * 8
                for j in range(8):
                    w_hi[o, c + j, tap] = main[tap * kk_n + kk, ct, :, j]
    corr = raw[main_u4 * 16:(main_u4 + c_u4) * 16]
    ints = raw[(main_u4 + c_u4) * 16:(main_u4 + c_u4 + 1) * 16].view(np.int32)
    rows = raw[(main_u4 + c_u4 + 1) * 16:].view(np.int8).astype(np.int64)
    return w_hi, corr, ints, rows[:C], rows[C:]


def decode_c6_pack(packed, C):
    """The operands a c6 kernel reads from cz_conv3x3_c6_pack_weights' bytes: dict with  w_hi [o, c, 9]  (the f16 fragments),
    w6 / l6 [o, c, 9]  (the bf6 grid values of w 2^sh[o] and (w - f16(w)) 2^sl[o], unscaled),  sh / sl [o]  (the per-row
    shifts),  x_exp, y_exp.  All float64 / int64 numpy.  (Layout: tests/test_c6_pack_cpu.py asserts it against the tensor.)"""
    ct_n, nb = C // 32, C // 64
    w_hi, corr, ints, sh, sl = _pack_regions(packed, C)
    g = corr.reshape(9 * nb + 1, 2, ct_n, 2048)
    assert not g[9 * nb].any() and not g[..., 1536:].any()      # the appended zero block; tails sit densely behind the heads
    pieces = np.concatenate([g[..., :1024].reshape(9 * nb + 1, 2, ct_n, 64, 16),
                             g[..., 1024:1536].reshape(9 * nb + 1, 2, ct_n, 64, 8)], -1)
    vals = BF6_TABLE[unpack_pieces(pieces)]                       # [tap * nb + b, q, ct, lane, e]
    out = np.zeros((2, C, C, 9))
    lane = np.arange(64)
    for tap in range(9):
        for b in range(nb):
            for ct in range(ct_n):
                o = ct * 32 + (lane & 31)
                c0 = b * 64 + (lane >> 5) * 32
                for e in range(32):
                    out[:, o, c0 + ELEM_CH[e], tap] = vals[tap * nb + b, :, ct, :, e]
    return {"w_hi": w_hi, "w6": out[0], "l6": out[1], "sh": sh, "sl": sl, "x_exp": int(ints[2]), "y_exp": int(ints[3])}


def decode_c8_pack(packed, C):
    """The same for cz_conv3x3_c8_pack_weights' bytes (e4m3 fragments; tests/test_c8_pack_cpu.py asserts this layout)."""
    import torch
    ct_n, nb = C // 32, C // 64
    w_hi, corr, ints, sh, sl = _pack_regions(packed, C)
    f8 = torch.from_numpy(corr.copy()).view(torch.float8_e4m3fn).double().numpy().reshape(9 * nb + 1, 2, ct_n, 2, 64, 16)
    out = np.zeros((2, C, C, 9))
    lane = np.arange(64)
    for tap in range(9):
        for b in range(nb):
            for ct in range(ct_n):
                o = ct * 32 + (lane & 31)
                c0 = b * 64 + (lane >> 5) * 32
                for j in range(32):
                    out[:, o, c0 + j, tap] = f8[tap * nb + b, :, ct, j // 16, :, j % 16]
    return {"w_hi": w_hi, "w6": out[0], "l6": out[1], "sh": sh, "sl": sl, "x_exp": 0, "y_exp": 0}


def filter_values(dec):
    """(w_hi, W, L) [o, c, 9] float64: the VALUES the products use -- the correction operands with their row shifts applied."""
    return dec["w_hi"], dec["w6"] * 2.0 ** -dec["sh"][:, None, None], dec["l6"] * 2.0 ** -dec["sl"][:, None, None]


# ---- the arithmetic (numpy or torch float64) ----------------------------------------------------------------------------------
def _zeros(like, shape):
    return np.zeros(shape) if _is_np(like) else like.new_zeros(shape)


def _taps(x):
    """The nine [n * 90, C] views of x [n, 90, C] a 3 x 3 'same' convolution reads, tap = 3 ky + kx (zero outside the board)."""
    n, c = x.shape[0], x.shape[-1]
    xp = _zeros(x, (n, 12, 11, c))
    xp[:, 1:11, 1:10, :] = x.reshape(n, 10, 9, c)
    return [xp[:, ky:ky + 10, kx:kx + 9, :].reshape(n * 90, c) for ky in range(3) for kx in range(3)]


def conv(x, w):
    """Plain float64 'same' convolution, x [n, 90, C], w [o, c, 9] -> [n, 90, o]."""
    y = None
    for tap, xt in enumerate(_taps(x)):
        t = xt @ w[:, :, tap].T
        y = t if y is None else y + t
    return y.reshape(x.shape[0], 90, w.shape[0])


def kloop_steps(C):
    """The K loop's steps in order: (tap, operand (0 = f16 main, 1 = W lo, 2 = L value), first channel, channels)."""
    return [(tap, op, b0 + c0, m) for tap in range(9) for b0 in range(0, C, 64)
            for op, c0, m in ((0, 0, 16), (0, 16, 16), (1, 0, 64), (0, 32, 16), (0, 48, 16), (2, 0, 64))]


def corr_conv(xv, wv, start):
    """The value of a c6 / c8 convolution on the operand VALUES xv = (hi, lo, val) [n, 90, C] and wv = (w_hi, W, L) [o, c, 9]:
        y = start + sum (w_hi hi + W lo + L val),
    start [n, 90, o] (or [o]) = what the accumulators begin with, and ACC, the bound on the fp32 accumulation of the K loop's
    steps in their order (module docstring).  -> (y, ACC), both [n, 90, o]."""
    n, C, O = xv[0].shape[0], xv[0].shape[-1], wv[0].shape[0]
    xt = [_taps(v) for v in xv]
    y = (_zeros(xv[0], (n, 90, O)) + start).reshape(n * 90, O)
    q = _zeros(xv[0], (n * 90, O))
    for tap, op, c0, m in kloop_steps(C):
        a, w = xt[op][tap][:, c0:c0 + m], wv[op][:, c0:c0 + m, tap].T
        s = abs(y) + abs(a) @ abs(w)                             # bound on |partial sum| inside this step
        q = q + m / 3.0 * s * s
        y = y + a @ w
    return y.reshape(n, 90, O), (LAMBDA * U * q ** 0.5).reshape(n, 90, O)


def c6_conv(xv, wv, bias, skip=None):
    """One convolution as a kernel runs it: accumulators starting at fp32(bias + skip) -> (y, bound), before any ReLU."""
    start = bias if skip is None else to_f32(bias + skip)
    y, acc = corr_conv(xv, wv, start)
    return y, acc + 2 * U * abs(start)


def image_interval(pre, bound, k):
    """The operands of the image (exponent k) a kernel writes for relu(pre') with |pre' - pre| <= bound (pre: the value before
    the ReLU -- an element below -bound is zero in the kernel too): the model's operand values for fp32(relu(pre)) and
    D = (D_hi, D_lo, D_val), how far the kernel's may lie from them (module docstring)."""
    mid = encode_values(to_f32(relu(pre)), k)
    t_hi = to_f32(relu(pre + bound))
    up, dn = encode_values(t_hi, k), encode_values(to_f32(relu(pre - bound)), k)
    d = [_max(abs(up[i] - mid[i]), abs(dn[i] - mid[i])) for i in range(3)]
    d[1] = _where(d[0] == 0, d[1], f16_ulp(t_hi) + bound)        # (hi moved: the lo piece jumps by up to an f16 ulp)
    return mid, d


def c6_block(xv, skip, wv1, b1, wv2, b2, k_mid, exact_mid=False, dx=None):
    """relu(conv2(image_k_mid(relu(conv1(x) + b1))) + b2 + skip) on the operand values xv (the block's input image), skip =
    the value that image stands for, wv1 / wv2 the filters' values -> dict: y (the block's fp32 output, ReLU'd, float64),
    bound (per element, module docstring), t (the intermediate activation), a1 (its bound), mid (its operand values).
    exact_mid: the first convolution is known to be exact (an identity filter on a representable sum): a1 = 0.
    dx = (D_hi, D_lo, D_val): the kernel's input operands may lie that far from xv (the image a block before wrote, from
    image_interval): carried through |filter 1| into a1 and, as D_hi + D_lo, through the skip connection."""
    m1, a1 = c6_conv(xv, wv1, b1)
    a1 = a1 * 0.0 if exact_mid else a1 + U * abs(m1)
    if dx is not None:
        a1 = a1 + conv(dx[0], abs(wv1[0])) + conv(dx[1], abs(wv1[1])) + conv(dx[2], abs(wv1[2]))
    mid, d = image_interval(m1, a1, k_mid)
    m2, bound = c6_conv(mid, wv2, b2, skip)
    if not exact_mid or dx is not None:
        bound = bound + conv(d[0], abs(wv2[0])) + conv(d[1], abs(wv2[1])) + conv(d[2], abs(wv2[2]))
    if dx is not None:
        bound = bound + dx[0] + dx[1]
    return {"y": relu(m2), "pre": m2, "bound": bound, "t": to_f32(relu(m1)), "a1": a1, "mid": mid}


def heads(y, y_bound, head_w, head_b):
    """relu(1 x 1 head convolution) of a block's output y [n, 90, C] with head_w [6, C], head_b [6] -> (features [n, 90, 6],
    bound): the block's bound through |head_w| plus the head's own fp32 sum -- C products and additions in some order, at most
    (C + 1) u sum |terms| (the deterministic bound: the order differs between the entry points)."""
    f = y @ head_w.T + head_b
    mag = abs(y) @ abs(head_w).T + abs(head_b)
    return relu(f), y_bound @ abs(head_w).T + (y.shape[-1] + 1) * U * mag


def value_piece_check(pair_value, hi6, k):
    """An image's value piece hi6 (grid values, numpy) against bf6(pair_value 2^-k), pair_value = hi + lo6 2^(k - 11) of the same
    image: the kernel converts its fp32 value, which the pair stands for to half a step of the lo piece (2^-14 relative, 2^(k - 16)
    absolute for small values), so the two agree except where the argument lies that close to a bf6 tie.  -> (fraction of
    elements near a tie, fraction that differ, number that differ away from a tie)."""
    arg = pair_value * 2.0 ** -k
    want = bf6_round(arg)
    nudge = np.maximum(arg * 2.0 ** -13, 2.0 ** -15)
    near = (bf6_round(arg + nudge) != want) | (bf6_round(arg - nudge) != want)
    differ = hi6 != want
    return float(near.mean()), float(differ.mean()), int((differ & ~near).sum())


def ratio(got, want, bound):
    """max over the elements of |got - want| / bound (an element whose terms are all zero has bound 0 and must be exact)."""
    return float((abs(got - want) / (bound + 1e-300)).max())


# ---- the inputs of the element tests (numpy; tests/test_c6_model_cpu.py and tests/test_gpu_c6_elements.py) -----------------------
K_X, K_MID, K_OUT = -3, 0, 4    # image exponents: all different, one negative; the intermediate one low enough that the large
                                # rows saturate both pieces of some elements


def planted(k):
    """fp32 values an image of exponent k gets wrong if anything is: 0; an f16 value plus a lo part in bf6's subnormals (lo
    2^(11 - k) = 1/8 and 3/16); just below, just above and well above the saturation point 28 2^k; an exact tie of the value
    piece (26 2^k: 24 | 28); an exact f16 tie (2049 / 2048: down to 1, lo = +2^-11 ...) and the fp32 number behind it (up,
    lo negative); a lo part that saturates its piece (f16 ties far above the image's range)."""
    s = 2.0 ** k
    v = [0.0, s * (1.0 + 2.0 ** -14), s * (0.5 + 3.0 * 2.0 ** -15), 27.9 * s, 28.0 * s, 30.0 * s, 41.9 * s, 26.0 * s,
         s * 2049.0 / 2048.0, s * (2049.0 / 2048.0 + 2.0 ** -22), 1.5 * s, s / 64.0, s * 2.0 ** -9, 2049.0 / 32.0 * s]
    return np.array(v, np.float32)


def activations(n, C, k, rng, also=(K_MID,)):
    """[n, 90, C] fp32 >= 0: half-normal values with a third of the image's range as their ~4 sigma point, a quarter of them
    exact zeros (what a ReLU leaves), and planted(k) at a few places of every board (another pixel and channel per board, so
    that every lane position and both halves of a piece meet one) -- and planted() of the exponents `also`: an identity first
    filter hands the image's value to the intermediate image, which then meets its own edge cases."""
    x = np.abs(rng.standard_normal((n, 90, C))) * (28.0 * 2.0 ** k / 12.0)
    x = np.where(rng.random((n, 90, C)) < 0.25, 0.0, x).astype(np.float32)
    p = np.concatenate([planted(k)] + [planted(a) for a in also])
    for b in range(n):
        for j, v in enumerate(p):
            x[b, (7 * b + 13 * j) % 90, (b * 5 + 37 * j) % C] = v
    return x


def filters(C, rng, identity=False, zero=False):
    """([o, c, 3, 3] fp32, bias [o] fp32): a usual-scale random filter whose output rows are scaled by 0.004 (every third) and by
    50 (every seventh from 1), the bias alike, as in the c8 test: rows of very different magnitude carry different shifts.
    identity: the centre-tap identity with zero bias; zero: all zero."""
    if identity or zero:
        w = np.zeros((C, C, 3, 3), np.float32)
        if identity:
            w[np.arange(C), np.arange(C), 1, 1] = 1.0
        return w, np.zeros(C, np.float32)
    w = rng.standard_normal((C, C, 3, 3)) / (3.0 * C ** 0.5)
    b = rng.standard_normal(C) * 0.5
    w[::3] *= 0.004
    b[::3] *= 0.004
    w[1::7] *= 50.0
    b[1::7] *= 50.0
    return w.astype(np.float32), b.astype(np.float32)
