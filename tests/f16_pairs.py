"""Float64 model of the fp16-pair ("f16x3") tower arithmetic and the per-element bounds its kernels are held to
(tests/test_gpu_f16x3.py; the bounds themselves are tested on faulty arithmetic in tests/test_f16x3_bounds_cpu.py), of the
same convolutions on bf16 pairs ("bf16x3") and on plain fp16 / bf16 operands (the part BF16 PAIRS AND PLAIN OPERANDS below;
tests/test_gpu_plain_bf16x3.py, tests/test_pair_bounds_cpu.py), and, in the last part of this docstring, of the heads' dense
tail on fp16 or bf16 pairs (tests/test_gpu_heads.py, tests/test_dense_bounds_cpu.py).

The arithmetic.  An fp32 operand v is stored as hi = fp16(v), lo = fp16(v - hi), both rounded to nearest even, and a
product is formed as  w_hi x_hi + w_lo x_hi + w_hi x_lo  (w_lo x_lo is dropped), accumulated in fp32.

Operand format.  e(v) = |v - hi - lo| <= 2^-22 |v| + 2^-25: hi keeps 11 bits, so |v - hi| <= 2^-11 |v|, and lo rounds
that remainder to 11 more bits (2^-22 |v|) while it is a normal fp16 (>= 2^-14); below 2^-14 lo is an fp16 subnormal,
whose step is 2^-24 (absolute error 2^-25).  A value below 2^-14 has a subnormal hi and is off by the same 2^-25.
The lo part of a typical filter tap (|w| ~ 1/(3 sqrt C) ~ 0.02, |lo| ~ 1e-5) is such a subnormal, and so is the lo part
of every activation below ~1/8: a matrix unit that flushed fp16 subnormals would silently fall back to fp16 precision.

The bounds, per output element y of a convolution with bias b and optional (hi, lo) skip s:

(a) against float64 arithmetic on THE SAME operands, y_a = sum_k (w_hi x_hi + w_lo x_hi + w_hi x_lo) + b + s_hi + s_lo:
    * fp32 accumulation.  The kernels' K loop runs K-steps of 16 input channels of one tap, tap-major, the three terms
      of a step one matrix instruction each.  A partial sum inside step s is P_(s-1) (the exact sum over the earlier
      steps) plus some of step s's 48 terms: |S| <= |P_(s-1)| + A_s, A_s = the sum of |term| over step s.  Every rounding
      of the accumulator is at most u |S| (u = 2^-24).  Counting one rounding per product (N_s = 48; an instruction
      that adds its 16 products before it rounds does fewer) and taking the rounding errors as independent and
      zero-mean (variance <= (u S)^2 / 3), the accumulation error stays below
          ACC = 8 u sqrt(sum_s N_s / 3 (|P_(s-1)| + A_s)^2),
      8 standard deviations of that upper model (< 1e-14 per element).  The deterministic worst case, u sum_s N_s
      (|P_(s-1)| + A_s), is about 10x larger on O(1) data and would not tell a flushed lo part from rounding.
    * epilogue: three fp32 additions (bias, skip hi, skip lo), each <= u of its result: EPI = 2^-22 (|y_conv| + |b| + |s|).
    * pair output: hi + lo stands for the fp32 result to e(y) = 2^-22 |y| + 2^-25 (nothing for fp32 output).
    bound_a = ACC + EPI (+ e(y)).
(b) against float64 arithmetic on THE EXACT fp32 operands, y_b = sum_k w x + b + s:
    w x - (three terms) = w_lo x_lo + dw x + (w_hi + w_lo) dx  with |dw| <= e(w), |dx| <= e(x), so
    bound_b = bound_a + sum_k (|w_lo x_lo| + e(w) |x| + |w_hi + w_lo| e(x)) + e(s).

Everything here works on numpy float64 arrays and on torch float64 tensors alike (only slicing, matmul, abs and
arithmetic), so the CPU test feeds the check the very function the GPU tests use.  Activations are channels-last
[n, 90, C] (the kernels' layout), filters [C_out, C_in, K, K].

BF16 PAIRS AND PLAIN OPERANDS (pair_conv / ConvCheck with fmt=BF16_PAIR, or plain=True).  The kernel is the same K loop
(csrc/xq_conv_kloop.h conv_kloop) for every operand type: tap-major, K-steps of 16 input channels, three matrix instructions per
step for pairs (w_hi x_hi, w_lo x_hi, w_hi x_lo) and ONE for plain operands, fp32 accumulation.

bf16 pairs ("bf16x3").  The arithmetic and both bounds are those above with the pair format e(v) = 2^-16 |v| + 2^-134 (BF16_PAIR;
derived in the dense-layer part below) wherever e() enters: the output pair's e(y) in (a), and e(w), e(x), e(s) in (b).  An
operand that is exactly 0 splits into (0, 0) and carries e = 0 (taken for bf16 pairs only, as DenseCheck does, so that the fp16
bounds stay what they were).  Feature planes (0 / 1) are exact in either format: x_exact=True sets e(x) = 0.  A product of two
bf16 values has at most 16 significant bits and an exponent inside fp32's range: exact in fp32, as a product of two fp16 values
is (at most 22 bits, down to 2^-48).

Plain operands (parts = 1, fp16 or bf16).  The kernel is handed the 2-byte values themselves, so only bound (a) applies:
against float64 on the same operands, y_a = sum_k w_T x_T + b + s.
    * accumulation: the model above with one term per step, N_s = min(16, C_in - 16 s) roundings, A_s = sum over the step of
      |w_T x_T|:  ACC = LAMBDA U sqrt(sum_s N_s / 3 (|P_(s-1)| + A_s)^2).
    * epilogue: the kernel adds the bias and then the one skip part in fp32 (k_conv3x3's epilogue: v = acc + b; v += s), one
      rounding of at most U |result| <= U (|y_conv| + |b| + |s|) per addition: EPI = n_add U (|y_conv| + |b| + |s|), n_add = 2
      with a skip and 1 without one (the input convolution: bias only).
    * fp32 output: bound_a = ACC + EPI.  A 2-byte output is the nearest-even cast of that fp32 value v (the GPU tests compare it
      bit for bit with the cast of the fp32 output of the same launch).  Where a kernel has no fp32 output (cz_input_conv) the
      2-byte result g = cast(v) is held to the float64 value directly: |g - v| <= ulp(g) / 2, with ulp(g) = 2^(max(e, e_min) - p + 1),
      2^e <= |g| < 2^(e + 1), p = 11 and e_min = -14 for fp16, p = 8 and e_min = -126 for bf16 (a result that rounds up to a power of
      two is off by half the spacing BELOW it, which is smaller): bound_a = ACC + EPI + ulp(g) / 2 (half_ulp below).  A store that
      truncated would be off by up to ulp(g), twice the dominant term.
ReLU is 1-Lipschitz and maps the reference the same way, so it adds nothing to either bound.

THE DENSE TAIL OF THE HEADS (csrc/xq_heads.hip: k_fc_tile, k_policy_normalize; pair_dense, DenseCheck, stat_rel,
softmax_check, value_check below).

Dense layers on (hi, lo) pairs.  y = sum_k (w_hi x_hi + w_lo x_hi + w_hi x_lo) + b over K-steps of 16 features in index
order, the three terms of a step one matrix instruction each (in that order), fp32 accumulation, one fp32 addition for the
bias.  Features [n, F], weights [n_out, F].

Pair formats.  fp16: e(v) as derived above (F16_PAIR).  bf16 (BF16_PAIR): bf16 keeps 8 significant bits, so
hi = bf16(v) is off by at most half a unit of the 8th bit, |v - hi| <= 2^-8 |v|; the remainder v - hi is exact in fp32 (it has
at most 16 significant bits) and lo = bf16(v - hi) rounds it to 8 more bits: |v - hi - lo| <= 2^-8 |v - hi| <= 2^-16 |v|.  bf16
has fp32's exponent range, so lo is a normal number down to 2^-126; below that its step is 2^-133 (absolute error 2^-134):
e(v) = 2^-16 |v| + 2^-134.  The dropped term is |w_lo x_lo| <= 2^-16 |w x|.  A value that is exactly 0 has e = 0 in either format
(DenseCheck uses that: the features are zero after a ReLU half of the time).

Logits, per element (DenseCheck):
(a) same operands:  ACC + U (|y| + |b|),  ACC = LAMBDA U sqrt(sum_s N_s / 3 (|P_(s-1)| + A_s)^2), N_s = 3 min(16, F - 16 s)
    (the accumulation model of the convolution's bound (a)), and the bias addition is one rounding of at most U |y + b|.
(b) exact fp32 operands:  (a) + sum_k (|w_lo x_lo| + e(w) |x| + |w_hi + w_lo| e(x)).

Value output  v = tanh(d), d = sum_j relu(y_j + b1_j) w2_j + b2  (value_check).  ReLU is 1-Lipschitz, so a hidden unit is off by
at most its logit bound B_j.  The kernel's fp32 dot (the library is built with -ffp-contract=off: a product and an addition
round separately): a lane adds its T = 32 ceil(tiles / 8) hidden units (tiles = ceil(n_hidden / 32); 2 tiles x 16 accumulator
rows per pass over the label tiles) one after the other, 2 T roundings; one shuffle addition joins the half-waves; the four
waves' sums are added to 0 in turn (the first addition is exact: 3 roundings).  Every one of these roundings is at most U times
a partial sum of |h_j w2_j| over a subset of the units, and a term passes through at most n = 2 T + 4 of them, so their sum
is at most gamma_n A with A = sum_j (|h_j| + B_j) |w2_j|, gamma_n = n U / (1 - n U).  The bias: U (|d - b2| + |b2|), one rounding of
the sum; b2 itself must be the fp32 value the kernel is handed (value_check refuses any other: a double such as 0.13 would
add its own conversion error, up to U |b2|, which this bound does not carry).
    |delta d| <= sum_j B_j |w2_j| + gamma_n A + U (|d - b2| + |b2|);  tanh is 1-Lipschitz;  + TANH_REL |v| for tanhf.

Softmax output  p_j = exp(l_j) / sum_k exp(l_k)  (softmax_check).  With logits off by delta_k, |delta_k| <= B_k, the exact
softmax of the kernel's logits is p_j exp(delta_j) sum_k exp(l_k) / sum_k exp(l_k + delta_k), a factor within
exp(+-(B_j + max_k B_k)) of p_j.  The kernel's own arithmetic on its logits adds the relative error STAT.  A quotient below
the smallest normal float 2^-126 keeps no relative accuracy, so the bound is
    |delta p_j| <= (expm1(B_j + max_k B_k) + STAT) p_j + 2^-126.

STAT, by counting roundings (first order in U; the products of two such terms are below 1e-9 of p).  fexp(x) =
v_exp_f32(x log2e): the fp32 constant and the product are each off by U relative, moving the exponent by 2 U |x| log2e, the
result by 2 U |x| relative; x itself is a rounded difference, U |x| more; the instruction adds EXP2_REL: 3 U |x| + EXP2_REL.
A lane walks G = 8 ceil(tiles / 8) groups of four labels (tiles = ceil(n_labels / 32)).  In each it rescales its sum
(one fexp, one product: EXP2_REL + U + 3 U Delta, Delta the rise of the running maximum) and adds four terms (4 U, all terms
positive).  The half-waves are joined by a rescaling and an addition (EXP2_REL + 2 U + 3 U Delta), the four waves by a rescaling
and four additions (EXP2_REL + 5 U + 3 U Delta).  The term of label k therefore carries at most
(G + 2) EXP2_REL + (5 G + 11) U + 3 U t_k, where t_k = max - l_k is what its own argument and all later rises add up to.
Weighted by p_k the last part is 3 U sum_k p_k t_k <= 3 U ln(n_labels) (sum_k p_k t_k = H(p) - ln(sum) <= the entropy).
k_policy_normalize: t_j = fl(l_j - max) moves exp by U t_j, and t_j <= 126 ln 2 < 88 where p_j >= 2^-126; expf adds EXPF_REL;
the division is correctly rounded (measured: 1.000 U): U.
    STAT = (G + 2) EXP2_REL + (5 G + 11 + 3 ln n_labels) U + 88 U + EXPF_REL + U.
For 2086 labels G = 72 and STAT = 708 U = 4.2e-5.

Library terms, MEASURED (the ROCm installation carries no accuracy statement for them): on an MI355X on 2026-10-17, fp32
results of the device library's exp, exp2 (the v_exp_f32 instruction plus a scaling for denormal results) and tanh, called
through PyTorch's elementwise kernels, against float64 of the same fp32 arguments, 2^25 arguments each (uniform random and an
even grid): exp on [-87, 0] 1.411 U relative, exp2 on [-125, 0] 1.393 U, tanh on [-20, 20] 2.486 U relative (|x| > 2^-12;
1.067 U on [2^-42, 0.25]).  Each constant is twice the measured maximum, rounded up.
tests/test_gpu_heads.py::test_library_terms_through_the_kernels holds the kernels' own tanhf / expf / fexp calls to these
constants on exact arguments (measured there: 0.42 and 0.47 of the constants)."""
import itertools

import numpy as np

U = 2.0 ** -24                  # fp32 unit roundoff
PAIR_REL = 2.0 ** -22           # e(v) = PAIR_REL |v| + PAIR_ABS for an fp16 (hi, lo) pair
PAIR_ABS = 2.0 ** -25
EPI_REL = 2.0 ** -22
LAMBDA = 8.0
CAP = 3.0e4                     # the guard's f16x3 admission cap on |activation| (agent/model.py guard_search)


F16_PAIR = (PAIR_REL, PAIR_ABS)                 # (relative, absolute) part of e(v), fp16 pairs: derived above
BF16_PAIR = (2.0 ** -16, 2.0 ** -134)           # bf16 pairs: derived in the module docstring's dense-layer part


def pair_err(v, fmt=F16_PAIR):
    """The format bound e(v) of a (hi, lo) pair of format `fmt` (F16_PAIR, BF16_PAIR) standing for v."""
    return fmt[0] * abs(v) + fmt[1]


def split16(v):
    """(hi, lo) fp16 pair of an fp32 numpy array, both rounded to nearest even (numpy's float16 conversion)."""
    v = np.asarray(v, dtype=np.float32)
    hi = v.astype(np.float16)
    return hi, (v - hi.astype(np.float32)).astype(np.float16)


def _new_zeros(like, shape):
    if isinstance(like, np.ndarray):
        return np.zeros(shape, dtype=like.dtype)
    return like.new_zeros(shape)


def taps(x, w):
    """Per tap (ky, kx) of a 'same' convolution: the [n * 90, C_in] activation rows that tap reads (zero outside the
    board) and the [C_in, C_out] filter slice.  x: [n, 90, C_in] channels-last, w: [C_out, C_in, K, K]."""
    n, c_in = x.shape[0], x.shape[-1]
    k = w.shape[-1]
    r = k // 2
    xp = _new_zeros(x, (n, 10 + 2 * r, 9 + 2 * r, c_in))
    xp[:, r:r + 10, r:r + 9, :] = x.reshape(n, 10, 9, c_in)
    for ky in range(k):
        for kx in range(k):
            yield xp[:, ky:ky + 10, kx:kx + 9, :].reshape(n * 90, c_in), w[:, :, ky, kx].T


def conv(x, w):
    """Float64 'same' convolution (cross-correlation, as Conv2D computes it) in the channels-last layout."""
    n = x.shape[0]
    y = None
    for xt, wt in taps(x, w):
        y = xt @ wt if y is None else y + xt @ wt
    return y.reshape(n, 90, w.shape[0])


def pair_conv(x_hi, x_lo, w_hi, w_lo, plain=False):
    """sum_k (w_hi x_hi + w_lo x_hi + w_hi x_lo) in float64 (products of fp16 values are exact, the sums good to 2^-50),
    and the accumulation bound ACC of the module docstring for it, K-step by K-step (16 input channels of one tap).
    plain=True: one term per step, sum_k w_hi x_hi (x_lo, w_lo unused), and a third of the roundings."""
    n, c_in, c_out = x_hi.shape[0], x_hi.shape[-1], w_hi.shape[0]
    y = q = None
    lo_taps = itertools.repeat((None, None)) if plain else taps(x_lo, w_lo)
    for (xh, wh), (xl, wl) in zip(taps(x_hi, w_hi), lo_taps):
        for c0 in range(0, c_in, 16):
            k = slice(c0, c0 + 16)
            if plain:
                c = xh[:, k] @ wh[k]
                a = abs(xh[:, k]) @ abs(wh[k])
            else:
                c = xh[:, k] @ wh[k] + xh[:, k] @ wl[k] + xl[:, k] @ wh[k]
                a = abs(xh[:, k]) @ abs(wh[k]) + abs(xh[:, k]) @ abs(wl[k]) + abs(xl[:, k]) @ abs(wh[k])
            s = a if y is None else abs(y) + a              # bound on |partial sum| inside this K-step
            m = (1 if plain else 3) * min(16, c_in - c0)    # roundings in it: one per product
            q = m / 3.0 * s * s if q is None else q + m / 3.0 * s * s
            y = c if y is None else y + c
    return y.reshape(n, 90, c_out), (LAMBDA * U * q ** 0.5).reshape(n, 90, c_out)


def _relu(t):
    return t * (t > 0)


F16_PLAIN = (11, -14)           # (significant bits p, smallest normal exponent e_min) of a plain 2-byte output: half_ulp
BF16_PLAIN = (8, -126)


def _err0(v, fmt):
    """e(v) with e(0) = 0 for bf16 pairs (module docstring, BF16 PAIRS AND PLAIN OPERANDS); fp16 pairs keep e(0) = 2^-25."""
    return pair_err(v, fmt) * (v != 0) if fmt is BF16_PAIR else pair_err(v, fmt)


def half_ulp(g, out_fmt):
    """ulp(g) / 2 of the 2-byte format out_fmt (F16_PLAIN, BF16_PLAIN) at its values g (float64): the most a nearest-even cast
    to g can have moved the value it rounded."""
    p, e_min = out_fmt
    e = (np.frexp(abs(g))[1] if isinstance(g, np.ndarray) else abs(g).frexp()[1].double()) - 1.0     # 2^e <= |g| < 2^(e + 1)
    sub = (e <= e_min) | (g == 0)                                # subnormal or zero: the spacing of the smallest binade
    return 2.0 ** (e * ~sub + e_min * sub - p)


class ConvCheck:
    """The per-element check of a convolution on (hi, lo) pairs of format `fmt` (module docstring), its float64 parts computed
    once for the operands: x_pair = (x_hi, x_lo), w_pair = (w_hi, w_lo) the pairs' values, x / w the fp32 operands they split;
    all float64, numpy arrays or torch tensors on one device.  Activations [n, 90, C_in], filters [C_out, C_in, K, K].
    x_exact: the activations are exact in the format (feature planes), e(x) = 0.
    plain=True: plain 2-byte operands, x_pair = (x_T,), w_pair = (w_T,) and x = w = None: bound (a) only."""

    def __init__(self, x_pair, w_pair, x=None, w=None, fmt=F16_PAIR, plain=False, x_exact=False):
        self.fmt, self.plain = fmt, plain
        if plain:
            self.y3, self.acc = pair_conv(x_pair[0], None, w_pair[0], None, plain=True)
            return
        (xh, xl), (wh, wl) = x_pair, w_pair
        self.y3, self.acc = pair_conv(xh, xl, wh, wl)
        self.exact = conv(x, w)
        self.rep = conv(abs(xl), abs(wl)) + conv(abs(x), _err0(w, fmt))
        if not x_exact:
            self.rep = self.rep + conv(_err0(x, fmt), abs(wh + wl))

    def ratios(self, got, bias, skip=None, relu=False, pair_out=False, out_fmt=None):
        """Worst |error| / bound over the output elements against (a) the same operands and (b) the exact fp32 operands
        (None for plain operands).  got: the kernel's result as float64 (hi + lo of a pair output); bias [C_out];
        skip = (s_hi, s_lo, s), or (s_T,) for plain operands, or None; out_fmt: F16_PLAIN / BF16_PLAIN when got is a plain
        2-byte output (adds half_ulp(got))."""
        ya, mag = self.y3 + bias, abs(self.y3) + abs(bias)
        if self.plain:
            if skip is not None:
                ya, mag = ya + skip[0], mag + abs(skip[0])
            if relu:
                ya = _relu(ya)
            bound_a = self.acc + (1 if skip is None else 2) * U * mag
            if out_fmt is not None:
                bound_a = bound_a + half_ulp(got, out_fmt)
            return float((abs(got - ya) / bound_a).max()), None
        yb, rep = self.exact + bias, self.rep
        if skip is not None:
            sh, sl, s = skip
            ya, yb, mag, rep = ya + sh + sl, yb + s, mag + abs(sh) + abs(sl), rep + _err0(s, self.fmt)
        if relu:
            ya, yb = _relu(ya), _relu(yb)
        bound_a = self.acc + EPI_REL * mag
        if pair_out:
            bound_a = bound_a + pair_err(ya, self.fmt)
        return float((abs(got - ya) / bound_a).max()), float((abs(got - yb) / (bound_a + rep)).max())

    def error(self, got, bias):
        """max |got - (exact conv + bias)|: the arithmetic's own error on fp32 operands (fp32 output, no skip, no ReLU)."""
        return float(abs(got - (self.exact + bias)).max())


def mixed_activations(shape, rng, cap=CAP):
    """fp32 activations [n, 90, C] (>= 0, as the tower's ReLU leaves them) mixed per element over the cases where a pair
    goes wrong: exact zeros, exact fp16 values (lo = 0), values with a subnormal hi (< 2^-14), values with a subnormal lo
    (2^-14 .. 2^-3), O(1) values, and a few large ones up to `cap`.  Board b draws from regime b % 3: 0 = all six kinds,
    1 = no large values, 2 = zeros and subnormal hi / lo only.  An output element sums 9 C inputs of one board: on boards
    1 and 2 the small values' errors are not buried under the rounding of a large neighbour's product."""
    p_all = np.array([[0.1, 0.15, 0.1, 0.25, 0.38, 0.02], [0.1, 0.15, 0.1, 0.25, 0.4, 0.0], [0.2, 0.0, 0.2, 0.6, 0.0, 0.0]])
    kind = np.stack([rng.choice(6, size=shape[1:], p=p_all[b % 3]) for b in range(shape[0])])
    logu = lambda lo, hi: np.exp2(rng.uniform(lo, hi, size=shape))
    v = np.zeros(shape)
    v = np.where(kind == 1, np.abs(rng.standard_normal(shape)).astype(np.float16).astype(np.float64), v)
    v = np.where(kind == 2, logu(-30.0, -14.0), v)
    v = np.where(kind == 3, logu(-14.0, -3.0), v)
    v = np.where(kind == 4, logu(-3.0, 2.0), v)
    v = np.where(kind == 5, logu(2.0, np.log2(cap)), v)
    return v.astype(np.float32)


# ---- the dense tail of the heads (csrc/xq_heads.hip: k_fc_tile, k_policy_normalize) -----------------------------------------
# (derivations: the module docstring's part THE DENSE TAIL OF THE HEADS)
EXPF_REL = 3.0 * U
EXP2_REL = 3.0 * U
TANH_REL = 5.0 * U
P_FLOOR = 2.0 ** -126


def bf16_round(a, nearest=True):
    """The bf16 value of fp32 numbers as a float32 array: rounded to nearest even, or (nearest=False) truncated."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    if nearest:
        u = u + 0x7FFF + ((u >> 16) & 1)
    return (u & 0xFFFF0000).astype(np.uint32).view(np.float32)


def split_pair(v, fmt=F16_PAIR):
    """(hi, lo) of an fp32 numpy array in pair format `fmt`, as float32 arrays, both parts rounded to nearest even."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if fmt is F16_PAIR:
        hi, lo = split16(v)
        return hi.astype(np.float32), lo.astype(np.float32)

    hi = bf16_round(v)
    return hi, bf16_round(v - hi)


def _fn(t, name):
    return getattr(np, name)(t) if isinstance(t, np.ndarray) else getattr(t, name)()


def _rowmax(t):
    return t.max(axis=1, keepdims=True) if isinstance(t, np.ndarray) else t.amax(dim=1, keepdim=True)


def pair_dense(x_hi, x_lo, w_hi, w_lo):
    """sum_k (w_hi x_hi + w_lo x_hi + w_hi x_lo) in float64 for features [n, F] and weights [n_out, F] (the products of the
    2-byte values are exact, the sums good to 2^-50), and the accumulation bound ACC for it, K-step by K-step."""
    f = x_hi.shape[-1]
    y = q = None
    for k0 in range(0, f, 16):
        k = slice(k0, k0 + 16)
        xh, xl, wh, wl = x_hi[:, k], x_lo[:, k], w_hi[:, k].T, w_lo[:, k].T
        c = xh @ wh + xh @ wl + xl @ wh
        a = abs(xh) @ abs(wh) + abs(xh) @ abs(wl) + abs(xl) @ abs(wh)
        s = a if y is None else abs(y) + a
        m = 3 * min(16, f - k0)
        q = m / 3.0 * s * s if q is None else q + m / 3.0 * s * s
        y = c if y is None else y + c
    return y, LAMBDA * U * q ** 0.5


class DenseCheck:
    """The per-element check of a dense layer on (hi, lo) pairs of format `fmt`, its float64 parts computed once for the
    operands: x_pair / w_pair the pairs' values, x / w the fp32 operands they split; all float64, numpy arrays or torch
    tensors on one device.  Features [n, F], weights [n_out, F]."""

    def __init__(self, x_pair, w_pair, x, w, fmt=F16_PAIR):
        (xh, xl), (wh, wl) = x_pair, w_pair
        self.y3, self.acc = pair_dense(xh, xl, wh, wl)
        self.exact = x @ w.T
        ex, ew = pair_err(x, fmt) * (x != 0), pair_err(w, fmt) * (w != 0)
        self.rep = abs(xl) @ abs(wl).T + abs(x) @ ew.T + ex @ abs(wh + wl).T

    def bounds(self, bias):
        """(y_a, bound_a, y_b, bound_b): the logits y + bias on the same / the exact operands and their bounds."""
        ba = self.acc + U * (abs(self.y3) + abs(bias))
        return self.y3 + bias, ba, self.exact + bias, ba + self.rep

    def ratios(self, got, bias):
        """Worst |error| / bound over the elements against (a) and (b); got: the kernel's logits as float64."""
        ya, ba, yb, bb = self.bounds(bias)
        return float((abs(got - ya) / ba).max()), float((abs(got - yb) / bb).max())


def stat_rel(n_labels):
    """STAT of the module docstring (dense tail, softmax output) for a softmax over n_labels."""
    g = 8 * -(-(-(-n_labels // 32)) // 8)
    return (g + 2) * EXP2_REL + (5 * g + 11 + 3 * float(np.log(n_labels))) * U + 88 * U + EXPF_REL + U


def softmax_check(logits, bound):
    """(p, bound_p): the float64 softmax of the reference logits [n, n_labels] and the bound on the kernel's probabilities,
    given the per-element bound on its logits."""
    e = _fn(logits - _rowmax(logits), "exp")
    p = e / e.sum(1)[:, None]
    return p, (_fn(bound + _rowmax(bound), "expm1") + stat_rel(logits.shape[1])) * p + P_FLOOR


def value_check(hidden, bound, w2, b2):
    """(v, bound_v, d): the float64 value tanh(relu(hidden) . w2 + b2) of the reference pre-activations hidden [n, n_hidden]
    (bias included), the bound on the kernel's value given the per-element bound on its pre-activations, and d.  b2: a Python
    float that fp32 holds exactly."""
    assert float(np.float32(b2)) == b2, "b2 must be exact in fp32: the kernel takes it as a float"
    h = hidden * (hidden > 0)
    t = 32 * -(-(-(-hidden.shape[1] // 32)) // 8)
    n = 2 * t + 4
    d0 = h @ w2
    v = _fn(d0 + b2, "tanh")
    bd = bound @ abs(w2) + n * U / (1.0 - n * U) * ((h + bound) @ abs(w2)) + U * (abs(d0) + abs(b2))
    return v, bd + TANH_REL * abs(v), d0 + b2


def dense_features(kind, n, f, rng):
    """The fp32 head features [n, f] of the dense tests: "O(1)" = relu(randn) 1.5, or "mixed" = mixed_activations over
    [n, 90, f / 90] (row r draws from regime r % 3; at most CAP) with rows 5, 12, 19, ... all zero."""
    if kind == "mixed":
        x = mixed_activations((n, 90, f // 90), rng, cap=CAP).reshape(n, f)
        x[5::7] = 0.0
        return x
    return (np.maximum(rng.standard_normal((n, f)), 0.0) * 1.5).astype(np.float32)
