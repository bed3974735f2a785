"""Float64 model of the fp16-pair ("f16x3") tower arithmetic and the per-element bounds its kernels are held to
(tests/test_gpu_f16x3.py; the bounds themselves are tested on faulty arithmetic in tests/test_f16x3_bounds_cpu.py).

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
[n, 90, C] (the kernels' layout), filters [C_out, C_in, K, K]."""
import numpy as np

U = 2.0 ** -24                  # fp32 unit roundoff
PAIR_REL = 2.0 ** -22           # e(v) = PAIR_REL |v| + PAIR_ABS for an fp16 (hi, lo) pair
PAIR_ABS = 2.0 ** -25
EPI_REL = 2.0 ** -22
LAMBDA = 8.0
CAP = 3.0e4                     # the guard's f16x3 admission cap on |activation| (agent/model.py guard_search)


def pair_err(v):
    """The format bound e(v) of an fp16 (hi, lo) pair standing for v."""
    return PAIR_REL * abs(v) + PAIR_ABS


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


def pair_conv(x_hi, x_lo, w_hi, w_lo):
    """sum_k (w_hi x_hi + w_lo x_hi + w_hi x_lo) in float64 (products of fp16 values are exact, the sums good to 2^-50),
    and the accumulation bound ACC of the module docstring for it, K-step by K-step (16 input channels of one tap)."""
    n, c_in, c_out = x_hi.shape[0], x_hi.shape[-1], w_hi.shape[0]
    y = q = None
    for (xh, wh), (xl, wl) in zip(taps(x_hi, w_hi), taps(x_lo, w_lo)):
        for c0 in range(0, c_in, 16):
            k = slice(c0, c0 + 16)
            c = xh[:, k] @ wh[k] + xh[:, k] @ wl[k] + xl[:, k] @ wh[k]
            a = abs(xh[:, k]) @ abs(wh[k]) + abs(xh[:, k]) @ abs(wl[k]) + abs(xl[:, k]) @ abs(wh[k])
            s = a if y is None else abs(y) + a              # bound on |partial sum| inside this K-step
            m = 3 * min(16, c_in - c0)                      # roundings in it: one per product
            q = m / 3.0 * s * s if q is None else q + m / 3.0 * s * s
            y = c if y is None else y + c
    return y.reshape(n, 90, c_out), (LAMBDA * U * q ** 0.5).reshape(n, 90, c_out)


def _relu(t):
    return t * (t > 0)


class ConvCheck:
    """The per-element check of a convolution on fp16 pairs (module docstring), its float64 parts computed once for the
    operands: x_pair = (x_hi, x_lo), w_pair = (w_hi, w_lo) the pairs' values, x / w the fp32 operands they split; all
    float64, numpy arrays or torch tensors on one device.  Activations [n, 90, C_in], filters [C_out, C_in, K, K]."""

    def __init__(self, x_pair, w_pair, x, w):
        (xh, xl), (wh, wl) = x_pair, w_pair
        self.y3, self.acc = pair_conv(xh, xl, wh, wl)
        self.exact = conv(x, w)
        self.rep = conv(abs(xl), abs(wl)) + conv(abs(x), pair_err(w)) + conv(pair_err(x), abs(wh + wl))

    def ratios(self, got, bias, skip=None, relu=False, pair_out=False):
        """Worst |error| / bound over the output elements against (a) the same operands and (b) the exact fp32 operands.
        got: the kernel's result as float64 (hi + lo of a pair output); bias [C_out]; skip = (s_hi, s_lo, s) or None."""
        ya, yb, mag, rep = self.y3 + bias, self.exact + bias, abs(self.y3) + abs(bias), self.rep
        if skip is not None:
            sh, sl, s = skip
            ya, yb, mag, rep = ya + sh + sl, yb + s, mag + abs(sh) + abs(sl), rep + pair_err(s)
        if relu:
            ya, yb = _relu(ya), _relu(yb)
        bound_a = self.acc + EPI_REL * mag
        if pair_out:
            bound_a = bound_a + pair_err(ya)
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
