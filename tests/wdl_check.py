"""The float64 yardstick and the per-element bounds of the win / draw / loss dense tail (csrc/xq_heads.hip: k_fc_tile<WDL>,
cz_heads_tail_wdl), derived from the arithmetic the kernel performs.  It continues tests/f16_pairs.py's part THE DENSE TAIL OF
THE HEADS and uses its constants (U = 2^-24, EXPF_REL, the pair formats) and its DenseCheck for the hidden layer.

What the kernel computes for one position.  Hidden pre-activations y_j + b1_j on (hi, lo) pairs exactly as k_fc_tile<VALUE>
(DenseCheck.bounds gives the reference and the per-element bound B_j on either set of operands), h_j = relu(.), then for each
class k in (win, draw, loss)
    l_k = sum_j h_j w2[k][j] + b2_k                                             (three fp32 dot products, one per class)
    m = max(max(l_W, l_L), l_D),  e_k = expf(l_k - m),  s = (e_W + e_L) + e_D
    wdl_k = e_k / s,    v = (e_W - e_L) / s.

Class logits (logit_check).  The three dot products run side by side through the reduction of the scalar head, so
f16_pairs.value_check's count holds for each of them, restated for what is built here: the library is compiled with
-ffp-contract=off, a product and an addition round separately; a lane adds its T = 32 ceil(tiles / 8) hidden units
(tiles = ceil(n_hidden / 32): two label tiles of 16 accumulator rows per pass, a wave takes every fourth pair) one after the
other into the class's accumulator, 2 T roundings; one shuffle addition joins the half-waves; the finishing lane adds the four
waves' sums to 0 in wave order (the first addition is exact: 3 roundings).  A term passes through at most n = 2 T + 4 roundings,
each at most U times a partial sum of |h_j w2_kj|, so with A_k = sum_j (|h_j| + B_j) |w2_kj| and gamma_n = n U / (1 - n U)
    |delta l_k| <= BL_k = sum_j B_j |w2_kj| + gamma_n A_k + U (|l_k - b2_k| + |b2_k|),
the last term being the one rounding of the bias addition.  b2_k must be the fp32 values the kernel is handed.

Probabilities (softmax_check).  With the kernel's logits off by delta_k, the exact softmax of ITS logits is within a factor
exp(+-(BL_j + max_k BL_k)) of p_j (f16_pairs' argument, unchanged).  The kernel's own arithmetic on its logits, first order in U:
  * t_j = fl(l_j - m) is off by U |t_j|, which moves exp by U |t_j| relative; |t_j| <= 126 ln 2 < 88 wherever p_j >= 2^-126;
  * expf adds EXPF_REL (f16_pairs: measured on the device library, doubled);
  * s: its three terms carry the two errors above, weighted by their share of the sum: EXPF_REL + U sum_k p_k |t_k|, and
    sum_k p_k |t_k| = H(p) - ln(sum_k e_k) <= H(p) <= ln 3 because the largest e_k is exactly 1; its two additions of positive
    terms add 2 U;
  * the division is one rounding: U.
    STAT3 = 88 U + 2 EXPF_REL + (3 + ln 3) U          (98.1 U = 5.9e-6 with EXPF_REL = 3 U).
Where e_j falls below the smallest normal float the result keeps no relative accuracy; both the kernel's quotient and the exact
one then lie in [0, 2^-126 (1 + STAT3)], so they differ by less than 2^-125:
    |delta wdl_j| <= BP_j = (expm1(BL_j + max_k BL_k) + STAT3) p_j + 2^-125.

Value (value_bound).  v = (e_W - e_L) / s is the difference of the two unrounded quotients e_W / s and e_L / s -- each within
its BP of p_W and p_L (BP counts the quotient's rounding, which they do not have: slack, not a gap) -- after one rounding of
the difference e_W - e_L and one of the quotient, each at most U |v| to first order:
    |delta v| <= BP_W + BP_L + 2 U |v|.
The test's planted rows sit at |v| = 1, p = (1, exp(-60), exp(-120)): there BP is STAT3-sized and the bound on v is ~2e-5.

Rows of wdl sum to 1 (ROWSUM_TOL).  The logits' errors cancel in the sum.  sum_k e_k / s with the kernel's s, a sum of positive
terms with two roundings, is within 2 U (1 + U) of 1; the three quotients' roundings add at most U sum_k wdl_k (or 2^-150 each
in the subnormal range): 3 U to first order, ROWSUM_TOL = 4 U with the second-order terms.  The test sums the three fp32 values
in float64.

Symmetry, exact.  max(max(W, L), D), (e_W + e_L) + e_D and e_W - e_L treat win and loss alike (an fp32 addition commutes and
a - b = -(b - a) exactly), so swapping rows 0 and 2 of w2 and of b2 negates v and swaps wdl's outer columns bit for bit."""
import numpy as np

import f16_pairs as fp

U = fp.U
STAT3 = 88.0 * U + 2.0 * fp.EXPF_REL + (3.0 + float(np.log(3.0))) * U
P_FLOOR3 = 2.0 ** -125
ROWSUM_TOL = 4.0 * U


def logit_check(hidden, bound, w2, b2):
    """(l [n, 3], bound_l [n, 3]): the float64 class logits relu(hidden) . w2[k] + b2[k] of the reference pre-activations
    hidden [n, n_hidden] (bias included) and the bound BL on the kernel's, given the per-element bound on its pre-activations.
    w2 [3, n_hidden] float64; b2: three Python floats that fp32 holds exactly.  numpy arrays or torch tensors."""
    assert len(b2) == 3 and all(float(np.float32(b)) == b for b in b2), "b2 must be exact in fp32: the kernel takes floats"
    h = hidden * (hidden > 0)
    t = 32 * -(-(-(-hidden.shape[1] // 32)) // 8)
    n = 2 * t + 4
    gamma = n * U / (1.0 - n * U)
    bias = (np.asarray(b2, dtype=np.float64) if isinstance(hidden, np.ndarray)
            else hidden.new_tensor(list(b2)))
    d0 = h @ w2.T
    bl = bound @ abs(w2).T + gamma * ((h + bound) @ abs(w2).T) + U * (abs(d0) + abs(bias))
    return d0 + bias, bl


def softmax_check(l, bl):
    """(p [n, 3], bound_p [n, 3]) from logit_check's results."""
    e = fp._fn(l - fp._rowmax(l), "exp")
    p = e / e.sum(1)[:, None]
    return p, (fp._fn(bl + fp._rowmax(bl), "expm1") + STAT3) * p + P_FLOOR3


def value_bound(p, bp):
    """(v [n], bound_v [n]): P(win) - P(loss) and the bound on the kernel's value."""
    v = p[:, 0] - p[:, 2]
    return v, bp[:, 0] + bp[:, 2] + 2.0 * U * abs(v)


def wdl_check(hidden, bound, w2, b2):
    """dict(l, bl, p, bp, v, bv): everything above for one set of operands."""
    l, bl = logit_check(hidden, bound, w2, b2)
    p, bp = softmax_check(l, bl)
    v, bv = value_bound(p, bp)
    return dict(l=l, bl=bl, p=p, bp=bp, v=v, bv=bv)
