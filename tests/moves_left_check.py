"""The float64 yardsticks and the bounds of the moves-left output: its row of the dense tail (csrc/xq_heads.hip:
k_fc_tile<VALUE_ML / WDL_ML>, cz_heads_tail_ml) and its loss (csrc/xq_train.hip: k_moves_left_loss, cz_moves_left_loss), each
derived from the arithmetic the kernel performs.  It continues tests/wdl_check.py and tests/f16_pairs.py and uses their
constants (U = 2^-24, EXPF_REL) and f16_pairs.DenseCheck for the hidden layer.

THE TAIL'S OUTPUT x (x_check).  The hidden pre-activations y_j + b1_j are k_fc_tile<VALUE>'s (DenseCheck.bounds gives the
reference and the per-element bound B_j on either set of operands), h_j = relu(.), and
    x = sum_j h_j w2[ml][j] + b2[ml]
is one more fp32 dot product that runs beside the value head's through the same reduction: wdl_check.logit_check's count
holds for it as for one more class.  A lane adds its T = 32 ceil(tiles / 8) hidden units (tiles = ceil(n_hidden / 32)) one
after the other, product and addition rounded separately (-ffp-contract=off): 2 T roundings; one shuffle addition joins the
half-waves; the finishing lane adds the four waves' sums to 0 in wave order (3 roundings): a term passes through at most
n = 2 T + 4 roundings.  With A = sum_j (|h_j| + B_j) |w2_j| and gamma_n = n U / (1 - n U)
    |delta x| <= BL = sum_j B_j |w2_j| + gamma_n A + U (|x - b| + |b|),
the last term being the one rounding of the bias addition; b must be the fp32 value the kernel is handed.  Nothing follows
the sum: the tail writes x raw, which is why the bound is that of a plain dot product.

THE LOSS (loss_check).  Per row, all in fp32, with e = expf(-|x|), l = log1pf(e), t = left / unit:
    y = max(x, 0) + l,   d = y - t,   loss = d^2 / 2 if |d| <= delta else delta (|d| - delta / 2),
    sg = 1 / (1 + e) if x >= 0 else e / (1 + e),   grad = cr (clamp(d, -delta, delta) sg),   cr = fl(fl(w_m fl(1 / B)) w_r).
First order in U throughout (products of two error terms are below 1e-13 of the quantities here).
  * l.  The argument -|x| is exact.  expf is off by EXPF_REL relative; log1p moves by e / (1 + e) times that, which is at
    most l times it (e / ((1 + e) log1p(e)) <= 1 on (0, 1]); log1pf adds LOG1P_REL:  E_l = (EXPF_REL + LOG1P_REL) l.
  * y.  For x <= 0 the addition 0 + l is exact; for x > 0 it is one rounding:  E_y = E_l + U y.
  * t is one correctly rounded quotient of two exact numbers (left < 2^24):  E_t = U t.
  * d is one rounded difference:  E_d = E_y + E_t + U |d|.
  * loss.  d^2 / 2 is (0.5 d) d, the first product exact: it moves by |d| E_d + E_d^2 / 2 and one rounding; delta (|d| -
    delta / 2) moves by delta E_d and two roundings (delta / 2 is exact).  The two forms agree to (|d| - delta)^2 / 2 <=
    E_d^2 / 2 where the kernel's d and the exact one fall on different sides of delta.  Both cases:
        E_loss = (min(|d|, delta) + E_d) E_d + 2 U loss + 2^-149.
  * sg.  e enters with EXPF_REL (a relative error of e moves e / (1 + e) and 1 / (1 + e) by no more than itself); the sum
    1 + e and the quotient are one rounding each:  sg is off by (EXPF_REL + 2 U) sg, and by at most 2^-126 where e has left
    the normal range (x < -87).
  * grad.  The float64 model forms cr = w_m w_r / B exactly; the kernel's has three roundings (the reciprocal, and two
    products; without row weights two).  clamp is 1-Lipschitz; its product with sg and the product with cr round once each:
        E_grad = (EXPF_REL + 7 U) |grad| + |cr| (sg E_d + 2^-126) + 2^-149
    (the last term: a result in the subnormal range, and the exact 0 of a row whose weight is 0).
Neither form of the loss or of sg can overflow or lose its sign for any finite x: e lies in [0, 1].

Library terms, MEASURED as f16_pairs' were (the ROCm installation carries no accuracy statement for them).  expf: EXPF_REL of
f16_pairs.  log1pf is reached through cz_moves_left_loss itself (tests/test_gpu_moves_left_trainer.py::
test_library_terms_through_the_loss_kernel): with left = 0, unit = 1 and a tiny power of two as delta the linear branch
returns delta (y - delta / 2) = delta y exactly, so y = log1pf(expf(x)) can be read back bit for bit for x <= 0; on every
fp16 value x in [-25, -2^-10] the composite was off by at most 1.92 U y on an MI355X (2026-10-20), of which expf may
have contributed up to its measured 1.41 U.  The two terms cannot be told apart from outside, so the constant is set on their
sum: LOG1P_REL = 2 U makes EXPF_REL + LOG1P_REL = 5 U, more than twice the composite's measured error; the test holds the
kernel to it.  Below x = -25 (e < 2^-36) log1p(e) = e to within e^2 / 2, far below one rounding, and nothing was measured."""
import numpy as np

import f16_pairs as fp

U = fp.U
LOG1P_REL = 2.0 * U
SOFTPLUS_REL = fp.EXPF_REL + LOG1P_REL
UNIT = 32.0                     # the test's own statement of agent/model.py MOVES_LEFT_UNIT / MOVES_LEFT_DELTA
DELTA = 0.5


def x_check(hidden, bound, w2, b):
    """(x [n], bound_x [n]): the float64 output relu(hidden) . w2 + b of the reference pre-activations hidden [n, n_hidden]
    (bias included) and the bound BL on the kernel's, given the per-element bound on its pre-activations.  w2 [n_hidden]
    float64; b: a Python float that fp32 holds exactly.  numpy arrays or torch tensors."""
    assert float(np.float32(b)) == b, "b must be exact in fp32: the kernel takes a float"
    h = hidden * (hidden > 0)
    t = 32 * -(-(-(-hidden.shape[1] // 32)) // 8)
    n = 2 * t + 4
    d0 = h @ w2
    bl = bound @ abs(w2) + n * U / (1.0 - n * U) * ((h + bound) @ abs(w2)) + U * (abs(d0) + abs(b))
    return d0 + b, bl


def softplus64(x):
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid64(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def loss_check(x, left, w_r=None, w_m=1.0, unit=UNIT, delta=DELTA):
    """dict(loss, e_loss, grad, e_grad): the float64 model of cz_moves_left_loss for the fp32 outputs x [B], the rows' targets
    left [B] (already gathered) and weights w_r [B] (None = 1), and the bounds on the kernel's results."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    left = np.asarray(left, dtype=np.float64)
    b = x.shape[0]
    wr = np.ones(b) if w_r is None else np.asarray(w_r, dtype=np.float32).astype(np.float64)
    l = np.log1p(np.exp(-np.abs(x)))
    y, sg = softplus64(x), sigmoid64(x)
    t = left / unit
    d = y - t
    ad = np.abs(d)
    loss = np.where(ad <= delta, 0.5 * d * d, delta * (ad - 0.5 * delta))
    e_d = SOFTPLUS_REL * l + U * y + U * t + U * ad
    e_loss = (np.minimum(ad, delta) + e_d) * e_d + 2.0 * U * loss + 2.0 ** -149
    cr = w_m * wr / b
    grad = cr * np.clip(d, -delta, delta) * sg
    e_grad = (fp.EXPF_REL + 7.0 * U) * np.abs(grad) + np.abs(cr) * (sg * e_d + 2.0 ** -126) + 2.0 ** -149
    return dict(loss=loss, e_loss=e_loss, grad=grad, e_grad=e_grad, d=d)
