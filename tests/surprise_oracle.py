"""The policy surprise record (cz_search_record_surprise, run.py self --record-surprise, run.py opt --surprise-weight)
restated in plain Python: the yardstick of tests/test_surprise_cpu.py and tests/test_gpu_surprise.py.

    M = sum m_j        P = sum float64(p_j)                   over the non-banned edges
    t_j = m_j / M      r_j = max(p_j / P, 1e-30)
    s = max( sum t_j * log(t_j / r_j), 0 )                    over the non-banned edges with m_j > 0

Every quotient, product and logarithm is one float64 operation (math.log); the sums are math.fsum's, exact.  M = 0 or not
P > 0 gives NaN.

THE BOUND of a kernel against this file, per row: 64 * 2^-53 * A + 1e-300 with A = sum |t_j log(t_j / r_j)|.  A term is
two quotients, one product and one logarithm of a few ulp each -- the device logarithm is documented to 1 ulp, math.log
is the C library's, below 1 ulp -- and the kernel adds at most nine levels deep (the lane's two terms, one carried sum,
six ladder steps and the ladder's read), so its sum is within 9 * 2^-53 * A of the exact sum of its own terms; doubled
for the two sides and rounded up to a power of two.

WHAT THE BOUND PRESUMES: that both sides divide by the same P.  The float64 sum of up to 128 float32 priors is exact in
every order while the nonzero priors span less than 2^22 between the smallest and the greatest (24 significant bits, 7
bits of carries, 22 bits of span: 53), and the bound holds for such rows; random_priors() draws them so.  Past that span
the kernel's P carries its own summation error, at most 7 roundings deep (the lane's second term and six ladder steps),
and math.fsum's one: r_j moves by up to 8 * 2^-53 relative, log(t_j / r_j) by as much absolutely, and s by that times
sum t_j = 1 -- an error that does not shrink with A.  bound_wide() adds 9 * 2^-53 for it (the ninth for the second-order
terms); a row with A < 0.14 may need it."""
import math
from collections import namedtuple

import numpy as np

BANNED = 0x8000
NAN = float("nan")
FLOOR = 1e-30
S_BOUND = 70.0                                          # ln 1e30 = 69.08 < 70 (include/czero.h CZ_SURPRISE_BOUND)
Entry = namedtuple("Entry", "moves n banned q s")       # what lib/data_helper.record_item reads of a VisitEntry


def surprise(labels, m, p):
    """labels (bit 15 = banned), m (the recorded counts), p (float32 priors without noise) of one root's edges ->
    (s, A): the surprise, NaN when no live edge has a count or the live priors do not sum to something positive, and
    A = sum |t_j log(t_j / r_j)|, the scale of the bound (0.0 beside NaN)."""
    live = [j for j in range(len(m)) if not int(labels[j]) & BANNED]
    M = sum(int(m[j]) for j in live)
    P = math.fsum(float(np.float32(p[j])) for j in live)
    if M == 0 or not P > 0.0:
        return NAN, 0.0
    terms = []
    for j in live:
        if int(m[j]) <= 0:
            continue
        t = float(int(m[j])) / float(M)
        r = max(float(np.float32(p[j])) / P, FLOOR)
        terms.append(t * math.log(t / r))
    return max(math.fsum(terms), 0.0), math.fsum(abs(x) for x in terms)


def bound(A):
    return 64.0 * 2.0 ** -53 * A + 1e-300


def bound_wide(A):
    """The bound for priors that span 2^22 or more: P's own summation error on top (the module docstring)."""
    return bound(A) + 9.0 * 2.0 ** -53


def same(got, want, A, wide=False):
    """NaN where the other is NaN, otherwise within the bound."""
    b = bound_wide(A) if wide else bound(A)
    return (got != got and want != want) or (got == got and want == want and abs(got - want) <= b)


def random_priors(rng, nm, span=6.0):
    """nm float32 priors as a search spreads them -- a softmax over the legal moves -- with logits within +-span: the
    greatest is at most e^(2 span) times the smallest (e^12 < 2^18 at the default), so their float64 sum is exact."""
    if nm == 0:
        return np.zeros(0, dtype=np.float32)
    x = rng.uniform(-span, span, nm)
    e = np.exp(x - x.max())
    return (e / e.sum()).astype(np.float32)
