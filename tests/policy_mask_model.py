"""float64 NumPy restatement of the masked policy loss (cz_policy_value_loss_l / cz_policy_wdl_loss_l, run.py opt --policy-mask
legal) for test_policy_mask_cpu.py and test_gpu_policy_mask.py.  NumPy only.

A row's index set A is its legal labels together with the support of its target; the softmax, Keras 2.0.8's clipped
categorical cross-entropy, the clip's gradient mask and the gradient are those of the unmasked loss restricted to A."""
import numpy as np

EPS, HI = np.float32(1e-7), np.float32(1.0 - 1e-7)


def index_set(legal, target):
    """A: bool [B, L] -- the legal labels and the target's support"""
    return np.asarray(legal, dtype=bool) | (np.asarray(target) != 0)


def masked_loss(logits, target, A, w_p=1.0, row_w=None):
    """logits float32 [B, L] (anything outside A, NaN and +-inf included), target [B, L], A bool [B, L] containing the
    target's support.  -> dict of float64 arrays: loss [B]; grad [B, L] = (w_p / B) row_w (p S - t m), exactly 0 outside A;
    mass [B], the share of the full softmax over all L columns that lies outside A; and margin [B] in float32: the largest
    logit outside A minus the largest inside, one float32 difference of two float32 numbers, so it is exact."""
    x32 = np.asarray(logits, dtype=np.float32)
    t = np.asarray(target, dtype=np.float64)
    A = np.asarray(A, dtype=bool)
    assert not ((t != 0) & ~A).any(), "A must contain the target's support"
    B = x32.shape[0]
    x = x32.astype(np.float64)
    xa = np.where(A, x, -np.inf)
    e = np.exp(xa - xa.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    pc = np.clip(p, np.float64(EPS), np.float64(HI))
    loss = -np.where(t != 0, t * np.log(pc), 0.0).sum(1)
    m = (p > EPS) & (p < HI)
    S = (t * m).sum(1, keepdims=True)
    w = np.ones(B) if row_w is None else np.asarray(row_w, dtype=np.float64)
    grad = (w_p / B) * w[:, None] * (p * S - t * m)
    grad[~A] = 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        ef = np.exp(x - np.nanmax(x, axis=1, keepdims=True))
        mass = np.where(A, 0.0, ef).sum(1) / ef.sum(1)
        margin = np.where(A, -np.inf, x32).max(1).astype(np.float32) - np.where(A, x32, -np.inf).max(1).astype(np.float32)
    return dict(loss=loss, grad=grad, mass=mass, margin=margin, p=p, clip_mask=m)
