"""The hash stub of stub_net with a third output, the network's raw moves-left x, in NumPy and in torch bit for bit.

    kq = 1 + ((mix64(h ^ C3) >> 40) & 0x7FF)         quanta of 1/16 ply: 1/16 .. 128 plies (h: the hash stub's position hash)
    x  = float32(log(expm1(kq / 512)))               what a network would have to put out for the search to read kq

The search turns x back into quanta as k = rint(512 * softplus(x)) (include/czero.h).  Over all 2048 values 512 * softplus(x)
lies within 1.3e-4 of kq -- in float32 in the stable form max(x, 0) + log1p(exp(-|x|)), in float32 in the naive form
log(1 + exp(x)), and in float64 -- so the rounding to kq has a margin of four orders of magnitude and no ulp of a device's
exp or log1p can move it (tests/test_moves_left_search_cpu.py asserts the table).  Both versions look x up in one float32 table
computed once in float64, which is what makes them agree bit for bit.

`variant` shapes the other two outputs for the property tests: "hash" is stub_net's policy and value, ("flat", v) a uniform
policy with the constant value v."""
import numpy as np

import stub_net

C3 = 0xD6E8FEB86659FD93
KQ_MAX = 2048
X_TABLE = np.log(np.expm1(np.arange(0, KQ_MAX + 1, dtype=np.float64).clip(min=0.5) / 512.0)).astype(np.float32)
X_TABLE[0] = np.float32(0.0)                                # (index 0 is never drawn)


def _h_numpy(planes, salt):
    pl = np.asarray(planes).reshape(len(planes), -1) != 0
    with np.errstate(over="ignore"):
        h0 = (pl.astype(np.uint64) * stub_net._C1[None, :pl.shape[1]]).sum(axis=1, dtype=np.uint64) + np.uint64(salt)
    return stub_net._mix64_np(h0)


def kq_numpy(planes, salt=0):
    """planes [n, 14|28, 10, 9] -> int64 [n]: the quanta the stub predicts for each position."""
    h = _h_numpy(planes, salt)
    return (1 + ((stub_net._mix64_np(h ^ np.uint64(C3)) >> np.uint64(40)) & np.uint64(0x7FF))).astype(np.int64)


def ml_stub_numpy(planes, salt=0, variant="hash"):
    """-> (policy float32 [n, 2086], value float32 [n], x float32 [n])"""
    if variant == "hash":
        p, v = stub_net.hash_stub_numpy(planes, salt)
    else:
        p, v = stub_net.uniform_stub_numpy(planes, variant[1])
    return p, v, X_TABLE[kq_numpy(planes, salt)]


_torch_tab = {}


def ml_stub_torch(planes, salt=0, variant="hash"):
    """ml_stub_numpy on any device, bit for bit."""
    import torch
    dev = planes.device
    if variant == "hash":
        p, v = stub_net.hash_stub_torch(planes, salt)
    else:
        n = planes.shape[0]
        p = torch.full((n, stub_net.N_LABELS), float(np.float32(1.0 / 2086.0)), dtype=torch.float32, device=dev)
        v = torch.full((n,), float(np.float32(variant[1])), dtype=torch.float32, device=dev)
    key = str(dev)
    if key not in _torch_tab:
        _torch_tab[key] = (torch.from_numpy(X_TABLE.copy()).to(dev), torch.from_numpy(stub_net._C1.view(np.int64).copy()).to(dev))
    tab, c1 = _torch_tab[key]
    n = planes.shape[0]
    pl = (planes.reshape(n, -1) != 0).to(torch.int64)
    h = stub_net._mix64_torch((pl * c1[None, :pl.shape[1]]).sum(dim=1) + stub_net._s64(salt))
    kq = 1 + ((stub_net._mix64_torch(h ^ stub_net._s64(C3)) >> 40) & 0x7FF)
    return p, v, tab[kq]


def softplus_f32(x):
    """The search's own form, float32 operation by operation: max(x, 0) + log1p(exp(-|x|))."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.maximum(x, np.float32(0.0)) + np.log1p(np.exp(-np.abs(x)).astype(np.float32)).astype(np.float32)).astype(np.float32)


def quanta_of_x(x):
    """k = min(rint(512 * softplus(x)), 16 * 1023) as include/czero.h states it; not finite or negative -> 0, +inf -> the cap."""
    t = (np.float32(512.0) * softplus_f32(x)).astype(np.float32)
    out = np.zeros(t.shape, dtype=np.int64)
    ok = t >= np.float32(0.0)                                # (False for NaN)
    big = ok & (t >= np.float32(16 * 1023))
    mid = ok & ~big
    out[big] = 16 * 1023
    out[mid] = np.rint(t[mid]).astype(np.int64)
    return out
