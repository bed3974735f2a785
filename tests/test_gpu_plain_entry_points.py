"""-m gpu: the plain entry points cz_input_conv / cz_resblock / cz_resblock_heads against their compact-queue forms (_q), which
are all cchess_alphazero/_native.py ever calls.  For every launch these entry points make, on outputs pre-filled with 0x5A bytes
and in this order:

  1. the _q form with n_dev = NULL;
  2. the _q form with a device-side board count of n - 2;
  3. directly after it, the plain form.

1 and 3 write equal bytes for all n boards (the plain form sees no count -- and no row list -- of the call before it); 2 equals 1
on boards 0 .. n - 3 and leaves the last two boards at the fill value.  n = 5: odd, so the kernels that take two boards per
workgroup or per tile get a half-empty last one, with and without the count.  Only equality of bytes is asserted: what the
kernels compute is pinned elsewhere (test_gpu_tower.py, test_gpu_c6_elements.py, test_gpu_conv*.py ...).

Also here because it needs a device: cz_resblock_chain refuses CZ_F16C86 under CZ_IP_PAIR=0 (after its device query)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import c6_model as m  # noqa: E402
from test_gpu_c6_elements import KM, KO, KX, _head_filters, _pack6, _pack8, _pair, _planes, _t  # noqa: E402

N, FILL = 5, 0x5A


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _out(nbytes):
    """an output buffer of nbytes per board"""
    import torch
    return torch.empty((N, nbytes), dtype=torch.uint8, device="cuda")


def _triple(call, outs):
    """call(q, n_dev) launches the plain (q False) or the _q form into the buffers `outs`."""
    import torch
    count = torch.tensor([N - 2], dtype=torch.int32, device="cuda")

    def run(q, n_dev):
        for o in outs:
            o.fill_(FILL)
        call(q, n_dev)
        torch.cuda.synchronize()
        return [o.cpu().numpy().copy() for o in outs]

    full, part, plain = run(True, None), run(True, count), run(False, None)
    for i, (f, c, p) in enumerate(zip(full, part, plain)):
        assert all((f[b] != FILL).any() for b in range(N)), (i, "a board was not written")
        assert np.array_equal(f, p), (i, "plain form != _q form with n_dev = NULL", np.argwhere((f != p).any(1)).ravel().tolist())
        assert np.array_equal(c[:N - 2], f[:N - 2]), (i, "counted boards differ")
        assert (c[N - 2:] == FILL).all(), (i, "a board behind the device count was written")


@functools.lru_cache(maxsize=None)
def _data(C_, kind):
    """x (the operand tuple on the device) and the block's (w1, b1, w2, b2) on the device, for kind in
    f16 / bf16 (split pairs), f16p1 (plain operands), c8, c6."""
    import torch
    from cchess_alphazero import _native
    rng = np.random.default_rng(7 + C_ + len(kind))
    x = m.activations(N, C_, KX if kind == "c6" else 0, rng)
    (w1, b1), (w2, b2) = m.filters(C_, rng), m.filters(C_, rng)
    if kind == "c6":
        xs, p1, p2 = _pair(x, KX), _pack6(w1, KX, KM), _pack6(w2, KM, KO)
    elif kind == "c8":
        xs, p1, p2 = _native.split_c8(torch.from_numpy(x).cuda()), _pack8(w1), _pack8(w2)
    else:
        dt = torch.bfloat16 if kind == "bf16" else torch.float16
        parts = 1 if kind == "f16p1" else 2
        xf = torch.from_numpy(x).cuda()
        hi = xf.to(dt)
        xs = (hi, (xf - hi.float()).to(dt)) if parts == 2 else (hi,)
        p1, p2 = (_native.pack_conv3x3_weights(torch.from_numpy(w), dt, parts) for w in (w1, w2))
    return xs, (p1.cuda(), _t(b1), p2.cuda(), _t(b2))


def _resblock(C_, kind, code, parts, f32=False):
    from cchess_alphazero import _native
    L = _native.lib()
    xs, dev = _data(C_, kind)
    px = 90 * C_
    outs = [_out(4 * px)] if f32 else [_out(2 * px)] + ([_out(2 * px)] if parts == 2 else [])
    yh, yl, yf = (None, None, outs[0]) if f32 else (outs[0], outs[1] if parts == 2 else None, None)

    def call(q, n_dev):
        a = [_p(xs[0]), _p(xs[1]) if parts == 2 else None, *map(_p, dev), _p(yh), _p(yl), _p(yf), N, C_, code, parts]
        rc = L.cz_resblock_q(*a, _p(n_dev), _native._stream()) if q else L.cz_resblock(*a, _native._stream())
        _native.check(rc, "cz_resblock")
    _triple(call, outs)


F16, BF16, F16C8, F16C6, F16C86 = 1, 2, 4, 5, 6


@pytest.mark.parametrize("what", ["pipe", "f32", "plain", "c8", "c6"])
def test_resblock_128(what):
    """k_resblock_pipe (pair output), k_resblock (fp32 output; plain operands: two boards per tile), k_resblock_c8 on c8 / c6"""
    kind, code, parts, f32 = {"pipe": ("f16", F16, 2, False), "f32": ("f16", F16, 2, True), "plain": ("f16p1", F16, 1, False),
                              "c8": ("c8", F16C8, 2, False), "c6": ("c6", F16C6, 2, False)}[what]
    _resblock(128, kind, code, parts, f32)


@pytest.mark.parametrize("what", ["f16", "c8", "c8_ip_pair_0"])
def test_resblock_192(what, monkeypatch):
    """k_resblock_ip (split pairs); c8: a pair of boards on four waves (k_resblock_ip4_c8), CZ_IP_PAIR=0: k_resblock_ip_c8"""
    monkeypatch.delenv("CZ_IP_PAIR", raising=False)
    if what == "c8_ip_pair_0":
        monkeypatch.setenv("CZ_IP_PAIR", "0")
    if what == "f16":
        _resblock(192, "f16", F16, 2)
    else:
        _resblock(192, "c8", F16C8, 2)


@pytest.mark.parametrize("kind,code", [("bf16", BF16), ("f16", F16), ("c8", F16C8), ("c6", F16C6)])
def test_resblock_heads(kind, code):
    from cchess_alphazero import _native
    L = _native.lib()
    xs, dev = _data(128, kind)
    hw, hb = (_t(a) for a in _head_filters(128, np.random.default_rng(3)))
    outs = [_out(4 * 90 * 4), _out(2 * 90 * 4)]

    def call(q, n_dev):
        a = [_p(xs[0]), _p(xs[1]), *map(_p, dev), _p(hw), _p(hb), _p(outs[0]), _p(outs[1]), N, 128, code, 4, 2]
        rc = L.cz_resblock_heads_q(*a, _p(n_dev), _native._stream()) if q else L.cz_resblock_heads(*a, _native._stream())
        _native.check(rc, "cz_resblock_heads")
    _triple(call, outs)


@pytest.mark.parametrize("code", [F16, F16C8])
def test_input_conv(code):
    """u8 planes, 14 planes, 128 filters, (hi, lo) f16 output and the c8 pair.  The _q form reads the boards through a
    permutation, the plain form gets the planes in that order."""
    import torch
    from cchess_alphazero import _native
    L = _native.lib()
    rng = np.random.default_rng(11)
    planes = torch.from_numpy(_planes(N, 14, rng)).cuda()
    perm = torch.tensor([3, 0, 4, 2, 1], dtype=torch.int32, device="cuda")
    permuted = planes[perm.long()].contiguous()
    assert not torch.equal(permuted, planes)
    w = torch.from_numpy((rng.standard_normal((128, 14, 5, 5)) * 0.1).astype(np.float32))
    wp = _native.pack_input_conv_weights(w, torch.float16, 2).cuda()
    bias = _t((rng.standard_normal(128) * 0.5).astype(np.float32))
    outs = [_out(2 * 90 * 128), _out(2 * 90 * 128)]

    def call(q, n_dev):
        tail = [_p(wp), _p(bias), _p(outs[0]), _p(outs[1]), N, 128, code, 2, 1]
        if q:
            rc = L.cz_input_conv_q(_p(planes), _native.U8, 14, *tail, _p(perm), _p(n_dev), _native._stream())
        else:
            rc = L.cz_input_conv(_p(permuted), _native.U8, 14, *tail, _native._stream())
        _native.check(rc, "cz_input_conv")
    _triple(call, outs)


def test_c86_chain_is_refused_on_the_six_wave_kernel(monkeypatch):
    """CZ_F16C86 exists on the four-wave kernel only: under CZ_IP_PAIR=0 cz_resblock_chain refuses it (real tensors throughout:
    nothing here could launch on a bad pointer)."""
    from cchess_alphazero import _native
    L = _native.lib()
    monkeypatch.setenv("CZ_IP_PAIR", "0")
    xs, dev = _data(192, "c8")
    arrays = [(C.c_void_p * 1)(t.data_ptr()) for t in dev]
    yh, yi = _out(2 * 90 * 192), _out(2 * 90 * 192)
    rc = L.cz_resblock_chain(_p(xs[0]), _p(xs[1]), 1, *arrays, _p(yh), _p(yi), None, N, 192, F16C86, None, _native._stream())
    assert rc == -1
    assert L.cz_last_error().decode() == ("cz_resblock_chain: CZ_F16C86 (a c6 chain that starts the tower) exists on the "
                                          "four-wave kernel only (CZ_IP_PAIR=0 is set)")
