"""Host side of the dense tail (csrc/xq_heads.hip, cz_fc_pack_weights): the fragment layout
[label tile][K-step + 2 pad steps][part: hi, lo][lane][8] with output o = 32 tile + (lane & 31) and input
k = 16 kstep + 8 (lane >> 5) + j, the nearest-even (hi, lo) split, the zero padding, and the argument checks.  No GPU involved."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "chinesechess-alphazero_amd"))
PAD = 2


def _weights(n_out, n_in):
    """fp32 weights whose lo parts are fp16 subnormals (|w| ~ 0.05: lo ~ 1e-5 < 2^-14), with a few planted values: 0, an exact
    fp16 value (lo = 0), a value below 2^-14 (subnormal hi), a tie of the hi rounding, and a large one."""
    import torch
    g = torch.Generator().manual_seed(n_out * 4096 + n_in)
    w = torch.randn(n_out, n_in, generator=g) * 0.05
    flat = w.view(-1)
    plant = [0.0, 0.5, 3.0e-6, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -8, -1234.567, 2.0 ** -14 + 2.0 ** -26]
    for i, v in enumerate(plant[:flat.numel()]):
        flat[(i * 7919) % flat.numel()] = v
    return w


@pytest.mark.parametrize("pair", ["float16", "bfloat16"])
@pytest.mark.parametrize("n_out", [2086, 256, 33, 1])
@pytest.mark.parametrize("n_in", [180, 360, 17])
def test_fc_pack_every_element(n_in, n_out, pair):
    import torch
    from cchess_alphazero import _native
    dt = getattr(torch, pair)
    w = _weights(n_out, n_in)
    tiles, ksteps = (n_out + 31) // 32, (n_in + 15) // 16
    n = _native.lib().cz_fc_packed_elems(n_out, n_in)
    assert n == tiles * (ksteps + PAD) * 2 * 64 * 8
    packed = _native.pack_fc_weights(w, dt)
    assert packed.dtype == dt and packed.numel() == n
    got = packed.view(tiles, ksteps + PAD, 2, 64, 8)
    # the formula, for every element at once: pad the matrix with zeros to whole tiles and steps, then index it
    full = torch.zeros(tiles * 32, (ksteps + PAD) * 16)
    full[:n_out, :n_in] = w
    lane = torch.arange(64)
    o = (torch.arange(tiles).view(-1, 1, 1, 1) * 32 + (lane & 31).view(1, 1, -1, 1)).expand(tiles, ksteps + PAD, 64, 8)
    k = (torch.arange(ksteps + PAD).view(1, -1, 1, 1) * 16 + ((lane >> 5) * 8).view(1, 1, -1, 1)
         + torch.arange(8).view(1, 1, 1, -1)).expand(tiles, ksteps + PAD, 64, 8)
    v = full[o, k]
    hi = v.to(dt)                                          # PyTorch's conversion rounds to nearest even
    lo = (v - hi.float()).to(dt)
    # bit for bit (a zero must be +0: the buffer is cleared, not computed)
    assert torch.equal(got[:, :, 0].view(torch.int16), hi.view(torch.int16))
    assert torch.equal(got[:, :, 1].view(torch.int16), lo.view(torch.int16))
    # the padding, stated on its own: both pad steps, inputs past n_in, outputs past n_out
    assert not got[:, ksteps:].view(torch.int16).any()
    mask = ((o >= n_out) | (k >= n_in)).unsqueeze(2).expand_as(got)
    assert not got.view(torch.int16)[mask].any()
    if pair == "float16" and n_in * n_out > 100:
        sub = (lo.float().abs() > 0) & (lo.float().abs() < 2.0 ** -14)
        assert sub[(o < n_out) & (k < n_in)].float().mean() > 0.5                    # most lo parts are fp16 subnormals, and they are kept
        assert torch.equal((hi.float() + lo.float())[sub], (got[:, :, 0].float() + got[:, :, 1].float())[sub])
    err = (hi.double() + lo.double() - v.double()).abs()
    rel, ab = (2.0 ** -22, 2.0 ** -25) if pair == "float16" else (2.0 ** -16, 2.0 ** -134)
    assert (err <= rel * v.double().abs() + ab).all()


def test_fc_packed_elems_limits():
    from cchess_alphazero import _native
    f = _native.lib().cz_fc_packed_elems
    f.restype = C.c_size_t
    assert f(1, 1) == 1 * 3 * 2 * 64 * 8
    assert f(65536, 2048) == 2048 * (128 + PAD) * 1024
    assert f(2086, 360) == 66 * 25 * 1024
    for n_out, n_in in ((0, 180), (180, 0), (-1, 180), (180, -1), (65537, 180), (2086, 2049), (0, 0)):
        assert f(n_out, n_in) == 0, (n_out, n_in)


def test_fc_pack_rejects_bad_arguments():
    import torch
    from cchess_alphazero import _native
    L = _native.lib()
    L.cz_fc_pack_weights.restype = C.c_int
    L.cz_fc_pack_weights.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    w = np.ones((33, 17), dtype=np.float32)
    out = np.full(2 * (2 + PAD) * 1024 + 16, 0x5A5A, dtype=np.uint16)      # 2 label tiles, 2 K-steps
    ERR_ARG = -1
    for dtype in (_native.F32, _native.U8, _native.F16C8, _native.F16C6, 99, -1):
        assert L.cz_fc_pack_weights(w.ctypes.data, 33, 17, dtype, out.ctypes.data) == ERR_ARG, dtype
    assert L.cz_fc_pack_weights(None, 33, 17, _native.F16, out.ctypes.data) == ERR_ARG
    assert L.cz_fc_pack_weights(w.ctypes.data, 33, 17, _native.F16, None) == ERR_ARG
    assert L.cz_fc_pack_weights(w.ctypes.data, 0, 17, _native.F16, out.ctypes.data) == ERR_ARG
    assert L.cz_fc_pack_weights(w.ctypes.data, 33, 2049, _native.F16, out.ctypes.data) == ERR_ARG
    assert b"cz_fc_pack_weights" in L.cz_last_error()
    assert (out == 0x5A5A).all()                           # a refused call writes nothing
    assert L.cz_fc_pack_weights(w.ctypes.data, 33, 17, _native.BF16, out.ctypes.data) == 0
    assert (out[-16:] == 0x5A5A).all() and not (out[:-16] == 0x5A5A).any()         # exactly cz_fc_packed_elems elements written
    with pytest.raises(_native.NativeError):
        _native.pack_fc_weights(torch.ones(3, 2049))
