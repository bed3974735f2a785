"""The hash stub of stub_net with a third output, win / draw / loss rows whose draw column the search reads, in NumPy and in
torch bit for bit.

    uv   = stub_net's 16-bit value field           v = (uv - 32768) / 32768
    room = 32768 - |uv - 32768|                    1 - |v| in units of 2^-15
    rd   = ((mix64(h ^ C4) >> 40) & 0x3F) % 33     0 .. 32
    dq   = room * rd                               0 .. 2^20: the quanta the search must read (include/czero.h)
    d    = float32(dq / 2^20)                      exact: dq has at most 21 bits

So d is an exact multiple of 2^-20 and d <= 1 - |v| always, and the search's rint(d * 2^20) is dq with nothing to round.
The other two columns are (1 + v - d) / 2 and (1 - v - d) / 2 in float32; nothing in the search reads them.

`variant` shapes the other two outputs: "hash" is stub_net's policy and value, ("flat", v) a uniform policy with the constant
value v, "peaked" stub_net's peaked policy (8 squarings) with the value 0.  With a constant value the room is capped at
floor((1 - |v|) * 32768), so that d <= 1 - |v| holds there too."""
import numpy as np

import stub_net

C4 = 0xA0761D6478BD642F
QUANTA = 1 << 20


def _h_numpy(planes, salt):
    pl = np.asarray(planes).reshape(len(planes), -1) != 0
    with np.errstate(over="ignore"):
        h0 = (pl.astype(np.uint64) * stub_net._C1[None, :pl.shape[1]]).sum(axis=1, dtype=np.uint64) + np.uint64(salt)
    return stub_net._mix64_np(h0)


def _room_cap(variant):
    if variant == "hash":
        return 32768
    v = 0.0 if variant == "peaked" else float(np.float32(variant[1]))
    return int(np.floor((1.0 - abs(v)) * 32768.0))


def dq_numpy(planes, salt=0, variant="hash"):
    """planes [n, 14|28, 10, 9] -> int64 [n]: the quanta of the stub's draw probability of each position."""
    h = _h_numpy(planes, salt)
    uv = ((stub_net._mix64_np(h ^ np.uint64(stub_net.C2)) >> np.uint64(40)) & np.uint64(0xFFFF)).astype(np.int64)
    room = np.minimum(32768 - np.abs(uv - 32768), _room_cap(variant))
    rd = ((stub_net._mix64_np(h ^ np.uint64(C4)) >> np.uint64(40)) & np.uint64(0x3F)).astype(np.int64) % 33
    return room * rd


def _pv_numpy(planes, salt, variant):
    if variant == "hash":
        return stub_net.hash_stub_numpy(planes, salt)
    if variant == "peaked":
        return stub_net.peaked_stub_numpy(planes, salt, 8, 0.0)
    return stub_net.uniform_stub_numpy(planes, variant[1])


def draw_stub_numpy(planes, salt=0, variant="hash"):
    """-> (policy float32 [n, 2086], value float32 [n], wdl float32 [n, 3])"""
    p, v = _pv_numpy(planes, salt, variant)
    d = (dq_numpy(planes, salt, variant).astype(np.float32) / np.float32(QUANTA)).astype(np.float32)
    one, two = np.float32(1.0), np.float32(2.0)
    wdl = np.stack([((one + v) - d) / two, d, ((one - v) - d) / two], axis=1).astype(np.float32)
    return p, v, wdl


_torch_tab = {}


def draw_stub_torch(planes, salt=0, variant="hash"):
    """draw_stub_numpy on any device, bit for bit."""
    import torch
    dev = planes.device
    n = planes.shape[0]
    if variant == "hash":
        p, v = stub_net.hash_stub_torch(planes, salt)
    elif variant == "peaked":
        p, v = stub_net.peaked_stub_torch(planes, salt, 8, 0.0)
    else:
        p = torch.full((n, stub_net.N_LABELS), float(np.float32(1.0 / 2086.0)), dtype=torch.float32, device=dev)
        v = torch.full((n,), float(np.float32(variant[1])), dtype=torch.float32, device=dev)
    key = str(dev)
    if key not in _torch_tab:
        _torch_tab[key] = torch.from_numpy(stub_net._C1.view(np.int64).copy()).to(dev)
    c1 = _torch_tab[key]
    pl = (planes.reshape(n, -1) != 0).to(torch.int64)
    h = stub_net._mix64_torch((pl * c1[None, :pl.shape[1]]).sum(dim=1) + stub_net._s64(salt))
    uv = (stub_net._mix64_torch(h ^ stub_net._s64(stub_net.C2)) >> 40) & 0xFFFF
    room = torch.clamp(32768 - (uv - 32768).abs(), max=_room_cap(variant))
    rd = ((stub_net._mix64_torch(h ^ stub_net._s64(C4)) >> 40) & 0x3F) % 33
    d = (room * rd).to(torch.float32) / float(QUANTA)
    wdl = torch.stack([((1.0 + v) - d) / 2.0, d, ((1.0 - v) - d) / 2.0], dim=1)
    return p, v, wdl


def draw_quanta(d):
    """dq = rint(d * 2^20) as include/czero.h states it: float32, NaN or d < 0 -> 0, d >= 1 -> 2^20."""
    d = np.asarray(d, dtype=np.float32)
    out = np.zeros(d.shape, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = d >= np.float32(0.0)                                # (False for NaN)
        big = ok & (d >= np.float32(1.0))
        mid = ok & ~big
        out[big] = QUANTA
        out[mid] = np.rint((d[mid] * np.float32(QUANTA)).astype(np.float32)).astype(np.int64)
    return out


# the grid of the conversion tests (tests/test_draw_search_cpu.py, tests/test_gpu_draw_search.py) and what it must give
GRID = np.array([0.0, -0.0, 1.0, 0.5, 2.0 ** -21, 3 * 2.0 ** -21, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23, -1e-3, np.nan, np.inf,
                 -np.inf, 1e-40], dtype=np.float32)
GRID_DQ = [0, 0, QUANTA, QUANTA // 2, 0, 2, QUANTA, QUANTA, 0, 0, QUANTA, 0, 0]
