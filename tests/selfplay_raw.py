"""One raw self-play loop for the "off means off" tests of the visit, value and surprise records: the bytes the device
rings hand out, through the library's own drain entry points, with nothing of the Python binding's sorting in between."""
import ctypes as C

import numpy as np

from test_gpu_search import stub_eval

SPEC = dict(kind="hash", salt=5)


def selfplay_raw(gpu, pc, seed, rounds, G, setup_before=None, setup_after=None, capacity=0, playout_cap=None,
                 drain="plain", fill=0.0, no_drops=True):
    """`rounds` rounds of G self-play games against the hash stub, drained every 16 rounds (before either ring can fill at
    the default capacity).  setup_before(s) / setup_after(s) run before / after the visit ring is switched on with
    `capacity`; playout_cap = (fast_sims, full_rate).  drain names the entry point: "plain" cz_search_drain_visits, "q"
    ..._q, "qs" ..._qs, "s" ..._qs with q_buf NULL; a buffer the drain does not write keeps `fill`.  no_drops: assert that
    the ring lost nothing.

    Returns (records, entries, counters).  A record is its 16-byte header and the `turns` moves it holds; an entry (row, q
    bytes, s bytes), row = its 16-byte header and the n_edges labels and counts it holds (the ring slot's other bytes
    belong to no entry).  Both sorted: games that end in one launch reach the rings in any order."""
    s = gpu.S.Search(pc, G, seed=seed)
    if setup_before:
        setup_before(s)
    s.record_visits(True, capacity=capacity)
    if playout_cap:
        s.set_playout_cap(*playout_cap)
    if setup_after:
        setup_after(s)
    ev = stub_eval(gpu, SPEC)
    s.start_selfplay(seed=seed, first_game_id=0)
    recs, entries = [], []
    cur = C.c_uint(0)

    def pull():
        n = C.c_int(0)
        buf = np.zeros((4096, s.record_stride), dtype=np.uint8)
        gpu.N.check(s.L.cz_search_drain_records(s.h, C.byref(cur), buf.ctypes.data, 4096, C.byref(n), s._stream()), "drain")
        for i in range(n.value):
            turns = int(buf[i, 4:8].view(np.int32)[0])
            recs.append(buf[i, :16 + 2 * turns].tobytes())
        gpu.N.check(s.L.cz_search_drain_visits(s.h, None, 0, C.byref(n), None, s._stream()), "count")
        vbuf = np.zeros((max(1, n.value), gpu.S.VISIT_STRIDE), dtype=np.uint8)
        qbuf = np.full(max(1, n.value), fill, dtype=np.float64)
        sbuf = np.full(max(1, n.value), fill, dtype=np.float64)
        st = s._stream()
        if drain == "plain":
            gpu.N.check(s.L.cz_search_drain_visits(s.h, vbuf.ctypes.data, n.value, C.byref(n), None, st), "visits")
        elif drain == "q":
            gpu.N.check(s.L.cz_search_drain_visits_q(s.h, vbuf.ctypes.data, qbuf.ctypes.data, n.value, C.byref(n), None, st),
                        "visits_q")
        else:
            gpu.N.check(s.L.cz_search_drain_visits_qs(s.h, vbuf.ctypes.data, qbuf.ctypes.data if drain == "qs" else None,
                                                      sbuf.ctypes.data, n.value, C.byref(n), None, st), "visits_qs")
        for i in range(n.value):
            ne = int(vbuf[i, 6])
            row = vbuf[i, :16 + 2 * ne].tobytes() + vbuf[i, 16 + 256:16 + 256 + 4 * ne].tobytes()
            entries.append((row, qbuf[i:i + 1].tobytes(), sbuf[i:i + 1].tobytes()))
    for r in range(rounds):
        s.round()
        p, v = ev(s.planes)
        s.policy.copy_(p)
        s.value.copy_(v)
        if r % 16 == 15:
            pull()
    pull()
    ctr = s.counters()
    s.close()
    if no_drops:
        assert ctr["visits_dropped"] == 0
    return sorted(recs), sorted(entries), ctr
