"""One raw self-play loop for the "off means off" tests of the visit entries and their side columns: the bytes the device
rings hand out, through the library's own drain entry points, with nothing of the Python binding's sorting in between."""
import ctypes as C

import numpy as np

from test_gpu_search import stub_eval

SPEC = dict(kind="hash", salt=5)
COLS = ("q", "s", "maxq")                                   # CZ_VISIT_COL_* order


def drain_cols(s, host, cols, max_entries, n_out):
    """cz_search_drain_visits_cols of the Search s on numpy buffers -> its return code.  host: the entries' array or None;
    cols: one float64 array or None per column of COLS; n_out: C.byref of a c_int, or None."""
    ptrs = (C.c_void_p * len(COLS))(*[c.ctypes.data if c is not None else None for c in cols])
    return s.L.cz_search_drain_visits_cols(s.h, host.ctypes.data if host is not None else None, ptrs, max_entries, n_out,
                                           None, s._stream())


def selfplay_raw(gpu, pc, seed, rounds, G, setup_before=None, setup_after=None, capacity=0, playout_cap=None,
                 columns=(), fill=0.0, no_drops=True):
    """`rounds` rounds of G self-play games against the hash stub, drained every 16 rounds (before either ring can fill at
    the default capacity).  setup_before(s) / setup_after(s) run before / after the visit ring is switched on with
    `capacity`; playout_cap = (fast_sims, full_rate).  columns, drawn from COLS: the side columns that
    cz_search_drain_visits_cols is asked for, () = the plain cz_search_drain_visits; a buffer that is not asked for keeps
    `fill`.  no_drops: assert that the ring lost nothing.

    Returns (records, entries, counters).  A record is its 16-byte header and the `turns` moves it holds; an entry (row, q
    bytes, s bytes, maxq bytes), row = its 16-byte header and the n_edges labels and counts it holds (the ring slot's other bytes
    belong to no entry).  Both sorted: games that end in one launch reach the rings in any order."""
    assert set(columns) <= set(COLS)
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
        side = np.full((len(COLS), max(1, n.value)), fill, dtype=np.float64)
        st = s._stream()
        if columns:
            want = [side[k] if c in columns else None for k, c in enumerate(COLS)]
            gpu.N.check(drain_cols(s, vbuf, want, n.value, C.byref(n)), "visits_cols")
        else:
            gpu.N.check(s.L.cz_search_drain_visits(s.h, vbuf.ctypes.data, n.value, C.byref(n), None, st), "visits")
        for i in range(n.value):
            ne = int(vbuf[i, 6])
            row = vbuf[i, :16 + 2 * ne].tobytes() + vbuf[i, 16 + 256:16 + 256 + 4 * ne].tobytes()
            entries.append((row,) + tuple(side[k, i:i + 1].tobytes() for k in range(len(COLS))))
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
