"""-m gpu: the library's half of the search options' exclusion matrix (the feature table of csrc/xq_search.hip) against the
Python table (cchess_alphazero/search_options.py EXCLUDES).  For every ordered pair (A, B) of the seven features, with A on,
B's C entry point is refused with CZ_ERR_ARG iff the Python table lists {A, B}, and the refusal reads `<B's entry point>: <A's
phrase>`; switching off is never refused.  The same for every ordered pair that involves one of the three rows with the larger
statistics blocks (moves-left utility, draw average, lower-confidence-bound move choice) against search_options.py's SIDE table.
One search object of 2 games, K = 4, 16 simulations; no round is run."""
import itertools
import types

import pytest

from cchess_alphazero import search_options as so
from test_gpu_search import gpu, play_config  # noqa: F401

pytestmark = pytest.mark.gpu
ERR_ARG = -1                                                # include/czero.h CZ_ERR_ARG


def _feature(entry, phrase, on, off, wrap_on, wrap_off):
    return types.SimpleNamespace(entry=entry, phrase=phrase, on=on, off=off, wrap_on=wrap_on, wrap_off=wrap_off)


# search_options key -> the C entry point, its phrase in a refusal, the raw on / off calls (L, handle, stream) and the
# wrapper's on / off calls
FEATURES = {
    "fast_sims": _feature("cz_search_set_playout_cap", "the playout cap is on (cz_search_set_playout_cap)",
                          lambda L, h, st: L.cz_search_set_playout_cap(h, 8, 0.25, st),
                          lambda L, h, st: L.cz_search_set_playout_cap(h, 0, 0.25, st),
                          lambda s: s.set_playout_cap(8, 0.25), lambda s: s.set_playout_cap(0)),
    "forced_playouts": _feature("cz_search_set_forced_playouts", "forced playouts are on (cz_search_set_forced_playouts)",
                                lambda L, h, st: L.cz_search_set_forced_playouts(h, 2.0, st),
                                lambda L, h, st: L.cz_search_set_forced_playouts(h, 0.0, st),
                                lambda s: s.set_forced_playouts(2.0), lambda s: s.set_forced_playouts(0.0)),
    "gumbel": _feature("cz_search_set_gumbel", "the Gumbel root search is on (cz_search_set_gumbel)",
                       lambda L, h, st: L.cz_search_set_gumbel(h, 8, 50.0, 1.0, st),
                       lambda L, h, st: L.cz_search_set_gumbel(h, 0, 50.0, 1.0, st),
                       lambda s: s.set_gumbel(8), lambda s: s.set_gumbel(0)),
    "solver": _feature("cz_search_set_solver", "the MCTS solver is on (cz_search_set_solver)",
                       lambda L, h, st: L.cz_search_set_solver(h, 1, st), lambda L, h, st: L.cz_search_set_solver(h, 0, st),
                       lambda s: s.set_solver(True), lambda s: s.set_solver(False)),
    "kld_gain": _feature("cz_search_set_kld_gain", "the KLD-gain stop is on (cz_search_set_kld_gain)",
                         lambda L, h, st: L.cz_search_set_kld_gain(h, 1e-3, 16, st),
                         lambda L, h, st: L.cz_search_set_kld_gain(h, 0.0, 16, st),
                         lambda s: s.set_kld_gain(1e-3, 16), lambda s: s.set_kld_gain(0.0)),
    "smart_pruning": _feature("cz_search_set_smart_pruning", "the unreachable-lead stop is on (cz_search_set_smart_pruning)",
                              lambda L, h, st: L.cz_search_set_smart_pruning(h, 1, st),
                              lambda L, h, st: L.cz_search_set_smart_pruning(h, 0, st),
                              lambda s: s.set_smart_pruning(True), lambda s: s.set_smart_pruning(False)),
    "eval_cache": _feature("cz_search_set_eval_cache", "the evaluation cache is on (cz_search_set_eval_cache)",
                           lambda L, h, st: L.cz_search_set_eval_cache(h, 10, st),
                           lambda L, h, st: L.cz_search_set_eval_cache(h, 0, st),
                           lambda s: s.set_eval_cache(10), lambda s: s.set_eval_cache(0)),
}
PAIRS = {frozenset(p[:2]) for p in so.EXCLUDES}
ATTRS = ("fast_sims", "forced_k", "gumbel_m", "gumbel_full", "eval_cache", "solver", "kld_gain", "kld_interval", "smart_pruning")


@pytest.fixture(scope="module")
def search(gpu):
    s = gpu.S.Search(play_config(simulation_num_per_move=16, search_threads=4), 2, seed=1)
    yield s
    s.close()


def _attrs(s):
    return {a: getattr(s, a, None) for a in ATTRS}


def _last_error(s):
    return s.L.cz_last_error().decode()


def test_the_features_here_are_the_python_tables():
    assert set().union(*PAIRS) == set(FEATURES) and len(PAIRS) == 11


@pytest.mark.parametrize("a, b", list(itertools.permutations(FEATURES, 2)))
def test_b_is_refused_beside_a_iff_the_python_table_lists_the_pair(gpu, search, a, b):
    s, L, A, B = search, search.L, FEATURES[a], FEATURES[b]
    st = s._stream()
    A.wrap_on(s)
    try:
        before = _attrs(s)
        rc = B.on(L, s.h, st)
        if frozenset((a, b)) in PAIRS:
            assert rc == ERR_ARG
            assert _last_error(s) == f"{B.entry}: {A.phrase}"
            with pytest.raises(gpu.N.NativeError):          # the wrapper is refused the same way and keeps its attributes
                B.wrap_on(s)
        else:
            assert rc == 0, _last_error(s)
        assert _attrs(s) == before
        assert B.off(L, s.h, st) == 0                       # switching off is never refused
        assert _attrs(s) == before
    finally:
        B.off(L, s.h, st)
        A.wrap_off(s)
    # everything is off again: each of the two goes on alone
    for f in (A, B):
        assert f.on(L, s.h, st) == 0 and f.off(L, s.h, st) == 0


def test_of_several_excluders_the_first_in_table_order_is_named(search):
    s, L = search, search.L
    st = s._stream()
    on = [FEATURES[k] for k in ("fast_sims", "kld_gain", "smart_pruning")]       # (these three compose)
    try:
        for f in on:
            f.wrap_on(s)
        assert L.cz_search_set_gumbel(s.h, 8, 50.0, 1.0, st) == ERR_ARG
        assert _last_error(s) == "cz_search_set_gumbel: the playout cap is on (cz_search_set_playout_cap)"
        assert s.gumbel_m == 0
        FEATURES["forced_playouts"].wrap_on(s)              # forced playouts come before the playout cap
        assert L.cz_search_set_gumbel(s.h, 8, 50.0, 1.0, st) == ERR_ARG
        assert _last_error(s) == "cz_search_set_gumbel: forced playouts are on (cz_search_set_forced_playouts)"
    finally:
        for f in on + [FEATURES["forced_playouts"]]:
            f.wrap_off(s)
    assert L.cz_search_set_gumbel(s.h, 8, 50.0, 1.0, st) == 0 and L.cz_search_set_gumbel(s.h, 0, 50.0, 1.0, st) == 0


# ---- the three rows of the larger statistics blocks (F_ML, F_DRAW, F_LCB) against search_options.SIDE ---------------------------
# Their raw calls need the rows the network would fill, so the dict is a fixture; its keys are SIDE's context names.
BLOCKS = ("moves_left", "draw", "lcb")
BLOCK_PAIRS = {frozenset((row.context, other)) for row in so.SIDE if row.context
               for other in [k for k, _ in row.excludes] + [earlier.context for earlier, _ in row.earlier]}
BLOCK_ATTRS = ATTRS + ("moves_left_slope", "moves_left_cap", "draw_on", "draw_score", "lcb", "lcb_min_ratio")


@pytest.fixture(scope="module")
def blocks(gpu, search):
    import ctypes as C
    t, d = gpu.torch, C.c_double
    x = t.zeros((search.slots,), dtype=t.float32, device="cuda")
    rows = t.zeros((search.slots, 3), dtype=t.float32, device="cuda")
    xp, rp = C.c_void_p(x.data_ptr()), C.c_void_p(rows.data_ptr())
    yield {
        "moves_left": _feature("cz_search_set_moves_left", "the moves-left utility is on (cz_search_set_moves_left)",
                               lambda L, h, st: L.cz_search_set_moves_left(h, d(0.01), d(0.1), xp, st),
                               lambda L, h, st: L.cz_search_set_moves_left(h, d(0.0), d(0.1), None, st),
                               lambda s: s.set_moves_left(0.01, 0.1), lambda s: s.set_moves_left(0.0)),
        "draw": _feature("cz_search_set_draw", "the draw average is on (cz_search_set_draw)",
                         lambda L, h, st: L.cz_search_set_draw(h, 1, d(0.25), rp, st),
                         lambda L, h, st: L.cz_search_set_draw(h, 0, d(0.0), None, st),
                         lambda s: s.set_draw(True, 0.25), lambda s: s.set_draw(False)),
        "lcb": _feature("cz_search_set_lcb", "the lower-confidence-bound move choice is on (cz_search_set_lcb)",
                        lambda L, h, st: L.cz_search_set_lcb(h, d(2.0), d(0.15), st),
                        lambda L, h, st: L.cz_search_set_lcb(h, d(0.0), d(0.15), st),
                        lambda s: s.set_lcb(2.0), lambda s: s.set_lcb(0.0)),
    }
    del x, rows


def test_the_block_rows_here_are_the_python_side_table():
    assert [r.context for r in so.SIDE if r.context] == list(BLOCKS)
    assert set().union(*BLOCK_PAIRS) <= set(FEATURES) | set(BLOCKS)
    by = {b: {next(iter(p - {b})) for p in BLOCK_PAIRS if b in p} for b in BLOCKS}
    lists = dict(moves_left=so.MOVES_LEFT_EXCLUDES, draw=so.DRAW_EXCLUDES, lcb=so.LCB_EXCLUDES)
    for b in BLOCKS:                                        # each list, and the other two of the three
        assert by[b] == {k for k, _ in lists[b]} | (set(BLOCKS) - {b})
    assert len(BLOCK_PAIRS) == 3 * 5 + 3


@pytest.mark.parametrize("a, b", [p for p in itertools.permutations(list(FEATURES) + list(BLOCKS), 2) if set(p) & set(BLOCKS)])
def test_a_block_row_is_refused_and_refuses_iff_the_python_lists_hold_the_pair(gpu, search, blocks, a, b):
    s, L = search, search.L
    A, B = ({**FEATURES, **blocks}[k] for k in (a, b))
    st = s._stream()
    attrs = lambda: {k: getattr(s, k, None) for k in BLOCK_ATTRS}
    A.wrap_on(s)
    try:
        before = attrs()
        rc = B.on(L, s.h, st)
        if frozenset((a, b)) in BLOCK_PAIRS:
            assert rc == ERR_ARG
            assert _last_error(s) == f"{B.entry}: {A.phrase}"
            with pytest.raises(gpu.N.NativeError):          # the wrapper is refused the same way and keeps its attributes
                B.wrap_on(s)
        else:
            assert rc == 0, _last_error(s)
        assert attrs() == before
        assert B.off(L, s.h, st) == 0                       # switching off is never refused
        assert attrs() == before
    finally:
        B.off(L, s.h, st)
        A.wrap_off(s)
    for f in (A, B):                                        # everything is off again: each of the two goes on alone
        assert f.on(L, s.h, st) == 0 and f.off(L, s.h, st) == 0


def test_the_block_rows_come_after_the_eight_in_table_order(search, blocks):
    """A block row is named only where no earlier row excludes the setter.  Of the rows that exclude cz_search_set_lcb no two can
    be on at once (each of them excludes the moves-left utility too), so its first excluder is its only one: the moves-left
    utility beside the playout cap, the evaluation cache beside the playout cap.  The order itself shows at
    cz_search_set_gumbel, which the playout cap (second row) and the moves-left utility (ninth) both exclude."""
    s, L = search, search.L
    st = s._stream()
    cap, cache, ml, lcb = FEATURES["fast_sims"], FEATURES["eval_cache"], blocks["moves_left"], blocks["lcb"]
    try:
        cap.wrap_on(s)                                      # (composes with all three)
        ml.wrap_on(s)
        assert lcb.on(L, s.h, st) == ERR_ARG and _last_error(s) == f"cz_search_set_lcb: {ml.phrase}"
        assert cache.on(L, s.h, st) == ERR_ARG and _last_error(s) == f"cz_search_set_eval_cache: {ml.phrase}"
        assert L.cz_search_set_gumbel(s.h, 8, 50.0, 1.0, st) == ERR_ARG
        assert _last_error(s) == f"cz_search_set_gumbel: {cap.phrase}"
        cap.wrap_off(s)
        assert L.cz_search_set_gumbel(s.h, 8, 50.0, 1.0, st) == ERR_ARG
        assert _last_error(s) == f"cz_search_set_gumbel: {ml.phrase}"
        ml.wrap_off(s)
        cap.wrap_on(s)
        cache.wrap_on(s)
        assert lcb.on(L, s.h, st) == ERR_ARG and _last_error(s) == f"cz_search_set_lcb: {cache.phrase}"
        assert (s.lcb, s.moves_left_slope) == (0.0, 0.0)
    finally:
        for f in (ml, cache, cap):
            f.wrap_off(s)
    assert lcb.on(L, s.h, st) == 0 and lcb.off(L, s.h, st) == 0


def test_the_full_gumbel_search_depends_on_the_gumbel_root_search(gpu, search):
    s, L = search, search.L
    st = s._stream()
    assert s.gumbel_m == 0
    assert L.cz_search_set_gumbel_full(s.h, 1, st) == ERR_ARG
    assert _last_error(s) == "cz_search_set_gumbel_full: the Gumbel root search is off (cz_search_set_gumbel)"
    assert L.cz_search_set_gumbel_full(s.h, 0, st) == 0
    with pytest.raises(gpu.N.NativeError):
        s.set_gumbel_full(True)
    assert s.gumbel_full is False
    try:
        s.set_gumbel(8)
        s.set_gumbel_full(True)
        assert s.gumbel_full is True
    finally:
        s.set_gumbel(0)                                     # clears the full search with it
    assert s.gumbel_full is False
    assert L.cz_search_set_gumbel_full(s.h, 1, st) == ERR_ARG
