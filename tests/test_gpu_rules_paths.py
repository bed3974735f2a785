"""-m gpu: the rule kernels' PATHS against the oracle, bit for bit (test_gpu_rules.py beside this file is thorough about
positions; every batch it compares has at least 420 boards, which is one of two forms).

csrc/xq_kernels.hip has two forms of move-gen / done / fused rules, chosen by batch size: below CZ_TPB_MIN_BOARDS = 256 one
wavefront per board (k_rules_fused, k_movegen, k_done on xq_rules.h), from 256 boards one lane per board (k_rules_tpb<DT> on
xq_tpb.h, then k_movegen_fix for lists longer than the TPB_ROW_CAP = 64 labels of an LDS row).  Here: the same boards through
both forms, the batch sizes around the switch and around a 64-board block with guard rows behind n, the four plane types of the
lane form, lists of 63 .. 66 moves on chosen lanes, the lane form's generic generator (more than 24 pieces, more than 9 of a
type), the catch kernels on whole move lists, and the grid-stride iterations of the wave kernels that grid_for caps at 8192
workgroups.  The boards come from tests/rule_boards.py (placement-legal, at most 128 moves per side: the kernels' domain) and
pass through the host build of xq_tpb.h in test_rule_boards_cpu.py, so a failure here alone is device glue.

Every output buffer is pre-filled with 0x5A bytes and has GUARD rows behind n: a kernel that skips a row, or writes one too
many, shows (the caching allocator would otherwise hand a kernel the right answers of the call before it)."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rule_boards as rb  # noqa: E402
from oracle import xq_oracle as xo  # noqa: E402

pytestmark = pytest.mark.gpu

SEED_LEGAL, SEED_OVERFULL = 1, 2          # as in test_rule_boards_cpu.py
MIN_TPB, ROW_CAP, WAVE_GRID = 256, 64, 8192      # CZ_TPB_MIN_BOARDS, TPB_ROW_CAP, grid_for's cap (csrc/xq_kernels.hip)
FILL, GUARD = 0x5A, 64
KEYS = ("moves", "counts", "over", "v", "final_move", "check", "planes")
OPENING = xo.state_to_board(xo.INIT_STATE)


@pytest.fixture(scope="module")
def nat():
    import torch
    from cchess_alphazero import _native
    _native.require_gpu()
    return _native, torch


@pytest.fixture(scope="module")
def fam(positions_1k):
    """name -> (boards, the oracle's outputs): computed once, read-only"""
    boards = {"directed": rb.directed(), "legal_placement": rb.legal_placement(SEED_LEGAL, 2000),
              "overfull": rb.overfull(SEED_OVERFULL, 2000),
              "golden": np.stack([xo.state_to_board(r["state"]) for r in positions_1k])}
    return {k: (b, xo.batch_rules(b)) for k, b in boards.items()}


@pytest.fixture(scope="module")
def edge_boards():
    """count -> boards with 63, 64, 65, 66 moves: of a game's piece counts, and overfull ones on the generic generator"""
    legal = rb.with_move_count(rb.legal_placement(SEED_LEGAL, 20000))
    over = rb.overfull(SEED_OVERFULL, 2000)
    many, of_one = rb.takes_generic_path(over)
    generic = rb.with_move_count(over[many | of_one])
    assert all(len(v) >= 20 for v in legal.values()) and all(len(v) >= 3 for v in generic.values())
    return {"legal_placement": legal, "overfull": generic}


# ---- launches into guarded buffers ---------------------------------------------------------------------------------------
def _up(torch, a):
    return torch.from_numpy(np.array(a)).cuda()          # a copy: the families are read-only


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class _Guarded:
    """byte buffers of n + GUARD rows filled with FILL; typed views of the first n rows go to the kernel"""

    def __init__(self, torch, n, **row_bytes):
        self.torch, self.n = torch, n
        self.raw = {k: torch.full((n + GUARD, b), FILL, dtype=torch.uint8, device="cuda") for k, b in row_bytes.items()}

    def view(self, k, dtype, *shape):
        return self.raw[k].view(dtype).view(self.n + GUARD, *shape)[:self.n]

    def check_guard(self, what):
        self.torch.cuda.synchronize()
        for k, r in self.raw.items():
            assert bool((r[self.n:] == FILL).all()), (what, k, "rows behind n were written")


def _fused(nat, boards, dtype=None, bits=False):
    """cz_rules_fused through _native.rules_fused(out=...); planes come back as float32 (bits: the raw 16-bit words too)"""
    N, torch = nat
    dtype = N.F32 if dtype is None else dtype
    n, esz = len(boards), {N.F32: 4, N.F16: 2, N.BF16: 2, N.U8: 1}[dtype]
    g = _Guarded(torch, n, moves=256, counts=1, over=1, v=1, final_move=2, check=1, planes=1260 * esz)
    out = dict(moves=g.view("moves", torch.uint16, 128), counts=g.view("counts", torch.uint8),
               over=g.view("over", torch.int8), v=g.view("v", torch.int8), final_move=g.view("final_move", torch.uint16),
               check=g.view("check", torch.uint8), planes=g.view("planes", N.torch_dtype(dtype), 14, 10, 9))
    N.rules_fused(_up(torch, boards), dtype, out=out)
    g.check_guard("cz_rules_fused n = %d" % n)
    res = {k: out[k].cpu().numpy() for k in KEYS if k != "planes"}
    res["planes"] = out["planes"].float().cpu().numpy()
    if bits:
        res["planes_bits"] = out["planes"].view(torch.int16).cpu().numpy().view(np.uint16)
    return res


def _movegen(nat, boards):
    """cz_movegen, the C ABI directly"""
    N, torch = nat
    n = len(boards)
    g = _Guarded(torch, n, moves=256, counts=1)
    mv, ct = g.view("moves", torch.uint16, 128), g.view("counts", torch.uint8)
    bd = _up(torch, boards)
    N.check(N.lib().cz_movegen(_ptr(bd), n, _ptr(mv), _ptr(ct), N._stream()), "cz_movegen")
    g.check_guard("cz_movegen n = %d" % n)
    return dict(moves=mv.cpu().numpy(), counts=ct.cpu().numpy())


def _done(nat, boards, need_check):
    """cz_done, the C ABI directly; without need_check the check pointer is NULL (include/czero.h)"""
    N, torch = nat
    n = len(boards)
    g = _Guarded(torch, n, over=1, v=1, final_move=2, check=1)
    o, v, fm = g.view("over", torch.int8), g.view("v", torch.int8), g.view("final_move", torch.uint16)
    ck = g.view("check", torch.uint8)
    bd = _up(torch, boards)
    N.check(N.lib().cz_done(_ptr(bd), n, int(need_check), _ptr(o), _ptr(v), _ptr(fm), _ptr(ck) if need_check else None,
                            N._stream()), "cz_done")
    g.check_guard("cz_done n = %d" % n)
    res = dict(over=o.cpu().numpy(), v=v.cpu().numpy(), final_move=fm.cpu().numpy())
    if need_check:
        res["check"] = ck.cpu().numpy()
    else:
        assert bool((g.raw["check"] == FILL).all())
    return res


def _in_slices(fn, boards, size=MIN_TPB - 1):
    """fn on slices of at most 255 boards (the wave-per-board form), joined"""
    parts = [fn(boards[i:i + size]) for i in range(0, len(boards), size)]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _tiled(a, n):
    return np.concatenate([a] * (-(-n // len(a))))


def _same(got, exp, keys, what):
    for k in keys:
        bad = got[k] != exp[k]
        assert not bad.any(), (what, k, "first bad row %d of %d" % (np.argwhere(bad)[0][0], len(bad)))


# ---- 1. form against form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["directed", "legal_placement", "overfull", "golden"])
def test_both_forms_on_the_same_boards(nat, fam, positions_1k, name):
    boards, exp = fam[name]
    if len(boards) <= MIN_TPB:                      # the written-out boards: repeated until the lane form takes them
        boards = _tiled(boards, MIN_TPB + 1)
        exp = {k: _tiled(v, MIN_TPB + 1) for k, v in exp.items()}
    no_check = ("over", "v", "final_move")
    for label, fn, keys in (("rules_fused", lambda b: _fused(nat, b), KEYS),
                            ("movegen", lambda b: _movegen(nat, b), ("moves", "counts")),
                            ("done(need_check=True)", lambda b: _done(nat, b, True), no_check + ("check",)),
                            ("done(need_check=False)", lambda b: _done(nat, b, False), no_check)):
        wave, lane = _in_slices(fn, boards), fn(boards)
        _same(wave, exp, keys, (name, label, "wave form against the oracle"))
        _same(lane, exp, keys, (name, label, "lane form against the oracle"))
        _same(wave, lane, keys, (name, label, "wave form against lane form"))       # all 128 slots, 0xFFFF fill included
        if label == "rules_fused" and name == "golden":
            for i, r in enumerate(positions_1k):                                    # as test_golden_suite_fused, wave form
                c = wave["counts"][i]
                assert " ".join(xo.label_str(int(m)) for m in wave["moves"][i, :c]) == r["moves"], r["state"]
                assert (wave["moves"][i, c:] == 0xFFFF).all()
                d = r["done"]
                assert bool(wave["over"][i]) == d[0] and int(wave["v"][i]) == d[1], r["state"]
                assert (None if wave["final_move"][i] == 0xFFFF else xo.label_str(int(wave["final_move"][i]))) == d[2]
                if len(d) > 3:
                    assert bool(wave["check"][i]) == d[3]
                assert zlib.crc32(wave["planes"][i].tobytes()) & 0xFFFFFFFF == r["planes_crc"]
    # the wrappers of cchess_alphazero/_native.py (their own buffers), lane form
    N, torch = nat
    bd = _up(torch, boards)
    mv, ct = N.movegen(bd)
    assert (mv.cpu().numpy() == exp["moves"]).all() and (ct.cpu().numpy() == exp["counts"]).all()
    for need_check in (True, False):
        o, v, fm, ck = (t.cpu().numpy() for t in N.done(bd, need_check=need_check))
        assert (o == exp["over"]).all() and (v == exp["v"]).all() and (fm == exp["final_move"]).all()
        assert (ck == (exp["check"] if need_check else 0)).all()


def test_the_generic_generator_runs_on_the_device(fam):
    """the overfull boards of the test above reach tpb_movegen_generic (more than 24 pieces) and the fallback of type_lists
    (more than 9 of one type) in the lane form, with long lists among them"""
    boards, exp = fam["overfull"]
    many, of_one = rb.takes_generic_path(boards)
    assert (many | of_one).sum() >= 1000 and many.sum() >= 1000 and of_one.sum() >= 1000
    assert (~many & of_one).sum() >= 2 and (many & ~of_one).sum() >= 2 and (~many & ~of_one).sum() >= 2
    assert ((many | of_one) & (exp["counts"] > ROW_CAP)).sum() >= 20
    many_opp, of_one_opp = rb.takes_generic_path(rb.flipped(boards))           # tpb_opponent_reaches: the opponent's lists
    assert (of_one_opp & (exp["over"] == 0)).sum() >= 100 and (~of_one_opp & (exp["over"] == 0)).sum() >= 20
    assert set(np.unique(exp["check"][of_one_opp & (exp["over"] == 0)])) == {0, 1}


# ---- 2. the switch and the tails -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 319, 320, 321])
def test_batch_sizes_around_the_switch_and_the_block(nat, fam, n):
    """prefixes of one array; the guard rows behind n are checked inside _fused / _movegen / _done"""
    boards, exp = fam["legal_placement"]
    boards, exp = boards[:n], {k: v[:n] for k, v in exp.items()}
    _same(_fused(nat, boards), exp, KEYS, ("rules_fused", n))
    _same(_movegen(nat, boards), exp, ("moves", "counts"), ("movegen", n))
    _same(_done(nat, boards, True), exp, ("over", "v", "final_move", "check"), ("done, need_check", n))
    _same(_done(nat, boards, False), exp, ("over", "v", "final_move"), ("done", n))


# ---- 3. the plane types --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [MIN_TPB - 1, 321])
def test_plane_types(nat, fam, n):
    """k_rules_tpb<DT> (n = 321) and k_rules_fused<DT> (n = 255) for the four plane types: the planes as numbers, the 16-bit
    types as bits (1.0 = 0x3C00 / 0x3F80), every other output the same for all four"""
    N, _ = nat
    boards, exp = fam["legal_placement"]
    boards, exp = boards[:n], {k: v[:n] for k, v in exp.items()}
    ones = {N.F16: 0x3C00, N.BF16: 0x3F80}
    first = None
    for dtype in (N.F32, N.F16, N.BF16, N.U8):
        got = _fused(nat, boards, dtype, bits=dtype in ones)
        _same(got, exp, KEYS, ("rules_fused", n, dtype))
        if dtype in ones:
            want = np.where(exp["planes"] == 1.0, ones[dtype], 0).astype(np.uint16)
            assert (got["planes_bits"] == want).all(), (n, dtype)
        first = first or got
        for k in KEYS:
            assert np.array_equal(got[k], first[k]), (n, dtype, k)


# ---- 4. the 64-move edge -------------------------------------------------------------------------------------------------
def _check_lists(nat, boards, what):
    exp = xo.batch_rules(boards)
    long_rows = np.flatnonzero(exp["counts"] > ROW_CAP)
    for label, got, keys in (("rules_fused", _fused(nat, boards), KEYS), ("movegen", _movegen(nat, boards), ("moves", "counts"))):
        _same(got, exp, keys, (what, label))
        for i in long_rows:                                     # a fix-up that never ran leaves the first 64 right
            c = int(exp["counts"][i])
            assert (got["moves"][i, ROW_CAP:c] == exp["moves"][i, ROW_CAP:c]).all(), (what, label, i)
            assert (got["moves"][i, ROW_CAP:c] != 0xFFFF).all() and (got["moves"][i, c:] == 0xFFFF).all(), (what, label, i)
    return exp


@pytest.mark.parametrize("family", ["legal_placement", "overfull"])
@pytest.mark.parametrize("count", [63, 64, 65, 66])
def test_lists_around_a_row_on_chosen_lanes(nat, edge_boards, family, count):
    """320 opening positions (44 moves) with boards of `count` moves on lane 0, lane 63, and the first and last lane of later
    blocks, the last block included"""
    sel = edge_boards[family][count]
    boards = np.tile(OPENING, (320, 1))
    places = (0, 63, 64, 255, 256, 319)
    for j, i in enumerate(places):
        boards[i] = sel[j % len(sel)]
    exp = _check_lists(nat, boards, (family, count))
    assert (exp["counts"][list(places)] == count).all() and (np.delete(exp["counts"], places) == 44).all()


@pytest.mark.parametrize("family", ["legal_placement", "overfull"])
def test_a_whole_block_and_a_single_tail_board_of_long_lists(nat, edge_boards, family):
    sel = edge_boards[family]
    block = np.stack([sel[63 + j % 4][(j // 4) % len(sel[63 + j % 4])] for j in range(64)])     # 63, 64, 65, 66, 63, ...
    boards = np.tile(OPENING, (320, 1))
    boards[64:128] = block
    exp = _check_lists(nat, boards, (family, "block 1 of 5"))
    assert (exp["counts"][64:128] == np.tile([63, 64, 65, 66], 16)).all()
    only_long = np.stack([sel[65 + j % 2][(j // 2) % len(sel[65 + j % 2])] for j in range(MIN_TPB)])
    exp = _check_lists(nat, only_long, (family, "every board long"))
    assert (exp["counts"] > ROW_CAP).all()
    tail = np.tile(OPENING, (257, 1))
    tail[256] = sel[65][0]
    exp = _check_lists(nat, tail, (family, "n = 257, tail board long"))
    assert exp["counts"][256] == 65 and (exp["counts"][:256] == 44).all()


# ---- 5. the catch kernels on whole move lists ----------------------------------------------------------------------------
def _all_moves(boards):
    """every (board, legal move) pair of the boards"""
    e = xo.batch_rules(boards, want_planes=False)
    rows = np.repeat(np.arange(len(boards)), e["counts"])
    moves = np.concatenate([e["moves"][i, :c] for i, c in enumerate(e["counts"])])
    return np.ascontiguousarray(boards[rows]), moves.astype(np.uint16)


def _oracle_catch(boards, moves):
    L = xo.lib()
    p = lambda b: b.ctypes.data_as(C.POINTER(C.c_int8))
    wcc = np.array([L.xqo_will_check_or_catch(p(b), int(m)) for b, m in zip(boards, moves)], dtype=np.uint8)
    bc = np.array([L.xqo_be_catched(p(b), int(m)) for b, m in zip(boards, moves)], dtype=np.uint8)
    return wcc, bc


def _device_catch(nat, boards, moves):
    N, torch = nat
    n = len(boards)
    g = _Guarded(torch, n, wcc=1, bc=1)
    w, b = g.view("wcc", torch.uint8), g.view("bc", torch.uint8)
    bd = _up(torch, boards)
    mv = _up(torch, moves.view(np.int16)).view(torch.uint16)
    N.check(N.lib().cz_check_or_catch(_ptr(bd), _ptr(mv), n, _ptr(w), N._stream()), "cz_check_or_catch")
    N.check(N.lib().cz_be_catched(_ptr(bd), _ptr(mv), n, _ptr(b), N._stream()), "cz_be_catched")
    g.check_guard("catch kernels n = %d" % n)
    return w.cpu().numpy(), b.cpu().numpy()


@pytest.mark.parametrize("name", ["directed", "legal_placement", "golden cases"])
def test_catch_kernels_on_every_legal_move(nat, fam, catch_cases, name):
    """will_check_or_catch and be_catched for EVERY move of each board (the list is in square order: its first entries, which
    test_gpu_rules.py samples, are always moves of the pieces on the lowest squares)"""
    if name == "golden cases":
        boards = np.stack([xo.state_to_board(c["state"]) for c in catch_cases])
    else:
        boards = fam[name][0][:300]
    boards, moves = _all_moves(boards)
    assert len(moves) > 400
    ew, eb = _oracle_catch(boards, moves)
    assert set(np.unique(ew)) == {0, 1} and set(np.unique(eb)) == {0, 1}
    gw, gb = _device_catch(nat, boards, moves)
    assert (gw == ew).all(), (name, "check_or_catch", int(np.flatnonzero(gw != ew)[0]))
    assert (gb == eb).all(), (name, "be_catched", int(np.flatnonzero(gb != eb)[0]))


# ---- 6. the grid stride of the wave kernels ------------------------------------------------------------------------------
def test_wave_kernels_past_their_grid(nat, fam):
    """encode (four types), has_attack, check_or_catch, be_catched at n = 8192 + 37: grid_for launches 8192 workgroups, so 37 of
    them run a second iteration on the LDS of the first.  600 distinct (board, move) pairs, tiled so that the two iterations of
    a workgroup see different boards; rows compared with the oracle and with the same call on the 600 pairs alone."""
    N, torch = nat
    n, distinct = WAVE_GRID + 37, 600
    pool = np.concatenate([fam["directed"][0], fam["legal_placement"][0][:700]])
    counts = rb.raw_counts(pool)
    pool, counts = pool[counts > 0][:distinct], counts[counts > 0][:distinct]
    rng = np.random.default_rng(5)
    pick = (rng.random(distinct) * counts).astype(np.int64)
    moves = np.array([xo.legal_moves_board(b)[k] for b, k in zip(pool, pick)], dtype=np.uint16)
    idx = np.arange(n) % distinct
    assert (WAVE_GRID % distinct) != 0 and not (pool[idx[:37]] == pool[idx[WAVE_GRID:]]).all(axis=1).any()
    windows = np.concatenate([np.arange(300), np.arange(WAVE_GRID - 300, n)])       # the first rows; around 8192 and the last rows
    big, big_moves = np.ascontiguousarray(pool[idx]), np.ascontiguousarray(moves[idx])
    # the oracle on the distinct pairs; a window row's expectation is its pair's
    ew, eb = _oracle_catch(pool, moves)
    eh = np.array([xo.lib().xqo_has_attack_chessman(b.ctypes.data_as(C.POINTER(C.c_int8))) for b in pool], dtype=np.uint8)
    ep = xo.batch_rules(pool)["planes"]
    assert set(np.unique(eh)) == {0, 1} and set(np.unique(ew)) == {0, 1} and set(np.unique(eb)) == {0, 1}
    gw, gb = _device_catch(nat, big, big_moves)
    sw, sb = _device_catch(nat, pool, moves)
    for got, small, exp, what in ((gw, sw, ew, "check_or_catch"), (gb, sb, eb, "be_catched")):
        assert (got[windows] == exp[idx[windows]]).all(), what
        assert (got == small[idx]).all(), what
    bd, bd_small = _up(torch, big), _up(torch, pool)
    gh, sh = N.has_attack(bd).cpu().numpy(), N.has_attack(bd_small).cpu().numpy()
    assert (gh[windows] == eh[idx[windows]]).all() and (gh == sh[idx]).all()
    for dtype in (N.F32, N.F16, N.BF16, N.U8):
        g = _Guarded(torch, n, planes=1260 * {N.F32: 4, N.F16: 2, N.BF16: 2, N.U8: 1}[dtype])
        pl = g.view("planes", N.torch_dtype(dtype), 14, 10, 9)
        N.check(N.lib().cz_encode(_ptr(bd), n, _ptr(pl), dtype, N._stream()), "cz_encode")
        g.check_guard("cz_encode")
        small = N.encode(bd_small, dtype)
        assert torch.equal(pl, small[torch.from_numpy(idx).cuda()]), dtype
        assert (pl[torch.from_numpy(windows).cuda()].float().cpu().numpy() == ep[idx[windows]]).all(), dtype
