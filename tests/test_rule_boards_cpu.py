"""CPU: the host build of the lane-per-board rules (csrc/xq_tpb.h through tests/lane_harness.cpp, as in test_lane_cpu.py)
against the oracle on the board families of tests/rule_boards.py -- the boards test_gpu_rules_paths.py sends to the device.  A
failure here is rule logic; one that shows on the GPU only is device glue.  Also the coverage the GPU tests rely on, asserted on
the inputs, so that a change of seed or of the generator cannot quietly empty a case."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rule_boards as rb  # noqa: E402
from oracle import xq_oracle as xo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20000
SEED_LEGAL, SEED_OVERFULL = 1, 2          # the seeds test_gpu_rules_paths.py uses too
TPB_ROW_CAP = 64                          # csrc/xq_kernels.hip: the list capacity k_rules_tpb passes to tpb_rules
FLAGS = ("over", "v", "final_move", "check")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("lane") / "liblane.so"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "lane_harness.cpp"), "-o", str(out)])
    return C.CDLL(str(out))


@pytest.fixture(scope="module")
def families():
    """name -> (boards, the oracle's outputs), computed once"""
    fam = {"directed": rb.directed(), "legal_placement": rb.legal_placement(SEED_LEGAL, N),
           "overfull": rb.overfull(SEED_OVERFULL, N)}
    return {k: (b, xo.batch_rules(b, want_planes=False)) for k, b in fam.items()}


def _host(harness, boards, need_check, cap):
    n = len(boards)
    boards = np.ascontiguousarray(boards)
    lab = np.zeros((n, rb.MAXMOVES), dtype=np.uint16)
    counts = np.zeros(n, dtype=np.int32)
    out = np.zeros((n, 4), dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    harness.tpb_boards(vp(boards), n, int(need_check), int(cap), vp(lab), vp(counts), vp(out))
    return dict(moves=lab, counts=counts, over=out[:, 0], v=out[:, 1], final_move=out[:, 2], check=out[:, 3])


def _first_bad(boards, bad):
    i = int(np.flatnonzero(bad)[0])
    return i, xo.board_to_state(boards[i])


def test_the_domain_filter():
    """what the families drop and keep: more than 128 moves for either side, a piece off its squares"""
    open_rooks = np.zeros(90, dtype=np.int8)
    open_rooks[[4, 85]] = [rb.KING, -rb.KING]
    open_rooks[[9 * y + x for y, x in zip(range(1, 9), (0, 1, 2, 3, 5, 6, 7, 8))]] = rb.ROOK      # 8 rooks, no two in a line
    assert rb.placement_legal(open_rooks).all() and rb.raw_counts(open_rooks)[0] > rb.MAXMOVES
    assert not rb.in_domain(open_rooks).any() and not rb.in_domain(rb.flipped(open_rooks)).any()
    # the example of DESIGN.md: elephants, a king and a pawn where they can never stand
    off = xo.state_to_board('9/e7s/5E3/1CS6/1E6C/9/9/3E1S3/SK3k3/3E1p3')
    off[(off == rb.KING) & (np.arange(90) != 56)] = 0
    assert (off == rb.KING).sum() == 1 and not rb.placement_legal(off).any()
    assert rb.in_domain(rb.directed()).all()
    for fam, seed in ((rb.legal_placement, SEED_LEGAL), (rb.overfull, SEED_OVERFULL)):
        boards = fam(seed, N)
        assert rb.placement_legal(boards).all()
        assert len(boards) + rb.dropped(fam, seed, N) == N and rb.dropped(fam, seed, N) <= N // 100
        assert ((boards == rb.KING).sum(axis=1) == 1).all() and ((boards == -rb.KING).sum(axis=1) == 1).all()
        assert np.array_equal(boards, fam(seed, N)) and not boards.flags.writeable
    assert np.array_equal(rb.legal_placement(SEED_LEGAL, 50), rb.legal_placement(SEED_LEGAL, 50))
    assert not np.array_equal(rb.legal_placement(SEED_LEGAL, 50), rb.legal_placement(SEED_LEGAL + 1, 50))


def test_coverage_of_the_families(families):
    legal, exp = families["legal_placement"]
    counts = rb.raw_counts(legal)
    assert (counts == exp["counts"]).all()
    for k, sel in rb.with_move_count(legal).items():
        assert len(sel) >= 20 and (rb.raw_counts(sel) == k).all(), (k, len(sel))
    for t, cap in rb.REAL_COUNTS.items():
        assert (legal == t).sum(axis=1).max() == cap and (legal == -t).sum(axis=1).max() == cap
    over_b, over_e = families["overfull"]
    many, of_one = rb.takes_generic_path(over_b)
    assert many.sum() >= 1000 and of_one.sum() >= 1000
    assert (~many & of_one).sum() >= 20 and (many & ~of_one).sum() >= 20        # each condition on its own too
    assert (~many & ~of_one).sum() >= 20                                        # and overfull boards on the per-type path
    long_generic = (many | of_one) & (over_e["counts"] > TPB_ROW_CAP)
    assert long_generic.sum() >= 100
    for k in (63, 64, 65, 66):
        assert ((over_e["counts"] == k) & (many | of_one)).sum() >= 20, k
    for name in ("legal_placement", "overfull"):
        e = families[name][1]
        assert set(np.unique(e["check"])) == {0, 1}, name
        assert (e["final_move"] != xo.NOMOVE).any() and (e["final_move"] == xo.NOMOVE).any(), name
        assert set(np.unique(e["over"])) == {0, 1}, name
    v = np.concatenate([families[k][1]["v"] for k in families])
    assert set(np.unique(v)) == {-1, 0, 1}
    d = families["directed"][1]
    assert set(np.unique(d["v"])) == {-1, 0, 1} and set(np.unique(d["check"])) == {0, 1}
    assert d["counts"].max() > TPB_ROW_CAP and d["counts"].min() == 0


def test_directed_boards_are_what_their_names_say(families):
    boards, e = families["directed"]
    row = dict(zip(rb.directed_names(), range(len(boards))))
    got = lambda name: (int(e["over"][row[name]]), int(e["v"][row[name]]), int(e["check"][row[name]]))
    assert got("empty") == (1, 1, 0) and got("mover without a king") == (1, -1, 0)
    assert got("opponent without a king") == (1, 1, 0) and got("neither king") == (1, 1, 0)
    assert got("kings facing, 0 blockers") == (1, 1, 0) and e["final_move"][row["kings facing, 0 blockers"]] == xo.NOMOVE
    assert got("kings facing, 1 blocker") == (0, 0, 0) and got("kings facing, 2 blockers") == (0, 0, 0)
    assert got("kings on different files") == (0, 0, 0)
    assert got("kings facing, the only blocker beside the opponent's king") == (0, 0, 0)
    assert got("kings facing, the only blocker beside the mover's king") == (0, 0, 0)
    assert got("kings facing on file 3, a rook behind") == (1, 1, 0)
    assert got("kings facing, blocker beside the file only") == (1, 1, 0)

    def to(name, x, y):                                       # where the piece on (x, y) can go, as "xy" strings
        return sorted(xo.label_str(m)[2:] for m in xo.legal_moves_board(boards[row[name]]) if xo.label_str(m)[:2] == "%d%d" % (x, y))

    assert "07" in to("cannon over a screen on file 0", 0, 0) and "89" in to("cannon over a screen on file 8", 8, 2)
    for name, (x, y), quiet in (("cannon with its screens on the edge files", (4, 5), 14),
                                ("cannon with its screens on the edge ranks", (1, 4), 15)):
        b = boards[row[name]]
        assert len(to(name, x, y)) == quiet and all(b[9 * int(t[1]) + int(t[0])] == 0 for t in to(name, x, y)), name   # no capture
    jumps = {"(4,3)": {"32", "52"}, "(5,4)": {"63", "65"}, "(4,5)": {"36", "56"}, "(3,4)": {"23", "25"}}
    every = {"32", "52", "63", "65", "36", "56", "23", "25"}
    for leg, gone in jumps.items():
        assert set(to("knight, leg %s blocked" % leg, 4, 4)) == every - gone, leg
    assert to("knight in the corner", 0, 0) == ["12", "21"] and to("knight in the corner", 8, 9) == ["68", "77"]
    assert to("elephant, one eye blocked", 2, 0) == ["02"]
    assert to("elephant at the river", 2, 4) == ["02", "42"] and to("elephant at the river", 6, 4) == ["82"]
    assert to("pawn on the last rank, x = 0", 0, 9) == ["19"] and to("pawn on the last rank, x = 8", 8, 9) == ["79"]
    assert to("pawn before and after the river", 2, 4) == ["25"] and to("pawn before and after the river", 6, 5) == ["55", "66", "75"]
    assert xo.label_str(e["final_move"][row["pawn on the last rank, x = 4: takes the king sideways"]]) == "4959"
    k = "king taken by the later type first"
    assert xo.label_str(e["final_move"][row[k]]) == "3749" and "49" in to(k, 4, 8)
    assert got("in check by the cannon in front of a blocked rook") == (0, 0, 1)
    assert got("not in check: two screens before the cannon") == (0, 0, 0)
    assert got("in check by a pawn beside the king") == (0, 0, 1)


@pytest.mark.parametrize("name", ["directed", "legal_placement", "overfull"])
def test_host_build_matches_the_oracle(harness, families, name):
    """tpb_rules with need_check = 1 and the full list: all 128 slots, the count, over, v, final_move and check, bit for bit"""
    boards, exp = families[name]
    got = _host(harness, boards, 1, rb.MAXMOVES)
    assert (got["counts"] == exp["counts"]).all(), _first_bad(boards, got["counts"] != exp["counts"])
    bad = (got["moves"] != exp["moves"]).any(axis=1)
    assert not bad.any(), _first_bad(boards, bad)
    for k in FLAGS:
        assert (got[k] == exp[k]).all(), (k, _first_bad(boards, got[k] != exp[k]))
    # need_check = 0: the same but no check flag
    got0 = _host(harness, boards, 0, rb.MAXMOVES)
    assert (got0["check"] == 0).all()
    for k in ("moves", "counts", "over", "v", "final_move"):
        assert np.array_equal(got0[k], got[k]), k


@pytest.mark.parametrize("name", ["directed", "legal_placement", "overfull"])
def test_host_build_with_the_kernels_row_capacity(harness, families, name):
    """the kernel's own call, cap = TPB_ROW_CAP: the count is still the full count, the first 64 labels are the oracle's first
    64, nothing is stored behind them, and the flags (final_move may be a move past the row) do not change"""
    boards, exp = families[name]
    got = _host(harness, boards, 1, TPB_ROW_CAP)
    assert (got["counts"] == exp["counts"]).all(), _first_bad(boards, got["counts"] != exp["counts"])
    bad = (got["moves"][:, :TPB_ROW_CAP] != exp["moves"][:, :TPB_ROW_CAP]).any(axis=1)
    assert not bad.any(), _first_bad(boards, bad)
    assert (got["moves"][:, TPB_ROW_CAP:] == xo.NOMOVE).all()
    for k in FLAGS:
        assert (got[k] == exp[k]).all(), (k, _first_bad(boards, got[k] != exp[k]))
    if name != "directed":
        # a king taken by a move that the row no longer holds: the flags come from the generator, not from the row
        idx = np.array([np.flatnonzero(exp["moves"][i] == exp["final_move"][i])[0] if exp["final_move"][i] != xo.NOMOVE else -1
                        for i in np.flatnonzero(exp["counts"] > TPB_ROW_CAP)])
        assert (idx >= TPB_ROW_CAP).sum() >= 3, name
