"""tests/footprint.py tells a clean kernel from faulty ones.  The "kernels" are torch-CPU stand-ins for a compact-queue launch
y[i] = 2 x[rows[i]] + 1, i < m, over pairs of rows; each faulty one breaks the contract in one place and must be reported
there: a byte in front of the output, one behind it, row m, the second slot of a half-empty last pair, an owned output that
depends on input row m, and one that depends on a queue slot that rows[:m] does not name."""
import numpy as np
import pytest
import torch

import footprint as fp

N, M, SLOTS, W = 5, 3, 8, 6


def _f(x):
    return 2.0 * x + 1.0


def k_correct(x, rows, y, m):
    for i in range(m):
        y.view[i] = _f(x.view[int(rows.view[i])])


def k_front_guard(x, rows, y, m):
    k_correct(x, rows, y, m)
    y.buf[y.start - 1] ^= 0x5A


def k_back_guard(x, rows, y, m):
    k_correct(x, rows, y, m)
    y.buf[y.start + y.nbytes + 300] ^= 0x5A


def k_row_m(x, rows, y, m):
    k_correct(x, rows, y, m)
    y.view[m, 2] = 3.25


def k_pair_slot(x, rows, y, m):
    """A pair kernel that stores both slots of every pair: an odd count's last pair writes row m."""
    for i in range(0, m, 2):
        for j in (i, i + 1):
            y.view[j] = _f(x.view[int(rows.view[min(j, m - 1)])])


def k_reads_row_m(x, rows, y, m):
    """The last board's value picks up a multiple of what the next queue entry points at."""
    k_correct(x, rows, y, m)
    y.view[m - 1] += 0.0 * x.view[int(rows.view[m])]        # (0 x NaN = NaN; 0 x finite = 0: only the poison shows)
    y.view[m - 1, 0] += x.view[int(rows.view[m]), 0] * 2.0 ** -20


def k_reads_other_slot(x, rows, y, m):
    """Reads every slot of the queue whether or not rows[:m] names it."""
    k_correct(x, rows, y, m)
    y.view[0, 1] += x.view[:, 1].sum() * 2.0 ** -20


def _launch(kernel, pattern, fill, m=M, n=N, permute=False):
    g = torch.Generator().manual_seed(4)
    src = torch.randn((SLOTS, W), generator=g)
    order = torch.randperm(SLOTS, generator=g)[:n].int() if permute else torch.arange(n).int()
    named = order[:m]
    x = fp.carve((SLOTS, W), torch.float32, 0, "cpu").load(src)
    other = [s for s in range(SLOTS) if s not in set(named.tolist())]
    fp.poison(x, named if permute else m, pattern, seed=7)
    rows = fp.carve((n,), torch.int32, 0, "cpu").load(order[:m].contiguous())
    fp.poison(rows, m, pattern, valid=("slots", other if other else list(range(SLOTS))), seed=8)
    y = fp.carve((n, W), torch.float32, fill, "cpu")
    kernel(x, rows, y, m)
    return x, rows, y, src, named


def _verdict(kernel, m=M, permute=False):
    """What the GPU file asserts per case, as a dict of Reports."""
    xa, ra, ya, src, named = _launch(kernel, "ff", 0x07, m, permute=permute)
    xb, rb, yb, _, _ = _launch(kernel, "random", fp.Stream(5), m, permute=permute)
    plain = _f(src[named.long()])
    return {"out A": fp.untouched(ya, m), "out B": fp.untouched(yb, m), "in A": fp.untouched(xa, 0), "in B": fp.untouched(xb, 0),
            "rows A": fp.untouched(ra, 0), "A == B": fp.same_owned(ya, yb, m), "A == plain": fp.same_owned(ya, plain, m)}


@pytest.mark.parametrize("permute", [False, True])
@pytest.mark.parametrize("m", [0, 1, 3, 4, 5])
def test_a_correct_kernel_passes(m, permute):
    v = _verdict(k_correct, m, permute)
    assert all(v.values()), v


def test_a_byte_in_the_front_guard_is_reported():
    v = _verdict(k_front_guard)
    for run in ("out A", "out B"):
        assert not v[run] and v[run].where == "front guard" and v[run].offset == -1, v
    assert v["A == B"] and v["A == plain"] and v["in A"] and v["in B"], v
    print("front guard:", v["out A"])


def test_a_byte_in_the_back_guard_is_reported():
    v = _verdict(k_back_guard)
    for run in ("out A", "out B"):
        assert not v[run] and v[run].where == "back guard" and v[run].offset == N * W * 4 + 300, v
    assert v["A == B"] and v["A == plain"], v
    print("back guard:", v["out A"])


def test_a_write_to_row_m_is_reported():
    v = _verdict(k_row_m)
    for run in ("out A", "out B"):
        assert not v[run] and v[run].where == "tail rows" and v[run].row == M and v[run].offset == (M * W + 2) * 4, v
    assert v["A == B"] and v["A == plain"], v
    print("row m:", v["out A"])


def test_the_second_slot_of_a_half_empty_pair_is_reported():
    v = _verdict(k_pair_slot, m=3)
    for run in ("out A", "out B"):
        assert not v[run] and v[run].where == "tail rows" and v[run].row == 3 and v[run].offset == 3 * W * 4, v
    assert v["A == B"] and v["A == plain"], v
    assert all(_verdict(k_pair_slot, m=4).values())                 # (an even count has no such slot)
    print("pair slot:", v["out A"])


def test_an_output_that_depends_on_input_row_m_is_reported():
    v = _verdict(k_reads_row_m)
    assert v["out A"] and v["out B"] and v["in A"] and v["in B"], v      # (it writes nothing it should not)
    assert not v["A == B"] and v["A == B"].where == "owned rows" and v["A == B"].row == M - 1, v
    assert not v["A == plain"] and v["A == plain"].row == M - 1, v
    print("reads row m:", v["A == B"])


def test_an_output_that_depends_on_an_unnamed_queue_slot_is_reported():
    v = _verdict(k_reads_other_slot, permute=True)
    assert v["out A"] and v["out B"], v
    assert not v["A == B"] and v["A == B"].row == 0 and v["A == B"].offset == 4, v
    assert not v["A == plain"], v
    print("reads an unnamed slot:", v["A == B"])


def test_untouched_ignores_exactly_the_owned_rows():
    y = fp.carve((N, W), torch.float32, fp.Stream(3), "cpu")
    y.view[:M] = 1.0
    assert fp.untouched(y, M)
    r = fp.untouched(y, M - 1)
    assert not r and r.where == "tail rows" and r.row == M - 1
    r = fp.untouched(y, 0)
    assert not r and r.where == "tail rows" and r.row == 0 and r.offset == 0


def test_carve_is_aligned_guarded_and_filled():
    for shape, dtype in (((5, 90, 256), torch.int8), ((3, 7), torch.float16), ((2, 96), torch.int32), ((1,), torch.int32)):
        for fill in (0x07, fp.Stream(11)):
            h = fp.carve(shape, dtype, fill, "cpu")
            assert h.view.data_ptr() % 256 == 0 and h.view.is_contiguous() and tuple(h.view.shape) == shape
            g = max(4 * h.row_bytes, 64 * 1024)
            assert h.start >= g and h.buf.numel() - h.start - h.nbytes >= g
            assert h.view.data_ptr() == h.buf.data_ptr() + h.start
            assert fp.untouched(h, 0)
            if fill == 0x07:
                assert int((h.buf != 7).sum()) == 0
            else:
                again = fp.carve(shape, dtype, fill, "cpu")
                assert len(np.unique(h.buf.numpy())) == 256
                assert torch.equal(h.buf, again.buf) and torch.equal(h.buf, h.ref)


@pytest.mark.parametrize("pattern", ["ff", "random"])
def test_poison_with_valid_stays_in_range(pattern):
    slots = [2, 5, 6]
    rows = fp.carve((N,), torch.int32, 0, "cpu").load(torch.tensor([0, 1], dtype=torch.int32))
    fp.poison(rows, 2, pattern, valid=("slots", slots))
    words = rows.buf[rows.start - rows.guard:rows.start + rows.nbytes + rows.guard].view(torch.int32)
    assert words.numel() > 2 * 16384 and set(words.tolist()) == {0, 1, 2, 5, 6}
    assert rows.view[:2].tolist() == [0, 1] and set(rows.view[2:].tolist()) <= set(slots)
    assert fp.untouched(rows, 0)
    for planes_in in (14, 28):
        w = (1 << planes_in) - 1
        masks = fp.carve((N, 96), torch.int32, 0, "cpu")
        fp.poison(masks, 2, pattern, valid=("words", w))
        words = masks.buf[masks.start - masks.guard:masks.start + masks.nbytes + masks.guard].view(torch.int32)
        assert int(words.min()) >= 0 and int(words.max()) <= w and int(masks.view[2:].max()) > 0
        assert int(masks.view[:2].abs().max()) == 0
    planes = fp.carve((N, 14, 10, 9), torch.uint8, 0, "cpu")
    fp.poison(planes, 2, pattern, valid=("bytes", 1))
    assert int(planes.buf.max()) == 1 and int(planes.view[:2].max()) == 0 and int(planes.view[2:].max()) == 1
    # no restriction: NaN in every float format, -1 in int8
    x = fp.carve((N, 4), torch.float16, 0, "cpu")
    fp.poison(x, 2, "ff")
    assert torch.isnan(x.view[2:]).all() and not torch.isnan(x.view[:2]).any()
    assert torch.isnan(x.buf[x.start - 8:x.start].view(torch.float32)).all()
    assert int(x.buf[x.start + x.nbytes:x.start + x.nbytes + 8].view(torch.int8).max()) == -1


def test_same_owned_masks_only_the_owned_dont_care_bytes():
    import c6_model
    mask = c6_model.image_mask(128)
    a = torch.zeros((3, 90, 256), dtype=torch.int8)
    b = a.clone()
    free = int(np.flatnonzero(~mask)[0])
    b[1, 4, free] = 9
    assert fp.same_owned(a, b, 3, mask) and not fp.same_owned(a, b, 3)
    assert fp.same_owned(a, b, 1)
    b[1, 4, int(np.flatnonzero(mask)[5])] = 9
    r = fp.same_owned(a, b, 3, mask)
    assert not r and r.row == 1
