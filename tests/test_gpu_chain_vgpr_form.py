"""-m gpu: the 128-filter chains of the four-wave pair kernel (k_resblock_ip4_c8<128>, csrc/xq_conv_ip4.hip) are compiled with the
matrix instructions' accumulators in VALU-visible registers; the one-block kernels (k_resblock_c8, csrc/xq_conv_block_c8.h) are not, so
they are an independent reference.  A chained launch is compared BYTE FOR BYTE with one launch per block of those kernels at
the smallest shapes where the pair kernel can go wrong:

  * 1 board (the pair's second board is missing), 2, 3 (a half-empty second pair), 5, 2 x CUs + 1 (a workgroup runs a second
    pair behind its first), and a device-side board count smaller than the launch shape;
  * chains of 1, 2 and 6 blocks, c6 and c8;
  * the three exits.  Operand image (and the c6 > c8 hand-over image): cz_resblock's.  fp16 pairs: hi = fp16(r), lo = fp16(r - hi)
    of the last one-block launch's fp32 result r.  Heads: the exit's own arithmetic restated in separate fp32 tensor operations
    on that r -- per pixel and head filter the products of a 32-channel block added in channel order from zero, the four
    blocks as (a0 + a1) + (a2 + a3), + bias, x > 0 ? x : 0 -- so that exit too is held to the one-block kernels bit for bit
    (tests/test_gpu_chain_prefetch.py compares it with the same exit behind a chain of one);
  * on a random network, and on the network of tests/test_gpu_chain_epilogues.py, whose zero filters leave exactly the chosen
    biases (-0, negatives, denormals, fp16 ties, 65504 / 65520, inf and NaN) in the accumulators that the first relu after
    each K loop reads out of the matrix instructions' destination registers."""
import functools

import pytest

from test_gpu_chain_epilogues import _net as _chosen_net, _planes as _chosen_planes
from test_gpu_chain_prefetch import TAIL_FILL, _filled, _first, _image, _net128, _tail_kept

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _shapes():
    """(boards of the launch, boards the device-side count leaves)"""
    big = 2 * _cus() + 1
    return [(1, 1), (2, 2), (3, 3), (5, 5), (big, big), (5, 3), (big, big - 2)]


def _eq(a, b, m):
    import torch
    return all(torch.equal(s[:m].contiguous().view(torch.uint8), t[:m].contiguous().view(torch.uint8)) for s, t in zip(a, b))


def _heads_of(r, hw, hb, npol):
    """The heads exit of the chain on the fp32 activation r [n, 90, 128], one rounding per tensor operation."""
    import torch
    n = r.shape[0]
    part = []
    for b32 in range(4):
        a = torch.zeros((n, 90, 6), dtype=torch.float32, device=r.device)
        for c in range(32 * b32, 32 * b32 + 32):
            a = a + r[:, :, c:c + 1] * hw[:, c].view(1, 1, 6)
        part.append(a)
    hv = ((part[0] + part[1]) + (part[2] + part[3])) + hb.view(1, 1, 6)
    hv = torch.where(hv > 0, hv, torch.zeros_like(hv)).permute(0, 2, 1).contiguous()       # [n, 6, 90]
    return hv[:, :npol].reshape(n, npol * 90), hv[:, npol:].reshape(n, (6 - npol) * 90)


def _check(tag, x, blocks, last_for, c6, heads, n, m, exits):
    """x: the image the chain's first block reads; blocks: the chain; last_for(exit): the last block's parameters for that exit."""
    import torch
    from cchess_alphazero import _native
    hw, hb, npol = heads
    count = torch.tensor([m], dtype=torch.int32, device="cuda") if m < n else None
    fmt = [_native.IMG_C6 if c6 else _native.IMG_C8] * len(blocks)
    fill = TAIL_FILL if m < n else 0                        # (a device-side count: rows >= m of the chain's outputs keep this byte)
    cur = x
    for bp in blocks[:-1]:                                  # one launch per block: the one-block kernels
        nxt = _image(n, c6)
        _native.resblock(cur, *bp, out=nxt, count=count)
        cur = nxt
    r = None
    for exit_ in exits:
        chain = blocks[:-1] + [last_for(exit_)]
        if exit_ in ("image", "hand_over"):
            c6_out = c6 and exit_ == "image"
            want, got = _image(n, c6_out), _image(n, c6_out, fill)
            _native.resblock(cur, *chain[-1], out=want, count=count)
            _native.tower(x, chain, _native.IMG_C6 if c6_out else _native.IMG_C8, out=got, count=count, fmt_x=fmt, fmt_y=fmt)
            assert int(want[0][:m].view(torch.int16).ne(0).sum()) > 0, tag + (exit_,)
        else:
            if r is None:
                r = torch.zeros((n, 90, 128), dtype=torch.float32, device="cuda")
                _native.resblock(cur, *chain[-1], out_f32=r, count=count)
            if exit_ == "pairs":
                hi = r.to(torch.float16)
                want = (hi, (r - hi.float()).to(torch.float16))
                got = tuple(_filled((n, 90, 128), torch.float16, fill) for _ in range(2))
                _native.tower(x, chain, _native.IMG_PAIR, out=got, count=count, fmt_x=fmt, fmt_y=fmt)
            else:
                want = _heads_of(r, hw, hb, npol)
                got = tuple(_filled((n, k * 90), torch.float32, fill) for k in (npol, 6 - npol))
                _native.tower(x, chain, _native.EXIT_HEADS, heads=(hw, hb, npol) + got, count=count, fmt_x=fmt, fmt_y=fmt)
                assert not torch.isnan(got[0][:m]).any() and not torch.isnan(got[1][:m]).any(), tag + (exit_,)
        assert _eq(want, got, m), tag + (exit_,)
        assert _tail_kept(got, m, fill), tag + (exit_,)


@pytest.mark.parametrize("nb", [1, 2, 6])
@pytest.mark.parametrize("arith", ["c6", "c8"])
def test_chain_equals_one_block_kernels_on_a_random_network(arith, nb):
    c6 = arith == "c6"
    n_max = max(n for n, _ in _shapes())
    g, planes_all = _net128(arith, nb + 1, n_max)
    assert g.block_kinds() == [arith] * (nb + 1), g.block_kinds()
    blocks = [g._block_params(i) for i in range(1, nb + 1)]
    heads = (g.head_w32, g.head_b32, g.policy_conv.weight.shape[0])
    # the c6 > c8 hand-over: a net whose block nb + 1 is f16x3, so that the chain's last block writes a c8 image
    g2 = _net128("c6>%d" % (nb + 1), nb + 2, n_max)[0] if c6 else None
    for n, m in _shapes():
        planes = planes_all[:n].contiguous()
        _check((arith, nb, n, m), _first(g, planes, c6), blocks, lambda e: blocks[-1], c6, heads, n, m,
               ["image", "heads"] + ([] if c6 else ["pairs"]))
        if c6:
            assert g2.block_kinds()[:nb + 1] == ["c6"] * (nb + 1), g2.block_kinds()
            blocks2 = [g2._block_params(i) for i in range(1, nb + 1)]
            _check((arith, nb, n, m), _first(g2, planes, c6), blocks2, lambda e: blocks2[-1], c6, heads, n, m, ["hand_over"])


@pytest.mark.parametrize("nonfinite", [False, True])
@pytest.mark.parametrize("arith", ["c6k0", "c6k12", "c8"])
def test_chain_equals_one_block_kernels_on_chosen_accumulator_values(arith, nonfinite):
    """Chains of two (blocks 1 - 2 behind the first launch) and of one (block 2 behind a one-block launch of block 1): epilogue 1
    reads the finite list out of K loop 1's accumulators, epilogue 2 / the exit the list on the skip out of K loop 2's."""
    from cchess_alphazero import _native
    g, params, hand, swept = _chosen_net(arith, nonfinite)
    assert swept["epilogue_2"][1] == 25 and swept["last"][1] == (32 if nonfinite else 28), swept
    c6 = arith.startswith("c6")
    heads = (g.head_w32, g.head_b32, g.policy_conv.weight.shape[0])
    last_for = lambda e: hand if e == "hand_over" else params[1]
    exits = ["image", "hand_over" if c6 else "pairs", "heads"]
    for n, m in _shapes():
        x0 = _image(n, c6)
        _native.input_resblock(_chosen_planes(n), g.in_table32, g.in_bias32, *g._block_params(0), out=x0)
        _check((arith, nonfinite, 2, n, m), x0, list(params), last_for, c6, heads, n, m, exits)
        mid = _image(n, c6)
        _native.resblock(x0, *params[0], out=mid)
        _check((arith, nonfinite, 1, n, m), mid, [params[1]], last_for, c6, heads, n, m, exits)
