"""-m gpu: the four-wave pair kernel (k_resblock_ip4_c8) carries state from one phase into the next -- the first filter
fragments of a K loop, the next block's scale bytes and exponent words, block g + 2's biases are requested one phase before
they are consumed, across blocks and across the pairs of a workgroup.  What that state can get wrong is a chain, not a block:
so a chained launch is compared BYTE FOR BYTE with one launch per block, for

  * chains of 1, 2, 6 and 8 blocks at 128 filters (cz_tower takes at most 8) and of 1, 2, 6 and 12 at 192 (cz_resblock_chain):
    one block per launch never rewrites its biases, and the parity of the running block count picks the bias buffer across pairs;
  * 1, 2, 3, 511, 513 and 2 x CUs x 3 + 1 boards: one board (it runs in both slots), an odd last board, several pairs per
    workgroup, a workgroup with no second pair; and a device-side board count smaller than the launch shape;
  * every exit of the 128-filter chains: the c6 / c8 image, the c6 > c8 hand-over image, fp16 pairs, the head features;
    c6, c8, c6>N and c8>N towers at 192 filters (the network's outputs: there the chains have no exits of their own).

The block-by-block side of the image exits runs on the one-block kernels (cz_resblock: k_resblock_c8 at 128 filters, the
six-wave k_resblock_ip_c8 at 192); the fp16-pair exit is hi = fp16(r), lo = fp16(r - hi) of the last block's fp32 result; the
head exit -- whose sums associate differently from the one-block HEADS kernel's -- is the same exit behind a chain of one."""
import pytest

from test_gpu_guard import peaked_net

pytestmark = pytest.mark.gpu


def _counts():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return [1, 2, 3, 511, 513, 2 * cus * 3 + 1]


def _net128(arith, blocks, n_max):
    import torch
    from cchess_alphazero.agent.model import calibration_planes, guarded_inference_net
    net = peaked_net(20.0, blocks=blocks)
    planes = calibration_planes(n_max, 14, seed=29)
    g = guarded_inference_net(net, torch.float32, trunk="mfma", arith=arith, guard=False, planes=planes[:256])
    assert g.arith_name == arith, (g.arith_name, arith)
    return g, planes


TAIL_FILL = 0x5A        # the byte the outputs of a launch with a device-side count start from: rows >= the count keep it


def _filled(shape, dtype, fill=0):
    """A tensor whose every BYTE is `fill` (0: zeros)."""
    import torch
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(fill)
    return t


def _image(n, c6, fill=0):
    import torch
    return (_filled((n, 90, 128), torch.float16, fill), _filled((n, 90, 256), torch.int8 if c6 else torch.uint8, fill))


def _tail_kept(out, m, fill):
    """Rows >= m of every tensor of `out` still hold the fill byte."""
    import torch
    return all(bool((t[m:].contiguous().view(-1).view(torch.uint8) == fill).all()) for t in out)


def _first(g, planes, c6):
    """The tower's first launch (input layer + block 0): the image block 1 reads."""
    from cchess_alphazero import _native
    x = _image(planes.shape[0], c6)
    _native.input_resblock(planes, g.in_table32, g.in_bias32, *g._block_params(0), out=x)
    return x


def _eq(a, b, m):
    import torch
    return all(torch.equal(s[:m].view(torch.uint8), t[:m].view(torch.uint8)) for s, t in zip(a, b))


# (arith, residual blocks of the net, blocks of the chain = net blocks 1 .. last, exit)
CASES_128 = [(arith, nb + 1 + extra, nb, exit_)
             for nb in (1, 2, 6, 8)
             for arith, extra, exit_ in (("c6", 0, "image"), ("c6", 0, "heads"), ("c8", 0, "image"), ("c8", 0, "heads"),
                                         ("c6>%d" % (nb + 1), 1, "hand_over"), ("c8>%d" % (nb + 1), 1, "pairs"))]


@pytest.mark.parametrize("arith,blocks,nb,exit_", CASES_128)
def test_128_filter_chain_equals_block_by_block(arith, blocks, nb, exit_):
    import torch
    from cchess_alphazero import _native
    counts = _counts()
    g, planes_all = _net128(arith, blocks, max(counts))
    c6 = arith.startswith("c6")
    assert g.block_kinds()[:nb + 1] == ["c6" if c6 else "c8"] * (nb + 1), g.block_kinds()
    fmt = [_native.IMG_C6 if c6 else _native.IMG_C8] * nb
    chain = [g._block_params(i) for i in range(1, nb + 1)]
    hw, hb = g.head_w32, g.head_b32
    npol = g.policy_conv.weight.shape[0]
    nval = hw.shape[0] - npol
    for n in counts:
        for short in (False, True):
            if short and n < 3:
                continue
            m = n - n // 4 if short else n
            count = torch.tensor([m], dtype=torch.int32, device="cuda") if short else None
            x0 = _first(g, planes_all[:n].contiguous(), c6)
            # one launch per block: the one-block kernels; the last block as the exit needs it
            cur = x0
            for i in range(1, nb):
                nxt = _image(n, c6)
                _native.resblock(cur, *g._block_params(i), out=nxt, count=count)
                cur = nxt
            tag = (arith, nb, exit_, n, m)
            fill = TAIL_FILL if short else 0
            if exit_ in ("image", "hand_over"):
                c6_out = c6 and exit_ == "image"
                want = _image(n, c6_out)
                _native.resblock(cur, *g._block_params(nb), out=want, count=count)
                got = _image(n, c6_out, fill)
                _native.tower(x0, chain, _native.IMG_C6 if c6_out else _native.IMG_C8, out=got, count=count, fmt_x=fmt, fmt_y=fmt)
                assert _eq(want, got, m), tag
                assert _tail_kept(got, m, fill), tag
            elif exit_ == "pairs":
                r = torch.zeros((n, 90, 128), dtype=torch.float32, device="cuda")
                _native.resblock(cur, *g._block_params(nb), out_f32=r, count=count)
                hi = r.to(torch.float16)
                want = (hi, (r - hi.float()).to(torch.float16))
                got = tuple(_filled((n, 90, 128), torch.float16, fill) for _ in range(2))
                _native.tower(x0, chain, _native.IMG_PAIR, out=got, count=count, fmt_x=fmt, fmt_y=fmt)
                assert _eq(want, got, m), tag
                assert _tail_kept(got, m, fill), tag
            else:
                feats = [tuple(_filled((n, k * 90), torch.float32, fill) for k in (npol, nval)) for _ in range(2)]
                _native.tower(cur, chain[-1:], _native.EXIT_HEADS, heads=(hw, hb, npol) + feats[0], count=count,
                              fmt_x=fmt[:1], fmt_y=fmt[:1])
                _native.tower(x0, chain, _native.EXIT_HEADS, heads=(hw, hb, npol) + feats[1], count=count, fmt_x=fmt, fmt_y=fmt)
                assert torch.isfinite(feats[1][0][:m]).all() and _eq(feats[0], feats[1], m), tag
                assert _tail_kept(feats[0], m, fill) and _tail_kept(feats[1], m, fill), tag


@pytest.mark.parametrize("arith,blocks", [("c6", 2), ("c6", 6), ("c6", 12), ("c8", 1), ("c8", 2), ("c8", 6), ("c8", 12),
                                          ("c6>1", 3), ("c6>2", 8), ("c6>6", 12), ("c8>3", 4), ("c8>2", 4), ("c8>6", 8)])
def test_192_filter_chain_equals_block_by_block(arith, blocks, monkeypatch):
    """The chains of a 192-filter tower (the c6 chain starts the tower on the input layer's c8 image) against one launch per
    block of the six-wave kernel."""
    import torch
    from cchess_alphazero.agent.model import calibration_planes, guarded_inference_net
    counts = _counts()
    net = peaked_net(20.0, blocks=blocks, filters=192)
    planes_all = calibration_planes(max(counts), 14, seed=31)
    g = guarded_inference_net(net, torch.float32, trunk="mfma", arith=arith, guard=False, planes=planes_all[:256])
    assert g.arith_name == arith and g.filters == 192
    for n in counts:
        for short in (False, True):
            if short and n < 3:
                continue
            m = n - n // 4 if short else n
            kw = {"rows": torch.arange(n, device="cuda").int(), "count": torch.tensor([m], dtype=torch.int32, device="cuda")} if short else {}
            planes = planes_all[:n].contiguous()
            g.chain_blocks = False
            monkeypatch.setenv("CZ_IP_PAIR", "0")
            p0, v0 = (t.clone() for t in g(planes, **kw))
            g.chain_blocks = True
            monkeypatch.setenv("CZ_IP_PAIR", "1")
            p1, v1 = g(planes, **kw)
            assert torch.isfinite(p1[:m]).all() and torch.equal(p0[:m], p1[:m]) and torch.equal(v0[:m], v1[:m]), (arith, blocks, n, m)
