"""-m gpu: the conversions in the epilogues of the four-wave pair kernel (k_resblock_ip4_c8<128>) on values a random network
never produces.  The tower convolutions of the net have ZERO weights, so an accumulator is exactly its folded bias (plus the
skip element in the second epilogue) and the biases choose what relu / fp16 / bf6 / e4m3 see:

    +-0, the smallest fp32 denormal, 2^-25 and 2^-24 (the fp16 denormal threshold and its tie), 2^-14 and its two neighbours,
    1 + 2^-11 (an fp16 tie) and 1 + 2^-11 +- 2^-23, 65504, 65519.996          -- everywhere: finite as fp16
    65520, 1e30, +inf, a quiet NaN                                             -- the chain's last epilogue / exit only

and the negatives of all of them.  A value whose fp16 is not finite may only leave the chain: a convolution that read it would
multiply it by the zero weights (NaN in every channel).  Layout of the second biases over the 128 channels (b1 of every block:
the finite list, cyclic): channels 0 .. 63 -- block 0 leaves zero there, block 1's epilogue 2 writes the finite list exactly,
block 2 passes the stream's value on (b2 = 0: relu(skip)); channels 64 .. 127 -- the first launch writes the finite list,
block 1 clears it, the last epilogue / exit gets the full list on a zero skip.

A chain of blocks 1 - 2 behind the first launch is compared BYTE FOR BYTE with two one-block launches (k_resblock_c8), for c6
(image exponents set by hand, no calibration: 0 -- the bf6 pieces resolve the values around 1 -- and 12 -- they hold 65504) and c8,
on 3 boards (a pair and an odd board) and 2 x CUs x 2 + 1 (a second pair per workgroup), for every exit cz_tower has behind the
chain: the image, the heads (against the same exit behind a chain of one, as tests/test_gpu_chain_prefetch.py), the fp16 pairs
(c8 chains; cz_tower refuses them behind a c6 chain, which gets its c6 > c8 hand-over image instead).  +inf and NaN: on every
exit, in a run of their own (nonfinite=True) -- through the head features they would turn every output into 0 / inf / NaN, so the
finite run is the one that tests the heads' arithmetic.

What the comparison sees: the values an epilogue 2 / exit writes (block 1's and block 2's: the same c6 unit, split and staging
code as epilogue 1's) and the skip elements epilogue 1 reads back out of the images.  What epilogue 1 WRITES (b1: the finite
list on all channels) goes through the same unit but meets zero filters and reaches no output; it is there so that every unit
runs on the list, and a wrong address of it would overwrite what the comparison does see.  The test counts, from the bias
tensors it loaded, the channels whose exact value reaches an output."""
import functools
import math
import struct

import pytest

from test_gpu_chain_prefetch import TAIL_FILL, _filled, _image as _filled_image, _tail_kept

pytestmark = pytest.mark.gpu

K_MID_OUT = {"c6k0": 0, "c6k12": 12}


def _values(nonfinite):
    import numpy as np
    f = np.float32
    fin = [0.0, 2.0 ** -149, 2.0 ** -25, 2.0 ** -24, 2.0 ** -14, float(np.nextafter(f(2.0 ** -14), f(0))),
           float(np.nextafter(f(2.0 ** -14), f(1))), 1 + 2.0 ** -11, 1 + 2.0 ** -11 - 2.0 ** -23, 1 + 2.0 ** -11 + 2.0 ** -23,
           65504.0, float(f(65519.996))]
    assert fin[-1] == 65520 - 2.0 ** -8 and len(set(fin)) == 12
    big = [65520.0, 1e30] + ([math.inf, math.nan] if nonfinite else [])
    finite = fin + [-v for v in fin]
    full = finite + big + [-v for v in big]
    return finite, full


def _cyc(vals, n, start=0):
    import torch
    return torch.tensor([vals[(start + i) % len(vals)] for i in range(n)], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _net(arith, nonfinite):
    """(InferenceNet with zero tower filters and the biases above, blocks 1 - 2's parameters, the hand-over form of block 2,
    the number of (channel, value) placements per kind of epilogue)."""
    import torch
    from cchess_alphazero import _native
    from cchess_alphazero.agent.model import CChessNet, InferenceNet
    torch.manual_seed(5)
    net = CChessNet(cnn_filter_num=128, res_layer_num=3).eval()
    with torch.no_grad():
        net.input_conv.weight.zero_()
        for blk in net.res:
            blk.conv1.weight.zero_()
            blk.conv2.weight.zero_()
    c6 = arith.startswith("c6")
    k = K_MID_OUT.get(arith, 0)
    g = InferenceNet(net, torch.float32, trunk="mfma", arith="c6" if c6 else "c8",
                     act_exps=([k] * 3, [k] * 3) if c6 else None).cuda()
    assert g.arith_name == ("c6" if c6 else "c8") and g.block_kinds() == ["c6" if c6 else "c8"] * 3
    assert float(g.in_bias32.abs().max()) == 0.0
    finite, full = _values(nonfinite)
    neg = torch.full((64,), -1e30)
    zero = torch.zeros(64)
    b2 = [torch.cat([neg, _cyc(finite, 64)]),                   # block 0: the stream is 0 | the finite list
          torch.cat([_cyc(finite, 64, 5), neg]),                # block 1: the finite list, exact | 0
          torch.cat([zero, _cyc(full, 64)])]                    # block 2: relu(skip) | the full list, exact
    b1 = [torch.zeros(128), _cyc(finite, 128, 3), _cyc(finite, 128, 11)]
    for i in range(3):
        getattr(g, f"tb{i}a").copy_(b1[i])
        getattr(g, f"tb{i}b").copy_(b2[i])
    assert torch.equal(g.tb2b.cpu().view(torch.int32), b2[2].view(torch.int32))       # (signs of zero, the NaN: as set)
    params = [g._block_params(i) for i in (1, 2)]
    hand = None
    if c6:
        w2 = _native.pack_conv3x3_c6_weights(torch.zeros((128, 128, 3, 3)), k, 127).view(torch.float16).cuda()
        hand = params[1][:2] + (w2, params[1][3])
    # channels whose output is exactly relu(bias) (zero skip underneath) and the distinct bit patterns among those biases
    key = lambda v: struct.pack("<f", v)
    listed = {key(v) for v in full}
    def visible(bias, skip_below):
        ch = [c for c in range(128) if float(skip_below[c]) <= 0 and key(float(bias[c])) in listed]
        return len(ch), len({key(float(bias[c])) for c in ch})
    b = [getattr(g, f"tb{i}b").cpu() for i in range(3)]
    swept = {"epilogue_2": visible(b[1], b[0]), "last": visible(b[2], b[1]),
             "skip_read": int((b[0] > 0).sum()) + int((b[1] > 0).sum())}
    return g, params, hand, swept


def _image(n, c6):
    import torch
    return (torch.zeros((n, 90, 128), dtype=torch.float16, device="cuda"),
            torch.zeros((n, 90, 256), dtype=torch.int8 if c6 else torch.uint8, device="cuda"))


def _eq(a, b):
    import torch
    return all(torch.equal(s.view(torch.uint8), t.view(torch.uint8)) for s, t in zip(a, b))


@functools.lru_cache(maxsize=None)
def _planes(n):
    from cchess_alphazero.agent.model import calibration_planes
    return calibration_planes(n, 14, seed=37).contiguous()


@pytest.mark.parametrize("nonfinite", [False, True])
@pytest.mark.parametrize("arith", ["c6k0", "c6k12", "c8"])
def test_chain_of_two_equals_block_by_block_on_chosen_values(arith, nonfinite):
    import torch
    from cchess_alphazero import _native
    g, params, hand, swept = _net(arith, nonfinite)
    # block 1: its 64 list channels and, of the other 64 (-1e30, itself on the list), those under a skip of zero; block 2: its 64
    # list channels and its zero biases above a cleared stream; every listed bit pattern; positive stream values read as skips
    assert swept == {"epilogue_2": (95, 25), "last": (99, 32 if nonfinite else 28), "skip_read": 33 + 29}, swept
    c6 = arith.startswith("c6")
    fmt = [_native.IMG_C6 if c6 else _native.IMG_C8] * 2
    hw, hb = g.head_w32, g.head_b32
    npol = g.policy_conv.weight.shape[0]
    nval = hw.shape[0] - npol
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    exits = ["image", "hand_over" if c6 else "pairs", "heads"]
    ran = 0

    def same_below(a, b, m):
        return all(torch.equal(s[:m].contiguous().view(torch.uint8), t[:m].contiguous().view(torch.uint8)) for s, t in zip(a, b))
    for n in (3, 2 * cus * 2 + 1):
        # the same chain with a device-side count one short of the launch shape, into outputs that start from the byte
        # TAIL_FILL: the same bytes below the count, the fill from it on
        short = dict(count=torch.tensor([n - 1], dtype=torch.int32, device="cuda"), fmt_x=fmt, fmt_y=fmt)
        x0 = _image(n, c6)
        _native.input_resblock(_planes(n), g.in_table32, g.in_bias32, *g._block_params(0), out=x0)
        # the first launch left relu(b2) of block 0 in the f16 image: 0 | the finite list
        got0 = x0[0][n - 1, 89].float().cpu()
        assert torch.equal(got0, g.tb0b.cpu().clamp(min=0).to(torch.float16).float()), (arith, n)
        mid = _image(n, c6)
        _native.resblock(x0, *params[0], out=mid)
        # ... and block 1 the finite list | 0 (its epilogue 2, exact: the skip is zero)
        assert torch.equal(mid[0][n - 1, 89].float().cpu(), g.tb1b.cpu().clamp(min=0).to(torch.float16).float()), (arith, n)
        for exit_ in exits:
            tag = (arith, nonfinite, n, exit_)
            if exit_ in ("image", "hand_over"):
                c6_out = c6 and exit_ == "image"
                blocks = [params[0], hand if exit_ == "hand_over" else params[1]]
                want, got = _image(n, c6_out), _image(n, c6_out)
                _native.resblock(mid, *blocks[1], out=want)
                _native.tower(x0, blocks, _native.IMG_C6 if c6_out else _native.IMG_C8, out=got, fmt_x=fmt, fmt_y=fmt)
                assert _eq(want, got), tag
                assert int(want[0].view(torch.int16).ne(0).sum()) > 0 and int(want[1].view(torch.uint8).ne(0).sum()) > 0, tag
                cut = _filled_image(n, c6_out, TAIL_FILL)
                _native.tower(x0, blocks, _native.IMG_C6 if c6_out else _native.IMG_C8, out=cut, **short)
                assert same_below(got, cut, n - 1) and _tail_kept(cut, n - 1, TAIL_FILL), tag
            elif exit_ == "pairs":
                r = torch.zeros((n, 90, 128), dtype=torch.float32, device="cuda")
                _native.resblock(mid, *params[1], out_f32=r)
                hi = r.to(torch.float16)
                want = (hi, (r - hi.float()).to(torch.float16))
                got = tuple(torch.zeros((n, 90, 128), dtype=torch.float16, device="cuda") for _ in range(2))
                _native.tower(x0, params, _native.IMG_PAIR, out=got, fmt_x=fmt, fmt_y=fmt)
                assert _eq(want, got), tag
                cut = tuple(_filled((n, 90, 128), torch.float16, TAIL_FILL) for _ in range(2))
                _native.tower(x0, params, _native.IMG_PAIR, out=cut, **short)
                assert same_below(got, cut, n - 1) and _tail_kept(cut, n - 1, TAIL_FILL), tag
            else:
                feats = [tuple(torch.zeros((n, kk * 90), dtype=torch.float32, device="cuda") for kk in (npol, nval)) for _ in range(2)]
                _native.tower(mid, params[1:], _native.EXIT_HEADS, heads=(hw, hb, npol) + feats[0], fmt_x=fmt[:1], fmt_y=fmt[:1])
                _native.tower(x0, params, _native.EXIT_HEADS, heads=(hw, hb, npol) + feats[1], fmt_x=fmt, fmt_y=fmt)
                assert _eq(feats[0], feats[1]), tag
                if not nonfinite:
                    assert torch.isfinite(feats[1][0]).all() and torch.isfinite(feats[1][1]).all(), tag
                cut = tuple(_filled((n, kk * 90), torch.float32, TAIL_FILL) for kk in (npol, nval))
                _native.tower(x0, params, _native.EXIT_HEADS, heads=(hw, hb, npol) + cut, **short)
                assert same_below(feats[1], cut, n - 1) and _tail_kept(cut, n - 1, TAIL_FILL), tag
            ran += 1
    assert ran == 6
