"""InferenceNet's launch plan (agent/model.py _plan / _build_plan) for networks built on the host and never run: which launches
one forward makes for every tower width, arithmetic and switch -- chains as tower_plan / ip_segments give them, else one
launch per block or per convolution -- and that plans are cached per switch setting and dropped with the module's tensors."""
import pytest
import torch

# (filters, blocks, arith, dtype)
NETS = [(32, 2, None, "float32"), (32, 2, None, "float16"),
        (128, 7, "c6", "float32"), (128, 7, "c6>3", "float32"), (128, 4, "c6>1", "float32"), (128, 12, "c6", "float32"),
        (128, 7, "c8", "float32"), (128, 7, "c8>3", "float32"), (128, 4, "c8>1", "float32"), (128, 7, "f16x3", "float32"),
        (128, 7, "bf16x3", "float32"), (128, 3, None, "float16"), (128, 3, None, "bfloat16"),
        (192, 10, "c6", "float32"), (192, 10, "c6>3", "float32"), (192, 10, "c8>6", "float32"), (192, 14, "c8", "float32"),
        (192, 4, "f16x3", "float32"), (192, 14, "bf16x3", "float32"), (192, 3, None, "float16"),
        (256, 26, None, "float16"), (256, 3, None, "bfloat16"), (256, 2, None, "float32")]
SWITCHES = ("chain_blocks", "chain_heads", "fused_blocks", "fused_input", "fused_heads")


@pytest.mark.parametrize("filters,blocks,arith,dtype", NETS)
def test_trunk_plan(filters, blocks, arith, dtype, monkeypatch):
    from cchess_alphazero import _native
    from cchess_alphazero.agent.model import CChessNet, InferenceNet, ip_segments, tower_plan
    torch.manual_seed(blocks)
    exps = ([0] * blocks, [1] * blocks) if arith and arith.startswith("c6") else None
    g = InferenceNet(CChessNet(cnn_filter_num=filters, res_layer_num=blocks).eval(), getattr(torch, dtype), trunk="mfma",
                     arith=arith, act_exps=exps)
    assert g.arith_name == (arith or "bf16x3")
    kinds, two = g.block_kinds(), g.parts == 2
    n8 = g.c8_blocks if g.arith == "c8" else 0
    for off in (None,) + SWITCHES:
        for s in SWITCHES:
            setattr(g, s, s != off)
        for six_wave in ("1", "0"):
            monkeypatch.setenv("CZ_IP_PAIR", six_wave)
            for planes_dtype in (torch.uint8, torch.float32):
                for heads in (True, False):
                    fused = g.fused_blocks and (filters in (128, 192) or (filters == 256 and not two))
                    first = (fused and g.fused_input and filters == 128 and two and planes_dtype == torch.uint8 and
                             arith != "c8>1")
                    assert g.takes_masks(planes_dtype) == first
                    if g.c6 and not (fused and (first or filters == 192)):
                        with pytest.raises(RuntimeError):
                            g._plan(planes_dtype, heads)
                        continue
                    steps, labels = g._plan(planes_dtype, heads)
                    assert g._plan(planes_dtype, heads)[0] is steps
                    assert steps[0].call == ("input_resblock" if first else "input_conv")
                    assert [i for st in steps for i in st.blocks] == list(range(blocks))       # every block once, in order
                    heads_fused = heads and fused and two and filters == 128
                    assert (steps[-1].to == "heads") == heads_fused
                    chained = g.chain_blocks and fused and (first or (filters == 192 and two) or filters == 256)
                    split = 0 < n8 < blocks and not (chained and filters == 128)     # (a 128-filter chain's exit hands over)
                    assert [st.blocks[-1] for st in steps if st.to == "pairs"] == ([n8 - 1] if split else [])
                    assert any(st.code == _native.F16C86 for st in steps) == (g.c6 and filters == 192)
                    if not chained:
                        assert labels is None
                        for st in steps[1:]:
                            assert len(st.blocks) == 1 and st.bl is None and st.timed == fused
                            assert st.call == (("resblock_heads" if st.to == "heads" else "resblock") if fused else
                                               "conv3x3_c8" if kinds[st.blocks[0]] == "c8" else "conv3x3")
                    elif filters == 128:
                        chain_heads = g.chain_heads and not (kinds[-1] == "pair" and g.operand_dtype == torch.bfloat16)
                        assert labels == tower_plan(kinds, heads_exit=heads_fused, chain_heads=chain_heads)
                        call = {"first": "input_resblock", "tower": "tower", "pairs": "tower_pairs",
                                "block": "resblock_heads" if heads_fused else "resblock"}
                        assert [st.call for st in steps] == [call[lb[0]] for lb in labels]
                        exits = {"c6": _native.IMG_C6, "c8": _native.IMG_C8, "pair": _native.IMG_PAIR, "heads": _native.EXIT_HEADS}
                        assert [st.code for st in steps if st.call == "tower"] == [exits[lb[2]] for lb in labels if lb[0] == "tower"]
                    elif filters == 192:
                        segs = ip_segments(kinds, first_alone=six_wave == "0")
                        assert labels == [("chain192" if k == "chain" else "block192", b, kinds[b[0]]) for k, b in segs]
                        assert [st.blocks for st in steps[1:]] == [tuple(b) for _, b in segs]
                        assert [st.call for st in steps[1:]] == ["resblock_chain" if k == "chain" else "resblock" for k, _ in segs]
                    else:
                        assert labels == [("chain256", list(range(lo, min(blocks, lo + 24))), "plain") for lo in range(0, blocks, 24)]
                        assert all(st.call == "tower_plain" for st in steps[1:])
                    for st in steps:
                        if st.bl is None:
                            continue
                        assert st.bl.n == len(st.blocks)                    # a chain's pointer arrays: its blocks, in order
                        for j, i in enumerate(st.blocks):
                            assert [st.bl.arrays[k][j] for k in range(4)] == [t.data_ptr() for t in g._block_params(i)]
                        if st.call == "tower":
                            fmt = [_native.IMG_C6 if kinds[st.blocks[0]] == "c6" else _native.IMG_C8] * len(st.blocks)
                            assert list(st.bl.fmt_x) == list(st.bl.fmt_y) == fmt
    assert len(g._plans) > 1
    g.cpu()                                                     # (.to / .cuda / .cpu: new tensors, no plan survives)
    assert g._plans == {}
