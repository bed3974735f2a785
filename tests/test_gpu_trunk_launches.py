"""-m gpu: what one forward of InferenceNet launches (agent/model.py: _build_plan's steps, run by _trunk_mfma) for every tower
width, arithmetic and switch: the _native entry points in order, each with all its arguments -- dtypes and shapes, which
buffer (the module's own by name, the others numbered in the order the forward first touches them), a chain's blocks and
image formats.  tests/golden/trunk_launches.json holds, per forward, a digest of the same recorder's calls from the dispatch the
launch plan replaced (one hand-written path per tower shape); a forward must make exactly the calls it made."""
import contextlib
import hashlib
import inspect
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trunk_launches.json")
ENTRY_POINTS = ("input_conv", "input_resblock", "resblock", "resblock_heads", "tower", "tower_pairs", "resblock_chain",
                "tower_plain", "split_bias_act", "conv3x3", "conv3x3_c8", "head_convs", "heads_tail")
# name: (filters, blocks, arith, dtype, (policy filters, value filters))
NETS = {
    "128x7 c6": (128, 7, "c6", "float32", (4, 2)),
    "128x7 c6>3": (128, 7, "c6>3", "float32", (4, 2)),
    "128x4 c6>1": (128, 4, "c6>1", "float32", (4, 2)),
    "128x12 c6": (128, 12, "c6", "float32", (4, 2)),
    "128x7 c8": (128, 7, "c8", "float32", (4, 2)),
    "128x7 c8>3": (128, 7, "c8>3", "float32", (4, 2)),
    "128x4 c8>1": (128, 4, "c8>1", "float32", (4, 2)),
    "128x7 f16x3": (128, 7, "f16x3", "float32", (4, 2)),
    "128x7 bf16x3": (128, 7, "bf16x3", "float32", (4, 2)),
    "128x3 c8 heads 2+1": (128, 3, "c8", "float32", (2, 1)),
    "128x3 fp16": (128, 3, None, "float16", (4, 2)),
    "128x3 bf16": (128, 3, None, "bfloat16", (4, 2)),
    "192x10 c6": (192, 10, "c6", "float32", (4, 2)),
    "192x10 c6>3": (192, 10, "c6>3", "float32", (4, 2)),
    "192x10 c8>6": (192, 10, "c8>6", "float32", (4, 2)),
    "192x14 c8": (192, 14, "c8", "float32", (4, 2)),
    "192x4 f16x3": (192, 4, "f16x3", "float32", (4, 2)),
    "192x14 bf16x3": (192, 14, "bf16x3", "float32", (4, 2)),
    "192x3 fp16": (192, 3, None, "float16", (4, 2)),
    "256x3 fp16": (256, 3, None, "float16", (4, 2)),
    "256x26 fp16": (256, 26, None, "float16", (4, 2)),
    "256x3 bf16": (256, 3, None, "bfloat16", (4, 2)),
    "256x2 fp32": (256, 2, None, "float32", (4, 2)),
    "32x2 fp32": (32, 2, None, "float32", (4, 2)),
    "32x2 fp16": (32, 2, None, "float16", (4, 2)),
}
# name: (InferenceNet attributes, CZ_IP_PAIR, planes dtype, compact queue, masks)
SETTINGS = {
    "default": ({}, "1", "uint8", False, False),
    "chain_blocks off": ({"chain_blocks": False}, "1", "uint8", False, False),
    "fused_blocks off": ({"fused_blocks": False}, "1", "uint8", False, False),
    "chain_heads off": ({"chain_heads": False}, "1", "uint8", False, False),
    "fused_heads off": ({"fused_heads": False}, "1", "uint8", False, False),
    "fused_input off": ({"fused_input": False}, "1", "uint8", False, False),
    "fp32 planes": ({}, "1", "float32", False, False),
    "compact queue, masks": ({}, "1", "uint8", True, True),
    "compact queue, chain_blocks off": ({"chain_blocks": False}, "1", "uint8", True, False),
    "CZ_IP_PAIR=0": ({}, "0", "uint8", False, False),
    "CZ_IP_PAIR=0, chain_blocks off": ({"chain_blocks": False}, "0", "uint8", False, False),
}


def _settings(filters, heads):
    """The settings a net is run with: every switch at 128 filters, the 192-filter kernel choice, the rest plainly."""
    names = ["default", "chain_blocks off", "fused_blocks off"]
    if filters == 128:
        names += ["chain_heads off", "fused_heads off", "fused_input off", "fp32 planes", "compact queue, masks"]
        names += ["compact queue, chain_blocks off"] if heads == (4, 2) else []
    if filters == 192:
        names += ["CZ_IP_PAIR=0", "CZ_IP_PAIR=0, chain_blocks off", "compact queue, masks"]
    return names


def _build(name):
    import torch
    from cchess_alphazero.agent.model import CChessNet, InferenceNet
    filters, blocks, arith, dtype, (npol, nval) = NETS[name]
    torch.manual_seed(filters * 100 + blocks)
    raw = CChessNet(cnn_filter_num=filters, res_layer_num=blocks, policy_filters=npol, value_filters=nval).eval()
    exps = ([0] * blocks, [1] * blocks) if arith and arith.startswith("c6") else None
    g = InferenceNet(raw, getattr(torch, dtype), trunk="mfma", arith=arith, act_exps=exps).cuda()
    assert g.arith_name == (arith or "bf16x3"), (name, g.arith_name)
    return g


@contextlib.contextmanager
def _recording(names):
    """Wrap the _native entry points with recorders that call through; yields the list of calls."""
    import torch
    from cchess_alphazero import _native
    calls, ids = [], {}

    def desc(v):
        if isinstance(v, torch.Tensor):
            name = names.get(v.data_ptr()) or "#%d" % ids.setdefault(v.data_ptr(), len(ids))
            return "%s%s@%s" % (str(v.dtype)[6:], list(v.shape), name)
        if isinstance(v, (tuple, list)):
            return [desc(t) for t in v]
        if isinstance(v, _native.BlockList):
            return {"n": v.n, "fmt_x": list(v.fmt_x) if v.fmt_x is not None else None,
                    "fmt_y": list(v.fmt_y) if v.fmt_y is not None else None,
                    "arrays": [[names.get(p) for p in a] for a in v.arrays]}       # (w1, b1, w2, b2 of every block)
        return v

    def recorder(name, fn):
        sig = inspect.signature(fn)

        def call(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            calls.append([name, {k: desc(v) for k, v in bound.arguments.items()}])
            return fn(*args, **kwargs)
        return call
    saved = {name: getattr(_native, name) for name in ENTRY_POINTS}
    try:
        for name, fn in saved.items():
            setattr(_native, name, recorder(name, fn))
        yield calls, ids
    finally:
        for name, fn in saved.items():
            setattr(_native, name, fn)


def launch_table():
    """{net: {setting: the calls of one forward, or the RuntimeError it raised}} for NETS x _settings."""
    import torch
    from cchess_alphazero.agent.model import calibration_planes
    from test_gpu_masks import _masks_from_planes
    planes8 = calibration_planes(64, 14, seed=9)[:37].contiguous()
    masks = _masks_from_planes(planes8).contiguous()
    rows = torch.randperm(37, generator=torch.Generator().manual_seed(2))[:30].int().cuda()
    count = torch.tensor([23], dtype=torch.int32, device="cuda")
    table = {}
    saved_env = os.environ.get("CZ_IP_PAIR")
    try:
        for net in NETS:
            g = _build(net)
            names = {t.data_ptr(): n for n, t in list(g.named_buffers()) + list(g.named_parameters())}
            table[net] = {}
            for setting in _settings(g.filters, NETS[net][4]):
                attrs, ip_pair, planes_dtype, compact, with_masks = SETTINGS[setting]
                for k in ("chain_blocks", "chain_heads", "fused_blocks", "fused_input", "fused_heads"):
                    setattr(g, k, attrs.get(k, True))
                os.environ["CZ_IP_PAIR"] = ip_pair
                planes = planes8 if planes_dtype == "uint8" else planes8.to(getattr(torch, planes_dtype))
                kw = dict(rows=rows, count=count) if compact else {}
                with _recording(names) as (calls, ids):
                    ids[planes.data_ptr()] = len(ids)                  # (the planes first: the input launch may convert them)
                    try:
                        g(planes, masks=masks if with_masks else None, **kw)
                        table[net][setting] = calls
                    except RuntimeError as e:
                        table[net][setting] = ["RuntimeError", str(e)] + calls
                torch.cuda.synchronize()
            del g
    finally:
        if saved_env is None:
            os.environ.pop("CZ_IP_PAIR", None)
        else:
            os.environ["CZ_IP_PAIR"] = saved_env
    return table


def digest(calls):
    """The digest of one forward's recorded calls (their JSON with sorted keys)."""
    return hashlib.sha256(json.dumps(calls, sort_keys=True, separators=(",", ":")).encode()).hexdigest()[:16]


def test_every_forward_makes_the_recorded_launches():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(launch_table()))                    # (tuples as lists, as the table was recorded)
    assert {net: sorted(s) for net, s in got.items()} == {net: sorted(s) for net, s in want.items()}
    for net in want:
        for setting in want[net]:
            assert digest(got[net][setting]) == want[net][setting], (net, setting, got[net][setting])


@pytest.mark.parametrize("net", ["128x7 c8>3", "192x10 c6>3", "256x26 fp16"])
def test_plans_follow_the_modules_tensors(net):
    """.cpu() / .cuda() replace every buffer: the next forward's chains point at the new ones, and moving again does not
    leave plans of the old tensors behind."""
    from cchess_alphazero.agent.model import calibration_planes
    g = _build(net)
    planes = calibration_planes(64, 14, seed=9)[:37].contiguous()
    for heads in (True, False):
        g.fused_heads = heads
        g(planes)
    cached = len(g._plans)
    assert cached == 2
    for _ in range(2):
        g.cpu().cuda()
        for heads in (True, False):
            g.fused_heads = heads
            g(planes)
        assert len(g._plans) == cached
        chains = 0
        for steps, _ in g._plans.values():
            for st in steps:
                chains += st.bl is not None
                for j, i in enumerate(st.blocks):
                    want = [t.data_ptr() for t in g._block_params(i)]
                    assert [t.data_ptr() for t in (st.w if st.bl is None else st.bl.blocks[j])] == want
                    if st.bl is not None:                           # (the pointer arrays the kernel reads)
                        assert [st.bl.arrays[k][j] for k in range(4)] == want
        assert chains >= 2
