"""The refusals of the network entry points of include/czero.h (the drop-in seam), through ctypes and without a
GPU: the return code and the exact cz_last_error() text of everything an entry point refuses BEFORE it asks the device for
anything, and the places where n_boards == 0 returns CZ_OK ahead of a later check.

Every case ends in CZ_ERR_ARG or in the n_boards == 0 return: none may get past validation (on a GPU machine such a call
would launch a kernel on the dummy host pointers used here).  A refusal never reads what a pointer points to.

Not here, because the entry point queries the device first (without a GPU that call answers CZ_ERR_HIP "cannot query the
device"): the filter / dtype refusal of cz_resblock, and CZ_F16C86 under CZ_IP_PAIR=0 in cz_resblock_chain (pinned in
tests/test_gpu_plain_entry_points.py).  cz_last_error() keeps 255 characters of a message."""
import ctypes as C

import pytest

F32, F16, BF16, U8, F16C8, F16C6, F16C86 = range(7)
IMG_C8, IMG_C6, IMG_PAIR, EXIT_HEADS = range(4)
OK, ERR_ARG = 0, -1

_BUF = C.create_string_buffer(4096)
P = C.addressof(_BUF)               # a dummy host pointer
NB = 3                              # blocks of a chain case


def blocks(n=NB, null_at=None):
    a = (C.c_void_p * max(n, 1))(*([P] * max(n, 1)))
    if null_at is not None:
        a[null_at] = None
    return a


def fmts(*v):
    return (C.c_int * len(v))(*v)


# entry point -> its arguments in order, with values that pass every check made before the device query
BASE = {
    "cz_conv3x3": [("x_hi", P), ("x_lo", P), ("w_packed", P), ("bias", P), ("skip_hi", None), ("skip_lo", None), ("y_hi", P),
                   ("y_lo", P), ("y_f32", None), ("n_boards", 5), ("channels", 128), ("dtype", F16), ("parts", 2), ("relu", 1),
                   ("stream", None)],
    "cz_conv3x3_c8": [("x_hi", P), ("x_c8", P), ("w_packed", P), ("bias", P), ("skip_hi", None), ("skip_c8", None), ("y_hi", P),
                      ("y_c8", P), ("y_f32", None), ("n_boards", 5), ("channels", 128), ("relu", 1), ("stream", None)],
    "cz_input_conv": [("planes", P), ("planes_dtype", U8), ("in_planes", 14), ("w_packed", P), ("bias", P), ("y_hi", P),
                      ("y_lo", P), ("n_boards", 5), ("channels", 128), ("dtype", F16), ("parts", 2), ("relu", 1),
                      ("stream", None)],
    "cz_resblock": [("x_hi", P), ("x_lo", P), ("w1_packed", P), ("bias1", P), ("w2_packed", P), ("bias2", P), ("y_hi", P),
                    ("y_lo", P), ("y_f32", None), ("n_boards", 5), ("channels", 128), ("dtype", F16), ("parts", 2),
                    ("stream", None)],
    "cz_resblock_heads": [("x_hi", P), ("x_lo", P), ("w1_packed", P), ("bias1", P), ("w2_packed", P), ("bias2", P),
                          ("head_w", P), ("head_b", P), ("policy_feat", P), ("value_feat", P), ("n_boards", 5),
                          ("channels", 128), ("dtype", F16), ("n_policy", 4), ("n_value", 2), ("stream", None)],
    "cz_input_resblock": [("planes_u8", P), ("in_planes", 14), ("in_table", P), ("in_bias", P), ("w1_packed", P), ("bias1", P),
                          ("w2_packed", P), ("bias2", P), ("y_hi", P), ("y_lo", P), ("n_boards", 5), ("channels", 128),
                          ("dtype", F16), ("rows", None), ("n_dev", None), ("stream", None)],
    "cz_input_resblock_m": [("planes_u8", P), ("masks", P), ("in_planes", 14), ("in_table", P), ("in_bias", P),
                            ("w1_packed", P), ("bias1", P), ("w2_packed", P), ("bias2", P), ("y_hi", P), ("y_lo", P),
                            ("n_boards", 5), ("channels", 128), ("dtype", F16), ("rows", None), ("n_dev", None),
                            ("stream", None)],
    "cz_resblock_chain": [("x_hi", P), ("x_img", P), ("n_blocks", NB), ("w1_packed", blocks()), ("bias1", blocks()),
                          ("w2_packed", blocks()), ("bias2", blocks()), ("y_hi", P), ("y_img", P), ("y_f32", None),
                          ("n_boards", 5), ("channels", 192), ("dtype", F16C8), ("n_dev", None), ("stream", None)],
    "cz_tower": [("x_hi", P), ("x_img", P), ("n_blocks", NB), ("w1_packed", blocks()), ("bias1", blocks()),
                 ("w2_packed", blocks()), ("bias2", blocks()), ("fmt_x", None), ("fmt_y", None), ("exit_fmt", IMG_C6),
                 ("y_hi", P), ("y_img", P), ("head_w", None), ("head_b", None), ("policy_feat", None), ("value_feat", None),
                 ("n_policy", 0), ("n_value", 0), ("n_boards", 5), ("n_dev", None), ("stream", None)],
    "cz_tower_pairs": [("x_hi", P), ("x_lo", P), ("n_blocks", NB), ("w1_packed", blocks()), ("bias1", blocks()),
                       ("w2_packed", blocks()), ("bias2", blocks()), ("y_hi", P), ("y_lo", P), ("head_w", None),
                       ("head_b", None), ("policy_feat", None), ("value_feat", None), ("n_policy", 0), ("n_value", 0),
                       ("n_boards", 5), ("dtype", F16), ("n_dev", None), ("stream", None)],
    "cz_tower_plain": [("x", P), ("n_blocks", NB), ("w1_packed", blocks()), ("bias1", blocks()), ("w2_packed", blocks()),
                       ("bias2", blocks()), ("y", P), ("n_boards", 5), ("channels", 256), ("dtype", F16), ("n_dev", None),
                       ("stream", None)],
    "cz_split_bias_act": [("x", P), ("bias", P), ("y_hi", P), ("y_lo", P), ("n_elems", 5 * 90 * 128), ("channels", 128),
                          ("dtype", F16), ("parts", 2), ("relu", 1), ("stream", None)],
    "cz_head_convs": [("x", P), ("dtype", F16), ("w", P), ("bias", P), ("policy_feat", P), ("value_feat", P), ("n_boards", 5),
                      ("channels", 128), ("n_policy", 4), ("n_value", 2), ("stream", None)],
    "cz_heads_tail": [("policy_feat", P), ("n_policy_feat", 360), ("wp_packed", P), ("bias_p", P), ("n_labels", 2086),
                      ("value_feat", P), ("n_value_feat", 180), ("w1_packed", P), ("bias1", P), ("n_hidden", 256), ("w2", P),
                      ("b2", 0.0), ("policy", P), ("value", P), ("stats_scratch", P), ("n_boards", 5), ("dtype", F16),
                      ("normalize", 1), ("n_dev", None), ("stream", None)],
}
BASE["cz_input_conv_q"] = BASE["cz_input_conv"][:-1] + [("rows", None), ("n_dev", None), ("stream", None)]
BASE["cz_resblock_q"] = BASE["cz_resblock"][:-1] + [("n_dev", None), ("stream", None)]
BASE["cz_resblock_heads_q"] = BASE["cz_resblock_heads"][:-1] + [("n_dev", None), ("stream", None)]
HEADS = dict(head_w=P, head_b=P, policy_feat=P, value_feat=P, n_policy=4, n_value=2)      # the heads exits of the two towers

MSG = {
    "conv_arg": "cz_conv3x3: bad argument",
    "conv_kind": "cz_conv3x3: unsupported channels / dtype (channels 32|128|192|256, bf16|f16)",
    "c8_arg": "cz_conv3x3_c8: bad argument (128 or 192 filters; output: y_f32, or the operand pair y_hi + y_c8)",
    "ic_arg": "cz_input_conv: bad argument",
    "ic_kind": "cz_input_conv: unsupported channels / dtype",
    "rb_arg": "cz_resblock: bad argument (parts = 1 writes y_hi only; y_f32 needs parts = 2)",
    "rbh_arg": "cz_resblock_heads: bad argument (split operands; n_policy + n_value == 6)",
    "rbh_kind": "cz_resblock_heads: 128 filters, bf16 / f16 split operands only (use cz_resblock + cz_head_convs)",
    "irb_arg": "cz_input_resblock: bad argument (u8 planes, in_planes even and <= 32)",
    "irb_kind": "cz_input_resblock: 128 filters; bf16 / f16 split operands or the c8 / c6 pair (use cz_input_conv + cz_resblock)",
    "chain_arg": "cz_resblock_chain: bad argument (192 filters, 1 .. 12 blocks, dtype CZ_F16C8 / CZ_F16C6 / CZ_F16C86 with y_f32 "
                 "or y_hi + y_img, or CZ_F16 / CZ_BF16 pair blocks with y_f32 or y_hi + y_lo)",
    "chain_null": "cz_resblock_chain: null block parameter",
    "tower_arg": "cz_tower: bad argument (1 .. 8 blocks; exit CZ_IMG_C8 / CZ_IMG_C6 / CZ_IMG_PAIR with y_hi + y_img, or "
                 "CZ_EXIT_HEADS with n_policy + n_value == 6)",
    "tower_null": "cz_tower: null block parameter",
    "tower_fmt": "cz_tower: one image format per chain, CZ_IMG_C8 or CZ_IMG_C6 (a hybrid tower is one chain per arithmetic -- "
                 "the exit of the first hands over; pair blocks: cz_tower_pairs)",
    "tower_exit": "cz_tower: a c6 chain ends on a c6 or c8 image, a c8 chain on a c8 image or fp16 pairs",
    "pairs_arg": "cz_tower_pairs: bad argument (1 .. 8 blocks of (hi, lo) f16 / bf16 operands; y_hi + y_lo, or the head "
                 "arguments with n_policy + n_value == 6)",
    "pairs_null": "cz_tower_pairs: null block parameter",
    "plain_arg": "cz_tower_plain: bad argument (256 filters, plain f16 / bf16 operands, 1 .. 24 blocks)",
    "plain_null": "cz_tower_plain: null block parameter",
    "split_arg": "cz_split_bias_act: bad argument",
    "hc_arg": "cz_head_convs: bad argument (channels % 32 == 0, n_policy + n_value == 6)",
    "hc_many": "cz_head_convs: too many boards",
    "hc_dtype": "cz_head_convs: unknown dtype",
    "ht_arg": "cz_heads_tail: bad argument (n_labels even; 180 or 360 features per head: 2 or 4 filters x 90 squares; dtype of "
              "the packed pairs: CZ_BF16 or CZ_F16)",
}

CASES = []      # (entry point, overrides of BASE, return code, MSG key or None)


def refuse(fn, msg, *overrides):
    CASES.extend((fn, o, ERR_ARG, msg) for o in overrides)


def passes(fn, *overrides):       # n_boards == 0 (n_elems == 0): CZ_OK
    CASES.extend((fn, o, OK, None) for o in overrides)


def nulls(*names):
    return [{n: None} for n in names]


def block_nulls(at=1):
    return [{n: blocks(null_at=at)} for n in ("w1_packed", "bias1", "w2_packed", "bias2")]


def chain(n, null_in=None):       # all four arrays at n blocks, the last entry of one of them NULL
    return dict({k: blocks(n, n - 1 if k == null_in else None) for k in ("w1_packed", "bias1", "w2_packed", "bias2")}, n_blocks=n)


def sums():                       # n_policy + n_value == 6 with both >= 1
    return [dict(n_policy=0, n_value=6), dict(n_policy=6, n_value=0), dict(n_policy=2, n_value=3), dict(n_policy=4, n_value=3)]


refuse("cz_conv3x3", "conv_arg", *nulls("x_hi", "x_lo", "w_packed", "bias", "y_hi", "y_lo"), dict(n_boards=-1), dict(parts=0),
       dict(parts=3), dict(skip_hi=P), dict(parts=1, y_hi=None))
refuse("cz_conv3x3", "conv_kind", *[dict(dtype=d) for d in (F32, U8, F16C8, F16C6, F16C86, 7)],
       *[dict(channels=c) for c in (0, 64, 160, 512)], dict(channels=64, parts=1, dtype=BF16))
passes("cz_conv3x3", dict(n_boards=0), dict(n_boards=0, dtype=F32, channels=64))

refuse("cz_conv3x3_c8", "c8_arg", *nulls("x_hi", "x_c8", "w_packed", "bias", "y_hi", "y_c8"), dict(n_boards=-1), dict(skip_hi=P),
       *[dict(channels=c) for c in (0, 32, 64, 256)])
passes("cz_conv3x3_c8", dict(n_boards=0))

for fn in ("cz_input_conv", "cz_input_conv_q"):         # a _q form reports under the plain form's name
    refuse(fn, "ic_arg", *nulls("planes", "w_packed", "bias", "y_hi", "y_lo"), dict(n_boards=-1), dict(parts=0), dict(parts=3),
           dict(in_planes=0), dict(in_planes=33))
    refuse(fn, "ic_kind", *[dict(dtype=d) for d in (F32, U8, F16C6, F16C86, 7)], *[dict(channels=c) for c in (0, 64, 160)],
           dict(planes_dtype=4), dict(planes_dtype=-1), dict(dtype=F16C8, channels=256), dict(dtype=F16C8, channels=32),
           dict(dtype=F16C8, parts=1), dict(dtype=F16C8, planes_dtype=F16), dict(dtype=F16C8, planes_dtype=BF16))
    passes(fn, dict(n_boards=0), dict(n_boards=0, dtype=F32))

for fn in ("cz_resblock", "cz_resblock_q"):
    refuse(fn, "rb_arg", *nulls("x_hi", "x_lo", "w1_packed", "bias1", "w2_packed", "bias2", "y_hi", "y_lo"), dict(n_boards=-1),
           dict(parts=0), dict(parts=3), dict(parts=1, y_hi=None), dict(parts=1, y_f32=P))
    # n_boards == 0 returns before the filter / dtype check
    passes(fn, dict(n_boards=0), dict(n_boards=0, channels=64), dict(n_boards=0, dtype=F32), dict(n_boards=0, dtype=7))

for fn in ("cz_resblock_heads", "cz_resblock_heads_q"):
    refuse(fn, "rbh_arg", *nulls("x_hi", "x_lo", "w1_packed", "bias1", "w2_packed", "bias2", "head_w", "head_b", "policy_feat",
                                 "value_feat"), dict(n_boards=-1), *sums())
    refuse(fn, "rbh_kind", *[dict(channels=c) for c in (0, 192, 256)], *[dict(dtype=d) for d in (F32, U8, F16C86, 7)])
    passes(fn, dict(n_boards=0), dict(n_boards=0, channels=192), dict(n_boards=0, dtype=F32))

for fn in ("cz_input_resblock", "cz_input_resblock_m"):
    refuse(fn, "irb_arg", *nulls("in_table", "in_bias", "w1_packed", "bias1", "w2_packed", "bias2", "y_hi", "y_lo"),
           dict(n_boards=-1), dict(in_planes=0), dict(in_planes=33), dict(in_planes=34), dict(in_planes=13))
    # here the filter / dtype check comes BEFORE the n_boards == 0 return
    refuse(fn, "irb_kind", *[dict(channels=c) for c in (0, 192, 256)], *[dict(dtype=d) for d in (F32, U8, F16C86, 7)],
           dict(n_boards=0, channels=192), dict(n_boards=0, dtype=F32))
    passes(fn, dict(n_boards=0), *[dict(n_boards=0, dtype=d) for d in (BF16, F16C8, F16C6)])
refuse("cz_input_resblock", "irb_arg", dict(planes_u8=None))
refuse("cz_input_resblock_m", "irb_arg", dict(planes_u8=None, masks=None))
passes("cz_input_resblock_m", dict(n_boards=0, planes_u8=None), dict(n_boards=0, masks=None))

refuse("cz_resblock_chain", "chain_arg", *nulls("x_hi", "x_img", "w1_packed", "bias1", "w2_packed", "bias2", "y_hi", "y_img"),
       dict(n_boards=-1), dict(n_blocks=0), dict(n_blocks=13), dict(n_blocks=-1), *[dict(channels=c) for c in (0, 128, 256)],
       *[dict(dtype=d) for d in (F32, U8, 7)], dict(dtype=F16, y_hi=None), dict(dtype=F16, channels=128))
for dt in (F16C8, F16C6, F16C86, F16, BF16):
    refuse("cz_resblock_chain", "chain_null", *[dict(o, dtype=dt) for o in block_nulls()],
           dict(w1_packed=blocks(null_at=NB - 1), dtype=dt, n_boards=0))      # ... before the n_boards == 0 return
    passes("cz_resblock_chain", dict(n_boards=0, dtype=dt), dict(n_boards=0, dtype=dt, y_hi=None, y_img=None, y_f32=P))
passes("cz_resblock_chain", dict(chain(12), n_boards=0))
refuse("cz_resblock_chain", "chain_null", dict(bias2=blocks(null_at=0)), chain(12, "w2_packed"))

refuse("cz_tower", "tower_arg", *nulls("x_hi", "x_img", "w1_packed", "bias1", "w2_packed", "bias2", "y_hi", "y_img"),
       dict(n_boards=-1), dict(n_blocks=0), dict(n_blocks=9), dict(exit_fmt=4), dict(exit_fmt=-1),
       *[dict(HEADS, exit_fmt=EXIT_HEADS, **{k: None}) for k in ("head_w", "head_b", "policy_feat", "value_feat")],
       *[dict(HEADS, exit_fmt=EXIT_HEADS, **s) for s in sums()])
refuse("cz_tower", "tower_null", *block_nulls(), *block_nulls(at=0), dict(n_boards=0, bias1=blocks(null_at=NB - 1)),
       chain(8, "w2_packed"), dict(fmt_x=fmts(1, 1, 0), fmt_y=fmts(1, 1, 0), bias1=blocks(null_at=1)))
refuse("cz_tower", "tower_fmt",
       dict(fmt_x=fmts(1, 0, 1), fmt_y=fmts(1, 0, 1)), dict(fmt_x=fmts(0, 0, 1), fmt_y=fmts(0, 0, 1)),     # mixed within a chain
       dict(fmt_x=fmts(0, 0, 0), fmt_y=fmts(0, 0, 1), exit_fmt=IMG_C8), dict(fmt_x=fmts(0, 0, 0), exit_fmt=IMG_C8),  # fy != fx
       dict(fmt_y=fmts(0, 0, 0)), dict(fmt_x=fmts(2, 2, 2), fmt_y=fmts(2, 2, 2)), dict(fmt_x=fmts(3, 3, 3), fmt_y=fmts(3, 3, 3)),
       dict(fmt_x=fmts(0, 1, 1), fmt_y=fmts(0, 1, 1), exit_fmt=EXIT_HEADS, **HEADS),
       dict(fmt_x=fmts(2, 1, 1), fmt_y=fmts(2, 1, 1), w1_packed=blocks(null_at=1)),      # block 0's format before block 1's NULL
       dict(fmt_x=fmts(1, 0, 1), fmt_y=fmts(1, 0, 1), n_boards=0))
refuse("cz_tower", "tower_exit", dict(exit_fmt=IMG_PAIR), dict(fmt_x=fmts(1, 1, 1), fmt_y=fmts(1, 1, 1), exit_fmt=IMG_PAIR),
       dict(fmt_x=fmts(0, 0, 0), fmt_y=fmts(0, 0, 0), exit_fmt=IMG_C6), dict(exit_fmt=IMG_PAIR, n_boards=0))
passes("cz_tower", dict(n_boards=0), dict(n_boards=0, exit_fmt=IMG_C8), dict(n_boards=0, exit_fmt=EXIT_HEADS, **HEADS),
       dict(n_boards=0, fmt_x=fmts(0, 0, 0), fmt_y=fmts(0, 0, 0), exit_fmt=IMG_PAIR), dict(n_boards=0, n_blocks=1),
       dict(chain(8), n_boards=0))

refuse("cz_tower_pairs", "pairs_arg", *nulls("x_hi", "x_lo", "w1_packed", "bias1", "w2_packed", "bias2", "y_hi", "y_lo"),
       dict(n_boards=-1), dict(n_blocks=0), dict(n_blocks=9), *[dict(dtype=d) for d in (F32, U8, F16C8, F16C6, 7)],
       *[dict(HEADS, **{k: None}) for k in ("head_b", "policy_feat", "value_feat")], *[dict(HEADS, **s) for s in sums()])
refuse("cz_tower_pairs", "pairs_null", *block_nulls(), *block_nulls(at=0), dict(n_boards=0, bias2=blocks(null_at=NB - 1)),
       dict(HEADS, w1_packed=blocks(null_at=2)))
passes("cz_tower_pairs", dict(n_boards=0), dict(n_boards=0, dtype=BF16), dict(HEADS, n_boards=0, y_hi=None, y_lo=None))

refuse("cz_tower_plain", "plain_arg", *nulls("x", "y", "w1_packed", "bias1", "w2_packed", "bias2"), dict(n_boards=-1),
       dict(n_blocks=0), dict(n_blocks=25), *[dict(channels=c) for c in (0, 128, 192)],
       *[dict(dtype=d) for d in (F32, U8, F16C8, 7)])
refuse("cz_tower_plain", "plain_null", *block_nulls(), *block_nulls(at=0), dict(n_boards=0, w2_packed=blocks(null_at=NB - 1)),
       chain(24, "bias1"))
passes("cz_tower_plain", dict(n_boards=0), dict(n_boards=0, dtype=BF16), dict(chain(24), n_boards=0))

refuse("cz_split_bias_act", "split_arg", *nulls("x", "y_hi", "y_lo"), dict(parts=0), dict(parts=3), dict(channels=0),
       dict(channels=-4), dict(channels=6, n_elems=60), dict(n_elems=5 * 90 * 128 + 4), *[dict(dtype=d) for d in (F32, U8, F16C8)])
passes("cz_split_bias_act", dict(n_elems=0), dict(n_elems=0, bias=None), dict(n_elems=0, parts=1, y_lo=None))

refuse("cz_head_convs", "hc_arg", *nulls("x", "w", "bias", "policy_feat", "value_feat"), dict(n_boards=-1), dict(channels=0),
       dict(channels=48), dict(channels=1056), *sums())
refuse("cz_head_convs", "hc_many", dict(n_boards=(1 << 31) // 90 + 1))
refuse("cz_head_convs", "hc_dtype", *[dict(dtype=d) for d in (U8, F16C8, 7, -1)])
passes("cz_head_convs", dict(n_boards=0), dict(n_boards=0, dtype=U8))

refuse("cz_heads_tail", "ht_arg", *nulls("policy_feat", "wp_packed", "bias_p", "value_feat", "w1_packed", "bias1", "w2", "policy",
                                         "value", "stats_scratch"), dict(n_boards=-1), *[dict(dtype=d) for d in (F32, U8, F16C8)],
       dict(n_labels=0), dict(n_labels=1), dict(n_labels=2087), dict(n_hidden=0), dict(n_policy_feat=0), dict(n_policy_feat=90),
       dict(n_policy_feat=270), dict(n_value_feat=90), dict(n_value_feat=0))
passes("cz_heads_tail", dict(n_boards=0), dict(n_boards=0, dtype=BF16, n_policy_feat=180, n_value_feat=360))


def _id(case):
    fn, over, rc, msg = case
    what = ",".join(f"{k}={'NULL' if v is None else 'P' if v == P else v if isinstance(v, (int, float)) else 'set'}" for k, v in over.items())
    return f"{fn}[{what}]->{msg or rc}"


def call(fn, over):
    from cchess_alphazero import _native
    L = _native.lib()
    names = [n for n, _ in BASE[fn]]
    assert set(over) <= set(names), (fn, over)
    args = [over.get(n, v) for n, v in BASE[fn]]
    rc = getattr(L, fn)(*args)
    return rc, L.cz_last_error().decode()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_refusal(case):
    fn, over, want_rc, msg = case
    assert want_rc == OK and over.get("n_boards", over.get("n_elems")) == 0 or want_rc == ERR_ARG      # nothing may launch
    rc, err = call(fn, over)
    assert rc == want_rc, (fn, over, rc, err)
    if msg is not None:
        assert err == MSG[msg][:255], (fn, over, err)


def test_every_entry_point_is_covered():
    assert {c[0] for c in CASES} == set(BASE)
    for fn in BASE:
        assert any(c[0] == fn and c[2] == OK for c in CASES) and any(c[0] == fn and c[2] == ERR_ARG for c in CASES)
