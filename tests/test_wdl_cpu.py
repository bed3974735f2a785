"""The win / draw / loss value head without a GPU: the model's files and shapes, the command line's refusals, and the
sharpness of tests/wdl_check.py's bounds (which tests/test_gpu_wdl_tail.py holds cz_heads_tail_wdl to) on a numpy model of
the kernel, in the spirit of tests/test_dense_bounds_cpu.py."""
import json
import os

import numpy as np
import pytest

import f16_pairs as fp
import wdl_check as wc

SMALL = dict(cnn_filter_num=16, res_layer_num=1, value_fc_size=24)


# ---- model files and shapes --------------------------------------------------------------------------------------------------
def _model(tmp_path, monkeypatch, **kw):
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    import torch
    from cchess_alphazero.agent.model import CChessModel, CChessNet
    from cchess_alphazero.config import Config
    m = CChessModel(Config("mini"))
    torch.manual_seed(1)
    m.model = CChessNet(**SMALL, **kw)
    return m


def test_wdl_model_survives_save_and_load(tmp_path, monkeypatch):
    import torch
    from cchess_alphazero.agent.model import CChessModel
    m = _model(tmp_path, monkeypatch, value_outputs=3)
    cfg_path, w_path = str(tmp_path / "m.json"), str(tmp_path / "m.h5")
    m.save(cfg_path, w_path)
    assert json.load(open(cfg_path))["value_outputs"] == 3
    back = CChessModel(m.config)
    assert back.load(cfg_path, w_path)
    assert back.model.cfg == m.model.cfg and back.model.wdl_head
    assert tuple(back.model.value_out.weight.shape) == (3, SMALL["value_fc_size"])
    x = (torch.rand((5, 14, 10, 9), generator=torch.Generator().manual_seed(2)) < 0.1).float()
    with torch.no_grad():
        for a, b in zip(m.model.eval()(x, logits=True), back.model.eval()(x, logits=True)):
            assert torch.equal(a, b)


def test_model_file_without_the_key_is_a_scalar_model(tmp_path, monkeypatch):
    from cchess_alphazero.agent.model import CChessModel, CChessNet
    m = _model(tmp_path, monkeypatch)
    cfg_path, w_path = str(tmp_path / "m.json"), str(tmp_path / "m.h5")
    m.save(cfg_path, w_path)
    cfg = json.load(open(cfg_path))
    assert cfg.pop("value_outputs") == 1                # a file written before the key existed
    json.dump(cfg, open(cfg_path, "w"))
    back = CChessModel(m.config)
    assert back.load(cfg_path, w_path)
    assert not back.model.wdl_head and back.model.cfg["value_outputs"] == 1
    ref = {k: tuple(v.shape) for k, v in CChessNet(**SMALL).state_dict().items()}
    assert {k: tuple(v.shape) for k, v in back.model.state_dict().items()} == ref
    assert ref["value_out.weight"] == (1, SMALL["value_fc_size"]) and ref["value_out.bias"] == (1,)
    with pytest.raises(ValueError, match="value_outputs"):
        CChessNet(**SMALL, value_outputs=2)


def test_forward_shapes_of_both_heads():
    import torch
    from cchess_alphazero.agent.model import CChessNet, flops_per_position
    torch.manual_seed(3)
    x = (torch.rand((4, 14, 10, 9)) < 0.1).float()
    scalar, wdl = CChessNet(**SMALL).eval(), CChessNet(**SMALL, value_outputs=3).eval()
    with torch.no_grad():
        for net in (scalar, wdl):
            p, v = net(x)
            assert tuple(p.shape) == (4, 2086) and tuple(v.shape) == (4,)
            assert torch.allclose(p.sum(1), torch.ones(4), atol=1e-5) and (v.abs() <= 1).all()
        lp, lv = scalar(x, logits=True)
        assert tuple(lp.shape) == (4, 2086) and tuple(lv.shape) == (4,)
        lp, lv = wdl(x, logits=True)
        assert tuple(lp.shape) == (4, 2086) and tuple(lv.shape) == (4, 3)
        w = wdl.wdl(x)
        assert tuple(w.shape) == (4, 3) and torch.allclose(w.sum(1), torch.ones(4), atol=1e-6)
        assert torch.equal(wdl(x)[1], w[:, 0] - w[:, 2])
        assert torch.equal(w, torch.softmax(lv, dim=1))
        with pytest.raises(RuntimeError, match="scalar value head"):
            scalar.wdl(x)
    assert flops_per_position(wdl.cfg) - flops_per_position(scalar.cfg) == 2 * 2 * SMALL["value_fc_size"]


def test_inference_net_library_path_computes_the_same_value():
    """The torch tail of InferenceNet (trunk="library" runs on the CPU): value = P(win) - P(loss) of the folded network, and
    wdl= receives the probabilities; a scalar net refuses wdl=."""
    import torch
    from cchess_alphazero.agent.model import CChessNet, InferenceNet
    torch.manual_seed(4)
    x = (torch.rand((6, 14, 10, 9)) < 0.1).float()
    net = CChessNet(**SMALL, value_outputs=3).eval()
    inf = InferenceNet(net, torch.float32, trunk="library")
    w = torch.empty((6, 3))
    p, v = inf(x, wdl=w)
    with torch.no_grad():
        pr, vr = net(x)
        wr = net.wdl(x)
    assert tuple(v.shape) == (6,) and (p - pr).abs().max() < 1e-5 and (v - vr).abs().max() < 1e-5
    assert (w - wr).abs().max() < 1e-5 and torch.equal(v, w[:, 0] - w[:, 2])
    with pytest.raises(RuntimeError, match="scalar value head"):
        InferenceNet(CChessNet(**SMALL).eval(), torch.float32, trunk="library")(x, wdl=w)


def test_keras_config_with_three_value_outputs_is_refused():
    from cchess_alphazero.lib import keras_io
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_model", "model_128f.json")
    cfg = json.load(open(gold))
    assert keras_io.config_from_keras(cfg)["cnn_filter_num"] == 128         # as it stands: a scalar model
    names = keras_io.names_from_keras(cfg)
    for layer in keras_io._layers(cfg):
        if layer["name"] == names["value_out"]:
            layer["config"]["units"] = 3
    with pytest.raises(keras_io.KerasFormatError, match="3 outputs"):
        keras_io.config_from_keras(cfg)


# ---- the command line --------------------------------------------------------------------------------------------------------
def _build(argv):
    from cchess_alphazero import manager
    return manager.build_config(manager.create_parser().parse_args(argv))


@pytest.mark.parametrize("cmd", ["self", "eval", "play"])
def test_value_head_is_an_option_of_opt_alone(cmd):
    with pytest.raises(SystemExit, match="--value-head is an option of `run.py opt`"):
        _build([cmd, "--value-head", "wdl"])
    with pytest.raises(SystemExit, match="--value-head is an option of `run.py opt`"):
        _build([cmd, "--value-head", "scalar"])


def test_value_head_reaches_the_trainer_config():
    assert _build(["opt"]).trainer.value_head is None
    assert _build(["opt", "--value-head", "wdl"]).trainer.value_head == "wdl"
    assert _build(["opt", "--value-head", "scalar", "--q-ratio", "0.5"]).trainer.value_head == "scalar"
    with pytest.raises(SystemExit):
        _build(["opt", "--value-head", "three"])


def test_q_ratio_with_a_wdl_head_is_refused():
    with pytest.raises(SystemExit, match="scalar q does not determine a distribution"):
        _build(["opt", "--value-head", "wdl", "--q-ratio", "0.25"])


def _worker(tmp_path, monkeypatch, best_outputs, **trainer):
    """An OptimizeWorker whose best model on disk has `best_outputs` value outputs (None: no best model)."""
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    import torch
    from cchess_alphazero.agent.model import CChessModel, CChessNet
    from cchess_alphazero.config import Config
    from cchess_alphazero.lib.model_helper import save_as_best_model
    from cchess_alphazero.worker import optimize
    cfg = Config("mini")
    cfg.opts.new = False
    for k, v in trainer.items():
        setattr(cfg.trainer, k, v)
    cfg.resource.create_directories()
    if best_outputs is not None:
        m = CChessModel(cfg)
        torch.manual_seed(5)
        m.model = CChessNet(**SMALL, value_outputs=best_outputs)
        save_as_best_model(m)
    return optimize.OptimizeWorker(cfg)


@pytest.mark.parametrize("best,flag", [(1, "wdl"), (3, "scalar")])
def test_a_head_that_contradicts_the_best_model_is_refused(tmp_path, monkeypatch, best, flag):
    w = _worker(tmp_path, monkeypatch, best, value_head=flag)
    with pytest.raises(ValueError) as e:
        w.load_model()
    assert "scalar" in str(e.value) and "wdl" in str(e.value) and f"--value-head {flag}" in str(e.value)


def test_q_ratio_with_a_wdl_best_model_is_refused(tmp_path, monkeypatch):
    w = _worker(tmp_path, monkeypatch, 3, q_ratio=0.5)
    with pytest.raises(ValueError, match="scalar q does not determine a distribution"):
        w.load_model()


def test_window_loss_refuses_q_ratio_for_wdl_logits():
    import torch
    from cchess_alphazero.lib.replay_window import ReplayWindow
    win = ReplayWindow.__new__(ReplayWindow)
    win.w = None
    with pytest.raises(ValueError, match="scalar q does not determine a distribution"):
        ReplayWindow.loss(win, torch.zeros((2, 2086)), torch.zeros((2, 3)), torch.zeros(2, dtype=torch.int32), q_ratio=0.5)
    with pytest.raises(ValueError, match=r"\[B, 3\]"):
        ReplayWindow.loss(win, torch.zeros((2, 2086)), torch.zeros((2, 2)), torch.zeros(2, dtype=torch.int32))


# ---- the bound is not vacuous ------------------------------------------------------------------------------------------------
def hidden_model(x, w, bias, drop_lh=False):
    """k_fc_tile's hidden layer for fp16 pairs in numpy (tests/test_dense_bounds_cpu.kernel_model, rounded once per matrix
    instruction): fp32 pre-activations [n, n_hidden].  drop_lh: without the w_lo x_hi term."""
    xh, xl = (t.astype(np.float64) for t in fp.split16(x))
    wh, wl = (t.astype(np.float64) for t in fp.split16(w))
    acc = np.zeros((x.shape[0], w.shape[0]), dtype=np.float32)
    for k0 in range(0, x.shape[1], 16):
        k = slice(k0, k0 + 16)
        for a, b in [(xh, wh)] + ([] if drop_lh else [(xh, wl)]) + [(xl, wh)]:
            acc = (acc + a[:, k] @ b[:, k].T).astype(np.float32)
    return acc + bias.astype(np.float32)


def tail_model(hidden, w2, b2, swap=False):
    """The finish of k_fc_tile<WDL> in numpy fp32: (wdl [n, 3], v [n]).  The dot products are added unit by unit in index order,
    every product and sum rounded (another order than the kernel's lanes and waves: the bound holds for any).  swap: the faulty
    kernel that reads the loss row for the win class and the other way round."""
    f = np.float32
    h = np.maximum(hidden, f(0))
    rows = [2, 1, 0] if swap else [0, 1, 2]
    l = np.zeros((hidden.shape[0], 3), dtype=f)
    for k in range(3):
        acc = np.zeros(hidden.shape[0], dtype=f)
        for j in range(hidden.shape[1]):
            acc = (acc + (h[:, j] * w2[rows[k], j]).astype(f)).astype(f)
        l[:, k] = acc + f(b2[rows[k]])
    m = np.maximum(np.maximum(l[:, 0], l[:, 2]), l[:, 1])
    e = np.exp((l - m[:, None]).astype(f)).astype(f)
    s = ((e[:, 0] + e[:, 2]).astype(f) + e[:, 1]).astype(f)
    return (e / s[:, None]).astype(f), ((e[:, 0] - e[:, 2]).astype(f) / s).astype(f)


@pytest.mark.parametrize("f,n_hid", [(180, 100), (360, 33)])
def test_wdl_bounds_pass_the_arithmetic_and_catch_its_faults(f, n_hid):
    """On the mixed data of f16_pairs.dense_features: the clean model stays inside the bounds on wdl and v (both sets of
    operands); a model that drops the w_lo x_hi term and one with win and loss swapped exceed them."""
    rng = np.random.default_rng(f + n_hid)
    n = 48
    x = fp.dense_features("mixed", n, f, rng)
    w1 = (rng.standard_normal((n_hid, f)) * 0.1).astype(np.float32)
    b1 = (rng.standard_normal(n_hid) * 0.2).astype(np.float32)
    w2 = (rng.standard_normal((3, n_hid)) * 0.2).astype(np.float32)
    b2 = tuple(float(np.float32(b)) for b in (0.13, -0.21, 0.05))
    xp = tuple(t.astype(np.float64) for t in fp.split16(x))
    wp = tuple(t.astype(np.float64) for t in fp.split16(w1))
    check = fp.DenseCheck(xp, wp, x.astype(np.float64), w1.astype(np.float64))
    h_a, hb_a, h_b, hb_b = check.bounds(b1.astype(np.float64))
    # as the GPU test: the ordinary rows' softmax out of saturation
    q = np.quantile(np.abs(np.maximum(h_b, 0) @ w2.astype(np.float64).T), 0.93)
    if q > 1.8:
        w2 = (w2.astype(np.float64) * (1.8 / q)).astype(np.float32)
    refs = [wc.wdl_check(h, hb, w2.astype(np.float64), b2) for h, hb in ((h_a, hb_a), (h_b, hb_b))]

    def ratios(wdl, v):
        return max(max((np.abs(wdl - r["p"]) / r["bp"]).max(), (np.abs(v - r["v"]) / r["bv"]).max()) for r in refs)
    clean = tail_model(hidden_model(x, w1, b1), w2, b2)
    got = {"clean": ratios(*clean), "no w_lo x_hi": ratios(*tail_model(hidden_model(x, w1, b1, drop_lh=True), w2, b2)),
           "W and L swapped": ratios(*tail_model(hidden_model(x, w1, b1), w2, b2, swap=True))}
    print(f, n_hid, {k: f"{v:.3g}" for k, v in got.items()})
    assert got["clean"] <= 1.0, got
    assert got["no w_lo x_hi"] > 1.0 and got["W and L swapped"] > 1.0, got
    assert (np.abs(clean[0].astype(np.float64).sum(1) - 1.0) <= wc.ROWSUM_TOL).all()
    # the exact symmetry holds in the model as it must in the kernel
    sw = tail_model(hidden_model(x, w1, b1), w2[[2, 1, 0]], b2[::-1])
    assert np.array_equal(sw[1], -clean[1]) and np.array_equal(sw[0][:, [2, 1, 0]], clean[0])


# ---- the refusals of the two entry points (before anything is asked of a device) -------------------------------------------------
def test_heads_tail_wdl_has_the_refusals_of_heads_tail():
    """cz_heads_tail_wdl through ctypes, in the manner of tests/test_nn_entry_args_cpu.py: CZ_ERR_ARG and the message for
    everything cz_heads_tail refuses, wdl = NULL accepted, n_boards == 0 returns CZ_OK first."""
    import ctypes as C
    from cchess_alphazero import _native
    import test_nn_entry_args_cpu as ea
    L = _native.lib()
    P = ea.P
    base = [("policy_feat", P), ("n_policy_feat", 360), ("wp_packed", P), ("bias_p", P), ("n_labels", 2086), ("value_feat", P),
            ("n_value_feat", 180), ("w1_packed", P), ("bias1", P), ("n_hidden", 256), ("w2", P), ("b2_win", 0.0),
            ("b2_draw", 0.0), ("b2_loss", 0.0), ("policy", P), ("value", P), ("wdl", P), ("stats_scratch", P), ("n_boards", 5),
            ("dtype", ea.F16), ("normalize", 1), ("n_dev", None), ("stream", None)]
    msg = ("cz_heads_tail_wdl: bad argument (n_labels even; 180 or 360 features per head: 2 or 4 filters x 90 squares; dtype of "
           "the packed pairs: CZ_BF16 or CZ_F16; wdl may be NULL)")

    def call(**over):
        assert set(over) <= {n for n, _ in base}
        rc = L.cz_heads_tail_wdl(*[over.get(n, v) for n, v in base])
        return rc, L.cz_last_error().decode()
    refused = ea.nulls("policy_feat", "wp_packed", "bias_p", "value_feat", "w1_packed", "bias1", "w2", "policy", "value",
                       "stats_scratch")
    refused += [dict(n_boards=-1), dict(n_labels=0), dict(n_labels=1), dict(n_labels=2087), dict(n_hidden=0),
                dict(n_policy_feat=0), dict(n_policy_feat=90), dict(n_policy_feat=270), dict(n_value_feat=90), dict(n_value_feat=0)]
    refused += [dict(dtype=d) for d in (ea.F32, ea.U8, ea.F16C8)]
    for over in refused:
        assert call(**over) == (ea.ERR_ARG, msg[:255]), over
        assert call(wdl=None, **over)[0] == ea.ERR_ARG, over
    for over in (dict(n_boards=0), dict(n_boards=0, wdl=None), dict(n_boards=0, dtype=ea.BF16, n_policy_feat=180, n_value_feat=360)):
        assert call(**over)[0] == ea.OK, over


def test_policy_wdl_loss_refuses_bad_arguments():
    from cchess_alphazero import _native
    import test_nn_entry_args_cpu as ea
    L = _native.lib()
    P = ea.P
    base = [("logits", P), ("ld", 2086), ("vlogits", P), ("idx", P), ("mirror", None), ("n_rows", 4), ("n_pos", 9),
            ("row_ptr", P), ("vis_label", P), ("vis_count", P), ("nnz", 3), ("played", P), ("z", P), ("row_w", None),
            ("mode", 1), ("w_p", 1.0), ("w_v", 1.0), ("policy_loss", P), ("value_ce", P), ("value_sqerr", P),
            ("grad_logits", P), ("grad_vlogits", P), ("stream", None)]
    msg = "cz_policy_wdl_loss: bad argument (ld >= 2086, mode 0 played / 1 visits)"

    def call(**over):
        assert set(over) <= {n for n, _ in base}
        rc = L.cz_policy_wdl_loss(*[over.get(n, v) for n, v in base])
        return rc, L.cz_last_error().decode()
    for over in ea.nulls("logits", "vlogits", "idx", "played", "z", "row_ptr", "vis_label", "vis_count", "policy_loss", "value_ce",
                         "value_sqerr", "grad_logits", "grad_vlogits") + [dict(n_rows=-1), dict(n_pos=-1), dict(ld=2085),
                                                                          dict(mode=2), dict(nnz=-1)]:
        assert call(**over) == (ea.ERR_ARG, msg), over
    assert call(n_rows=0)[0] == ea.OK and call(n_rows=0, logits=None)[0] == ea.OK
