"""The moves-left output without a GPU: its targets, its meaning m(x), the model's files and shapes, the command line's and
the trainer's refusals, the two entry points' refusals, and the sharpness of tests/moves_left_check.py's bound on x (which
tests/test_gpu_moves_left_tail.py holds cz_heads_tail_ml to) on a numpy model of the kernel, as tests/test_wdl_cpu.py."""
import json
import math

import numpy as np
import pytest

import f16_pairs as fp
import moves_left_check as mc
from cchess_alphazero.lib.replay_window import moves_left_targets

SMALL = dict(cnn_filter_num=16, res_layer_num=1, value_fc_size=24)


# ---- targets and meaning -----------------------------------------------------------------------------------------------------
def test_targets_count_the_record_items_to_the_end_of_the_game():
    """Games of 0, 1, 2 and 7 items in one file: the position before item t of an L-item game gets L - t, the last one 1."""
    from cchess_alphazero.lib.record_decoder import split_games
    init = "rkemsmekr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9/RKEMSMEKR"
    item = ["0001", 1]
    data = []
    for n in (0, 1, 2, 7):
        data += [init] + [list(item) for _ in range(n)]
    lens = [len(g) - 1 for g in split_games(data)]
    assert lens == [0, 1, 2, 7]
    left = moves_left_targets(lens)
    assert left.dtype == np.int32 and left.tolist() == [1, 2, 1, 7, 6, 5, 4, 3, 2, 1]
    assert moves_left_targets([]).shape == (0,) and moves_left_targets([0, 0]).shape == (0,)
    with pytest.raises(ValueError):
        moves_left_targets([3, -1])


def test_meaning_of_the_raw_output():
    import torch
    from cchess_alphazero.agent.model import MOVES_LEFT_BIAS, MOVES_LEFT_DELTA, MOVES_LEFT_UNIT, moves_left_plies
    assert MOVES_LEFT_UNIT == 32.0 == mc.UNIT and MOVES_LEFT_DELTA == 0.5 == mc.DELTA
    m = moves_left_plies(torch.tensor([-100.0, 0.0, 100.0, MOVES_LEFT_BIAS], dtype=torch.float64))
    assert torch.isfinite(m).all() and 0.0 <= m[0].item() < 1e-40
    assert abs(m[1].item() - 32.0 * math.log(2.0)) < 1e-12 and m[2].item() == 3200.0
    assert abs(m[3].item() - 64.0) < 1e-12
    m32 = moves_left_plies(torch.tensor([-100.0, 100.0, MOVES_LEFT_BIAS]))
    assert torch.isfinite(m32).all() and m32[1].item() == 3200.0 and abs(m32[2].item() - 64.0) < 1e-4


# ---- model files and shapes --------------------------------------------------------------------------------------------------
def _model(tmp_path, monkeypatch, seed=1, **kw):
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    import torch
    from cchess_alphazero.agent.model import CChessModel, CChessNet
    from cchess_alphazero.config import Config
    m = CChessModel(Config("mini"))
    torch.manual_seed(seed)
    m.model = CChessNet(**SMALL, **kw)
    return m


TODAY_KEYS = ["cnn_filter_num", "cnn_first_filter_size", "cnn_filter_size", "res_layer_num", "value_fc_size", "input_depth",
              "policy_filters", "value_filters", "n_labels", "value_outputs"]


@pytest.mark.parametrize("outputs", [1, 3])
def test_a_net_without_the_output_writes_the_files_it_wrote(tmp_path, monkeypatch, outputs):
    """No moves_left key, the JSON text of the ten keys a model file has had, no tensor of the new layer, and -- because the
    new layer is built last -- the same draws from the seed for every other layer: the weight file's digest is unchanged."""
    import torch
    plain = _model(tmp_path, monkeypatch, value_outputs=outputs)
    cfg_path, w_path = str(tmp_path / "p" / "m.json"), str(tmp_path / "p" / "m.h5")
    plain.save(cfg_path, w_path)
    text = open(cfg_path).read()
    want = dict(cnn_filter_num=16, cnn_first_filter_size=5, cnn_filter_size=3, res_layer_num=1, value_fc_size=24,
                input_depth=14, policy_filters=4, value_filters=2, n_labels=2086, value_outputs=outputs)
    assert list(want) == TODAY_KEYS and text == json.dumps(want)
    assert not plain.model.moves_left_head and not any("moves_left" in k for k in plain.model.state_dict())
    with_ml = _model(tmp_path, monkeypatch, value_outputs=outputs, moves_left=True)
    sd, sd_ml = plain.model.state_dict(), with_ml.model.state_dict()
    assert list(sd_ml)[:len(sd)] == list(sd) and list(sd_ml)[len(sd):] == ["moves_left_out.weight", "moves_left_out.bias"]
    assert all(torch.equal(sd[k], sd_ml[k]) for k in sd)
    # the digest is that of the state dict alone: dropping the new layer's two tensors gives the plain net's file
    with_ml.model.__delattr__("moves_left_out")
    del with_ml.model.cfg["moves_left"]
    with_ml.save(str(tmp_path / "q" / "m.json"), str(tmp_path / "q" / "m.h5"))
    assert with_ml.digest == plain.digest and open(str(tmp_path / "q" / "m.json")).read() == text


@pytest.mark.parametrize("outputs", [1, 3])
def test_a_net_with_the_output_survives_save_and_load(tmp_path, monkeypatch, outputs):
    import torch
    from cchess_alphazero.agent.model import MOVES_LEFT_BIAS, CChessModel, moves_left_plies
    m = _model(tmp_path, monkeypatch, value_outputs=outputs, moves_left=True)
    assert m.model.moves_left_head and tuple(m.model.moves_left_out.weight.shape) == (1, SMALL["value_fc_size"])
    assert m.model.moves_left_out.bias.item() == pytest.approx(MOVES_LEFT_BIAS, rel=1e-7)
    cfg_path, w_path = str(tmp_path / "m.json"), str(tmp_path / "m.h5")
    m.save(cfg_path, w_path)
    cfg = json.load(open(cfg_path))
    assert cfg["moves_left"] == 1 and list(cfg) == TODAY_KEYS + ["moves_left"]
    back = CChessModel(m.config)
    assert back.load(cfg_path, w_path)
    assert back.model.cfg == m.model.cfg and back.model.moves_left_head
    x = (torch.rand((5, 14, 10, 9), generator=torch.Generator().manual_seed(2)) < 0.1).float()
    with torch.no_grad():
        for logits in (False, True):
            a, b = m.model.eval()(x, logits=logits, moves_left=True), back.model.eval()(x, logits=logits, moves_left=True)
            assert len(a) == len(b) == 3 and tuple(a[2].shape) == (5,)
            assert all(torch.equal(s, t) for s, t in zip(a, b))
            two = m.model(x, logits=logits)                      # without the keyword: what a forward returns today
            assert len(two) == 2 and torch.equal(two[0], a[0]) and torch.equal(two[1], a[1])
        # a fresh model predicts about 64 plies: the bias alone gives 64, the default-initialised row moves it a little
        assert (moves_left_plies(a[2]) - 64.0).abs().max() < 16.0


def test_asking_a_net_without_the_output_raises():
    import torch
    from cchess_alphazero.agent.model import CChessNet, InferenceNet, flops_per_position
    x = (torch.rand((3, 14, 10, 9), generator=torch.Generator().manual_seed(3)) < 0.1).float()
    plain, with_ml = CChessNet(**SMALL).eval(), CChessNet(**SMALL, moves_left=True).eval()
    with pytest.raises(RuntimeError, match="no moves-left output"):
        plain(x, moves_left=True)
    out = torch.empty(3)
    with pytest.raises(RuntimeError, match="no moves-left output"):
        InferenceNet(plain, torch.float32, trunk="library")(x, moves_left=out)
    assert flops_per_position(with_ml.cfg) - flops_per_position(plain.cfg) == 2 * SMALL["value_fc_size"]
    # the torch tail of InferenceNet (trunk="library" runs on the CPU) computes the module's x
    inf = InferenceNet(with_ml, torch.float32, trunk="library")
    assert inf.moves_left_head and not InferenceNet(plain, torch.float32, trunk="library").moves_left_head
    p, v = inf(x, moves_left=out)
    with torch.no_grad():
        pr, vr, xr = with_ml(x, moves_left=True)
    assert (out - xr).abs().max() < 1e-5 and (p - pr).abs().max() < 1e-5 and (v - vr).abs().max() < 1e-5
    p0, v0 = inf(x)
    assert torch.equal(p0, p) and torch.equal(v0, v)


# ---- the command line and the trainer ----------------------------------------------------------------------------------------
def _build(argv):
    from cchess_alphazero import manager
    return manager.build_config(manager.create_parser().parse_args(argv))


@pytest.mark.parametrize("w", ["-1", "-0.001", "nan", "inf", "-inf"])
def test_manager_refuses_a_negative_or_non_finite_weight(w):
    with pytest.raises(SystemExit, match="expected a finite W >= 0"):
        _build(["opt", "--moves-left=" + w])


def test_weight_reaches_the_trainer_config_and_is_an_option_of_opt():
    assert _build(["opt"]).trainer.moves_left == 0.0
    assert _build(["opt", "--moves-left", "0.25"]).trainer.moves_left == 0.25
    assert _build(["opt", "--moves-left", "0.5", "--augment", "mirror", "--surprise-weight", "0.5", "--q-ratio", "0.25"]
                  ).trainer.moves_left == 0.5
    assert _build(["opt", "--moves-left", "1", "--value-head", "wdl"]).trainer.moves_left == 1.0
    assert _build(["self"]).trainer.moves_left == 0.0
    with pytest.raises(SystemExit, match="--moves-left is an option of `run.py opt`"):
        _build(["self", "--moves-left", "0.5"])


def _worker(tmp_path, monkeypatch, best, **trainer):
    """An OptimizeWorker whose best model on disk is CChessNet(**SMALL, **best) (best None: no best model)."""
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
    if best is not None:
        m = CChessModel(cfg)
        torch.manual_seed(5)
        m.model = CChessNet(**SMALL, **best)
        save_as_best_model(m)
    return optimize.OptimizeWorker(cfg)


def test_a_best_model_without_the_output_is_refused(tmp_path, monkeypatch):
    w = _worker(tmp_path, monkeypatch, {}, moves_left=0.5)
    with pytest.raises(ValueError) as e:
        w.load_model()
    assert "--moves-left 0.5: the best model has no moves-left output" in str(e.value) and "--new" in str(e.value)


@pytest.mark.parametrize("w", [-0.5, float("nan"), float("inf")])
def test_the_worker_refuses_what_the_manager_refuses(tmp_path, monkeypatch, w):
    with pytest.raises(ValueError, match="expected a finite W >= 0"):
        _worker(tmp_path, monkeypatch, None, moves_left=w)


def test_window_loss_needs_a_window_with_targets():
    import torch
    from cchess_alphazero.lib.replay_window import ReplayWindow
    win = ReplayWindow.__new__(ReplayWindow)
    win.w = win.left = None
    with pytest.raises(ValueError, match="moves_left=True"):
        ReplayWindow.loss(win, torch.zeros((2, 2086)), torch.zeros(2), torch.zeros(2, dtype=torch.int32),
                          moves_left=(torch.zeros(2), 1.0))


# ---- the float64 model of the loss -------------------------------------------------------------------------------------------
def test_loss_model_is_huber_of_softplus_in_units():
    x = np.array([-100.0, -3.0, 0.0, 2.5, 16.0, 16.0, 100.0], dtype=np.float32)
    left = np.array([1, 8, 22, 64, 496, 528, 500])
    r = mc.loss_check(x, left, w_m=2.0)
    y = np.log1p(np.exp(x.astype(np.float64)))
    d = y - left / 32.0
    assert np.allclose(r["d"], d, rtol=0, atol=1e-12)
    assert abs(d[4] - 0.5) < 1e-6 and abs(d[5] + 0.5) < 1e-6                  # |d| = delta: the two forms meet
    want = np.where(np.abs(d) <= 0.5, d * d / 2, 0.5 * (np.abs(d) - 0.25))
    assert np.allclose(r["loss"], want, rtol=1e-12, atol=0)
    # the gradient is the derivative of w_m mean(loss), written out: Huber'(d) sigmoid(x) w_m / B
    num = 2.0 / 7 * (np.where(np.abs(d) <= 0.5, 1, 0) * d + np.where(np.abs(d) > 0.5, 0.5 * np.sign(d), 0)) / (1 + np.exp(-x.astype(np.float64)))
    assert np.allclose(r["grad"], num, rtol=1e-9, atol=1e-300)
    assert np.isfinite(r["loss"]).all() and np.isfinite(r["grad"]).all() and (r["e_loss"] > 0).all() and (r["e_grad"] > 0).all()


# ---- the bound on x is not vacuous -------------------------------------------------------------------------------------------
def tail_model(hidden, row, b):
    """The moves-left row of k_fc_tile<VALUE_ML / WDL_ML> in numpy fp32: the dot product added unit by unit in index order,
    every product and sum rounded (another order than the kernel's lanes and waves: the bound holds for any)."""
    f = np.float32
    h = np.maximum(hidden, f(0))
    acc = np.zeros(hidden.shape[0], dtype=f)
    for j in range(hidden.shape[1]):
        acc = (acc + (h[:, j] * row[j]).astype(f)).astype(f)
    return acc + f(b)


@pytest.mark.parametrize("f,n_hid", [(180, 100), (360, 33)])
def test_bound_on_x_passes_the_arithmetic_and_catches_its_faults(f, n_hid):
    """On the mixed data of f16_pairs.dense_features, w2 = [win, draw, loss, moves left]: the clean model stays inside the
    bound on x (both sets of operands); a model that drops the w_lo x_hi term and one that reads the moves-left row from
    the win row exceed it."""
    from test_wdl_cpu import hidden_model
    rng = np.random.default_rng(f + n_hid + 1)
    n = 48
    x = fp.dense_features("mixed", n, f, rng)
    w1 = (rng.standard_normal((n_hid, f)) * 0.1).astype(np.float32)
    b1 = (rng.standard_normal(n_hid) * 0.2).astype(np.float32)
    w2 = (rng.standard_normal((4, n_hid)) * 0.2).astype(np.float32)
    b = float(np.float32(1.8545866))
    xp = tuple(t.astype(np.float64) for t in fp.split16(x))
    wp = tuple(t.astype(np.float64) for t in fp.split16(w1))
    h_a, hb_a, h_b, hb_b = fp.DenseCheck(xp, wp, x.astype(np.float64), w1.astype(np.float64)).bounds(b1.astype(np.float64))
    refs = [mc.x_check(h, hb, w2[3].astype(np.float64), b) for h, hb in ((h_a, hb_a), (h_b, hb_b))]

    def ratio(got):
        return max((np.abs(got - r) / br).max() for r, br in refs)
    got = {"clean": ratio(tail_model(hidden_model(x, w1, b1), w2[3], b)),
           "no w_lo x_hi": ratio(tail_model(hidden_model(x, w1, b1, drop_lh=True), w2[3], b)),
           "the win row": ratio(tail_model(hidden_model(x, w1, b1), w2[0], b))}
    print(f, n_hid, {k: f"{v:.3g}" for k, v in got.items()})
    assert got["clean"] <= 1.0, got
    assert got["no w_lo x_hi"] > 1.0 and got["the win row"] > 1.0, got


# ---- the refusals of the two entry points (before anything is asked of a device) -------------------------------------------------
def test_heads_tail_ml_has_the_refusals_of_its_neighbours():
    from cchess_alphazero import _native
    import test_nn_entry_args_cpu as ea
    L = _native.lib()
    P = ea.P
    base = [("policy_feat", P), ("n_policy_feat", 360), ("wp_packed", P), ("bias_p", P), ("n_labels", 2086), ("value_feat", P),
            ("n_value_feat", 180), ("w1_packed", P), ("bias1", P), ("n_hidden", 256), ("value_outputs", 3), ("w2", P),
            ("b2", P), ("policy", P), ("value", P), ("wdl", P), ("moves_left", P), ("stats_scratch", P), ("n_boards", 5),
            ("dtype", ea.F16), ("normalize", 1), ("n_dev", None), ("stream", None)]
    msg = ("cz_heads_tail_ml: bad argument (n_labels even; 180 or 360 features per head: 2 or 4 filters x 90 squares; dtype of "
           "the packed pairs: CZ_BF16 or CZ_F16; value_outputs 1 or 3; moves_left is required; wdl only with value_outputs 3, "
           "may be NULL)")

    def call(**over):
        assert set(over) <= {n for n, _ in base}
        rc = L.cz_heads_tail_ml(*[over.get(n, v) for n, v in base])
        return rc, L.cz_last_error().decode()
    refused = ea.nulls("policy_feat", "wp_packed", "bias_p", "value_feat", "w1_packed", "bias1", "w2", "b2", "policy", "value",
                       "moves_left", "stats_scratch")
    refused += [dict(n_boards=-1), dict(n_labels=0), dict(n_labels=1), dict(n_labels=2087), dict(n_hidden=0),
                dict(n_policy_feat=0), dict(n_policy_feat=90), dict(n_policy_feat=270), dict(n_value_feat=90), dict(n_value_feat=0),
                dict(value_outputs=0), dict(value_outputs=2), dict(value_outputs=4), dict(value_outputs=1)]   # (1: wdl is given)
    refused += [dict(dtype=d) for d in (ea.F32, ea.U8, ea.F16C8)]
    for over in refused:
        assert call(**over) == (ea.ERR_ARG, msg[:255]), over
    for over in (dict(n_boards=0), dict(n_boards=0, wdl=None), dict(n_boards=0, wdl=None, value_outputs=1),
                 dict(n_boards=0, dtype=ea.BF16, n_policy_feat=180, n_value_feat=360)):
        assert call(**over)[0] == ea.OK, over


def test_moves_left_loss_refuses_bad_arguments():
    from cchess_alphazero import _native
    import test_nn_entry_args_cpu as ea
    L = _native.lib()
    P = ea.P
    base = [("x", P), ("idx", P), ("n_rows", 4), ("n_pos", 9), ("left", P), ("row_w", None), ("unit", 32.0), ("delta", 0.5),
            ("w_m", 1.0), ("loss", P), ("grad_x", P), ("stream", None)]
    msg = "cz_moves_left_loss: bad argument (unit and delta positive and finite, w_m >= 0 and finite)"

    def call(**over):
        assert set(over) <= {n for n, _ in base}
        rc = L.cz_moves_left_loss(*[over.get(n, v) for n, v in base])
        return rc, L.cz_last_error().decode()
    bad = [float("nan"), float("inf"), -1.0]
    for over in ea.nulls("x", "idx", "left", "loss", "grad_x") + [dict(n_rows=-1), dict(n_pos=-1)] + \
            [dict(unit=v) for v in bad + [0.0]] + [dict(delta=v) for v in bad + [0.0]] + [dict(w_m=v) for v in bad]:
        assert call(**over) == (ea.ERR_ARG, msg), over
    assert call(n_rows=0)[0] == ea.OK and call(n_rows=0, x=None)[0] == ea.OK
