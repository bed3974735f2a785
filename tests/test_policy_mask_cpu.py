"""run.py opt --policy-mask legal without a GPU: the float64 model of the masked loss (tests/policy_mask_model.py) against
float64 torch autograd, the legal sets of the test positions and their mirror images, the command line's and the trainer's
refusals, and what the trainer asks of a window's loss() with the option on and off."""
import types

import numpy as np
import pytest

import policy_mask_cases as cases
import policy_mask_model as pmm
from oracle import xq_oracle as xo


# ---- the model against autograd ----------------------------------------------------------------------------------------
def test_model_matches_float64_autograd_of_the_masked_fill():
    """Both sides are float64 evaluations of one formula: the clipped cross-entropy of softmax(masked_fill(x, ~A, -inf))."""
    import torch
    rng = np.random.default_rng(0)
    B, L = 12, 2086
    legal = rng.random((B, L)) < 0.02
    t = np.zeros((B, L), dtype=np.float32)
    for r in range(B):
        k = rng.choice(np.flatnonzero(legal[r]), size=min(5, int(legal[r].sum())), replace=False)
        w = rng.integers(1, 40, size=len(k))
        t[r, k] = (w / w.sum()).astype(np.float32)
    t[0, np.flatnonzero(~legal[0])[0]] = 0.25                    # a target entry outside the legal set joins A
    x = rng.normal(0, 2, size=(B, L)).astype(np.float32)
    for r in range(0, B, 3):                                     # peaked rows: clipped target entries, large illegal mass
        pool = np.flatnonzero(legal[r]) if (r // 3) % 2 == 0 else np.flatnonzero(~legal[r] & (t[r] == 0))
        x[r, pool[0]] += 40.0
    A = pmm.index_set(legal, t)
    wp = 1.25
    got = pmm.masked_loss(x, t, A, w_p=wp)
    assert ((t > 0) & ~got["clip_mask"]).any(), "no clipped target entry in the case"
    lg = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    tt = torch.from_numpy(t.astype(np.float64))
    p = torch.softmax(lg.masked_fill(torch.from_numpy(~A), float("-inf")), 1)
    eps, hi = float(pmm.EPS), float(pmm.HI)
    pc = torch.where((p > eps) & (p < hi), p, p.clamp(eps, hi).detach())
    rows = -(tt * torch.log(pc)).sum(1)
    (wp * rows.mean()).backward()
    assert np.abs(got["loss"] - rows.detach().numpy()).max() < 1e-12
    assert np.abs(got["grad"] - lg.grad.numpy()).max() < 1e-12
    assert (got["grad"][~A] == 0).all() and (lg.grad.numpy()[~A] == 0).all()
    # the diagnostics against a direct statement
    full = torch.softmax(torch.from_numpy(x.astype(np.float64)), 1).numpy()
    assert np.abs(got["mass"] - np.where(A, 0.0, full).sum(1)).max() < 1e-12
    assert got["margin"].dtype == np.float32
    assert got["mass"].max() > 0.99 and got["mass"].min() < 0.9
    # nothing outside A matters
    for fill in (1e4, np.inf, -np.inf, np.nan):
        y = np.where(A, x, np.float32(fill)).astype(np.float32)
        again = pmm.masked_loss(y, t, A, w_p=wp)
        assert again["loss"].tobytes() == got["loss"].tobytes() and again["grad"].tobytes() == got["grad"].tobytes()


# ---- legal sets ------------------------------------------------------------------------------------------------------
def test_test_positions_have_every_class():
    boards = cases.class_boards()
    assert {k: len(v) for k, v in boards.items()} == cases.EXPECTED
    games, classes = cases.one_ply_games()
    assert len(games) == sum(cases.EXPECTED.values()) and set(classes) == set(cases.CLASSES)
    counts = {c: sorted({len(xo.get_legal_moves(g[0])) for g, k in zip(games, classes) if k == c}) for c in cases.CLASSES}
    assert counts["63"] == [63] and counts["64"] == [64] and counts["65"] == [65] and counts["66"] == [66]
    assert max(counts["short"]) < 8 and counts["long"] == [68, 74]
    for g in games:
        assert g[1][0] in xo.get_legal_moves(g[0])


def test_mirror_of_a_legal_set_is_the_legal_set_of_the_mirrored_board():
    from cchess_alphazero import _native
    M = _native.label_mirror().astype(np.int64)
    games, _ = cases.one_ply_games()
    states = [g[0] for g in games] + [xo.INIT_STATE]
    legal = cases.legal_mask_of_states(states)
    mirrored = cases.legal_mask_of_states([xo.board_to_state(cases.mirror_board(xo.state_to_board(s))) for s in states])
    through_m = np.zeros_like(legal)
    for r in range(len(states)):
        through_m[r, M[np.flatnonzero(legal[r])]] = True
    assert (through_m == mirrored).all()
    sizes = np.array([len(xo.get_legal_moves(s)) for s in states])
    assert (legal.sum(1) <= sizes).all() and (legal.sum(1) < sizes).any()     # some of these lists hold a label twice


# ---- flag and config ---------------------------------------------------------------------------------------------------
def _build(argv):
    from cchess_alphazero import manager
    return manager.build_config(manager.create_parser().parse_args(argv))


def test_flag_is_an_option_of_opt():
    from cchess_alphazero.config import Config
    assert Config("mini").trainer.policy_mask == "none" and Config("normal").trainer.policy_mask == "none"
    assert _build(["opt"]).trainer.policy_mask == "none"
    assert _build(["opt", "--policy-mask", "legal"]).trainer.policy_mask == "legal"
    assert _build(["opt", "--policy-mask", "none"]).trainer.policy_mask == "none"
    cfg = _build(["opt", "--policy-mask", "legal", "--policy-targets", "visits", "--augment", "mirror", "--q-ratio", "0.25",
                  "--surprise-weight", "0.5", "--moves-left", "0.5"])
    assert cfg.trainer.policy_mask == "legal" and cfg.trainer.augment == "mirror"
    assert _build(["opt", "--policy-mask", "legal", "--value-head", "wdl"]).trainer.policy_mask == "legal"
    for cmd in ("self", "eval", "reanalyse"):
        assert _build([cmd]).trainer.policy_mask == "none"
        assert _build([cmd, "--policy-mask", "none"]).trainer.policy_mask == "none"
        with pytest.raises(SystemExit, match="--policy-mask is an option of `run.py opt`"):
            _build([cmd, "--policy-mask", "legal"])
    with pytest.raises(SystemExit):
        _build(["opt", "--policy-mask", "pseudo"])


def _config(tmp_path, monkeypatch, **trainer):
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    from cchess_alphazero.config import Config
    cfg = Config("mini")
    for k, v in trainer.items():
        setattr(cfg.trainer, k, v)
    return cfg


def test_worker_rejects_an_unknown_mask(tmp_path, monkeypatch):
    from cchess_alphazero.worker.optimize import OptimizeWorker
    for bad in ("pseudo", "", None, True):
        with pytest.raises(ValueError, match="trainer.policy_mask"):
            OptimizeWorker(_config(tmp_path, monkeypatch, policy_mask=bad))
    assert OptimizeWorker(_config(tmp_path, monkeypatch)).legal_mask is False
    assert OptimizeWorker(_config(tmp_path, monkeypatch, policy_mask="legal")).legal_mask is True


# ---- what the trainer asks of a window ---------------------------------------------------------------------------------
class LossWindow:
    """Stands in for ReplayWindow in step() and evaluate(): records the keywords of every loss() call."""

    def __init__(self):
        self.calls = []

    def planes(self, idx, mirror=None):
        import torch
        return torch.zeros((idx.shape[0], 14, 10, 9))

    def loss(self, logits, v, idx, targets="played", weights=(1.0, 1.0), mirror=None, **kw):
        import torch
        self.calls.append(dict(kw))
        stats = kw.get("mask_stats")
        if stats is not None:
            b = idx.shape[0]
            for k in (tuple(stats) or ("off_mask", "illegal_mass", "illegal_margin")):
                stats[k] = torch.zeros(b, dtype=torch.int32) if k == "off_mask" else torch.full((b,), 0.5)
        pm, vm = logits.detach().mean() * 0 + 2.0, v.detach().mean() * 0 + 1.0
        return logits.mean() * 0 + v.mean() * 0 + pm + vm, pm, vm


def _stand_in_worker(tmp_path, monkeypatch, **trainer):
    import torch
    from cchess_alphazero.agent.model import CChessNet
    from cchess_alphazero.worker.optimize import OptimizeWorker
    ow = OptimizeWorker(_config(tmp_path, monkeypatch, batch_size=4, **trainer))
    torch.manual_seed(0)
    ow.model = types.SimpleNamespace(model=CChessNet(cnn_filter_num=8, res_layer_num=1, value_fc_size=8))
    ow.compile_model()
    ow.window = LossWindow()
    return ow


def test_stand_in_window_is_asked_nothing_new_without_the_option(tmp_path, monkeypatch):
    import torch
    ow = _stand_in_worker(tmp_path, monkeypatch)
    idx = torch.arange(6, dtype=torch.int32)
    ow.step(idx[:4])
    ow.evaluate(idx)
    assert ow.window.calls == [{}, {}, {}]                      # one step, two validation batches
    assert ow.off_mask_sum is None


def test_stand_in_window_gets_legal_mask_with_the_option(tmp_path, monkeypatch):
    import torch
    ow = _stand_in_worker(tmp_path, monkeypatch, policy_mask="legal")
    idx = torch.arange(6, dtype=torch.int32)
    ow.step(idx[:4])
    assert len(ow.window.calls) == 1 and ow.window.calls[0]["legal_mask"] is True
    assert set(ow.window.calls[0]["mask_stats"]) == {"off_mask"}             # a step asks for no diagnostics
    assert int(ow.off_mask_sum) == 0
    out = {}
    ow.evaluate(idx, mask_out=out)
    assert all(c["legal_mask"] is True for c in ow.window.calls[1:]) and len(ow.window.calls) == 3
    assert all(set(c["mask_stats"]) == {"off_mask", "illegal_mass", "illegal_margin"} for c in ow.window.calls[1:])
    assert out == dict(val_illegal_mass=0.5, val_illegal_margin=0.5, off_mask_targets=0)
    ow.evaluate(idx, legal_mask=False)                                           # val_policy_full: the unmasked loss
    assert ow.window.calls[3:] == [{}, {}]
