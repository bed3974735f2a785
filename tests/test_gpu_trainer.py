"""-m gpu: run.py opt -- the trainer's device data path (cz_replay_games / cz_gather_planes through lib/replay_window.py)
against record_decoder.expand_records and the reference's own expanding_data(use_history=True)
(tests/golden/trainer_records_history.json), the loss kernel (cz_policy_value_loss) against float64 NumPy and torch
autograd, SGD steps against a pure-torch trainer, a seeded overfit, and a self -> opt cycle end to end."""
import copy
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import xq_oracle as xo

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS, HI = np.float32(1e-7), np.float32(1.0 - 1e-7)


@pytest.fixture(scope="module")
def dev():
    import torch
    from cchess_alphazero import _native
    _native.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def random_games(seed, n_games, max_plies=40, pi=False):
    """Random legal games from the oracle; pi=True gives items synthetic visit counts over the legal moves: some with a
    zero sum, some without pi."""
    rng = np.random.default_rng(seed)
    games = []
    for _ in range(n_games):
        state, data = xo.INIT_STATE, [xo.INIT_STATE]
        for ply in range(int(rng.integers(0, max_plies))):
            if xo.done(state)[0]:
                break
            mv = xo.get_legal_moves(state)
            m = mv[int(rng.integers(len(mv)))]
            item = [m, 1 if ply % 2 == 0 else -1]
            if pi:
                kind = rng.integers(6)
                if kind > 0:
                    k = int(rng.integers(1, len(mv) + 1))
                    moves = list(rng.choice(mv, size=k, replace=False))
                    counts = [0] * k if kind == 1 else [int(c) for c in rng.integers(0, 50, size=k)]
                    item.append([[str(a), c] for a, c in zip(moves, counts)])
            data.append(item)
            state = xo.step(state, m)
        games.append(data)
    return games


def engine_games():
    with open(os.path.join(GOLDEN, "engine_records.json")) as f:
        return [g["data"] for g in json.load(f)["games"]]


def window_of(games, depth=14, capacity=10 ** 6):
    from cchess_alphazero.lib.replay_window import ReplayWindow
    w = ReplayWindow(capacity, depth=depth)
    w.add_games(games)
    return w


def all_idx(w):
    import torch
    return torch.arange(len(w), dtype=torch.int32, device="cuda")


# ---- 1. the window against expand_records ----------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["oracle", "engine"])
def test_window_matches_expand_records(dev, source):
    from cchess_alphazero.lib.record_decoder import _visit_targets, expand_records
    games = random_games(5, 24, pi=True) if source == "oracle" else random_pi(engine_games(), 7)
    w = window_of(games)
    planes, played, vals, offsets = expand_records(games)
    assert len(w) == offsets[-1] == planes.shape[0] and w.n_games == len(games)
    got = w.planes(all_idx(w))
    assert got.dtype == planes.dtype and got.shape == planes.shape
    assert got.cpu().numpy().tobytes() == planes.cpu().numpy().tobytes()
    assert (w.played[:len(w)].long().cpu() == played.cpu()).all()
    assert w.z[:len(w)].cpu().numpy().tobytes() == vals.cpu().numpy().tobytes()
    items = [it for g in games for it in g[1:]]
    dense = _visit_targets(items, played).cpu().numpy()
    mine = w.dense_targets(np.arange(len(w)), "visits")
    assert mine.tobytes() == dense.tobytes()
    kinds = {("pi" if len(it) == 3 and sum(c for _, c in it[2]) > 0 else "zero" if len(it) == 3 else "none")
             for it in items}
    assert kinds == {"pi", "zero", "none"}


def random_pi(games, seed):
    """engine_records.json carries no pi: give its items synthetic visit counts over the oracle's legal moves."""
    rng = np.random.default_rng(seed)
    out = []
    for g in games:
        state, data = g[0], [g[0]]
        for item in g[1:]:
            mv = xo.get_legal_moves(state)
            kind = rng.integers(5)
            it = [item[0], item[1]]
            if kind > 0:
                moves = list(rng.choice(mv, size=int(rng.integers(1, len(mv) + 1)), replace=False))
                it.append([[str(a), 0 if kind == 1 else int(rng.integers(0, 30))] for a in moves])
            data.append(it)
            state = xo.step(state, item[0])
        out.append(data)
    return out


def test_window_appends_files_in_order(dev):
    """Two batches appended: the second's prev indices point into its own games, the planes equal one decode of both."""
    from cchess_alphazero.lib.record_decoder import expand_records
    a, b = random_games(11, 5, pi=True), random_games(12, 6, pi=True)
    w = window_of(a)
    w.add_games(b)
    planes = expand_records(a + b)[0]
    assert w.planes(all_idx(w)).cpu().numpy().tobytes() == planes.cpu().numpy().tobytes()
    assert w.dense_targets(np.arange(len(w))).tobytes() == window_of(a + b).dense_targets(np.arange(len(w))).tobytes()


# ---- 2. history mode against the reference's expanding_data(use_history=True) ----------------------------------------
def test_history_planes_match_reference(dev):
    with open(os.path.join(GOLDEN, "trainer_records_history.json")) as f:
        ref = json.load(f)["games"]
    games = engine_games()
    assert len(ref) == len(games)
    w = window_of(games, depth=28)
    planes = w.planes(all_idx(w)).cpu().numpy()
    k = 0
    for g, r in zip(games, ref):
        n = len(g) - 1
        assert [n, 28, 10, 9] == r["planes_shape"]
        assert hashlib.sha256(np.ascontiguousarray(planes[k:k + n]).tobytes()).hexdigest() == r["planes_sha256"], g
        assert [int(x) for x in w.played[k:k + n].cpu()] == r["policy_argmax"]
        assert [float(x) for x in w.z[k:k + n].cpu()] == r["value"]
        k += n
    assert k == len(w)


# ---- 3. errors, empty games, the capacity ----------------------------------------------------------------------------
def test_window_errors_and_limits(dev, tmp_path):
    from cchess_alphazero.lib.data_helper import write_game_data_to_file
    from cchess_alphazero.lib.replay_window import ReplayWindow
    good = random_games(3, 3, max_plies=12)
    w = window_of(good)
    n = len(w)
    bad = [xo.INIT_STATE, ["0001", 1], ["4445", -1]]           # ply 1 moves from an empty square
    with pytest.raises(ValueError, match=r"game 1, ply 1"):
        w.add_games([good[0], bad])
    with pytest.raises(ValueError, match=r"game 0, ply 0"):
        w.add_games([[xo.INIT_STATE, ["4445", 1]]])
    assert len(w) == n                                          # unchanged after a failed load
    assert w.add_games([[xo.INIT_STATE], [xo.INIT_STATE]]) == 0 and len(w) == n
    # the capacity is checked before each file; the file that reaches it is loaded whole
    paths = []
    for i, g in enumerate([g for g in random_games(4, 30, max_plies=20) if len(g) > 3][:6]):
        paths.append(str(tmp_path / f"play_{i}.json"))
        write_game_data_to_file(paths[-1], g)
    from cchess_alphazero.worker.optimize import OptimizeWorker
    ow = OptimizeWorker.__new__(OptimizeWorker)             # (fill_window needs only the window)
    ow.window = ReplayWindow(10)
    order = list(paths)
    ow.fill_window(order)
    loaded = paths[len(order):][::-1]                        # taken from the end of the list
    w = ow.window
    assert w.full and w.files == loaded
    sizes = [len(json.load(open(p))) - 1 for p in loaded]
    assert len(w) == sum(sizes) and sum(sizes[:-1]) < 10
    assert w.boards.shape[0] == len(w)                       # beyond the capacity: exactly the room the last file needs
    small = ReplayWindow(1000)
    small.load_file(paths[0])
    assert small.boards.shape[0] <= 1000                     # growth stops at the capacity
    # malformed files are skipped, one at a time, and the rest is loaded
    junk = {"dict.json": '{"a": 1}', "nostate.json": '[1, 2]', "item.json": json.dumps([xo.INIT_STATE, "0001"]),
            "value.json": json.dumps([xo.INIT_STATE, ["0001", "x"]]), "pi.json": json.dumps([xo.INIT_STATE, ["0001", 1, [3]]]),
            "cut.json": '["' + xo.INIT_STATE + '", ["00'}
    bad_paths = []
    for name, text in junk.items():
        bad_paths.append(str(tmp_path / name))
        with open(bad_paths[-1], "w") as f:
            f.write(text)
    ow.window = ReplayWindow(10 ** 6)
    order = [paths[0]] + bad_paths
    ow.fill_window(order)
    assert order == [] and ow.window.files == [paths[0]] and len(ow.window) == sizes_of(paths[0])


def sizes_of(path):
    return len(json.load(open(path))) - 1


# ---- 4. the loss kernel ----------------------------------------------------------------------------------------------
def loss_case(dev, seed=0, B=24):
    """A window whose rows are one-hot (no pi), visit counts, zero-sum visits; logits with peaked rows where some
    targets get p < 1e-7 (the clip's mask)."""
    import torch
    games = random_games(seed, 8, max_plies=30, pi=True)
    w = window_of(games)
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(w), size=B).astype(np.int32)
    logits = rng.normal(0, 2, size=(B, 2086)).astype(np.float32)
    for r in range(0, B, 3):                                   # peaked: one logit far above the rest
        logits[r, rng.integers(2086)] += 40.0
    v = np.tanh(rng.normal(size=B)).astype(np.float32)
    return w, torch.from_numpy(idx).to(dev), torch.from_numpy(logits).to(dev), torch.from_numpy(v).to(dev)


@pytest.mark.parametrize("targets", ["played", "visits"])
def test_loss_kernel_matches_float64_and_autograd(dev, targets):
    import torch
    from cchess_alphazero import _native
    from cchess_alphazero.lib.replay_window import MODES
    w, idx, logits, v = loss_case(dev, seed=1 if targets == "visits" else 2)
    B = idx.shape[0]
    wp, wv = 1.25, 0.75
    n = len(w)
    pl, se, gl, gv = _native.policy_value_loss(logits, v, idx, w.played[:n], w.z[:n], w.row_ptr[:n + 1],
                                               w.vis_label[:w.nnz], w.vis_count[:w.nnz], MODES[targets], wp, wv)
    t = w.dense_targets(idx, targets)
    z = w.z[:n].cpu().numpy()[idx.cpu().numpy()]
    # float64 restatement of the clipped cross-entropy (Keras 2.0.8) and the squared error
    x = logits.cpu().numpy().astype(np.float64)
    p = np.exp(x - x.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    pc = np.clip(p, np.float64(EPS), np.float64(HI))
    lo_ref = -(t * np.log(pc)).sum(1)
    assert np.allclose(pl.cpu().numpy(), lo_ref, rtol=1e-6, atol=1e-7)
    vv = v.cpu().numpy().astype(np.float64)
    assert np.allclose(se.cpu().numpy(), (vv - z) ** 2, rtol=1e-6, atol=1e-9)
    m = (p > EPS) & (p < HI)
    assert ((t > 0) & ~m).any(), "no target entry with a clipped probability in the case"
    S = (t * m).sum(1, keepdims=True)
    g_ref = wp / B * (p * S - t * m)
    assert np.abs(gl.cpu().numpy() - g_ref).max() < 1e-6
    assert np.abs(gv.cpu().numpy() - wv * 2 * (vv - z) / B).max() < 1e-6
    # torch autograd of the dense formula
    lg = logits.clone().requires_grad_(True)
    vg = v.clone().requires_grad_(True)
    tt = torch.from_numpy(t).to(dev)
    pr = torch.softmax(lg, 1)
    prc = torch.where((pr > float(EPS)) & (pr < float(HI)), pr, pr.clamp(float(EPS), float(HI)).detach())
    loss = wp * (-(tt * torch.log(prc)).sum(1)).mean() + wv * ((vg - torch.from_numpy(z).to(dev)) ** 2).mean()
    loss.backward()
    assert (lg.grad - gl).abs().max().item() < 1e-6 and (vg.grad - gv).abs().max().item() < 1e-6
    # the autograd.Function of the window
    lg2 = logits.clone().requires_grad_(True)
    vg2 = v.clone().requires_grad_(True)
    tot, pm, vm = w.loss(lg2, vg2, idx, targets, (wp, wv))
    tot.backward()
    assert abs(tot.item() - loss.item()) <= 1e-6 * abs(loss.item())
    assert torch.equal(lg2.grad, gl) and torch.equal(vg2.grad, gv)


def test_visits_without_any_visit_entry_is_the_one_hot(dev):
    """Records without pi (the default `run.py self`, the reference's records): the window has no visit entries, and the
    visits mode takes every row's one-hot -- the same bits as the played mode."""
    import torch
    from cchess_alphazero import _native
    w = window_of(random_games(31, 8, max_plies=30))
    assert w.nnz == 0 and len(w) > 0
    rng = np.random.default_rng(4)
    idx = torch.from_numpy(rng.integers(0, len(w), size=20).astype(np.int32)).to(dev)
    logits = torch.from_numpy(rng.normal(0, 2, size=(20, 2086)).astype(np.float32)).to(dev)
    v = torch.from_numpy(np.tanh(rng.normal(size=20)).astype(np.float32)).to(dev)
    out = {}
    for targets in ("played", "visits"):
        lg, vg = logits.clone().requires_grad_(True), v.clone().requires_grad_(True)
        tot, pm, vm = w.loss(lg, vg, idx, targets)
        tot.backward()
        out[targets] = (tot.detach(), pm, vm, lg.grad, vg.grad)
    for a, b in zip(out["played"], out["visits"]):
        assert torch.equal(a, b)
    n = len(w)
    a = _native.policy_value_loss(logits, v, idx, w.played[:n], w.z[:n], mode=1)      # no visit arrays at all
    b = _native.policy_value_loss(logits, v, idx, w.played[:n], w.z[:n], mode=0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_loss_kernel_is_deterministic_and_takes_a_leading_dimension(dev):
    import torch
    from cchess_alphazero import _native
    w, idx, logits, v = loss_case(dev, seed=3)
    n = len(w)
    args = (w.played[:n], w.z[:n], w.row_ptr[:n + 1], w.vis_label[:w.nnz], w.vis_count[:w.nnz], 1, 1.0, 1.0)
    a = _native.policy_value_loss(logits, v, idx, *args)
    wide = torch.zeros((logits.shape[0], 2100), device=dev)
    wide[:, :2086] = logits
    b = _native.policy_value_loss(wide[:, :2086], v, idx, *args)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- 5. SGD steps against a pure-torch trainer ----------------------------------------------------------------------
def small_config(tmp_path, monkeypatch, **trainer):
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    from cchess_alphazero.config import Config
    cfg = Config("mini")
    cfg.model.cnn_filter_num, cfg.model.res_layer_num = 32, 2
    for k, v in trainer.items():
        setattr(cfg.trainer, k, v)
    return cfg


def test_sgd_steps_match_pure_torch(dev, tmp_path, monkeypatch):
    import torch
    from cchess_alphazero.agent.model import CChessModel
    from cchess_alphazero.lib.record_decoder import expand_records
    from cchess_alphazero.worker.optimize import OptimizeWorker, l2_parameters
    cfg = small_config(tmp_path, monkeypatch, batch_size=32, policy_targets="visits", loss_weights=[1.25, 1.0])
    games = random_games(21, 10, pi=True)
    ow = OptimizeWorker(cfg)
    ow.model = CChessModel(cfg)
    ow.model.build(seed=3)
    ow.model.model.cuda().train()
    ref = copy.deepcopy(ow.model.model)
    ow.compile_model()
    ow.update_learning_rate(0)
    ow.window = window_of(games)
    planes, pol, vals, _ = expand_records(games, targets="visits")
    opt = torch.optim.SGD(ref.parameters(), lr=0.01, momentum=0.9)
    rng = np.random.default_rng(0)
    wp, wv = cfg.trainer.loss_weights
    for _ in range(3):
        idx = rng.permutation(len(ow.window))[:32].astype(np.int32)
        ow.step(torch.from_numpy(idx).to(dev))
        it = torch.from_numpy(idx.astype(np.int64)).to(dev)
        logits, v = ref(planes[it], logits=True)
        p = torch.softmax(logits, 1)
        pc = torch.where((p > float(EPS)) & (p < float(HI)), p, p.clamp(float(EPS), float(HI)).detach())
        loss = wp * (-(pol[it] * torch.log(pc)).sum(1)).mean() + wv * ((v - vals[it]) ** 2).mean()
        loss = loss + cfg.model.l2_reg * sum((x * x).sum() for x in l2_parameters(ref))
        opt.zero_grad()
        loss.backward()
        opt.step()
    for (name, a), b in zip(ow.model.model.state_dict().items(), ref.state_dict().values()):
        if a.dtype.is_floating_point:
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), name
        else:
            assert torch.equal(a, b), name


# ---- 6. a seeded overfit ---------------------------------------------------------------------------------------------
def test_overfit_128_positions(dev, tmp_path, monkeypatch):
    import torch
    from cchess_alphazero.agent.model import CChessModel
    from cchess_alphazero.worker.optimize import OptimizeWorker
    cfg = small_config(tmp_path, monkeypatch, batch_size=128)
    ow = OptimizeWorker(cfg)
    ow.model = CChessModel(cfg)
    ow.model.build(seed=7)
    ow.model.model.cuda().train()
    ow.compile_model()
    ow.update_learning_rate(0)
    ow.window = window_of(random_games(9, 12, max_plies=60))
    assert len(ow.window) >= 128
    idx = torch.arange(128, dtype=torch.int32, device=dev)
    first = None
    for s in range(300):
        _, pm, _ = ow.step(idx)
        if first is None:
            first = pm.item()
    last = pm.item()
    assert last < 0.5 * first, (first, last)


# ---- 7. self -> opt end to end --------------------------------------------------------------------------------------
def test_selfplay_then_opt_cycle(dev, tmp_path, monkeypatch):
    import torch
    from cchess_alphazero import manager
    from cchess_alphazero.agent.model import CChessModel, guarded_inference_net
    from cchess_alphazero.lib.data_helper import get_game_data_filenames, read_game_data_from_file
    from cchess_alphazero.worker import optimize
    from cchess_alphazero.worker.self_play import SelfPlayWorker
    monkeypatch.setenv("DATA_DIR", str(tmp_path / "data"))
    monkeypatch.setenv("PROJECT_DIR", str(tmp_path))
    args = manager.create_parser().parse_args(["opt", "--policy-targets", "visits", "--record-visits"])
    cfg = manager.build_config(args)
    cfg.resource.create_directories()
    cfg.model.cnn_filter_num, cfg.model.res_layer_num = 32, 2
    for k, v in dict(simulation_num_per_move=12, search_threads=4, max_game_length=8).items():
        setattr(cfg.play, k, v)
    cfg.engine.games_per_gpu, cfg.engine.report_every_rounds = 16, 16
    cfg.play_data.max_file_num = 1000
    rc = cfg.resource
    model = CChessModel(cfg)
    model.build(seed=0)
    model.save(rc.model_best_config_path, rc.model_best_weight_path)
    digest0 = model.digest
    sp = SelfPlayWorker(cfg, model=model)
    sp.run(max_rounds=4000, max_games=12)
    sp.close()
    files = get_game_data_filenames(rc)
    assert len(files) >= 2
    assert any(len(it) == 3 for p in files for it in read_game_data_from_file(p)[1:])
    ow = optimize.OptimizeWorker(cfg)
    ow.start()
    assert ow.count >= 1 and ow.history and all(np.isfinite(h["train"]).all() for h in ow.history)
    best = CChessModel(cfg)
    assert best.load(rc.model_best_config_path, rc.model_best_weight_path) and best.digest != digest0
    assert os.path.exists(best._pt(rc.next_generation_weight_path)) and os.path.exists(rc.next_generation_config_path)
    trained = os.listdir(os.path.join(rc.data_dir, "trained"))
    assert sorted(trained) == sorted(os.path.basename(p) for p in files)
    assert get_game_data_filenames(rc) == []
    raw = best.model.cuda().eval()
    net = guarded_inference_net(raw, torch.float32, trunk="mfma", arith="c6")
    x = torch.from_numpy(np.stack([xo.state_to_planes(xo.INIT_STATE)] * 4)).to(dev)
    with torch.no_grad():
        pr, vr = raw(x)
    p, v = net(x)
    assert (p[:4] - pr).abs().max().item() < 1e-4 and (v[:4] - vr).abs().max().item() < 1e-4
    # a second run without data trains nothing and writes nothing
    digest1 = best.digest
    ow2 = optimize.OptimizeWorker(cfg)
    steps = ow2.start()
    assert ow2.count == 0 and steps == cfg.trainer.start_total_steps
    assert CChessModel.fetch_digest(best._pt(rc.model_best_weight_path)) == digest1
