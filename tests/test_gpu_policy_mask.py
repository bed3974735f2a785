"""-m gpu: run.py opt --policy-mask legal -- the masked loss kernels (cz_policy_value_loss_l / cz_policy_wdl_loss_l) against the
float64 model of tests/policy_mask_model.py with legal sets from the oracle, bit for bit against the unmasked entry points
on logits set to -inf outside the row's index set, their indifference to everything outside it, mirror flags, a target label
outside the legal moves, the rows they are held to, and the trainer with the option on and off.

Positions: rows of oracle random games (both colours to move; one-hot, visit and zero-sum visit targets; every other item with
a search value q) and the one-ply games of tests/policy_mask_cases.py (move lists of 63 .. 66 entries around the 64 a lane pass
marks, the shortest lists of the family, the two long written-out positions)."""
import copy
import ctypes as C

import numpy as np
import pytest

import policy_mask_cases as cases
import policy_mask_model as pmm
from oracle import xq_oracle as xo
from test_gpu_trainer import EPS, HI, random_games, small_config, window_of

pytestmark = pytest.mark.gpu
NL = 2086
WP, WV = 1.25, 0.75


@pytest.fixture(scope="module")
def dev():
    import torch
    from cchess_alphazero import _native
    _native.require_gpu()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def states_of(games):
    """the state before every item of every game, in the window's order"""
    out = []
    for g in games:
        s = g[0]
        for item in g[1:]:
            out.append(s)
            s = xo.step(s, item[0])
    return out


def mirrored_state(s):
    return xo.board_to_state(cases.mirror_board(xo.state_to_board(s)))


def with_q(games, seed):
    """every other item as [move, z, pi or None, 1, q]"""
    rng = np.random.default_rng(seed)
    out = []
    for g in games:
        data = [g[0]]
        for k, it in enumerate(g[1:]):
            data.append([it[0], it[1], it[2] if len(it) > 2 else None, 1, round(float(rng.uniform(-1, 1)), 3)] if k % 2 else it)
        out.append(data)
    return out


class Case:
    pass


@pytest.fixture(scope="module")
def case(dev):
    """The window, the oracle's legal sets of its positions and of their mirror images, and B = 64 rows that hold every class."""
    import torch
    c = Case()
    rand = with_q(random_games(1, 8, max_plies=30, pi=True), 1)
    one, classes = cases.one_ply_games()
    games = rand + one
    c.w = window_of(games)
    c.n = len(c.w)
    n_rand = sum(len(g) - 1 for g in rand)
    assert c.n == n_rand + len(one)
    states = states_of(games)
    assert (c.w.boards[:c.n].cpu().numpy() == np.stack([xo.state_to_board(s) for s in states])).all()
    c.legal = cases.legal_mask_of_states(states)
    c.legal_m = cases.legal_mask_of_states([mirrored_state(s) for s in states])
    c.classes = np.array(["random"] * n_rand + classes)
    rng = np.random.default_rng(7)
    take = {"short": 2, "long": 2, "63": 9, "64": 9, "65": 9, "66": 7}
    pick = np.concatenate([np.flatnonzero(c.classes == k)[:m] for k, m in take.items()] +
                          [rng.choice(n_rand, size=64 - sum(take.values()), replace=False)])
    c.idx_np = rng.permutation(pick).astype(np.int32)
    assert len(c.idx_np) == 64 == len(set(c.idx_np)) and set(c.classes[c.idx_np]) == set(cases.CLASSES) | {"random"}
    has_q = np.isfinite(c.w.q[:c.n].cpu().numpy()[c.idx_np])
    assert has_q.any() and not has_q.all()
    c.idx = torch.from_numpy(c.idx_np).to(dev)
    c.t_all = {m: c.w.dense_targets(np.arange(c.n), m) for m in ("played", "visits")}
    c.logits_np = make_logits(rng, c.legal[c.idx_np], c.t_all["visits"][c.idx_np])
    c.logits = torch.from_numpy(c.logits_np).to(dev)
    c.v = torch.from_numpy(np.tanh(rng.normal(size=64)).astype(np.float32)).to(dev)
    c.vl = torch.from_numpy(rng.normal(size=(64, 3)).astype(np.float32)).to(dev)
    c.row_w = torch.from_numpy(rng.uniform(0.25, 2.0, size=c.n).astype(np.float32)).to(dev)
    c.flags_np = rng.integers(0, 2, size=64).astype(np.uint8)
    assert 0 < c.flags_np.sum() < 64
    c.flags = torch.from_numpy(c.flags_np).to(dev)
    return c


def make_logits(rng, legal, target):
    """normal(0, 2); every third row peaked by +40, in turn on a legal column that is no target entry where there is one (a
    clipped target entry) and on an illegal column (an illegal mass near 1)"""
    B = legal.shape[0]
    x = rng.normal(0, 2, size=(B, NL)).astype(np.float32)
    for r in range(0, B, 3):
        if (r // 3) % 2 == 0:
            pool = np.flatnonzero(legal[r] & (target[r] == 0))
            pool = pool if len(pool) else np.flatnonzero(legal[r])
        else:
            pool = np.flatnonzero(~legal[r] & (target[r] == 0))
        x[r, pool[rng.integers(len(pool))]] += 40.0
    return x


def window_args(c, mode, played=None):
    from cchess_alphazero.lib.replay_window import MODES
    w, n = c.w, c.n
    return (w.played[:n] if played is None else played, w.z[:n], w.row_ptr[:n + 1], w.vis_label[:w.nnz], w.vis_count[:w.nnz],
            MODES[mode], WP, WV)


def masked(c, logits, mode="visits", v=None, idx=None, played=None, **kw):
    """-> dict of the masked scalar-head kernel's outputs"""
    from cchess_alphazero import _native
    out = _native.policy_value_loss(logits, c.v if v is None else v, c.idx if idx is None else idx,
                                    *window_args(c, mode, played), boards=c.w.boards[:c.n], off_mask=True, mask_diag=True, **kw)
    return dict(zip(("pl", "se", "gl", "gv", "off", "mass", "margin"), out))


def bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return bool((bits(a) == bits(b)).all())


def fill_outside(c, logits, A, value):
    import torch
    return torch.where(torch.from_numpy(A).to(logits.device), logits, torch.full_like(logits, value))


def check_against_model(c, got, logits_np, t, A, row_w=None):
    m = pmm.masked_loss(logits_np, t, A, w_p=WP, row_w=row_w)
    assert ((t > 0) & ~m["clip_mask"]).any(), "no target entry with a clipped probability in the case"
    assert m["mass"].max() > 0.99, "no row with an illegal mass near 1 in the case"
    assert np.allclose(got["pl"].cpu().numpy(), m["loss"], rtol=1e-6, atol=1e-7)
    gl = got["gl"].cpu().numpy()
    assert np.abs(gl - m["grad"]).max() < 1e-6
    assert (gl[~A] == 0).all()
    assert np.abs(got["mass"].cpu().numpy() - m["mass"]).max() < 1e-6
    assert (got["margin"].cpu().numpy() == m["margin"]).all()
    assert (got["off"].cpu().numpy() == 0).all()
    return m


# ---- 0. the host helper ------------------------------------------------------------------------------------------------
def test_legal_labels_of_the_window_are_the_oracles(dev, case):
    c = case
    assert (c.w.legal_labels(np.arange(c.n)) == c.legal).all()
    got = c.w.legal_labels(c.idx, mirror=c.flags)
    want = np.where(c.flags_np[:, None] != 0, c.legal_m[c.idx_np], c.legal[c.idx_np])
    assert (got == want).all() and (c.legal_m[c.idx_np] != c.legal[c.idx_np]).any()


# ---- 1. against the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["played", "visits"])
def test_masked_kernel_matches_the_float64_model(dev, case, mode):
    import torch
    c = case
    got = masked(c, c.logits, mode)
    t = c.t_all[mode][c.idx_np]
    A = pmm.index_set(c.legal[c.idx_np], t)
    assert not ((t != 0) & ~c.legal[c.idx_np]).any()                # valid records: A is the legal set
    check_against_model(c, got, c.logits_np, t, A)
    z = c.w.value_targets(c.idx)
    assert np.allclose(got["se"].cpu().numpy(), (c.v.cpu().numpy().astype(np.float64) - z) ** 2, rtol=1e-6, atol=1e-9)
    # the window's autograd Function hands out the same gradients, and the per-row tensors on request
    lg, vg = c.logits.clone().requires_grad_(True), c.v.clone().requires_grad_(True)
    stats = {}
    tot, pm, vm = c.w.loss(lg, vg, c.idx, mode, (WP, WV), legal_mask=True, mask_stats=stats)
    tot.backward()
    assert torch.equal(lg.grad, got["gl"]) and torch.equal(vg.grad, got["gv"]) and torch.equal(pm, got["pl"].mean())
    assert set(stats) == {"off_mask", "illegal_mass", "illegal_margin"}
    assert torch.equal(stats["illegal_mass"], got["mass"]) and torch.equal(stats["illegal_margin"], got["margin"])
    only = dict(off_mask=None)
    c.w.loss(c.logits, c.v, c.idx, mode, (WP, WV), legal_mask=True, mask_stats=only)
    assert set(only) == {"off_mask"} and torch.equal(only["off_mask"], got["off"])
    with pytest.raises(ValueError):
        c.w.loss(c.logits, c.v, c.idx, mode, (WP, WV), mask_stats={})


# ---- 2. the identity, bit for bit ----------------------------------------------------------------------------------------
def assert_identity(a, b, A_dev, names):
    """a: masked on x; b: unmasked on x with -inf outside A"""
    for k in names:
        assert same_bits(a[k], b[k]), k
    assert bool((bits(a["gl"]) == bits(b["gl"]))[A_dev].all())
    assert bool((a["gl"][~A_dev] == 0).all()) and bool((b["gl"][~A_dev] == 0).all())


@pytest.mark.parametrize("variant", ["plain", "mirror", "q_ratio", "row_w", "wdl"])
def test_masked_equals_unmasked_on_minus_inf(dev, case, variant):
    import torch
    from cchess_alphazero import _native
    c = case
    flags = c.flags if variant == "mirror" else None
    t = c.w.dense_targets(c.idx, "visits", mirror=flags)
    legal = np.where(c.flags_np[:, None] != 0, c.legal_m[c.idx_np], c.legal[c.idx_np]) if variant == "mirror" \
        else c.legal[c.idx_np]
    A = pmm.index_set(legal, t)
    A_dev = torch.from_numpy(A).to(dev)
    x_inf = fill_outside(c, c.logits, A, float("-inf"))
    kw = dict(mirror=flags)
    if variant == "q_ratio":
        kw.update(q=c.w.q[:c.n], q_ratio=0.375)
    if variant == "row_w":
        kw.update(row_w=c.row_w)
    if variant == "wdl":
        names = ("pl", "ce", "se", "gl", "gv")
        a = dict(zip(names, _native.policy_wdl_loss(c.logits, c.vl, c.idx, *window_args(c, "visits"), mirror=flags,
                                                    boards=c.w.boards[:c.n])))
        b = dict(zip(names, _native.policy_wdl_loss(x_inf, c.vl, c.idx, *window_args(c, "visits"), mirror=flags)))
        assert_identity(a, b, A_dev, ("pl", "ce", "se", "gv"))
        return
    a = masked(c, c.logits, "visits", **kw)
    b = dict(zip(("pl", "se", "gl", "gv"), _native.policy_value_loss(x_inf, c.v, c.idx, *window_args(c, "visits"), **kw)))
    assert_identity(a, b, A_dev, ("pl", "se", "gv"))
    if variant == "q_ratio":                                        # the mix reached the value half
        plain = masked(c, c.logits, "visits")
        assert not same_bits(a["se"], plain["se"]) and same_bits(a["gl"], plain["gl"])
    if variant == "row_w":
        plain = masked(c, c.logits, "visits")
        assert not same_bits(a["gl"], plain["gl"]) and same_bits(a["pl"], plain["pl"])


def test_identity_on_the_grid_stride_path(dev, case):
    """B = 8192 + 7 rows: more rows than the grid has workgroups"""
    import torch
    from cchess_alphazero import _native
    c = case
    B = 8192 + 7
    rng = np.random.default_rng(11)
    idx_np = c.idx_np[rng.integers(0, 64, size=B)]
    idx = torch.from_numpy(idx_np).to(dev)
    A_dev = torch.from_numpy(pmm.index_set(c.legal[idx_np], c.t_all["visits"][idx_np])).to(dev)
    g = torch.Generator(device=dev).manual_seed(5)
    x = 2.0 * torch.randn((B, NL), generator=g, device=dev)
    x[::3, 17] += 40.0
    v = torch.tanh(torch.randn((B,), generator=g, device=dev))
    x_inf = torch.where(A_dev, x, torch.full_like(x, float("-inf")))
    a = masked(c, x, "visits", v=v, idx=idx)
    b = dict(zip(("pl", "se", "gl", "gv"), _native.policy_value_loss(x_inf, v, idx, *window_args(c, "visits"))))
    assert_identity(a, b, A_dev, ("pl", "se", "gv"))
    assert bool((a["off"] == 0).all()) and bool(torch.isfinite(a["pl"]).all())


# ---- 3. nothing outside A matters -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [1e4, float("inf"), float("-inf"), float("nan")])
def test_columns_outside_the_index_set_do_not_matter(dev, case, fill):
    from cchess_alphazero import _native
    c = case
    A = pmm.index_set(c.legal[c.idx_np], c.t_all["visits"][c.idx_np])
    y = fill_outside(c, c.logits, A, fill)
    a, b = masked(c, c.logits, "visits"), masked(c, y, "visits")
    for k in ("pl", "se", "gl", "gv", "off"):
        assert same_bits(a[k], b[k]), k
    names = ("pl", "ce", "se", "gl", "gv", "off")
    wa = dict(zip(names, _native.policy_wdl_loss(c.logits, c.vl, c.idx, *window_args(c, "visits"), boards=c.w.boards[:c.n],
                                                 off_mask=True)))
    wb = dict(zip(names, _native.policy_wdl_loss(y, c.vl, c.idx, *window_args(c, "visits"), boards=c.w.boards[:c.n],
                                                 off_mask=True)))
    for k in names:
        assert same_bits(wa[k], wb[k]), k


# ---- 4. mirror flags -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["played", "visits"])
def test_flagged_rows_match_the_model_on_the_mirrored_board(dev, case, mode):
    import torch
    c = case
    t = c.w.dense_targets(c.idx, mode, mirror=c.flags)
    legal = np.where(c.flags_np[:, None] != 0, c.legal_m[c.idx_np], c.legal[c.idx_np])
    assert not ((t != 0) & ~legal).any()
    A = pmm.index_set(legal, t)
    rng = np.random.default_rng(13)
    x_np = make_logits(rng, legal, t)
    got = masked(c, torch.from_numpy(x_np).to(dev), mode, mirror=c.flags)
    check_against_model(c, got, x_np, t, A)


# ---- 5. a target label outside the legal moves -------------------------------------------------------------------------------
def test_a_target_outside_the_legal_moves_joins_the_index_set(dev, case):
    c = case
    base = masked(c, c.logits, "played")
    r0 = 5
    i0 = int(c.idx_np[r0])
    lab = int(np.flatnonzero(~c.legal[i0])[3])
    played = c.w.played[:c.n].clone()
    played[i0] = lab
    got = masked(c, c.logits, "played", played=played)
    off = got["off"].cpu().numpy()
    assert off[r0] == 1 and off.sum() == 1
    t = c.t_all["played"][c.idx_np].copy()
    t[r0] = 0
    t[r0, lab] = 1.0
    A = pmm.index_set(c.legal[c.idx_np], t)
    assert A[r0, lab] and A[r0].sum() == c.legal[i0].sum() + 1
    m = pmm.masked_loss(c.logits_np, t, A, w_p=WP)
    pl = got["pl"].cpu().numpy()
    assert np.isfinite(pl[r0]) and np.allclose(pl, m["loss"], rtol=1e-6, atol=1e-7)
    gl = got["gl"].cpu().numpy()
    assert np.abs(gl - m["grad"]).max() < 1e-6 and (gl[~A] == 0).all() and gl[r0, lab] != 0
    assert np.abs(got["mass"].cpu().numpy() - m["mass"]).max() < 1e-6 and (got["margin"].cpu().numpy() == m["margin"]).all()
    others = np.arange(64) != r0
    for k in ("pl", "se", "gl", "gv", "off", "mass", "margin"):
        assert (bits(got[k]).cpu().numpy()[others] == bits(base[k]).cpu().numpy()[others]).all(), k


# ---- 6. the rows the kernels are held to -------------------------------------------------------------------------------------
@pytest.mark.parametrize("wdl", [False, True])
def test_out_of_range_rows_and_guard_rows(dev, case, wdl):
    import torch
    from cchess_alphazero import _native
    c = case
    B, G = 64, 3
    idx_np = c.idx_np.copy()
    bad = {2: -1, 9: c.n, 30: 2 ** 31 - 1, 63: -2 ** 31}
    for r, i in bad.items():
        idx_np[r] = i
    idx = torch.from_numpy(idx_np).to(dev)
    logits = c.logits.clone()
    logits[list(bad)] = float("nan")                               # a row that is not to be read
    vcols = 3 if wdl else 1
    F, I = 12345.0, 0x5A5A5A5A
    out = {k: torch.full((B + G,) + shape, F, dtype=torch.float32, device=dev)
           for k, shape in dict(pl=(), se=(), ce=(), gl=(NL,), gv=(vcols,), mass=(), margin=()).items()}
    out["off"] = torch.full((B + G,), I, dtype=torch.int32, device=dev)
    w, n = c.w, c.n
    p = lambda t: C.c_void_p(t.data_ptr())                         # noqa: E731
    common = (p(idx), None, B, n, p(w.row_ptr), p(w.vis_label), p(w.vis_count), w.nnz, p(w.played), p(w.z))
    tail = (p(w.boards), p(out["off"]), p(out["mass"]), p(out["margin"]), _native._stream())
    if wdl:
        rc = _native.lib().cz_policy_wdl_loss_l(p(logits), NL, p(c.vl), *common, None, 1, WP, WV, p(out["pl"]), p(out["ce"]),
                                                p(out["se"]), p(out["gl"]), p(out["gv"]), *tail)
    else:
        rc = _native.lib().cz_policy_value_loss_l(p(logits), NL, p(c.v), *common, None, 0.0, None, 1, WP, WV, p(out["pl"]),
                                                  p(out["se"]), p(out["gl"]), p(out["gv"]), *tail)
    assert rc == 0
    torch.cuda.synchronize()
    used = [k for k in out if wdl or k != "ce"]
    for k in used:
        assert bool((out[k][B:] == (I if k == "off" else F)).all()), f"{k}: guard rows written"
        assert bool((out[k][list(bad)] == 0).all()), f"{k}: an out-of-range row is not zero"
    if not wdl:
        assert bool((out["ce"] == F).all())
    good = np.array([r for r in range(B) if r not in bad])
    ref = _native.policy_wdl_loss(c.logits, c.vl, c.idx, *window_args(c, "visits"), boards=w.boards[:n], off_mask=True,
                                  mask_diag=True) if wdl else tuple(masked(c, c.logits, "visits").values())
    names = ("pl", "ce", "se", "gl", "gv", "off", "mass", "margin") if wdl else ("pl", "se", "gl", "gv", "off", "mass", "margin")
    for k, t in zip(names, ref):
        if k in ("gl", "gv"):                                      # (the gradients' scale is 1 / B in both runs)
            assert (bits(out[k][:B].reshape(B, -1)).cpu().numpy()[good] == bits(t.reshape(B, -1)).cpu().numpy()[good]).all(), k
        else:
            assert (bits(out[k][:B]).cpu().numpy()[good] == bits(t).cpu().numpy()[good]).all(), k
    # a NULL boards pointer is an argument error, whatever else is passed
    rc = _native.lib().cz_policy_value_loss_l(p(logits), NL, p(c.v), *common, None, 0.0, None, 1, WP, WV, p(out["pl"]),
                                              p(out["se"]), p(out["gl"]), p(out["gv"]), None, None, None, None,
                                              _native._stream())
    assert rc == _native.lib().cz_policy_wdl_loss_l(p(logits), NL, p(c.vl), *common, None, 1, WP, WV, p(out["pl"]), p(out["ce"]),
                                                    p(out["se"]), p(out["gl"]), p(out["gv"]), None, None, None, None,
                                                    _native._stream()) != 0
    assert b"boards" in _native.lib().cz_last_error()


# ---- 7. the trainer ----------------------------------------------------------------------------------------------------------
def build_worker(cfg, seed):
    from cchess_alphazero.agent.model import CChessModel
    from cchess_alphazero.worker.optimize import OptimizeWorker
    ow = OptimizeWorker(cfg)
    ow.model = CChessModel(cfg)
    ow.model.build(seed=seed)
    ow.model.model.cuda().train()
    ow.compile_model()
    ow.update_learning_rate(0)
    return ow


def test_masked_sgd_steps_match_pure_torch(dev, tmp_path, monkeypatch):
    import torch
    from cchess_alphazero.lib.record_decoder import expand_records
    from cchess_alphazero.worker.optimize import l2_parameters
    cfg = small_config(tmp_path, monkeypatch, batch_size=32, policy_targets="visits", loss_weights=[1.25, 1.0],
                       policy_mask="legal")
    games = random_games(21, 10, pi=True)
    ow = build_worker(cfg, 3)
    ref = copy.deepcopy(ow.model.model)
    ow.window = window_of(games)
    legal = torch.from_numpy(cases.legal_mask_of_states(states_of(games))).to(dev)
    planes, pol, vals, _ = expand_records(games, targets="visits")
    assert not bool(((pol != 0) & ~legal).any())
    opt = torch.optim.SGD(ref.parameters(), lr=0.01, momentum=0.9)
    rng = np.random.default_rng(0)
    wp, wv = cfg.trainer.loss_weights
    for _ in range(3):
        idx = rng.permutation(len(ow.window))[:32].astype(np.int32)
        ow.step(torch.from_numpy(idx).to(dev))
        it = torch.from_numpy(idx.astype(np.int64)).to(dev)
        logits, v = ref(planes[it], logits=True)
        p = torch.softmax(logits.masked_fill(~legal[it], float("-inf")), 1)
        pc = torch.where((p > float(EPS)) & (p < float(HI)), p, p.clamp(float(EPS), float(HI)).detach())
        loss = wp * (-(pol[it] * torch.log(pc)).sum(1)).mean() + wv * ((v - vals[it]) ** 2).mean()
        loss = loss + cfg.model.l2_reg * sum((x * x).sum() for x in l2_parameters(ref))
        opt.zero_grad()
        loss.backward()
        opt.step()
    assert int(ow.off_mask_sum) == 0
    for (name, a), b in zip(ow.model.model.state_dict().items(), ref.state_dict().values()):
        if a.dtype.is_floating_point:
            assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), name
        else:
            assert torch.equal(a, b), name


def test_masked_overfit_128_positions(dev, tmp_path, monkeypatch):
    import torch
    cfg = small_config(tmp_path, monkeypatch, batch_size=128, policy_mask="legal")
    ow = build_worker(cfg, 7)
    ow.window = window_of(random_games(9, 12, max_plies=60))
    assert len(ow.window) >= 128
    idx = torch.arange(128, dtype=torch.int32, device=dev)
    first = None
    for s in range(100):
        _, pm, _ = ow.step(idx)
        if first is None:
            first = pm.item()
    assert pm.item() < first, (first, pm.item())


@pytest.mark.parametrize("mask", ["legal", "none"])
def test_history_carries_the_mask_figures_only_with_the_mask(dev, tmp_path, monkeypatch, mask):
    cfg = small_config(tmp_path, monkeypatch, batch_size=64, policy_targets="visits", augment="mirror", policy_mask=mask)
    ow = build_worker(cfg, 5)
    ow.window = window_of(random_games(33, 12, max_plies=40, pi=True))
    assert len(ow.window) > 128
    ow.train_epoch(2)
    new = {"val_illegal_mass", "val_illegal_margin", "off_mask_targets", "val_policy_full"}
    assert len(ow.history) == 2
    for h in ow.history:
        if mask == "none":
            assert not new & set(h)
            continue
        assert new <= set(h) and "val_mirror" in h
        assert h["off_mask_targets"] == 0 and 0.0 <= h["val_illegal_mass"] <= 1.0
        assert np.isfinite(h["val_illegal_margin"]) and np.isfinite(h["val_policy_full"])
        # p over the legal moves >= p over all labels, entry by entry, and the clip is monotone
        assert h["val"][1] <= h["val_policy_full"] + 1e-6
