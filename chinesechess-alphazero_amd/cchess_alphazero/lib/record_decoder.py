"""Batched decoder of play records into training tensors -- the GPU form of the reference trainer's
``expanding_data`` / ``convert_to_trainging_data`` (cchess_alphazero/worker/optimize.py:234-281):
replay every game with ``senv.step``, encode each visited position into the 14 input planes, one-hot policy
from the played move, value per ply.

All games advance together: ply t of every game is one ``cz_step`` launch (one wavefront per game), and all
positions are encoded by one ``cz_encode`` launch.
"""
import numpy as np

from cchess_alphazero import _native
from cchess_alphazero.environment.lookup_tables import label_index
from cchess_alphazero.environment.static_env import state_to_array


def split_games(data):
    """A record file may hold several games flat-concatenated (``nb_game_in_file`` > 1, self_play.py:215):
    a game starts at every string item."""
    games, cur = [], None
    for item in data:
        if isinstance(item, str):
            cur = [item]
            games.append(cur)
        else:
            cur.append(item)
    return games


def expand_records(games, dtype=_native.F32, targets="played"):
    """games: list of ``[init_state, [move, value], ...]`` (items may be ``[move, value, pi]``, written with
    engine.record_visits, or ``[move, value, pi or None, weight]``, written with a playout cap: like the reference's
    expanding_data this keeps every position and ignores the weight).  Returns device tensors (planes [N,14,10,9],
    policy, value [N] float32) and the per-game offsets, positions ordered game by game, ply by ply (the order
    ``expanding_data`` produces).
    targets="played": policy = the played move's label index [N] int64 (the reference trainer's one-hot).
    targets="visits": policy = dense float32 [N, 2086] search policies: count / sum(counts) over pi for items that
    carry one, the one-hot of the played move for items that do not."""
    import torch
    if targets not in ("played", "visits"):
        raise ValueError(f"targets={targets!r}: expected 'played' or 'visits'")
    _native.require_gpu()
    n_games = len(games)
    lens = [len(g) - 1 for g in games]
    T = max(lens) if lens else 0
    boards = torch.from_numpy(np.stack([state_to_array(g[0]) for g in games])).cuda()
    moves = np.zeros((n_games, max(T, 1)), dtype=np.int32)
    for i, g in enumerate(games):
        for t, item in enumerate(g[1:]):
            moves[i, t] = label_index(item[0])
    moves_d = torch.from_numpy(moves).cuda()
    lens_d = torch.tensor(lens, device="cuda")
    all_boards = torch.empty((T, n_games, 90), dtype=torch.int8, device="cuda")
    for t in range(T):
        all_boards[t] = boards
        nxt, ne = _native.step(boards, moves_d[:, t].to(torch.uint16).contiguous())
        bad = (ne == 0xFF) & (lens_d > t)
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            raise ValueError(f"No chessman in {games[i][1 + t][0]} (game {i}, ply {t})")
        boards = torch.where((lens_d > t)[:, None], nxt, boards)
    keep = (torch.arange(T, device="cuda")[:, None] < lens_d[None, :])            # [T, G]
    order = keep.t().reshape(-1).nonzero().squeeze(1)                              # game-major
    flat = all_boards.permute(1, 0, 2).reshape(-1, 90)[order].contiguous()
    planes = _native.encode(flat, dtype)
    pol = moves_d.reshape(-1)[order].to(torch.int64)
    vals = torch.tensor([item[1] for g in games for item in g[1:]], dtype=torch.float32, device="cuda")
    offsets = np.concatenate([[0], np.cumsum(lens)])
    if targets == "visits":
        pol = _visit_targets([item for g in games for item in g[1:]], pol)
    return planes, pol, vals, offsets


def _visit_targets(items, played):
    """items: the records' move items, in position order; played: their label indices (device int64 [N]).
    -> float32 [N, 2086]: count / sum(counts) where the item has pi, else one-hot of the played move."""
    import torch
    n = len(items)
    rows, cols, w = [], [], []
    has_pi = np.zeros(n, dtype=bool)
    for r, item in enumerate(items):
        if len(item) < 3 or item[2] is None:         # (a fast ply without visit recording: [move, value, None, 0])
            continue
        total = sum(c for _, c in item[2])
        if total <= 0:
            continue
        has_pi[r] = True
        for mv, c in item[2]:
            rows.append(r)
            cols.append(label_index(mv))
            w.append(c / total)                                   # float64 quotient, rounded once to float32
    out = torch.zeros((n, _native.NLABELS), dtype=torch.float32, device="cuda")
    if n == 0:
        return out
    hp = torch.from_numpy(has_pi).cuda()
    idx = torch.nonzero(~hp).squeeze(1)
    out[idx, played[idx]] = 1.0
    if rows:
        out.index_put_((torch.tensor(rows, device="cuda"), torch.tensor(cols, device="cuda")),
                       torch.tensor(w, dtype=torch.float64).to(torch.float32).cuda(), accumulate=False)
    return out
