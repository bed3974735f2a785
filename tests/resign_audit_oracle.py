"""The resignation audit (cz_search_record_maxq, lib/resign_audit.py, run.py self --resign-audit) restated for the tests:
the max q of a root in plain Python, the games of the C oracle with the max q of every searched ply, and a per-game
restatement of the audit -- the yardsticks of tests/test_resign_audit_cpu.py and tests/test_gpu_resign_audit.py.

The one configuration both use: hash stub salt 3, seed 7, game ids 0 .. 15, 64 simulations, search_threads 8, noise_eps 0,
tau_decay_rate 0.98, min_resign_turn 4, max_game_length 60, enable_resign_rate 1.0 (every game plays on without
resignation).  Its games: 4 wins, 5 losses and 7 draws for the first mover."""
import functools
import types

import selfplay_oracle as so
from oracle import xq_oracle as xo

SPEC = dict(kind="hash", salt=3)
SEED = 7
GAME_IDS = tuple(range(16))
BANNED = 0x8000
# T -> (would, fp) over the 16 games, as measured with the oracle when the feature was specified
TABLE = {-0.5: (5, 0), -0.2: (7, 2), -0.1: (9, 4), 0.0: (12, 7), 0.3: (14, 12)}
RESULTS = dict(wins=4, losses=5, draws=7)


def play_config(**kw):
    d = dict(simulation_num_per_move=64, search_threads=8, c_puct=1.5, noise_eps=0.0, dirichlet_alpha=0.2,
             tau_decay_rate=0.98, virtual_loss=3, resign_threshold=-0.92, min_resign_turn=4, max_game_length=60,
             enable_resign_rate=1.0)
    d.update(kw)
    return types.SimpleNamespace(**d)


def root_maxq(labels, n, w):
    """choose_action's number: the maximum over the non-banned edges of n ? w / n : 0.0 in float64, starting from -100."""
    best = -100.0
    for lab, nj, wj in zip(labels, n, w):
        if int(lab) & BANNED:
            continue
        q = float(wj) / float(int(nj)) if int(nj) else 0.0
        best = q if q > best else best
    return best


def oracle_game(pc, seed, game_id, spec=None):
    """One game of the C oracle's player through selfplay_oracle.start_game: start_game's dict with `trace`, the
    (ply, maxq) of every action() call, max q from node_stats right after it with the ply's bans."""
    cfg = so.oracle_cfg(pc)
    pl = xo.Player(cfg, spec or SPEC, enable_resign=so.resign_enabled(cfg, seed, game_id), seed=seed, game_id=game_id)
    trace = []

    def ply(state, turns, no_act, increase_temp):
        action, _ = pl.action(state, turns, no_act, increase_temp, xo.philox_uniform(seed, game_id, 1, turns))
        st = pl.node_stats(state)
        lab = [int(l) | (BANNED if xo.label_str(int(l)) in no_act else 0) for l in st["moves"]]
        trace.append((turns, root_maxq(lab, st["n"], st["w"])))
        return action
    out = so.start_game(cfg, seed, game_id, ply)
    pl.close()
    out["trace"] = trace
    out["game_id"] = game_id
    return out


@functools.lru_cache(maxsize=None)
def games():
    """The 16 games of the configuration above, computed once per process; treat them as read-only."""
    return tuple(oracle_game(play_config(), SEED, g) for g in GAME_IDS)


_EXTRA = {}


def game(game_id):
    """Game `game_id` of the configuration: one of games(), or computed on demand (and kept) for a later id."""
    if game_id in GAME_IDS:
        return games()[game_id]
    if game_id not in _EXTRA:
        _EXTRA[game_id] = oracle_game(play_config(), SEED, game_id)
    return _EXTRA[game_id]


def choose_restated(game_list, grid, target, min_events, min_resign_turn):
    """choose_threshold in words: the largest T of the grid at which at least min_events games would have resigned and at
    most the share `target` of them wrongly; None when there is none."""
    best = None
    for T in grid:
        would, fp = restate(game_list, float(T), min_resign_turn)
        if would >= min_events and fp <= target * would and (best is None or T > best):
            best = float(T)
    return best


def restate(game_list, T, min_resign_turn):
    """(would, fp) at ONE threshold, game by game, in words: walk the searched plies in order; the first one past
    min_resign_turn whose max q is strictly below T is where the mover would have resigned; it is a false positive iff
    that mover did not lose."""
    would = fp = 0
    for g in game_list:
        for ply, mq in g["trace"]:
            if ply > min_resign_turn and mq < T:
                would += 1
                mover_result = g["value"] if ply % 2 == 0 else -g["value"]
                if mover_result >= 0:
                    fp += 1
                break
    return would, fp
