"""Playout cap randomization (cz_search_set_playout_cap, run.py self --fast-sims N --full-rate P) restated over the oracle:
tests/selfplay_oracle.py's start_game played as selfplay_game plays it -- ONE oracle player for the whole game, the tree
carried from ply to ply -- with the ply's budget written into that player's own copy of the configuration before every
action() call.  Move choice, game rules and the store lottery are the same code as selfplay_game's.

The lottery, as in the engine: ply `turns` of game `game_id` is a full search iff
philox(seed, game_id, stream 2, draw turns) < full_rate; rates 0 and 1 draw nothing; fast_sims = 0 switches the cap off.
Fast plies carry no root noise; the oracle configurations of these tests have noise_eps = 0 throughout.

`struct xqo_player` (oracle/xq_mcts.c) begins with its xqo_play_cfg, which is xo.PlayCfg field for field, so a cast of the
player handle reaches simulation_num_per_move.  The helper refuses to run unless every field read back through that cast
equals the configuration the player was created with.

tests/test_playout_cap_cpu.py pins this file to selfplay_game (cap off, rate 1) and to the games of a configuration with
simulation_num_per_move = fast_sims (rate 0); the GPU is then compared with the mixed schedules."""
import ctypes as C

import selfplay_oracle as so
from oracle import xq_oracle as xo

LOTTERY_STREAM = 2          # stream 0: the per-game lotteries, stream 1: the move choice


def ply_is_full(seed, game_id, turns, fast_sims, full_rate, uniform=xo.philox_uniform):
    """The per-ply lottery; `uniform` is only called for 0 < full_rate < 1 with the cap on."""
    if fast_sims <= 0 or full_rate >= 1.0:
        return True
    if full_rate <= 0.0:
        return False
    return uniform(seed, game_id, LOTTERY_STREAM, turns) < full_rate


def _player_cfg(pl, cfg):
    """The configuration inside the oracle player, after checking that the cast really lands on it."""
    inner = C.cast(pl.h, C.POINTER(xo.PlayCfg)).contents
    for name, _ in xo.PlayCfg._fields_:
        if getattr(inner, name) != getattr(cfg, name):
            raise AssertionError(f"xqo_player does not begin with its configuration: {name} reads "
                                 f"{getattr(inner, name)!r}, created with {getattr(cfg, name)!r}")
    return inner


def capped_selfplay_game(cfg, stub, seed, game_id, fast_sims, full_rate, init_state=None, trace=None):
    """selfplay_game with a per-ply budget.  Returns its dict plus `fast` (one bool per action() call, the resignation
    ply included: the schedule), `sum_n` (the root's visit count when each move was chosen), `sims` (simulations run in
    the whole game) and `idle_fast` (fast plies that searched nothing: the reused root already had >= fast_sims visits
    and no ban / increase_temp reset it).  `trace` receives selfplay_game's dict per action() call plus `fast`."""
    if fast_sims and not 1 <= fast_sims <= cfg.simulation_num_per_move:
        raise ValueError(f"fast_sims {fast_sims} outside 1 .. {cfg.simulation_num_per_move}")
    if cfg.noise_eps != 0.0:
        raise ValueError("the capped oracle needs noise_eps = 0 (fast plies have no root noise, full plies would)")
    pl = xo.Player(cfg, stub, enable_resign=so.resign_enabled(cfg, seed, game_id), seed=seed, game_id=game_id)
    inner = _player_cfg(pl, cfg)
    full_sims = cfg.simulation_num_per_move
    fast, sum_n, idle_fast = [], [], 0

    def ply(state, turns, no_act, increase_temp):
        nonlocal idle_fast
        full = ply_is_full(seed, game_id, turns, fast_sims, full_rate)
        inner.simulation_num_per_move = full_sims if full else fast_sims
        before = pl.counters()["sims"]
        action, _ = pl.action(state, turns, no_act, increase_temp, xo.philox_uniform(seed, game_id, 1, turns))
        st = pl.node_stats(state)
        fast.append(not full)
        sum_n.append(st["sum_n"])
        if not full and pl.counters()["sims"] == before:
            idle_fast += 1
        if trace is not None:
            trace.append(dict(state=state, action=action, moves=st["moves"], n=st["n"], sum_n=st["sum_n"],
                              no_act=list(no_act), inc=increase_temp, fast=not full))
        return action

    out = so.start_game(cfg, seed, game_id, ply, init_state)
    out.update(fast=fast, sum_n=sum_n, sims=pl.counters()["sims"], idle_fast=idle_fast)
    inner.simulation_num_per_move = full_sims
    pl.close()
    return out


def move_flags(ref):
    """The record's per-move `fast` list of an oracle game: one flag per move, False for the appended king capture (a
    resignation ply has a schedule entry but no move)."""
    return ref["fast"][:ref["searched"]] + [False] * (ref["turns"] - ref["searched"])


__all__ = ["capped_selfplay_game", "ply_is_full", "move_flags", "so"]
