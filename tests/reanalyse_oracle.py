"""The scripted game (cz_search_set_script, run.py reanalyse) restated over tests/selfplay_oracle.py's start_game: the loop
is the same code as self-play's, the player is ONE oracle player that never resigns, and the move it returns is the
script's, not its own.  Every ply -- the position after the script's last move included, where the player returns None and
start_game ends the game -- is searched by one action() call, with the tree carried from ply to ply, the no_act list and
increase_temp of the loop and, with a playout cap, the ply's budget of playout_cap_oracle.

What the engine takes from the script instead of from the loop is NOT restated here: the game's value is z, it is stored
without a lottery and the king capture is recorded only when the script holds it.  The tests compare moves, turns and z with
the script itself, and the searches with this trace."""
import playout_cap_oracle as pco
import selfplay_oracle as so
from oracle import xq_oracle as xo


def scripted_game(cfg, stub, seed, game_id, script, init_state=None, trace=None, fast_sims=0, full_rate=1.0):
    """script: the moves as label strings.  Returns start_game's dict (searched = the script moves start_game applied; value,
    store and resigned are the loop's own and mean nothing here).  `trace` (a list) receives one dict per action() call:
    selfplay_game's keys (state, action -- the player's OWN choice --, moves, n, sum_n, no_act, inc) plus w, p, the
    scripted move (None at the end) and fast."""
    script = list(script)
    pl = xo.Player(cfg, stub, enable_resign=False, seed=seed, game_id=game_id)
    inner = pco._player_cfg(pl, cfg) if fast_sims else None
    full_sims = cfg.simulation_num_per_move

    def ply(state, turns, no_act, increase_temp):
        full = pco.ply_is_full(seed, game_id, turns, fast_sims, full_rate)
        if inner is not None:
            inner.simulation_num_per_move = full_sims if full else fast_sims
        action, _ = pl.action(state, turns, no_act, increase_temp, xo.philox_uniform(seed, game_id, 1, turns))
        move = script[turns] if turns < len(script) else None
        if trace is not None:
            st = pl.node_stats(state)
            trace.append(dict(state=state, action=action, moves=st["moves"], n=st["n"], sum_n=st["sum_n"], w=st["w"],
                              p=st["p"], no_act=list(no_act), inc=increase_temp, scripted=move, fast=not full))
        return move

    out = so.start_game(cfg, seed, game_id, ply, init_state)
    if inner is not None:
        inner.simulation_num_per_move = full_sims
    pl.close()
    return out
