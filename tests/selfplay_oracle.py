"""SelfPlayWorker.start_game (reference worker/self_play.py:95-212) restated in Python over the oracle's rule functions
(test infrastructure), with the start position as an argument -- what `senv.INIT_STATE` is to the reference -- and the
player as a callable: start_game is the loop, once, and selfplay_game plays it with ONE oracle player; the capped and the
Gumbel games (playout_cap_oracle, gumbel_oracle) bring their own.  tests/test_selfplay_oracle_cpu.py pins selfplay_game
to the C restatement (oracle xqo_selfplay_game, itself pinned to
games recorded from the reference) from INIT_STATE, and to the reference's own games from other positions
(tests/golden/book_games.json, K = 1); the GPU's book games are then compared with it for K > 1, where the reference
is racy and parity is defined by the canonical order.

Random draws, as in the engine: random() -> philox(seed, game_id, stream 0, draw 0 resign lottery / draw 1 store
lottery), np.random.choice of ply t -> philox(seed, game_id, stream 1, t).  Draw 2 of stream 0 is the book-rate lottery
(book_lottery below)."""
from oracle import xq_oracle as xo


def oracle_cfg(pc, K=None, use_history=False):
    """pc: config.play-like object (the fields Search reads) -> the oracle's PlayCfg; K overrides search_threads."""
    return xo.play_cfg(simulation_num_per_move=pc.simulation_num_per_move,
                       search_threads=pc.search_threads if K is None else K, c_puct=pc.c_puct, noise_eps=0.0,
                       dirichlet_alpha=pc.dirichlet_alpha, tau_decay_rate=pc.tau_decay_rate, virtual_loss=pc.virtual_loss,
                       resign_threshold=pc.resign_threshold, min_resign_turn=pc.min_resign_turn, evaluate=0,
                       max_game_length=pc.max_game_length, enable_resign_rate=pc.enable_resign_rate,
                       use_history=int(use_history))


def book_lottery(seed, game_id, rate):
    """True when game `game_id` starts from the book at --book-rate `rate` (rates 0 and 1 draw nothing)."""
    if rate <= 0.0:
        return False
    return rate >= 1.0 or xo.philox_uniform(seed, game_id, 0, 2) < rate


def resign_enabled(cfg, seed, game_id):
    """The game's resign lottery, :102-105."""
    return xo.philox_uniform(seed, game_id, 0, 0) > cfg.enable_resign_rate


def start_game(cfg, seed, game_id, ply, init_state=None):
    """The loop.  ply(state, turns, no_act, increase_temp) -> the move of the position, None to resign: the player's
    action() (:124).  Returns dict(init_state, moves [labels as strings], value (from the first mover's view), turns,
    store, searched (ply() calls that returned a move), resigned, final_state)."""
    state = init_state or xo.INIT_STATE                                                         # :110
    history = [state]
    value = turns = no_eat_count = 0
    game_over = check = resigned = False
    final_move = None
    no_act, increase_temp = [], False
    while not game_over:
        action = ply(state, turns, no_act, increase_temp)                                       # :124
        if action is None:                                                                      # :126-129
            value, resigned = -1, True
            break
        history.append(action)
        state, no_eat = xo.new_step(state, action)                                              # :136
        turns += 1
        no_eat_count = no_eat_count + 1 if no_eat else 0
        history.append(state)
        if no_eat_count >= 120 or turns / 2 >= cfg.max_game_length:                             # :149-151
            game_over, value = True, 0
        else:
            d = xo.done(state, need_check=True)                                                 # :153
            game_over, value, final_move = d[0], d[1], d[2]
            check = d[3] if len(d) > 3 else False
            if not game_over and not xo.has_attack_chessman(state):                             # :154-158
                game_over, value = True, 0
            increase_temp, no_act = False, []
            if not game_over and not check and state in history[:-1]:                           # :161-175
                free_move = 0
                for i in range(len(history) - 1):
                    if history[i] == state:
                        if xo.will_check_or_catch(state, history[i + 1]):
                            no_act.append(history[i + 1])
                        elif not xo.be_catched(state, history[i + 1]):
                            increase_temp = True
                            free_move += 1
                            if free_move >= 3:
                                game_over, value = True, 0
                                break
    searched = turns
    if final_move:                                                                              # :177-184
        history.append(final_move)
        state = xo.step(state, final_move)
        turns += 1
        value = -value
        history.append(state)
    if turns % 2 == 1:                                                                          # :190-191
        value = -value
    store = xo.philox_uniform(seed, game_id, 0, 1) > 0.9 if turns < 10 else True                # :194-200
    return dict(init_state=history[0], moves=history[1::2], value=value, turns=turns, store=bool(store),
                searched=searched, resigned=resigned, final_state=state)


def selfplay_game(cfg, stub, seed, game_id, init_state=None, trace=None):
    """start_game played by ONE oracle player.  cfg: xo.PlayCfg.  Returns start_game's dict; `trace` (a list) receives
    one dict per action() call: state, action, the root's moves and visit counts."""
    pl = xo.Player(cfg, stub, enable_resign=resign_enabled(cfg, seed, game_id), seed=seed, game_id=game_id)

    def ply(state, turns, no_act, increase_temp):
        action, _ = pl.action(state, turns, no_act, increase_temp, xo.philox_uniform(seed, game_id, 1, turns))
        if trace is not None:
            st = pl.node_stats(state)
            trace.append(dict(state=state, action=action, moves=st["moves"], n=st["n"], sum_n=st["sum_n"],
                              no_act=list(no_act), inc=increase_temp))
        return action

    out = start_game(cfg, seed, game_id, ply, init_state)
    pl.close()
    return out
