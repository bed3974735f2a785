"""A classifier of finished games (test infrastructure): replays a game -- start state + moves -- through the oracle's
rule functions alone, with no search, along the branches of SelfPlayWorker.start_game (reference worker/self_play.py
:95-212) or, with arena=True, of EvaluateWorker.start_game (worker/evaluator.py:147-250: the repetition handling comes
BEFORE the move and has no be_catched branch), and says how the game ended and what the loop must have handed to every
search on the way.  tests/test_endings_oracle_cpu.py pins it, ply by ply, to the `trace` of tests/selfplay_oracle.py and
tests/arena_oracle.py on games recorded from the reference.

    classify(init_state, moves, max_game_length, arena=False) -> dict(
        ending    'no_eat120' (120 plies without a capture, BEFORE the length cap: turns < 2 * max_game_length),
                  'length', 'no_attack', 'free3', 'mate' (done() without a move to append), 'king_capture' (done() with
                  the appended capture as the last move), 'resign' (the moves stop while the game is still on)
        value     from the first mover's view, as the loop computes it (resign: the mover of the last search loses)
        turns     len(moves);  searched: moves that came from a search (all but an appended king capture)
        states    the position searched at ply t, t = 0 .. searched (the resignation's search included)
        bans      bans[t]: the no_act list handed to the search of ply t ([] / None as the loop has it)
        inc       inc[t]: the increase_temp flag handed to the search of ply t
        scans     one dict(ply, matches) per repetition check that found the position again: `ply` = the plies played
                  when the check ran (the index of the checked position in the game's history), `matches` = the plies of
                  the earlier equal positions the check walked over, ascending (it stops at the third free repetition)
        block0_late, block1, both   see scan_flags
        inc_sampled   plies t with inc[t] set whose search went on to choose a move (moves[t] exists).  In self-play that
                      move is sampled at tau = 0.5 (player.py apply_temperature); in an arena with config.opts.evaluate
                      the flag restarts the search from zero visits (sum_n) but the move stays the argmax
        ban_plies     plies t with a non-empty bans[t]
    )

The device walks a game's history 64 plies per ballot; scan_flags names the trips a scan needs:
    block0_late  a match below ply 64 in a scan that ran after more than 64 plies
    block1       a match at ply >= 64
    both         both in one scan."""
import types

from oracle import xq_oracle as xo

DRAWS = ("no_eat120", "length", "no_attack", "free3")
BLOCK = 64


def scan_flags(scans):
    late = [any(m < BLOCK for m in s["matches"]) and s["ply"] > BLOCK for s in scans]
    hi = [any(m >= BLOCK for m in s["matches"]) for s in scans]
    return dict(block0_late=any(late), block1=any(hi), both=any(a and b for a, b in zip(late, hi)))


def _repetitions(history, state, arena, scans, turns):
    """The loop over history[:-1] of both workers: (no_act, increase_temp, third free repetition)."""
    no_act, inc, free, matches = [], bool(arena), 0, []
    draw = False
    for i in range(0, len(history) - 1, 2):
        if history[i] != state:
            continue
        matches.append(i // 2)
        if xo.will_check_or_catch(state, history[i + 1]):
            no_act.append(history[i + 1])
        elif arena or not xo.be_catched(state, history[i + 1]):
            inc = True
            free += 1
            if free >= 3:
                draw = True
                break
    scans.append(dict(ply=turns, matches=matches))
    return no_act, inc, draw


def classify(init_state, moves, max_game_length, arena=False):
    state = init_state
    history = [state]
    turns = no_eat_count = value = 0
    check = False
    ending = final_move = None
    states, bans, incs, scans = [], [], [], []
    no_act, inc = ([], False) if not arena else (None, False)
    while ending is None:
        if arena:                                               # evaluator.py:182-203
            no_act, inc = None, False
            if not check and state in history[:-1]:
                no_act, inc, draw = _repetitions(history, state, True, scans, turns)
                if draw:
                    ending, value = "free3", 0
                    break
        states.append(state)
        bans.append(no_act)
        incs.append(inc)
        if turns >= len(moves):                                 # action() returned None
            ending, value = "resign", -1
            break
        action = moves[turns]
        history.append(action)
        state, no_eat = xo.new_step(state, action)
        turns += 1
        no_eat_count = no_eat_count + 1 if no_eat else 0
        history.append(state)
        if no_eat_count >= 120 or turns / 2 >= max_game_length:
            ending, value = ("no_eat120" if turns < 2 * max_game_length else "length"), 0
            break
        d = xo.done(state, need_check=True)
        over, value, final_move = d[0], d[1], d[2]
        check = d[3] if len(d) > 3 else False
        if over:
            ending = "king_capture" if final_move else "mate"
            break
        if not xo.has_attack_chessman(state):
            ending, value = "no_attack", 0
            break
        if not arena:                                           # self_play.py:160-175
            no_act, inc = [], False
            if not check and state in history[:-1]:
                no_act, inc, draw = _repetitions(history, state, False, scans, turns)
                if draw:
                    ending, value = "free3", 0
    searched = turns
    if ending == "king_capture":
        if moves[turns:] != [final_move]:
            raise ValueError(f"the game must end with the king capture {final_move}: {moves[turns:]}")
        state = xo.step(state, final_move)
        turns += 1
        value = -value
    elif turns != len(moves):
        raise ValueError(f"{ending} after {turns} plies, but the game has {len(moves)} moves")
    if turns % 2 == 1:
        value = -value
    out = dict(ending=ending, value=value, turns=turns, searched=searched, final_state=state, states=states, bans=bans,
               inc=incs, scans=scans,
               inc_sampled=[t for t, f in enumerate(incs) if f and t < searched],
               ban_plies=[t for t, b in enumerate(bans) if b])
    out.update(scan_flags(scans))
    return out


def coverage(results, both=True):
    """The counts the coverage condition is stated on, over classify() results."""
    n = {e: sum(1 for r in results if r["ending"] == e) for e in
         ("no_eat120", "free3", "no_attack", "length", "mate", "king_capture", "resign")}
    for k in ("block0_late", "block1") + (("both",) if both else ()):
        n[k] = sum(1 for r in results if r[k])
    n["ban_plies"] = sum(len(r["ban_plies"]) for r in results)
    n["inc_sampled"] = sum(len(r["inc_sampled"]) for r in results)
    return n


def assert_coverage(results, both=True):
    """Issue "Test the self-play and arena game loops on their rare endings": at least two games each of no_eat120,
    free3 and no_attack, one at the length cap, one each of the scan classes, two plies with a ban, two plies with
    increase_temp handed to a search that chose a move."""
    n = coverage(results, both)
    need = dict(no_eat120=2, free3=2, no_attack=2, length=1, block0_late=1, block1=1, ban_plies=2, inc_sampled=2)
    if both:
        need["both"] = 1
    short = {k: (n[k], v) for k, v in need.items() if n[k] < v}
    assert not short, f"coverage condition missed (have, need): {short}; all counts: {n}"
    return n


# ---- the runs of tests/test_gpu_endings.py at K > 1 ------------------------------------------------------------------------
# Chosen on the oracle (tests/test_endings_oracle_cpu.py asserts what their games reach): (K, stub salt, c_puct, history
# planes, game ids).  Seed, tau, max_game_length and the book are those of tests/golden/endings_games.json; 16
# simulations.  At K = 8 a 16-simulation search is two batches wide and repeats positions rarely: of the 32 games of a
# run at c_puct 1.5, salts 1-300 x seeds 4242-4245, none met the coverage condition; at c_puct 0.5 about one salt in
# fifty does.  The ids are the fewest games of the run's first 32 that carry the condition (the device plays all 32
# slots, slot g's first game being id g) plus its shortest mate and king capture of 8 plies or more.
SELFPLAY_SIMS = 16
SELFPLAY_CASES = [
    (8, 43, 0.5, False, (0, 2, 12, 15, 17, 21, 22, 26, 28)),
    (3, 25, 1.5, False, (0, 1, 7, 16, 20, 21, 27, 28, 30)),
    (8, 17, 0.5, True, (2, 4, 5, 8, 10, 13, 17, 20, 30)),
]
ARENA_K8 = dict(salts=(42, 142), seed=5042, c_puct=0.5, sims=16)
ARENA_K8_INDICES = (0, 2, 5, 7, 12, 15, 16, 24, 29)


def selfplay_cfg(c, K=1, use_history=False):
    """c: a config of endings_games.json -> the oracle's PlayCfg."""
    return xo.play_cfg(simulation_num_per_move=c["sims"], search_threads=K, c_puct=c["c_puct"], tau_decay_rate=c["tau"],
                       max_game_length=c["max_game_length"], enable_resign_rate=c["enable_resign_rate"],
                       resign_threshold=c["resign_threshold"], min_resign_turn=c["min_resign_turn"],
                       use_history=int(use_history))


def arena_pc(a, K=1):
    """a: the arena settings of endings_games.json -> a config.play-like object."""
    return types.SimpleNamespace(simulation_num_per_move=a["sims"], search_threads=K, c_puct=a["c_puct"],
                                 dirichlet_alpha=0.2, tau_decay_rate=a["tau"], virtual_loss=3, noise_eps=0.0,
                                 max_game_length=a["max_game_length"])


def arena_u_fn(seed):
    return lambda idx, ply: xo.philox_uniform(seed, idx, 1, ply)


def assert_trace_agrees(c, trace, what):
    """classify() result c against an oracle trace: the position, the ban list and the increase_temp flag of every search."""
    assert len(trace) == len(c["states"]), what
    for t, e in enumerate(trace):
        assert (e["state"], e["no_act"], e["inc"]) == (c["states"][t], c["bans"][t], c["inc"][t]), (what, t)


def arena_moves(init_state, trace, turns):
    """The moves of an arena game from its trace: the searched ones, then the king capture the loop appends (it is in no
    trace: the final_move of done() in the last position)."""
    moves = [e["action"] for e in trace if e["action"] is not None]
    if turns > len(moves):
        state = init_state
        for m in moves:
            state = xo.step(state, m)
        moves.append(xo.done(state)[2])
    return moves
