"""Golden games that reach the rare endings of the game loops, produced by the REFERENCE's own
SelfPlayWorker.start_game (worker/self_play.py:95-212) and EvaluateWorker.start_game (worker/evaluator.py:147-250) with
`senv.INIT_STATE` set to the sparse endgame positions of tests/golden/endgame_book.txt: from those a 10-simulation search
at max_game_length = 100 plays games that end by the 120-plies-without-capture draw, by the "no attacking piece" draw, by
three free repetitions and at the length cap, with perpetual-check bans and with repetitions found after more than 64
plies.  No reference code is modified or copied.

Environment control as in make_golden_book.py / make_golden_mcts.py (whose helpers are imported): stub networks, Philox
draws, search_threads = 1, noise 0.  Self-play game `game_id` starts from book[game_id % n] (cz_search_set_book at rate
1), arena game `idx` from book[(idx // 2) % n] (worker/evaluator.py book_states).  The salt, the seed and the game ids
were chosen with the oracle (tests/selfplay_oracle.py, tests/arena_oracle.py + tests/game_endings.py) so that the recorded
games meet the coverage condition that tests/test_endings_oracle_cpu.py asserts; what is recorded is what the reference did.

    python tests/golden/make_golden_endings.py          -> tests/golden/endings_games.json
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_book as mb  # noqa: E402  (puts the reference and tests/ on sys.path)
import make_golden_mcts as mg  # noqa: E402

senv = mg.senv
ref_player = mg.ref_player

SELFPLAY = dict(name="hash_tau09", stub=dict(kind="hash", salt=8), sims=10, tau=0.9, max_game_length=100, seed=4242,
                c_puct=1.5, enable_resign_rate=1.0, resign_threshold=-0.92, min_resign_turn=20)
SELFPLAY_IDS = [0, 3, 4, 5, 6, 9, 10, 12, 13, 17, 22, 27, 28]

ARENA = dict(salts=(36, 136), sims=10, tau=0.9, max_game_length=100, seed=5036, c_puct=1.0, evaluate=True)
ARENA_IDS = [0, 1, 2, 5, 8, 12, 19, 30]


def selfplay_games(sp, book):
    orig_action = ref_player.CChessPlayer.action
    log = []

    def logged_action(self, state, turns, no_act=None, depth=None, infinite=False, hist=None, increase_temp=False,
                      _orig=orig_action):
        r = _orig(self, state, turns, no_act, depth, infinite, hist, increase_temp)
        node = self.tree[state]
        n = [int(node.a[m].n) if m in node.a else 0 for m in node.legal_moves]
        log.append(dict(action=r[0], crc=mg.visit_crc(node.legal_moves, n), sum_n=int(node.sum_n),
                        no_act=list(no_act or []), inc=bool(increase_temp)))
        return r

    # the king capture start_game appends (:177-184) is the final_move of the last senv.done() it called
    orig_done = senv.done
    last_done = []

    def logged_done(*a, **kw):
        r = orig_done(*a, **kw)
        last_done[:] = [r]
        return r

    ref_player.CChessPlayer.action = logged_action
    sp.CChessPlayer.action = logged_action
    senv.done = logged_done
    games = []
    try:
        for gid in SELFPLAY_IDS:
            del log[:]
            g = mb.record_game(sp, SELFPLAY, book[gid % len(book)], gid)
            searched = [p["action"] for p in log if p["action"] is not None]
            moves = searched + ([last_done[0][2]] if g["turns"] > len(searched) else [])
            assert len(moves) == g["turns"] and None not in moves, g
            assert g["moves"] is None or g["moves"] == moves, (g["moves"], moves)
            g["moves"], g["searched"] = moves, len(searched)
            g["plies"] = [dict(p) for p in log]                 # one per action() call: what the loop handed to it
            games.append(g)
            print("self-play game", gid, "pos", gid % len(book), "turns", g["turns"], "value", g["value"],
                  "ban plies", sum(1 for p in log if p["no_act"]), "inc plies", sum(1 for p in log if p["inc"]), flush=True)
    finally:
        ref_player.CChessPlayer.action = orig_action
        sp.CChessPlayer.action = orig_action
        senv.done = orig_done
    return games


def arena_games(ev, book):
    games = []
    for idx in ARENA_IDS:
        init = book[(idx // 2) % len(book)]
        g = mg._arena_game(ev, dict(ARENA, name=f"arena_{idx}", idx=idx, init_state=init))
        searched = [p["action"] for p in g["plies"]]
        assert None not in searched
        # start_game returns no move list: the searched moves, then the appended king capture (:235-240) if turns counts one
        state = init
        for m in searched:
            state = senv.step(state, m)
        g["moves"] = searched + ([senv.done(state)[2]] if g["turns"] > len(searched) else [])
        assert len(g["moves"]) == g["turns"] and None not in g["moves"], g["name"]
        g["searched"] = len(searched)
        for k in ARENA:                                     # (the run's settings are recorded once, beside the games)
            del g[k]
        for p in g["plies"]:
            del p["tree"]
        games.append(g)
    return games


def main():
    mg._shim_tf()
    import cchess_alphazero.worker.evaluator as ev
    import cchess_alphazero.worker.self_play as sp
    book = mb.read_book(os.path.join(HERE, "endgame_book.txt"))
    for s in book:                                     # the book is valid under the reference's own rules
        assert not senv.done(s)[0] and senv.has_attack_chessman(s), s
    selfplay = dict(SELFPLAY, games=selfplay_games(sp, book))
    arena = dict(ARENA, games=arena_games(ev, book))
    meta = mg.meta()
    meta["generator"] = "tests/golden/make_golden_endings.py"
    meta["reference"] = ("NeymarL/ChineseChess-AlphaZero, SelfPlayWorker.start_game and EvaluateWorker.start_game, "
                         "search_threads=1")
    with open(os.path.join(HERE, "endings_games.json"), "w") as f:
        json.dump({"meta": meta, "book": book, "configs": [selfplay], "arena": arena}, f, separators=(",", ":"))


if __name__ == "__main__":
    main()
