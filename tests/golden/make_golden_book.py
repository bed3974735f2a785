"""Golden self-play games from a start-position book, produced by the REFERENCE's own SelfPlayWorker.start_game
(worker/self_play.py:95-212) with `senv.INIT_STATE` -- the module attribute start_game reads when it is called (:110) --
set to each position of tests/golden/book.txt.  No reference code is modified or copied.

Environment control as in make_golden_mcts.py (whose helpers are imported): keras / tensorflow are mocks, the stub
networks of tests/stub_net.py answer the pipe, random.random / np.random.choice consume the Philox stream
(seed, game_id, stream 0 / 1), search_threads = 1, noise 0.  Game `game_id` starts from book[game_id % n]: the rule of
cz_search_set_book at rate 1.

    python tests/golden/make_golden_book.py          -> tests/golden/book_games.json
"""
import json
import os
import sys
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_mcts as mg  # noqa: E402  (puts the reference and tests/ on sys.path)
import stub_net  # noqa: E402

senv = mg.senv
ref_player = mg.ref_player

N_GAMES = 70          # game ids 0 .. 69 per configuration: ten passes over the seven positions

# the two stub networks, two settings of tau_decay_rate; config "a" also draws the resign lottery both ways
CONFIGS = [
    dict(name="hash_tau098", stub=dict(kind="hash", salt=71), sims=30, tau=0.98, max_game_length=20, seed=4101,
         c_puct=1.5, enable_resign_rate=0.5, resign_threshold=-0.5, min_resign_turn=4),
    dict(name="uniform_tau09", stub=dict(kind="uniform", value=0.1), sims=20, tau=0.9, max_game_length=16, seed=4102,
         c_puct=1.5, enable_resign_rate=1.0, resign_threshold=-0.92, min_resign_turn=20),
]


def read_book(path):
    """The positions of the book file in the mover's frame (the reference's own fen_to_state / fliped_state)."""
    out = []
    with open(path) as f:
        for line in f:
            line = line.split("#")[0].strip()
            if not line:
                continue
            parts = line.split()
            if len(parts) == 1:
                out.append(parts[0])
            else:
                state = senv.fen_to_state(line)
                out.append(senv.fliped_state(state) if parts[1] == "b" else state)
    return out


def record_game(sp, c, init_state, game_id):
    cfg = mg.make_cfg(c["sims"], c_puct=c["c_puct"], tau_decay_rate=c["tau"], max_game_length=c["max_game_length"],
                      enable_resign_rate=c["enable_resign_rate"], resign_threshold=c["resign_threshold"],
                      min_resign_turn=c["min_resign_turn"])
    cfg.play_data.nb_game_in_file = 1
    seed = c["seed"]
    calls = {"choice": 0, "random": 0}

    def fake_choice(a, p=None, _c=calls):
        u = stub_net.philox_uniform(seed, game_id, 1, _c["choice"])
        _c["choice"] += 1
        return stub_net.numpy_choice(p, u)

    def fake_random(_c=calls):
        u = stub_net.philox_uniform(seed, game_id, 0, _c["random"])
        _c["random"] += 1
        return u

    np.random.choice = fake_choice
    np.random.dirichlet = lambda alpha, size=None: np.full(len(alpha), 1.0 / len(alpha))
    sp.random = fake_random
    saved = {}

    def fake_save(self, idx, data, _s=saved):
        _s["data"] = data

    sp.SelfPlayWorker.save_play_data = fake_save
    sp.SelfPlayWorker.remove_play_data = lambda self: None
    pipe = stub_net.StubPipe(mg.stub_fn(c["stub"]))
    worker = sp.SelfPlayWorker(cfg, pipes=[pipe], pid=0, use_history=False)
    init_saved = sp.senv.INIT_STATE
    sp.senv.INIT_STATE = init_state
    try:
        v, turns, state, store = worker.start_game(1, defaultdict(ref_player.VisitState))
    finally:
        sp.senv.INIT_STATE = init_saved
    data = saved.get("data")
    if store:
        assert data[0] == init_state and len(data) == turns + 1
    # (start_game keeps no move list of a game it does not store: main() logs the moves at the player)
    return dict(game_id=game_id, position=init_state, value=v, turns=turns, store=bool(store),
                moves=None if data is None else [d[0] for d in data[1:]], final_state=state,
                n_random_calls=calls["random"], n_choice_calls=calls["choice"])


def main():
    mg._shim_tf()
    import cchess_alphazero.worker.self_play as sp
    book = read_book(os.path.join(HERE, "book.txt"))
    for s in book:                                     # the book is valid under the reference's own rules
        assert not senv.done(s)[0] and senv.has_attack_chessman(s), s
    # a game that is not stored keeps no move list in start_game: log the moves at the player
    orig_action = ref_player.CChessPlayer.action
    log = []

    def logged_action(self, state, turns, no_act=None, depth=None, infinite=False, hist=None, increase_temp=False,
                      _orig=orig_action):
        r = _orig(self, state, turns, no_act, depth, infinite, hist, increase_temp)
        log.append(r[0])
        return r

    ref_player.CChessPlayer.action = logged_action
    sp.CChessPlayer.action = logged_action
    # ... and the king capture start_game appends (:177-184) is the final_move of the last senv.done() it called
    orig_done = senv.done
    last_done = []

    def logged_done(*a, **kw):
        r = orig_done(*a, **kw)
        last_done[:] = [r]
        return r

    senv.done = logged_done
    configs = []
    for c in CONFIGS:
        games = []
        for gid in range(N_GAMES):
            del log[:]
            g = record_game(sp, c, book[gid % len(book)], gid)
            searched = [a for a in log if a is not None]
            # searched moves, then the appended king capture if there was one (turns counts it)
            if g["moves"] is None:
                g["moves"] = searched + ([last_done[0][2]] if g["turns"] > len(searched) else [])
                assert len(g["moves"]) == g["turns"] and None not in g["moves"], g
            else:
                assert g["moves"][:len(searched)] == searched, (g["moves"], searched)
            g["searched"] = len(searched)
            games.append(g)
            print(c["name"], "game", gid, "pos", gid % len(book), "turns", g["turns"], "value", g["value"],
                  "store", g["store"], flush=True)
        configs.append(dict(c, games=games))
    ref_player.CChessPlayer.action = orig_action
    sp.CChessPlayer.action = orig_action
    senv.done = orig_done
    meta = mg.meta()
    meta["generator"] = "tests/golden/make_golden_book.py"
    meta["reference"] = "NeymarL/ChineseChess-AlphaZero, SelfPlayWorker.start_game, search_threads=1"
    with open(os.path.join(HERE, "book_games.json"), "w") as f:
        json.dump({"meta": meta, "book": book, "configs": configs}, f, separators=(",", ":"))


if __name__ == "__main__":
    main()
