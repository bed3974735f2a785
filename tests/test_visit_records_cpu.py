"""Root visit records in play records (engine.record_visits), the parts that need no GPU: the command-line switch, the
raw-entry -> pi conversion of the record writer, and that a pi-record file replays like its two-element form."""
import json

import numpy as np

from oracle import xq_oracle as xo


def test_record_visits_flag_reaches_the_engine_config():
    from cchess_alphazero.manager import build_config, create_parser
    off = build_config(create_parser().parse_args(["self"]))
    assert off.engine.record_visits is False
    on = build_config(create_parser().parse_args(["self", "--record-visits"]))
    assert on.engine.record_visits is True


def test_pi_keeps_edge_order_and_drops_banned_and_unvisited_edges():
    from cchess_alphazero.environment.lookup_tables import ActionLabelsRed
    from cchess_alphazero.lib.data_helper import pi_from_visits
    labels = [ActionLabelsRed.index(m) for m in ("7770", "1242", "0010", "3134", "7967")]
    moves = np.array(labels, dtype=np.uint16)
    n = np.array([5, 0, 12, 30, 1], dtype=np.int32)
    banned = np.array([False, False, False, True, False])
    pi = pi_from_visits(moves, n, banned, ActionLabelsRed)
    assert pi == [["7770", 5], ["0010", 12], ["7967", 1]]          # edge order, not label order
    total = sum(c for _, c in pi)
    # calc_policy (player.py:375-406): banned edges zeroed, then normalised over the rest
    policy = {m: c / total for m, c in pi}
    assert abs(sum(policy.values()) - 1.0) < 1e-12 and "3134" not in policy
    assert pi_from_visits(moves[:0], n[:0], banned[:0], ActionLabelsRed) == []
    # labels are passed through as given: the mover's frame, like the record's own moves
    assert pi_from_visits(np.array([labels[0]]), np.array([3]), np.array([False]), ActionLabelsRed) == [["7770", 3]]


def _random_game(rng, plies):
    state, data = xo.INIT_STATE, [xo.INIT_STATE]
    for t in range(plies):
        legal = xo.get_legal_moves(state)
        if not legal:
            break
        mv = legal[int(rng.integers(len(legal)))]
        counts = rng.integers(0, 9, len(legal))
        pi = [[m, int(c)] for m, c in zip(legal, counts) if c > 0] or [[mv, 1]]
        data.append([mv, 1 if t % 2 == 0 else -1, pi])
        state = xo.step(state, mv)
    return data


def test_pi_record_file_replays_like_its_two_element_form(tmp_path):
    from cchess_alphazero.lib.data_helper import read_game_data_from_file, write_game_data_to_file
    from cchess_alphazero.lib.record_decoder import split_games
    rng = np.random.default_rng(5)
    games = [_random_game(rng, 30), _random_game(rng, 17)]
    games[1][-1] = games[1][-1][:2]                         # an unsearched last move keeps the two-element form
    flat = [x for g in games for x in g]                    # nb_game_in_file = 2: one flat list
    path = tmp_path / "play_x.json"
    write_game_data_to_file(str(path), flat)
    back = read_game_data_from_file(str(path))
    assert back == json.loads(json.dumps(flat))
    split = split_games(back)
    assert len(split) == 2
    for g in split:
        stripped = [g[0]] + [it[:2] for it in g[1:]]
        # what the reference trainer reads (worker/optimize.py:245-246): item[0], item[1]
        seen = []
        for data in (g, stripped):
            state, pos = data[0], []
            for item in data[1:]:
                pos.append(state)
                state = xo.step(state, item[0])
            seen.append((pos, [item[1] for item in data[1:]]))
        assert seen[0] == seen[1]
