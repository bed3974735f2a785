"""run.py reanalyse without a device: the loader (lib/reanalyse.py) on every record form, the writer's output under
record_decoder, the refusals of the option table and the command line, and the scripted oracle (tests/reanalyse_oracle.py)
on a game's own moves.  The device's half is tests/test_gpu_reanalyse.py."""
import json

import numpy as np
import pytest

import reanalyse_oracle as ro
import selfplay_oracle as so
from cchess_alphazero import manager, search_options as sopt
from cchess_alphazero.config import Config
from cchess_alphazero.environment.lookup_tables import ActionLabelsRed, label_index
from cchess_alphazero.environment.static_env import INIT_STATE, state_to_array
from cchess_alphazero.lib import reanalyse as ra
from cchess_alphazero.lib.record_decoder import split_games
from conftest import load_golden
from oracle import xq_oracle as xo

SPEC = dict(kind="hash", salt=31)


def _cfg(K=1, sims=16, mgl=8):
    return xo.play_cfg(simulation_num_per_move=sims, search_threads=K, c_puct=1.5, noise_eps=0.0, dirichlet_alpha=0.2,
                       tau_decay_rate=0.9, virtual_loss=3, resign_threshold=-0.92, min_resign_turn=20, evaluate=0,
                       max_game_length=mgl, enable_resign_rate=1.0, use_history=0)


def _record(init, moves, z, form=2):
    """A record game in one of the forms lib/data_helper.py describes: `form` fields per item (the last move keeps two, as
    an appended king capture does)."""
    tail = [[[moves[0], 7], [moves[-1], 9]], 1, 0.25, 1.5]
    game = [init]
    for i, m in enumerate(moves):
        item = [m, z if i % 2 == 0 else -z]
        game.append(item + tail[:form - 2] if i < len(moves) - 1 or len(moves) == 1 else item)
    return game


@pytest.fixture(scope="module")
def games():
    """Six oracle self-play games: three from the opening position, three from book positions (one with a mover's frame
    of its own)."""
    book = load_golden("book_games.json")["book"]
    out = []
    for gid in range(6):
        init = None if gid < 3 else book[gid % len(book)]
        g = so.selfplay_game(_cfg(), SPEC, 77, gid, init_state=init)
        out.append((g["init_state"], g["moves"], int(g["value"])))
    return out


# ---- 1. the loader -------------------------------------------------------------------------------------------------------
def test_loader_packs_every_record_form(games, tmp_path):
    recs = [_record(init, moves, z, form=2 + i) for i, (init, moves, z) in enumerate(games[:5])]
    recs.append(_record(*games[5]))
    assert {len(it) for r in recs for it in r[1:]} == {2, 3, 4, 5, 6}
    assert any(r[0] != INIT_STATE for r in recs)                        # a book-start record
    path = tmp_path / "play_several.json"
    path.write_text(json.dumps([x for r in recs for x in r]))           # several games, flat, as nb_game_in_file > 1 writes
    loaded = ra.load_games(str(path))
    assert loaded == recs == split_games(json.loads(path.read_text()))
    scripts, kept, aside = ra.pack_scripts(loaded, 2 * 8 + 3)
    assert not aside and kept == [ra.Source(0, i) for i in range(6)]
    # what expand_records and cz_replay_games are given for the same file (lib/record_decoder.py, lib/replay_window.py)
    lens = [len(g) - 1 for g in loaded]
    assert np.array_equal(scripts.init_boards, np.stack([state_to_array(g[0]) for g in loaded]))
    assert np.array_equal(scripts.init_boards, np.stack([xo.state_to_board(g[0]) for g in loaded]))
    assert scripts.labels.tolist() == [label_index(it[0]) for g in loaded for it in g[1:]]
    assert np.array_equal(scripts.offsets, np.concatenate([[0], np.cumsum(lens)]))
    assert scripts.z.tolist() == [z for _, _, z in games]
    assert (scripts.init_boards.dtype, scripts.labels.dtype, scripts.offsets.dtype, scripts.z.dtype) == \
           (np.int8, np.uint16, np.int32, np.int8)
    for i, (init, moves, z) in enumerate(games):
        b, lab, zi = ra.script_of(scripts, i)
        assert [ActionLabelsRed[int(x)] for x in lab] == moves and zi == z


def test_loader_sets_aside_empty_and_overlong_games(games):
    init, moves, z = games[0]
    recs = [_record(init, moves, z), [INIT_STATE], _record(init, (moves * 9)[:20], z), _record(*games[3])]
    src = [ra.Source(3, i) for i in range(4)]
    scripts, kept, aside = ra.pack_scripts(recs, 19, sources=src)
    assert kept == [src[0], src[3]] and [s for s, _ in aside] == [src[1], src[2]]
    assert aside[0][1] == "empty" and "20 plies" in aside[1][1]
    assert len(scripts.z) == 2 and scripts.offsets.tolist() == [0, len(moves), len(moves) + len(games[3][1])]
    kingless = _record(init.replace("s", "1", 1), moves, z)            # a start position the search could not vouch for
    assert [why for _, why in ra.pack_scripts([kingless], 19)[2]] == ["a start position without one king a side"]
    nothing, kept, aside = ra.pack_scripts([[INIT_STATE]], 19)
    assert kept == [] and nothing.init_boards.shape == (0, 90) and nothing.offsets.tolist() == [0]


def test_batches_take_whole_files_up_to_the_budget():
    assert ra.batches([5, 5, 5], 10) == [(0, 2), (2, 3)]
    assert ra.batches([50, 1, 1], 10) == [(0, 1), (1, 3)]              # a file over the budget is a batch of its own
    assert ra.batches([], 10) == [] and ra.batches([3], 10) == [(0, 1)]


# ---- 2. the writer -------------------------------------------------------------------------------------------------------
def test_writer_keeps_the_sources_moves_and_values(games, tmp_path):
    from cchess_alphazero.lib.data_helper import read_game_data_from_file, write_game_data_to_file
    out = []
    for i, (init, moves, z) in enumerate(games):
        source = _record(init, moves, 0.5 * z if i == 0 else z, form=2 + i % 3)      # (a value that is no integer stays)
        drained = [INIT_STATE] + [[m, 9, [[m, 16]], 1, 0.125, 2.0] for m in moves[:-1]] + [[moves[-1], 9]]
        new = ra.rewrite_game(source, drained)
        assert new[0] == init
        assert [it[:2] for it in new[1:]] == [it[:2] for it in source[1:]]
        assert all(it[2:] == [[[it[0], 16]], 1, 0.125, 2.0] for it in new[1:-1]) and len(new[-1]) == 2
        out += new
        with pytest.raises(ValueError):
            ra.rewrite_game(source, drained[:-1])
        with pytest.raises(ValueError):
            ra.rewrite_game(source, [INIT_STATE] + [["0001", 0]] * len(moves))
    path = str(tmp_path / "play_out.json")
    write_game_data_to_file(path, out)
    back = split_games(read_game_data_from_file(path))
    assert [(g[0], [it[0] for it in g[1:]]) for g in back] == [(init, moves) for init, moves, _ in games]
    from cchess_alphazero.worker.reanalyse import output_name
    cfg = Config("mini")
    assert output_name(cfg, "/x/trained/play_20240101-000000.1.json") == "play_20240101-000000.1.json"
    assert output_name(cfg, "/x/old/game7.json") == "play_game7.json"


# ---- 3. the option table -------------------------------------------------------------------------------------------------
EXCLUDED = dict(gumbel=(dict(gumbel=8), ["--gumbel", "8"]), solver=(dict(solver=True), ["--solver"]),
                kld_gain=(dict(kld_gain=1e-3), ["--kld-gain", "1e-3"]),
                smart_pruning=(dict(smart_pruning=True), ["--smart-pruning"]))


def test_the_scripts_exclusions_are_the_issues():
    assert [k for k, _ in sopt.SCRIPT_EXCLUDES] == list(EXCLUDED) and sopt.SCRIPT_NEEDS[0] == "record_visits"
    # the script is no value of the table: the pins of tests/test_search_options_cpu.py hold
    assert len(sopt.EXCLUDES) == 11 and len(sopt.DEFAULTS) == 16


@pytest.mark.parametrize("key", list(EXCLUDED))
def test_a_script_is_refused_beside_each_excluded_option(key):
    values, words = EXCLUDED[key]
    sopt.check(dict(values, record_visits=True))                         # fine without a script
    for flags in (False, True):
        with pytest.raises(sopt.SearchOptionError, match=f"a script excludes {sopt.VALUES[key].flag if flags else key}: "):
            sopt.check(dict(values, record_visits=True), flags=flags, script=True)
    with pytest.raises(SystemExit):
        manager.build_config(manager.create_parser().parse_args(["reanalyse"] + words))


def test_a_script_needs_the_visit_record_and_takes_the_rest():
    with pytest.raises(sopt.SearchOptionError, match="a script needs record_visits"):
        sopt.check(dict(fast_sims=8), script=True)
    sopt.check(dict(record_visits=True, fast_sims=8, forced_playouts=2.0, record_q=True, record_surprise=True,
                    leaf_mirror=0.5), script=True)
    parse = manager.create_parser().parse_args
    cfg = manager.build_config(parse(["reanalyse", "--record-q", "--record-surprise", "--fast-sims", "8", "--full-rate", "0.5",
                                      "--forced-playouts", "2", "--leaf-mirror", "0.5", "--sims", "24", "--records", "/r",
                                      "--out", "/o", "--reanalyse-plies", "5000"]))
    e = cfg.engine
    assert e.record_visits is True and (e.record_q, e.record_surprise, e.fast_sims, e.full_rate) == (True, True, 8, 0.5)
    assert (e.reanalyse_records, e.reanalyse_out, e.reanalyse_plies) == ("/r", "/o", 5000)
    assert cfg.play.simulation_num_per_move == 24
    assert manager.build_config(parse(["reanalyse"])).engine.record_visits is True    # implied
    for words in (["--eval-cache", "10"], ["--book", "b.txt"], ["--resign-audit"], ["--reanalyse-plies", "0"]):
        with pytest.raises(SystemExit):
            manager.build_config(parse(["reanalyse"] + words))
    for words in (["--records", "/r"], ["--out", "/o"], ["--reanalyse-plies", "9"]):
        with pytest.raises(SystemExit):
            manager.build_config(parse(["self"] + words))
    assert manager.build_config(parse(["self"])).engine.record_visits is False


def test_the_engine_refuses_before_it_asks_for_a_device(monkeypatch, games):
    from cchess_alphazero import _native
    from cchess_alphazero.engine import SelfPlayEngine

    def no_device():
        raise AssertionError("the options are checked before a device is asked for")
    monkeypatch.setattr(_native, "require_gpu", no_device)
    monkeypatch.delenv("CZ_BOOK", raising=False)
    scripts, _, _ = ra.pack_scripts([_record(*games[0])], 19)
    cfg = Config("mini")
    for key, (values, _) in EXCLUDED.items():
        if key == "smart_pruning":
            continue                                        # (not an option of the self-play engine)
        with pytest.raises(ValueError, match=f"a script excludes {key}"):
            SelfPlayEngine(cfg, 2, script=scripts, record_visits=True, **values)
    with pytest.raises(ValueError, match="a script needs record_visits"):
        SelfPlayEngine(cfg, 2, script=scripts)
    with pytest.raises(ValueError, match="a script excludes resign_audit"):
        SelfPlayEngine(cfg, 2, script=scripts, record_visits=True, resign_audit=True)
    with pytest.raises(ValueError, match="a script excludes a book"):
        SelfPlayEngine(cfg, 2, script=scripts, record_visits=True, book=[INIT_STATE])


# ---- 4. the scripted oracle on a game's own moves ------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4])
def test_scripted_oracle_on_a_games_own_moves_is_selfplay(K):
    """A game that the rules ended: walking its own moves with the same network and seed searches what self-play searched."""
    cfg = _cfg(K=K, sims=16, mgl=6)
    checked = 0
    for gid in range(3):
        t0, t1 = [], []
        ref = so.selfplay_game(cfg, SPEC, 5, gid, trace=t0)
        assert not ref["resigned"]
        for script in (ref["moves"], ref["moves"][:ref["searched"]]):       # with and without an appended king capture
            del t1[:]
            out = ro.scripted_game(cfg, SPEC, 5, gid, script, trace=t1)
            assert out["moves"] == ref["moves"] and out["searched"] == ref["searched"]
            assert len(t1) == len(t0)
            for a, b in zip(t0, t1):
                assert (a["state"], a["action"], a["no_act"], a["inc"], a["sum_n"]) == \
                       (b["state"], b["action"], b["no_act"], b["inc"], b["sum_n"])
                assert (a["moves"] == b["moves"]).all() and (a["n"] == b["n"]).all()
                assert b["scripted"] == b["action"] and not b["fast"]
                checked += 1
    assert checked > 30


def test_scripted_oracle_searches_the_position_after_a_cut_script():
    cfg = _cfg(sims=16, mgl=6)
    ref = so.selfplay_game(cfg, SPEC, 5, 0)
    trace = []
    out = ro.scripted_game(cfg, dict(kind="hash", salt=5), 19, 0, ref["moves"][:5], trace=trace)
    assert out["moves"] == ref["moves"][:5] and out["resigned"] and len(trace) == 6
    assert [e["scripted"] for e in trace] == ref["moves"][:5] + [None]
