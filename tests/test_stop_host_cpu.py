"""The host layers of the stop rules (run.py self --kld-gain, run.py eval --smart-pruning, the UCI option SmartPruning) that need
no device: the command line, the configuration's defaults, the UCI option, the counter names and the visit-entry flag."""
import io
import re
import os

import numpy as np
import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_command_line_accepts_and_refuses():
    from cchess_alphazero import manager
    parse = manager.create_parser().parse_args
    cfg = manager.build_config(parse(["self"]))
    assert cfg.engine.kld_gain == 0.0 and cfg.engine.kld_interval == 100 and cfg.engine.smart_pruning is False
    cfg = manager.build_config(parse(["self", "--kld-gain", "2e-4"]))
    assert cfg.engine.kld_gain == 2e-4 and cfg.engine.kld_interval == 100
    cfg = manager.build_config(parse(["self", "--kld-gain", "1e-3", "--kld-interval", "50"]))
    assert (cfg.engine.kld_gain, cfg.engine.kld_interval) == (1e-3, 50)
    assert manager.build_config(parse(["eval", "--smart-pruning"])).engine.smart_pruning is True
    # the options the rules compose with
    cfg = manager.build_config(parse(["self", "--kld-gain", "1e-3", "--record-visits", "--fast-sims", "8", "--forced-playouts", "2",
                                      "--record-q", "--record-surprise", "--leaf-mirror", "0.5"]))
    assert cfg.engine.kld_gain == 1e-3 and cfg.engine.fast_sims == 8
    for cmd in ("eval", "opt"):
        with pytest.raises(SystemExit, match="--kld-gain is an option of `run.py self`"):
            manager.build_config(parse([cmd, "--kld-gain", "1e-3"]))
    for cmd in ("self", "opt"):
        with pytest.raises(SystemExit, match="--smart-pruning is an option of `run.py eval`"):
            manager.build_config(parse([cmd, "--smart-pruning"]))
    for bad in ("-1", "nan", "inf"):
        with pytest.raises(SystemExit, match="--kld-gain"):
            manager.build_config(parse(["self", "--kld-gain", bad]))
    with pytest.raises(SystemExit, match="--kld-interval"):
        manager.build_config(parse(["self", "--kld-gain", "1e-3", "--kld-interval", "0"]))
    # the excluded combinations, in the solver's wording
    for extra, why in ((["--gumbel", "8", "--record-visits"], "--kld-gain excludes --gumbel: each defines its own root rule"),
                       (["--solver"], "--kld-gain excludes --solver: each defines its own root rule"),
                       (["--eval-cache", "10"], "--kld-gain excludes --eval-cache: the cache has a kernel instantiation of its own")):
        with pytest.raises(SystemExit, match=re.escape(why)):
            manager.build_config(parse(["self", "--kld-gain", "1e-3"] + extra))
    with pytest.raises(SystemExit, match=re.escape("--smart-pruning excludes --solver")):
        manager.build_config(parse(["eval", "--smart-pruning", "--solver"]))


def test_uci_option_and_defaults():
    from cchess_alphazero import uci
    from cchess_alphazero.config import Config
    cfg = Config(config_type="mini")
    assert cfg.engine.kld_gain == 0.0 and cfg.engine.kld_interval == 100 and cfg.engine.smart_pruning is False
    u = uci.UCI(cfg, out=io.StringIO())
    assert any(line == "option name SmartPruning type check default false" for line in uci.ENGINE_ID)
    assert any(line.startswith("option name Solver") for line in uci.ENGINE_ID)
    u.handle("setoption name SmartPruning value true")
    assert cfg.engine.smart_pruning is True
    u.handle("setoption name SmartPruning value false")
    assert cfg.engine.smart_pruning is False


def test_counter_names_and_the_entry_flag():
    from cchess_alphazero import _native_search as S
    names = S.COUNTER_NAMES
    i = names.index("decided_plies")
    assert names[i + 1:i + 5] == ["kld_plies", "kld_sims_cut", "lead_plies", "lead_sims_cut"]
    assert names[i + 5] == "cyc_select"                         # the tuning build's counters stay last
    # the names are the enum of csrc/xq_search.h, in its order
    with open(os.path.join(ROOT, "chinesechess-alphazero_amd", "csrc", "xq_search.h")) as f:
        enum = re.search(r"enum Counter : int \{(.*?)\n\};", f.read(), re.S).group(1)
    enum = re.sub(r"//[^\n]*", "", enum)
    ids = [x.strip() for x in re.sub(r"#\w+[^\n]*", "", enum).replace("= 0", "").split(",") if x.strip()]
    assert ids[-1] == "CT_COUNT" and [x[3:].lower() for x in ids[:-1]] == names
    assert S.VISIT_EARLY == 16
    with open(os.path.join(ROOT, "include", "czero.h")) as f:
        assert "#define CZ_VISIT_EARLY 16u" in f.read()
    # an entry's flag byte: bit 4 is `early`, the layout is what it was
    row = np.zeros(16 + 6 * 2, dtype=np.uint8)
    row[6], row[7] = 2, S.VISIT_EARLY | S.VISIT_FAST
    e = S.Search.parse_visit_entry(row.tobytes())
    assert e.early and e.fast and not e.pruned and not e.gumbel and len(e.n) == 2
    row[7] = 0
    assert not S.Search.parse_visit_entry(row.tobytes()).early


def test_a_stored_entry_has_no_side_column_or_all_of_them():
    """parse_visit_entry: the trimmed entry alone, or followed by one float64 per side column (q, s, maxq); nothing between."""
    from cchess_alphazero import _native_search as S
    ne = 3
    head = np.zeros(16, dtype=np.uint8)
    head[0:4] = np.array([7], dtype=np.uint32).view(np.uint8)            # game_id
    head[4:6] = np.array([5], dtype=np.uint16).view(np.uint8)            # ply
    head[6], head[7] = ne, 1 | S.VISIT_PRUNED | S.VISIT_NO_RESIGN
    head[8:12] = np.array([40], dtype=np.int32).view(np.uint8)           # sum_n
    head[12:16] = np.array([44], dtype=np.uint32).view(np.uint8)         # raw_total
    labels = np.array([11, 0x8000 | 12, 13], dtype=np.uint16)
    counts = np.array([30, 0, 9], dtype=np.int32)
    bare = head.tobytes() + labels.tobytes() + counts.tobytes()
    assert len(bare) == 16 + 6 * ne

    def fields(e):
        return (e.moves.tolist(), e.n.tolist(), e.banned.tolist(), e.sum_n, e.ply, e.resign, e.fast, e.pruned, e.raw_total,
                e.gumbel, e.early, e.no_resign)
    want = ([11, 12, 13], [30, 0, 9], [False, True, False], 40, 5, True, False, True, 44, False, False, True)
    e = S.Search.parse_visit_entry(bare)
    assert fields(e) == want and (e.q, e.s, e.maxq) == (None, None, None)
    nan = float("nan")
    for side, got in (((0.25, 1.5, -0.75), (0.25, 1.5, -0.75)), ((nan, nan, -100.0), (None, None, -100.0)),
                      ((-2.0, nan, nan), (-2.0, None, None)), ((nan, 0.0, nan), (None, 0.0, None)),
                      ((nan, nan, nan), (None, None, None))):
        row = bare + np.array(side, dtype=np.float64).tobytes()
        assert len(row) == 40 + 6 * ne
        e = S.Search.parse_visit_entry(row)
        assert fields(e) == want and (e.q, e.s, e.maxq) == got
    for extra in (8, 16, 4, 32):                                         # 24 + 6 ne and 32 + 6 ne were rows once
        with pytest.raises(ValueError):
            S.Search.parse_visit_entry(bare + bytes(extra))
    with pytest.raises(ValueError):
        S.Search.parse_visit_entry(bare[:-1])
