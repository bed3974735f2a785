"""CPU checks of the cross-game evaluation cache (cz_search_set_eval_cache; run.py self --eval-cache LOG2): the command
line's refusals and its way into config.engine.eval_cache, the engine's argument check where no device is needed, and
the table's layout and slot function (csrc/xq_evalcache.h compiled with g++: the text the search kernels compile).  What
the cache does to a search -- nothing -- is tests/test_gpu_eval_cache.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE_BOUND = 640                      # the issue's bound on an entry's stride


def _config(*argv):
    from cchess_alphazero import manager
    return manager.build_config(manager.create_parser().parse_args(list(argv)))


# ---- 1. the command line ------------------------------------------------------------------------------------------------------
def test_the_flag_reaches_the_engine_section_and_is_off_by_default():
    assert _config("self").engine.eval_cache == 0
    assert _config("eval").engine.eval_cache == 0
    assert _config("self", "--eval-cache", "0").engine.eval_cache == 0
    for v in (10, 16, 22, 24):
        assert _config("self", "--eval-cache", str(v)).engine.eval_cache == v
    from cchess_alphazero.config import Config
    assert Config("normal").engine.eval_cache == 0


@pytest.mark.parametrize("value", ["9", "25", "-1", "1", "64"])
def test_sizes_outside_0_or_10_to_24_are_refused(value):
    with pytest.raises(SystemExit, match="--eval-cache"):
        _config("self", "--eval-cache", value)


@pytest.mark.parametrize("cmd", ["eval", "opt", "play", "sl", "ob"])
def test_every_other_sub_command_is_refused(cmd):
    with pytest.raises(SystemExit, match="run.py self"):
        _config(cmd, "--eval-cache", "16")
    assert _config(cmd).engine.eval_cache == 0


def test_a_28_plane_configuration_is_refused(monkeypatch):
    from cchess_alphazero import manager
    from cchess_alphazero.config import Config

    def with_history(config_type="mini"):
        c = Config(config_type=config_type)
        c.model.input_depth = 28
        return c
    monkeypatch.setattr(manager, "Config", with_history)
    with pytest.raises(SystemExit, match="14-plane"):
        _config("self", "--eval-cache", "16")
    assert _config("self").engine.eval_cache == 0          # (the flag off: nothing to refuse)


# ---- 2. the engine's argument check, before it asks for a device -----------------------------------------------------------------
def test_the_engine_refuses_history_and_bad_sizes_without_a_device():
    from cchess_alphazero.config import Config
    from cchess_alphazero.engine import SelfPlayEngine
    cfg = Config("mini")
    with pytest.raises(ValueError, match="use_history"):
        SelfPlayEngine(cfg, 4, use_history=True, eval_cache=16)
    for bad in (9, 25, -3):
        with pytest.raises(ValueError, match="eval_cache"):
            SelfPlayEngine(cfg, 4, eval_cache=bad)
    cfg.engine.eval_cache = 16                              # (the configuration's value is checked the same way)
    with pytest.raises(ValueError, match="use_history"):
        SelfPlayEngine(cfg, 4, use_history=True)


# ---- 3. layout and slot function --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = tmp_path_factory.mktemp("evalcache") / "libevalcache.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "evalcache_harness.cpp"), "-o", str(out)])
    L = C.CDLL(str(out))
    L.ec_layout.argtypes = [C.c_void_p]
    L.ec_bytes.argtypes = [C.c_int]
    L.ec_bytes.restype = C.c_uint64
    L.ec_slots.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.ec_meta_word.argtypes = [C.c_int, C.c_int]
    L.ec_meta_word.restype = C.c_uint32
    return L


def test_the_entry_holds_what_the_issue_lists_within_the_stride_bound(harness):
    from cchess_alphazero import _native_search as S
    lay = np.zeros(8, dtype=np.int32)
    harness.ec_layout(lay.ctypes.data_as(C.c_void_p))
    stride, key, claim, meta, value, p, lo, hi = lay.tolist()
    assert stride == S.EVAL_CACHE_STRIDE == 576 and stride <= STRIDE_BOUND and stride % 64 == 0
    assert (lo, hi) == S.EVAL_CACHE_LOG2 == (10, 24)
    # the 48-byte position, three words and a pad, 128 float32 priors: nothing overlaps, nothing is left over
    assert key == 0 and claim == 48 and meta == 52 and value == 56 and p == 64 and p + 4 * 128 == stride
    with open(os.path.join(ROOT, "include", "czero.h")) as f:
        assert f"#define CZ_EVAL_CACHE_STRIDE {stride}\n" in f.read()


def test_entries_times_stride_stays_within_the_documented_bound(harness):
    for log2 in range(10, 25):
        b = harness.ec_bytes(log2)
        assert b == 576 << log2 <= STRIDE_BOUND << log2
    assert harness.ec_bytes(24) <= 10 << 30                 # the largest table: under 10 GiB of a 288 GB device
    assert harness.ec_bytes(22) == 2415919104               # the size the measurements use: 2.25 GiB


def _slots(harness, hashes, mirrored, log2):
    out = np.zeros(len(hashes), dtype=np.uint32)
    harness.ec_slots(hashes.ctypes.data_as(C.c_void_p), len(hashes), int(mirrored), log2, out.ctypes.data_as(C.c_void_p))
    return out


@pytest.mark.parametrize("log2", [10, 16, 24])
def test_the_slot_function_stays_inside_the_table_and_separates_the_mirror_twin(harness, log2):
    rng = np.random.default_rng(20261019)
    n = 1 << 16
    h = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    a, b = _slots(harness, h, False, log2), _slots(harness, h, True, log2)
    assert a.max() < (1 << log2) and b.max() < (1 << log2)
    assert (_slots(harness, h, False, log2) == a).all()     # a function of its arguments
    # a key and its mirror-bit twin share a slot no more often than two unrelated keys do: rate 2^-log2, and the count is
    # Poisson -- mean + 6 sigma + 1 bounds it
    mean = n / (1 << log2)
    assert (a == b).sum() <= mean + 6.0 * np.sqrt(mean) + 1.0
    assert (a != b).any()
    # and the slots are spread: every one of the first 1024 slot classes is used by these 65536 keys
    assert len(np.unique(a >> max(log2 - 10, 0))) == 1024


def test_the_mirror_bit_and_the_move_count_are_part_of_the_match_word(harness):
    words = {harness.ec_meta_word(nm, mir) for nm in range(129) for mir in (0, 1)}
    assert len(words) == 2 * 129 and 0 not in words         # (a cleared entry, all zero, matches nothing)
