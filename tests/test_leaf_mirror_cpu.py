"""run.py self / eval --leaf-mirror P without a GPU: the command line, the configuration it reaches, and the library's
argument check (the search behind it: tests/test_gpu_leaf_mirror.py)."""
import ctypes as C
import types

import pytest

from cchess_alphazero import _native, _native_search  # noqa: F401  (declares the search entry points)
from cchess_alphazero.manager import build_config, create_parser


def _config(*argv):
    return build_config(create_parser().parse_args(list(argv)))


def test_the_default_is_off():
    assert create_parser().parse_args(["self"]).leaf_mirror == 0.0
    assert _config("self").engine.leaf_mirror == 0.0
    assert _config("eval").engine.leaf_mirror == 0.0


def test_the_rate_reaches_the_engine_config():
    assert _config("self", "--leaf-mirror", "0.5").engine.leaf_mirror == 0.5
    assert _config("self", "--leaf-mirror", "1").engine.leaf_mirror == 1.0


@pytest.mark.parametrize("bad", ["-1", "1.5", "nan"])
def test_a_rate_outside_0_1_is_refused(bad):
    with pytest.raises(SystemExit):
        _config("self", "--leaf-mirror", bad)


def test_the_flag_is_documented_for_self_and_eval():
    assert "(self, eval)" in [a for a in create_parser()._actions if a.dest == "leaf_mirror"][0].help


def test_the_rate_reaches_the_evaluator():
    from cchess_alphazero.worker.evaluator import EvaluateWorker
    stub = lambda planes: None
    cfg = _config("eval", "--leaf-mirror", "0.5")
    assert cfg.engine.leaf_mirror == 0.5
    assert EvaluateWorker(cfg, evaluators=(stub, stub)).leaf_mirror == 0.5
    assert EvaluateWorker(_config("eval"), evaluators=(stub, stub)).leaf_mirror == 0.0
    assert EvaluateWorker(types.SimpleNamespace(), evaluators=(stub, stub)).leaf_mirror == 0.0


def test_the_library_refuses_a_null_handle():
    L = _native.lib()
    _native_search.declare(L)
    assert L.cz_search_set_leaf_mirror(None, C.c_double(0.5), None, None) == -1      # CZ_ERR_ARG
    assert b"cz_search_set_leaf_mirror" in L.cz_last_error()
