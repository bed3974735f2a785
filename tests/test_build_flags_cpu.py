"""build.py's per-source compiler flags (no compile, no GPU): the four-wave chain unit csrc/xq_conv_ip4.hip, and no other source,
is compiled with the matrix instructions' accumulators in VALU-visible registers (-mllvm -amdgpu-mfma-vgpr-form); every other
source gets exactly FLAGS; every source of SOURCES exists.  The tools that compile the chain kernel on their own
(tools/ip4_isa_phases.py) take their flags from build.flags_for, so they report the kernel that runs."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "chinesechess-alphazero_amd"))

import build  # noqa: E402

CHAIN_UNIT = "xq_conv_ip4.hip"
OPTION = ["-mllvm", "-amdgpu-mfma-vgpr-form"]


def _has_option(flags):
    return any(flags[i:i + 2] == OPTION for i in range(len(flags) - 1))


def test_the_chain_unit_carries_the_option():
    assert CHAIN_UNIT in build.SOURCES
    flags = build.flags_for(CHAIN_UNIT)
    assert flags[:len(build.FLAGS)] == build.FLAGS and _has_option(flags)
    assert build.flags_for(os.path.join(build.CSRC, CHAIN_UNIT)) == flags         # (build() passes paths)


def test_no_other_source_carries_it():
    assert not _has_option(build.FLAGS)
    assert set(build.EXTRA_FLAGS) == {CHAIN_UNIT}
    for s in build.SOURCES:
        if s != CHAIN_UNIT:
            assert build.flags_for(s) == build.FLAGS, s
            assert build.flags_for(os.path.join(build.CSRC, s)) == build.FLAGS, s


def test_every_source_exists_once():
    assert len(set(build.SOURCES)) == len(build.SOURCES)
    for s in build.SOURCES:
        assert os.path.isfile(os.path.join(build.CSRC, s)), s
    assert set(build.EXTRA_FLAGS) <= set(build.SOURCES)
    assert build._sources() == [os.path.join(build.CSRC, s) for s in build.SOURCES]
