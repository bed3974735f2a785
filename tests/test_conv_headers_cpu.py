"""The network units' internal headers (csrc/xq_conv_*.h, csrc/xq_nn_*.h, csrc/xq_c8_kloop.h) stand alone: each includes what it
uses, so that the device-only syntax check of the header by itself succeeds.  The xq_conv_*.h kernel headers are the parts of ONE
translation unit, csrc/xq_conv.hip, which includes them in order (each header's first comment says so); this test keeps a header
from leaning on whatever xq_conv.hip happened to include before it.  The filters' host-side packing, csrc/xq_conv_pack.hip, is a
unit of its own that holds no kernel.  Needs hipcc, no GPU."""
import glob
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "chinesechess-alphazero_amd", "csrc")
HEADERS = sorted(glob.glob(os.path.join(CSRC, "xq_conv_*.h")) + glob.glob(os.path.join(CSRC, "xq_nn_*.h")) +
                 [os.path.join(CSRC, "xq_c8_kloop.h")])

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not on PATH")


def test_every_included_header_is_found():
    """the glob sees at least the headers xq_conv.hip includes (so the check below cannot pass on an empty list)"""
    with open(os.path.join(CSRC, "xq_conv.hip")) as f:
        included = set(re.findall(r'^#include "(xq_conv_\w+\.h)"', f.read(), re.M))
    assert len(included) >= 8, included
    assert included <= {os.path.basename(h) for h in HEADERS}
    assert os.path.exists(os.path.join(CSRC, "xq_c8_kloop.h"))


def test_pack_unit_has_no_kernel():
    """csrc/xq_conv_pack.hip is host code: it defines no kernel and launches none"""
    with open(os.path.join(CSRC, "xq_conv_pack.hip")) as f:
        text = f.read()
    assert "__global__" not in text
    assert "hipLaunchKernelGGL" not in text and "<<<" not in text


@pytest.mark.parametrize("header", HEADERS, ids=[os.path.basename(h) for h in HEADERS])
def test_header_compiles_alone(header):
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only", "-x", "hip",
                        os.path.basename(header)], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
