"""The search's internal headers (csrc/xq_search_*.h) stand alone: each includes what it uses, so that the device-only
syntax check of the header by itself succeeds.  They are the parts of ONE translation unit, csrc/xq_search.hip, which
includes them in order (each header's first comment says why they are not units of their own); this test keeps a header
from leaning on whatever xq_search.hip happened to include before it.  Needs hipcc, no GPU."""
import glob
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "chinesechess-alphazero_amd", "csrc")
HEADERS = sorted(glob.glob(os.path.join(CSRC, "xq_search_*.h")))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not on PATH")


def test_every_included_header_is_found():
    """the glob sees at least the headers xq_search.hip includes (so the check below cannot pass on an empty list)"""
    with open(os.path.join(CSRC, "xq_search.hip")) as f:
        included = set(re.findall(r'^#include "(xq_search_\w+\.h)"', f.read(), re.M))
    assert len(included) >= 2, included
    assert included <= {os.path.basename(h) for h in HEADERS}


@pytest.mark.parametrize("header", HEADERS, ids=[os.path.basename(h) for h in HEADERS])
def test_header_compiles_alone(header):
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only", "-x", "hip",
                        os.path.basename(header)], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
