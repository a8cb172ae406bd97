"""Every kernel table of the LDS family sets its own dynamic-LDS attribute, whichever table a process launches first.

k_batch_elim (rank_batch) and k_batch_det (det_batch) take the same argument type, BatchArgs; the record of the classes whose
hipFuncAttributeMaxDynamicSharedMemorySize is set belongs to the kernel table (ElimKernels::attr_done in csrc/engine.hip), not to
the argument type.  A record shared between the two tables would leave whichever ran second in a process without the attribute,
and only the last class needs it: its 147 KiB of LDS cannot be launched otherwise.  One dense 112 x 112 matrix mod 65521 is the
smallest even size of that class (padded image 112 * 113 = 12656 words > 12288).

The record lives as long as the process, so each order runs in a fresh child process (a new interpreter, started and waited for;
no process replaces its program).  A child checks every step against the host references of the det and charpoly tests and
raises at the first that is wrong, which ends it with a non-zero status before anything further is started."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_charpoly import host_charpoly
from test_gpu_det import host_det

pytestmark = pytest.mark.gpu

N, P, SEED = 112, 65521, 0x1D5A
TESTS = os.path.dirname(os.path.abspath(__file__))

CHILD = r"""
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import numpy as np
import spasm_jl_amd as S
from test_gpu_det import csr_of
want = json.loads(sys.argv[3])
A = csr_of(S, np.random.default_rng(want["seed"]).integers(0, want["p"], size=(want["n"], want["n"]), dtype=np.int64), want["p"])
def det():
    assert S.det_batch([A]).tolist() == [want["det"]]
    st = S.det_stats()
    assert st["lds_path"] == 1 and st["launches"] == 1, st
def rank():
    assert S.rank_batch([A]) == [want["n"]]
    st = S.batch_stats()
    assert st["lds_path"] == 1 and st["launches"] == 1 and st["max_image_words"] == want["n"] * (want["n"] + 1), st
def charpoly():
    got = S.charpoly_batch([A])
    assert len(got) == 1 and got[0].tolist() == want["coef"]
    st = S.charpoly_stats()
    assert st["lds_path"] == 1 and st["launches"] == 1, st
for step in sys.argv[4].split(","):
    {"det": det, "rank": rank, "charpoly": charpoly}[step]()
print("ok", sys.argv[4])
"""


@pytest.fixture(scope="module")
def want():
    D = np.random.default_rng(SEED).integers(0, P, size=(N, N), dtype=np.int64)
    det = host_det(D, P)
    assert det != 0   # so the rank is N
    coef = [v - P if v > P // 2 else v for v in host_charpoly(D, P)]
    assert coef[N] == 1 and coef[0] == det   # N is even: chi(0) = det(-A) = det(A)
    return {"seed": SEED, "n": N, "p": P, "det": det, "coef": coef}


def test_each_kernel_table_sets_its_own_lds_attribute_in_either_order(want):
    for order in ("det,rank,charpoly", "rank,det,charpoly"):
        r = subprocess.run([sys.executable, "-c", CHILD, os.path.dirname(TESTS), TESTS, json.dumps(want), order], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (order, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        assert r.stdout.split("\n")[-2] == "ok " + order
