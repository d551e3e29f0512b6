"""The stages of csrc/finalize.hip behind the tokenize-and-count kernel against host
references, directly on crafted records (not through a corpus): bin/finalize_test
(tests/native/finalize_test.cpp, built by `make`) runs the partial-record merge, the DF
histogram in its four forms (LDS narrow and wide, sliced, device atomics) and the
score-and-order stage with its five kernels, each compared exactly (scores as bit patterns)
with a plain loop, at the thresholds of kernels.h where the kernels switch path.  The score
cases also require the class totals, hand-offs and chunk tasks the host expects, so a case
that misses its path fails.  One process per group; the program ends at its first HIP error."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "parallel-systems-mpi-tfidf_amd", "bin", "finalize_test")


# ok lines, one per case, the same on every device (sizes may follow the CU count):
# merge  9 run lengths + the 2^32-1 sum + 5 documents among 1000 + 3 sizes of random runs
# df     narrow 5 V x 2 tables, wide 8 counts x 2 ranks + both halves, sliced 4 V, the last
#        sliced V and the atomic fallback
# score  classes 3 + 2, bucket fill 6 + consecutive ranks, rank width 1 + 4 + 3, wide ranks
#        2 V x 2 tables + 2^27+1, persistence 3
@pytest.mark.parametrize("group,nok", [("merge", 14), ("df", 33), ("score", 28), ("chain", 1)])
def test_finalize_stages_against_host_reference(group, nok):
    assert os.path.exists(EXE), "bin/finalize_test not built; run __graft_entry__.build()"
    r = subprocess.run([EXE, group], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL OK" in r.stdout
    assert r.stdout.count("ok  ") == nok
