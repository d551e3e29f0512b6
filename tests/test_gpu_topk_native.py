"""The top-k kernel of csrc/query.hip (k_query_topk through launch_query_topk) round by round on
crafted arrays against plain host sorts (no engine, no corpus): bin/topk_test
(tests/native/topk_test.cpp, built by `make`, links query.o alone).  Its own driver follows the
contract of QTopkArgs in csrc/kernels.h up to four launches (N = 65537 and 70001 at k = 1024:
[17, 5, 2, 1] and [18, 5, 2, 1]), which no corpus of test size reaches through the library: later
rounds with several output slices, lists that straddle a slice boundary, short lists beside
all-ones entries, scores of +0.0, the smallest subnormal and DBL_MAX, ids above 2^31, and the
clause test of the first round at every boundary of the count word's fields.  After every launch
the whole output buffer, filled with all-ones before it, must be the host's image of that round;
every comparison is exact.  The program ends at its first HIP error or mismatch."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "parallel-systems-mpi-tfidf_amd", "bin", "topk_test")


# ok lines, one per case: rounds 9 values of N x 4 of k x 6 hit patterns; clauses 3 of N x 3 of k
@pytest.mark.parametrize("group,nok", [("rounds", 216), ("clauses", 9)])
def test_topk_rounds_against_host_sorts(group, nok):
    assert os.path.exists(EXE), "bin/topk_test not built; run __graft_entry__.build()"
    r = subprocess.run([EXE, group], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL OK" in r.stdout
    assert r.stdout.count("ok  ") == nok
    if group == "rounds":                                           # the fourth launch was really taken
        assert sum("k=1024" in l and l.endswith(": 4 launches") for l in r.stdout.splitlines()) == 12
