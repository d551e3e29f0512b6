"""The scan, cut and word-gather kernels of csrc/match.hip against plain host loops, directly on
crafted term tables (no engine, no corpus): bin/match_test (tests/native/match_test.cpp, built by
`make`, links match.o and prims.o alone).  Both source forms of the table (a run's keys and
corpus, a model's offsets and blob); every pattern over {a, b, c} up to five bytes against every
such term, both flag settings and d = 0..2, the distances against a full host matrix; terms of
62..67 bytes against 63- and 64-byte patterns; tables of tile * grid * 3 + 1 terms and that +- 1
under the grid of one CU; a list capacity below the matches; the sort in both forms, the cut and
the words.  Every comparison is exact; the program ends at its first HIP error or mismatch.  One
process per group."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "parallel-systems-mpi-tfidf_amd", "bin", "match_test")


# ok lines, one per case: dist 2 forms x 2 flags x 3 budgets + 2 x 2 long; scan 3 sizes x 2 forms;
# select 2 forms x (1 capacity + 2 sorts x 3 cuts)
@pytest.mark.parametrize("group,nok", [("dist", 16), ("scan", 6), ("select", 14)])
def test_match_kernels_against_host_loops(group, nok):
    assert os.path.exists(EXE), "bin/match_test not built; run __graft_entry__.build()"
    r = subprocess.run([EXE, group], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL OK" in r.stdout
    assert r.stdout.count("ok  ") == nok
