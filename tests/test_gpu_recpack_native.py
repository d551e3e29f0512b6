"""The packed-record path of csrc/finalize.hip against host references, directly on crafted
records: bin/recpack_test (tests/native/recpack_test.cpp, built by `make`) runs the packed DF
pass (K1's count << sbits | slot words in, rank << cb | count out; narrow and wide form, both
rank maps), the packed score kernels (documents of 1 .. 4096 pairs at every size where a kernel
or a branch changes, rank widths 1 .. 22 bits, counts 1 and the field's maximum, skewed documents
for both radix paths, presorted two-word documents mixed in, rec_cnt poisoned under the packed
records) and k_rec_unpack, each compared exactly (scores as bit patterns) with a host loop.  One
process per group; the program ends at its first HIP error."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "parallel-systems-mpi-tfidf_amd", "bin", "recpack_test")


# ok lines: chain 7 cases x (2 DF maps + score) + the one-workgroup (wide) DF and score;
# score 3 rank widths; guard 1; unpack 8 sizes
@pytest.mark.parametrize("group,nok", [("chain", 23), ("score", 3), ("guard", 1), ("unpack", 8)])
def test_recpack_stages_against_host_reference(group, nok):
    assert os.path.exists(EXE), "bin/recpack_test not built; run __graft_entry__.build()"
    r = subprocess.run([EXE, group], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL OK" in r.stdout
    assert r.stdout.count("ok  ") == nok
