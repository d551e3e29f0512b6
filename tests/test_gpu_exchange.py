"""The multi-rank half of csrc/finalize.hip against host references, launcher by launcher on
crafted inputs (not through a group of contexts): bin/exchange_test
(tests/native/exchange_test.cpp, built by `make`) runs the hash-owner DF exchange's kernels,
the dense exchange in both numberings, the cross-rank check of long terms and the in-process
transport's copy and sum kernels, each compared exactly with a plain loop, at up to 1024 ranks,
with empty segments, buckets past the 1024 records staged in LDS and sizes past every grid cap.
The chain group runs the whole owner exchange for R simulated ranks in one process.  One
process per group; the program ends at its first HIP error."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "parallel-systems-mpi-tfidf_amd", "bin", "exchange_test")


# ok lines, one per case, the same on every device:
# owner  partition 6 V x 7 R = 42; offsets 4 R; aggregate (6 sizes with empty senders + one key
#        copied 6 counts beside 300 keys + all records one key at 3 sizes + 5000 records of three
#        keys) x 3 forms = 48; back 7 R x 3 V = 21
# dense  keys by rank 3 V; table numbering 3 R + n past 8192 workgroups; merge numbering key
#        shapes + 5 R
# long   list 3 V; bytes 1 (7 lengths x 16 source residues); verify equal bytes 3 R + 5 differences
# xport  xcopy 6 segment shapes + 2 refused lists; xsum slice 3 source counts x 5 lengths;
#        sum rows 3 row counts x 4 lengths + 2 row counts at 1 100 000
# chain  4 R
@pytest.mark.parametrize("group,nok", [("owner", 115), ("dense", 13), ("long", 12), ("xport", 37), ("chain", 4)])
def test_exchange_stages_against_host_reference(group, nok):
    assert os.path.exists(EXE), "bin/exchange_test not built; run __graft_entry__.build()"
    r = subprocess.run([EXE, group], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL OK" in r.stdout
    assert r.stdout.count("ok  ") == nok
