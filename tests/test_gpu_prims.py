"""The device-wide primitives of csrc/prims.hip against host references, directly (not
through a corpus): bin/prims_test (tests/native/prims_test.cpp, built by `make`) compares
the exclusive scans with a host prefix sum, the radix and tile sorts with std::stable_sort
(values = input indices, so stability is checked by equality), and the varying-byte probes
with a host AND/OR, at the tile boundaries and at the limits where the launchers switch
form (1024 scan tiles, 1024 radix tiles = 2 097 152 keys, SORT_TILE_MAXN).  One process
per group; the program ends at its first HIP error."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(REPO, "parallel-systems-mpi-tfidf_amd", "bin", "prims_test")


# ok lines: one per (primitive, n) — scans 2 types x 11 sizes, radix 2 x 12, tile sorts
# 2 x (10 sizes + the refusal above SORT_TILE_MAXN), masks 2 types x 4 cases
@pytest.mark.parametrize("group,nok", [("scan", 22), ("radix", 24), ("tile", 22), ("mask", 8)])
def test_prims_against_host_reference(group, nok):
    assert os.path.exists(EXE), "bin/prims_test not built; run __graft_entry__.build()"
    r = subprocess.run([EXE, group], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL OK" in r.stdout
    assert r.stdout.count("ok  ") == nok
