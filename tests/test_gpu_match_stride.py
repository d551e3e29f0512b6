"""Term matching on the stride corpus (tests/stride_corpus.py) with TFIDF_GRID_CUS = 1 and unset:
with one CU the scan's workgroups stride over the term table's tiles three times and more
(asserted from MT_WG_PER_CU of kernels.h), the prefix `w` matches every term, and with
list_records = 1024 it makes the list grow and the group fall into batches.  The fuzzy patterns
lie around the words padded to 15, 16 and 17 bytes, where the term's bytes come from the key or
from the corpus.  The rows equal the reference's and those under the device's own CU count."""
import pytest

import match_corpus as MC
import match_ref as R
import stride_corpus as SC
import tfidf_abi
from helpers import docs_to_arrays
from test_gpu_grid_stride import device_cus
from test_gpu_match import same_rows

pytestmark = pytest.mark.gpu

MT_NT, MT_WG = SC.kernels_h("MT_NT"), SC.kernels_h("MT_WG_PER_CU")


@pytest.fixture(scope="module")
def want():
    c = SC.build()
    terms, df, _ = MC.dictionary(c["docs"])
    padded = [t for t in terms if len(t) in (15, 16, 17)]
    assert {len(t) for t in padded} == {15, 16, 17}
    pats, kinds = [b"w", b"w0", b"w00005", b"x"], [1, 1, 1, 1]
    for t in padded[:12]:
        pats += [t, t[:-1], t[:7] + t[8:], t[:3] + b"9" + t[4:], t + b"x", t[:-2] + b"yx"]
    pats += [SC.word(100), SC.word(101)[:-1], b"w0010", b"v00100", b"0w0100"]
    pats = [p for p in pats if len(p) <= 64]
    kinds += [0] * (len(pats) - len(kinds))
    rows = R.expand(terms, df, pats, kinds, 2, 50, True, 0, R.Bags(terms))
    assert rows[0][0] == len(terms) > 1024 and rows[3][0] == 0
    return dict(arrays=docs_to_arrays(c["docs"]), V=len(terms), pats=pats, kinds=kinds, rows=rows, got={})


@pytest.mark.parametrize("cus", ["1", None])
def test_match_at_this_cu_count(want, cus, monkeypatch):
    if cus is None:
        monkeypatch.delenv("TFIDF_GRID_CUS", raising=False)
    else:
        monkeypatch.setenv("TFIDF_GRID_CUS", cus)
        tiles = -(-want["V"] // MT_NT)
        assert -(-tiles // min(tiles, int(cus) * MT_WG)) >= 3
    with tfidf_abi.Engine(0) as e:                                       # the environment is read at tfidf_open
        assert e.grid_cus() == (int(cus) if cus else device_cus())
        e.run_host(*want["arrays"])
        for records in (0, 1024):
            got = e.match_terms(want["pats"], kinds=want["kinds"], max_expansions=50, list_records=records)
            R.check(got, want["rows"], 50)
            info = e.match_info()
            if records:
                assert info["list_records"] == want["V"] and info["ngroups"] > 2
            else:
                assert info["ngroups"] == info["nbatches"] == -(-len(want["pats"]) // 64)
            for other in want["got"].values():                             # the same rows at every setting
                same_rows(got, other)
            want["got"][(cus, records)] = got
