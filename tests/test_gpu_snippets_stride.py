"""Snippets on the stride corpus (tests/stride_corpus.py) with TFIDF_GRID_CUS = 1 and unset: the
jobs are every document under four queries, so with one CU the tile kernels (count and write) and
the per-job kernels (select, emit, fill) stride over their work three times and more (asserted from
SN_WG_PER_CU of kernels.h).  The results equal the reference's and those under the device's own CU
count."""
import pytest

import snippet_ref as R
import stride_corpus as SC
import tfidf_abi
from helpers import docs_to_arrays
from test_gpu_grid_stride import device_cus
from test_gpu_snippets import same

pytestmark = pytest.mark.gpu

SN_WG, SN_TILE, SN_SLICE = SC.kernels_h("SN_WG_PER_CU"), SC.kernels_h("SN_TILE"), SC.kernels_h("SN_SLICE")


@pytest.fixture(scope="module")
def want():
    docs = SC.build()["docs"]
    by_id = {i + 1: d for i, d in enumerate(docs)}
    queries = [b" ".join(SC.word(k) for k in ks) for ks in ((0, 1, 2, 3), (5, 6, 7), (100, 101, 4), (1, 50, 999999))]
    jobs = [(q, d) for d in by_id for q in range(len(queries))]
    rows, qterms = R.run(by_id, queries, jobs, window=8, max_marks=4)
    assert {len(SC.word(k)) for k in (5, 6, 7)} == {15, 16, 17} and sum(r["nmatch"] > 0 for r in rows) >= 3 * SN_WG
    return dict(arrays=docs_to_arrays(docs), docs=docs, queries=queries, jobs=jobs, rows=rows, qterms=qterms, got=[])


@pytest.mark.parametrize("cus", ["1", None])
def test_snippets_at_this_cu_count(want, cus, monkeypatch):
    if cus is None:
        monkeypatch.delenv("TFIDF_GRID_CUS", raising=False)
    else:
        monkeypatch.setenv("TFIDF_GRID_CUS", cus)
        wgs = int(cus) * SN_WG
        tiles = sum(-(-len(d) // SN_TILE) for d in want["docs"]) * 4          # a lower bound: bases are unaligned
        slices = sum(-(-r["nmatch"] // SN_SLICE) for r in want["rows"])
        assert tiles // wgs >= 3 and slices // wgs >= 3 and len(want["jobs"]) // wgs >= 3
    with tfidf_abi.Engine(0) as e:                                            # the environment is read at tfidf_open
        assert e.grid_cus() == (int(cus) if cus else device_cus())
        e.run_host(*want["arrays"])
        got = e.snippets(want["queries"], want["jobs"], window=8, max_marks=4)
        R.check(got, want["rows"], want["qterms"])
        assert e.snippet_info()["ntiles"] >= sum(-(-len(d) // SN_TILE) for d in want["docs"]) * 4
        for other in want["got"]:                                             # the same at every setting
            same(got, other)
        want["got"].append(got)
