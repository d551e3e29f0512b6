"""tfidf_query_clauses on the stride corpus (tests/stride_corpus.py) with TFIDF_GRID_CUS = 1, 2 and
unset, both rankings, against tests/clause_ref.py.  With one CU a wave of k_doc_score and a
workgroup of k_doc_score_big take several documents one after the other, so the clause
instantiations carry their count words (12 + 12 + 8 bits, filled by the postings' increments)
from one trip to the next.  The reference knows nothing of the grid: equality at every setting is
grid independence.  All comparisons are exact."""
import numpy as np
import pytest

import oracle_py
import stride_corpus as SC
import tfidf_abi
from clause_ref import ClauseRef, make_clause_queries, make_unsatisfiable_queries, texts
from helpers import docs_to_arrays
from test_gpu_query import check

pytestmark = pytest.mark.gpu

N = SC.NDOCS
KS = (1, 10, 1024)
RANKINGS = ("tfidf", "bm25")


def block_word(b, j=0):
    return SC.word(SC.NCOMMON + SC.BLOCK * (b % SC.NBIG) + j)


@pytest.fixture(scope="module")
def want():
    """the corpus, the queries and every reference answer, computed once for the three settings"""
    c = SC.build()
    data, off = docs_to_arrays(c["docs"])
    ora = oracle_py.run(data, off)
    ref = ClauseRef(ora, N, N)
    rng = np.random.default_rng(11)
    qs = make_clause_queries(ref, rng, 60) + make_unsatisfiable_queries(ref, rng, 12)
    planted = []
    for b in (3, 7, 12):
        common = SC.word(b)
        # a block's word: two big documents hold it
        planted.append(dict(must=block_word(b), should=common, must_not=b"", m=0))
        # the next block's word removes the one of the two that holds both blocks
        planted.append(dict(must=block_word(b, 5), should=common, must_not=block_word(b + 1, 1), m=1))
        # a common word as must, a block's word as must_not: every big document but two
        planted.append(dict(must=common, should=block_word(b + 2) + b" " + SC.word(b + 1), must_not=block_word(b, 9), m=0))
    big_ids = {c["order"][p] for p in c["big"]}
    hits = [{d for d, _ in ref.rank(q)[0]} for q in planted]
    for i in range(0, len(planted), 3):
        assert len(hits[i]) == 2 and hits[i] <= big_ids
        assert len(hits[i + 1]) == 1 and hits[i + 1] < hits[i]
        assert len(hits[i + 2] & big_ids) == SC.NBIG - 2 and len(hits[i + 2]) > SC.NBIG
    qs += planted
    trips = SC.trips(1, N, len(c["big"]), int(ora["npairs"]), 0, 0)
    assert trips["k_doc_score"] >= 3 and trips["k_doc_score_big"] >= 3      # at one CU
    return dict(data=data, off=off, qs=qs, refs={r: [ref.rank(q, r) for q in qs] for r in RANKINGS})


@pytest.mark.parametrize("cus", ["1", "2", None])
def test_clauses_at_this_cu_count(want, cus, monkeypatch):
    if cus is None:
        monkeypatch.delenv("TFIDF_GRID_CUS", raising=False)
    else:
        monkeypatch.setenv("TFIDF_GRID_CUS", cus)
    must, should, must_not, m = texts(want["qs"])
    with tfidf_abi.Engine(0) as e:                                  # the environment is read at tfidf_open
        if cus:
            assert e.grid_cus() == int(cus)
        e.run_host(want["data"], want["off"])
        for r in RANKINGS:
            for k in KS:
                res = e.query_clauses(must, should, must_not, k, m, True if r == "bm25" else None)
                check(res, want["refs"][r], k)
        assert e.clause_info()["ngroups"] == 2
