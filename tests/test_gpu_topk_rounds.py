"""The top-k driver past its second round: tfidf_query, tfidf_query_bm25, tfidf_query_clauses (both
rankings) and tfidf_similar on the 20000 documents of tests/topk_corpus.py, where the first round
has five slices and k = 1024 and k = 1000 take three launches ([5, 2, 1]: a later round with two
output slices, a third launch back into the first candidate buffer, at k = 1000 a list that
straddles the second round's slice boundary), against the plain Python references of the query,
BM25, clause and similar tests.  test_topk_corpus_cpu.py shows on the references alone that the
winners lie in every first-round and both second-round slices.  Everything is compared exactly: ids
and counts as integers, scores as u64 bit patterns.

Each call runs at k = 1024, 1000, 10 and 1024 again on one engine: the last call works in candidate
buffers that hold the lists of the calls between and must repeat the first bit for bit.  The
kernel's rounds beyond three, and its edges on crafted arrays: test_gpu_topk_native.py."""
import numpy as np
import pytest

import tfidf_abi
import topk_corpus as TC
from clause_ref import texts
from test_gpu_clause import same
from test_gpu_query import check
from test_gpu_similar import check as check_similar, same_result

pytestmark = pytest.mark.gpu

CALLS = ("query", "bm25", "clauses tfidf", "clauses bm25", "similar")


def call(e, name, k, rows):
    if name == "query":
        return e.query(TC.PLAIN, k)
    if name == "bm25":
        return e.query_bm25(TC.PLAIN, k)
    if name == "similar":
        return e.similar(k, rows)
    must, should, must_not, m = texts(TC.CLAUSES)
    return e.query_clauses(must, should, must_not, k, m, True if name == "clauses bm25" else None)


def info(e, name):
    return {"query": e.query_info, "bm25": e.bm25_info, "similar": e.similar_info}.get(name, e.clause_info)()


def batch(e, rows):
    """every call at every k of TC.KS, in that order: {call: [result per k]}"""
    return {name: [call(e, name, k, rows) for k in TC.KS] for name in CALLS}


@pytest.fixture(scope="module")
def tc(engine):
    """the corpus and the references once; the one run and the one batch the module's tests look at"""
    t = TC.references()
    engine.run_host(t["data"], t["off"])
    t["got"] = batch(engine, t["similar"])
    return t


def want_of(tc, name):
    return {"query": tc["plain"], "bm25": tc["bm25"], "clauses tfidf": tc["clauses"]["tfidf"],
            "clauses bm25": tc["clauses"]["bm25"]}[name]


@pytest.mark.parametrize("name", CALLS[:4])
def test_three_rounds_vs_reference(tc, name):
    assert [TC.rounds(TC.N, k) for k in TC.KS] == [[5, 2, 1], [5, 2, 1], [5, 1], [5, 2, 1]]
    refs, got = want_of(tc, name), tc["got"][name]
    for k, res in zip(TC.KS, got):
        check(res, refs, k)
        assert res["nmatch"].tolist() == [len(h) for h, _ in refs]          # summed over five slices
    same(got[0], got[3])                                                    # over the stale lists of k = 1000 and k = 10
    assert max(len(h) for h, _ in refs) == TC.N - 5 and int(got[0]["nhits"].max()) == 1024


def test_three_rounds_similar_vs_reference(tc):
    got = tc["got"]["similar"]
    for k, res in zip(TC.KS, got):
        check_similar(res, tc["rows"], k)
    same_result(got[0], got[3])
    assert got[0]["nmatch"].tolist() == [TC.N - 6] * 5 + [0, 0]             # every other document with a token


def test_ids_alone_order_the_word_of_every_document(tc):
    """b"all": more than 4096 documents tie for the best score, and the rows are their lowest ids in
    ascending order, which lie in every first-round slice"""
    for name in ("query", "bm25"):
        for k, res in zip(TC.KS, tc["got"][name]):
            row = res["doc"][TC.ALL_QUERY, :k].tolist()
            assert row == sorted(row) and len(set(res["score"][TC.ALL_QUERY, :k].tolist())) == 1
            assert int(res["nmatch"][TC.ALL_QUERY]) == TC.N - 5
        row = tc["got"][name][0]["doc"][TC.ALL_QUERY].tolist()
        assert {tc["pos"][d] // TC.QT_SLICE for d in row} == set(range(5))


def test_a_repeated_call_allocates_nothing(engine, tc):
    for name in CALLS:
        first = call(engine, name, 1024, tc["similar"])
        a0 = engine.alloc_counters()
        second = call(engine, name, 1024, tc["similar"])
        assert engine.alloc_counters() == a0, name                          # no device allocation at this N
        (same_result if name == "similar" else same)(first, second)
        (same_result if name == "similar" else same)(first, tc["got"][name][0])


def test_several_groups_through_the_same_buffers(tc, monkeypatch):
    """TFIDF_QUERY_ACC_MB=1 (read when the engine opens): a query of 20000 documents takes 240000
    bytes of accumulators and 2 * 61460 of candidates at k = 1024, so two queries fill a group and
    the batch goes through the three rounds group after group in the same two candidate buffers"""
    monkeypatch.setenv("TFIDF_QUERY_ACC_MB", "1")
    with tfidf_abi.Engine(0) as e:
        e.run_host(tc["data"], tc["off"])
        for name in CALLS:
            for k, want in zip(TC.KS, tc["got"][name]):
                got = call(e, name, k, tc["similar"])
                (same_result if name == "similar" else same)(got, want)
                i = info(e, name)
                assert i["ngroups"] > 1, (name, k)
                if k == 1024:
                    assert i["group_rows" if name == "similar" else "group_queries"] == 2, name
    assert np.array_equal(tc["got"]["query"][0]["doc"], tc["got"]["query"][3]["doc"])
