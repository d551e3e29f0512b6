"""tfidf_query_clauses without a GPU: the reference of tests/clause_ref.py against an independent
formulation (Python sets per document, the OR ranking of test_gpu_query.Ref) on every golden;
tfidf_clauses_check rule by rule; argument errors; the exports and the structures' layout."""
import ctypes as C

import numpy as np
import pytest

import oracle_py
import tfidf_abi
from clause_ref import ClauseRef, make_clause_queries, make_unsatisfiable_queries, tokenize
from conftest import golden_cases
from helpers import load_golden
from test_gpu_query import Ref as OrRef

OK, E_INVAL = 0, tfidf_abi.E_INVAL


@pytest.mark.parametrize("case", golden_cases())
def test_reference_against_sets_per_document(case):
    g = load_golden(case)
    ora = oracle_py.run(g["data"], g["off"])
    ref = ClauseRef(ora, len(g["off"]) - 1)
    orref = OrRef(ora)
    doc_terms = {}
    for d, t in zip(ora["doc"].tolist(), ora["term"].tolist()):
        doc_terms.setdefault(d, set()).add(ora["terms"][t])
    rng = np.random.default_rng(5)
    qs = make_clause_queries(ref, rng, 150) + make_unsatisfiable_queries(ref, rng, 40)
    for q in qs:
        M, S, X = (set(tokenize(q[name])) for name in ("must", "should", "must_not"))
        want = {d for d, T in doc_terms.items() if M <= T and not (X & T) and len(S & T) >= q["m"] and ((M | S) & T)}
        hits, nfound = ref.rank(q)
        assert {d for d, _ in hits} == want, q
        assert nfound == len((M | S) & set(ora["terms"])), q
        # consequence 2: the OR ranking of must + " " + should, restricted; no score bit differs
        or_hits, or_found = orref.rank(q["must"] + b" " + q["should"])
        assert hits == [(d, s) for d, s in or_hits if d in want] and nfound == or_found, q
        assert {d for d, _ in ref.rank(q, "bm25")[0]} == want, q
        if q["kind"] is None:                   # by construction of the generator
            assert q["d0"] in want, q
            assert q["d1"] is None or (q["d1"] not in want and q["d1"] != q["d0"]), q
        else:
            assert not want, q
    # consequence 1 in the reference itself: a should text alone is the OR ranking
    for q in qs[:40]:
        plain = dict(must=b"", should=q["should"], must_not=b"", m=0)
        assert ref.rank(plain) == orref.rank(q["should"])


def words(n, prefix=b"w"):
    return b" ".join(prefix + b"%d" % i for i in range(n))


def test_clauses_check_limits():
    chk = tfidf_abi.clauses_check
    T, X = tfidf_abi.CLAUSE_MAX_TERMS, tfidf_abi.CLAUSE_MAX_NOT
    assert (T, X) == (4095, 255)
    assert chk(must=[b"", words(T)]) == OK and chk(must=[b"", words(T + 1)]) == E_INVAL
    assert chk(should=[words(T), b""]) == OK and chk(should=[words(T + 1), b""]) == E_INVAL
    assert chk(must_not=[words(X)]) == OK and chk(must_not=[words(X + 1)]) == E_INVAL
    # the limits count distinct terms, cut at their first NUL: repeats are free
    assert chk(must_not=[words(X) + b" " + words(X) + b" w0\0x w1\0y"]) == OK
    assert chk(must=[words(T)], should=[words(T, b"s")], must_not=[words(X, b"x")], min_should=[T]) == OK
    assert chk(should=[b"a"], min_should=[T]) == OK and chk(should=[b"a"], min_should=[T + 1]) == E_INVAL
    assert chk() == OK and chk(should=[]) == OK                   # no query at all
    assert chk(should=[b"a b"], bm25=True) == OK
    assert chk(should=[b"a b"], bm25=dict(k1=2.0, b=0.5)) == OK


def test_clauses_check_structure():
    L = tfidf_abi.lib()
    make = tfidf_abi.make_clauses

    def chk(c):
        return L.tfidf_clauses_check(C.byref(c))

    assert L.tfidf_clauses_check(None) == E_INVAL
    c, keep = make(must=[b"a", b"b"], should=[b"c"])              # an unequal nqueries
    assert chk(c) == E_INVAL
    c, keep = make(must=[b"a"], should=[b"c"], nqueries=2)
    assert chk(c) == E_INVAL
    c, keep = make(should=[b"a"])
    assert chk(c) == OK
    c.ranking = 2                                                 # an unknown ranking
    assert chk(c) == E_INVAL
    c, keep = make(should=[b"a"], bm25=dict(k1=1.0))
    assert chk(c) == OK
    c.ranking = tfidf_abi.RANK_TFIDF                              # bm25 set with TFIDF_RANK_TFIDF
    assert chk(c) == E_INVAL
    c, keep = make(should=[b"a"], bm25=dict(b=1.5))               # bad BM25 parameters
    assert chk(c) == E_INVAL
    c, keep = make(should=[b"a"])
    for size in (0, 8, C.sizeof(tfidf_abi.Clauses) - 1):          # a short size
        c.size = size
        assert chk(c) == E_INVAL
    c.size = C.sizeof(tfidf_abi.Clauses) + 8                      # a later, longer struct is accepted
    assert chk(c) == OK
    c, keep = make(should=[b"a b", b"c"])
    off = keep[1][1]
    off[1] = 5                                                    # a non-monotone q_off: 0, 5, 4
    assert chk(c) == E_INVAL
    off[1] = 3
    assert chk(c) == OK
    keep[0].nbytes = 3                                            # q_off[nqueries] > nbytes
    assert chk(c) == E_INVAL
    c, keep = make(nqueries=65536)                                # TFIDF_QUERY_MAX_QUERIES, every text empty
    assert chk(c) == OK
    c.nqueries = 65537
    assert chk(c) == E_INVAL


def test_clause_null_arguments_are_invalid():
    L = tfidf_abi.lib()
    c, keep = tfidf_abi.make_clauses(should=[b"a"])
    h = tfidf_abi.Hits()
    for fn in (L.tfidf_query_clauses, L.tfidf_group_query_clauses):
        assert fn(None, None, 3, None) == E_INVAL
        assert fn(None, C.byref(c), 3, C.byref(h)) == E_INVAL
        assert fn(None, None, 3, C.byref(h)) == E_INVAL
    ci = tfidf_abi.ClauseInfo()
    ci.size = C.sizeof(tfidf_abi.ClauseInfo)
    assert L.tfidf_last_clause_info(None, C.byref(ci)) == E_INVAL
    assert not h.doc and not h.score and h.nqueries == 0


def test_clause_names_are_exported_and_structures_mirror_the_header():
    L = tfidf_abi.lib()
    for name in ("tfidf_clauses_check", "tfidf_query_clauses", "tfidf_group_query_clauses", "tfidf_last_clause_info"):
        assert name in tfidf_abi.EXPORTS
        assert hasattr(L, name)
    assert L.tfidf_abi_version() == tfidf_abi.ABI_VERSION == 2      # the change is additive
    # include/tfidf.h, LP64: u64, two u32, five pointers; tfidf_bm25_info's 80 bytes and two u32
    assert C.sizeof(tfidf_abi.Clauses) == 56
    assert tfidf_abi.Clauses.ranking.offset == 12 and tfidf_abi.Clauses.must.offset == 16
    assert tfidf_abi.Clauses.min_should.offset == 40 and tfidf_abi.Clauses.bm25.offset == 48
    assert C.sizeof(tfidf_abi.ClauseInfo) == C.sizeof(tfidf_abi.Bm25Info) + 8 == 88
    assert tfidf_abi.ClauseInfo.avgdl.offset == 72
    assert tfidf_abi.ClauseInfo.nq_unsatisfiable.offset == 80 and tfidf_abi.ClauseInfo.ngroups_tab_lds.offset == 84
