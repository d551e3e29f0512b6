"""BM25 ranking (tfidf_query_bm25 / tfidf_group_query_bm25 / `tfidf --query F --bm25`) against
a plain Python ranking of the oracle's pairs.

Reference (include/tfidf.h): a query is tokenised like a document; w = tokens per term;
idf = math.log(1 + (N - df + 0.5) / (df + 0.5)); W = w * idf; avgdl = L / n (or the caller's);
K(d) = k1 * ((1 - b) + b * (docSize / avgdl)); sat = (c * (k1 + 1)) / (c + K(d));
score(q, d) = the sum over d's pairs, in pair order, of fl(W * sat): one Python float
operation per rounding of the definition, never fused.  Hits = documents with at least one
query term, ordered by (score descending, document id ascending).  doc rows, nhits, nmatch
and nterms_found are compared exactly, scores as u64 bits."""
import ctypes as C
import math
import os
import shutil
import subprocess
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest

import oracle_py
import tfidf_abi
import tfidf_configs
from conftest import golden_cases, GOLDEN
from helpers import docs_to_arrays, load_golden
from test_gpu_query import Ref, bits, check, make_queries, tokenize

pytestmark = pytest.mark.gpu

KS = [1, 3, 10, 1024]
DEFAULT = (1.2, 0.75)
PARAMS = [DEFAULT, (0.0, 0.75), (2.0, 0.0), (0.9, 1.0)]
K_FUSION = (1.5, 0.4)    # b with a full significand: b * x needs its own rounding to match


class Bm25Ref:
    """the oracle's pairs, indexed by term; ranks a query with a plain loop"""

    def __init__(self, ora, ndocs, n_total=0):
        self.tid = {t: i for i, t in enumerate(ora["terms"])}
        term = ora["term"]
        self.by_term = np.argsort(term, kind="stable")
        self.first = np.searchsorted(term[self.by_term], np.arange(len(ora["terms"]) + 1))
        self.doc = ora["doc"].tolist()
        self.count = ora["count"].tolist()
        self.docsize = ora["docsize"].tolist()
        self.N = int(n_total) if n_total else ndocs
        self.df = [0] * len(ora["terms"])
        for t, d in zip(term.tolist(), ora["df"].tolist()):
            self.df[t] = d
        self.L = sum(self.count)            # every token of a document is in one of its pairs
        self.n = ndocs
        self.avgdl = self.L / self.n if self.L else 0.0

    def idf(self, t: int) -> float:
        num = float(self.N - self.df[t]) + 0.5
        den = float(self.df[t]) + 0.5
        ratio = num / den
        return math.log(1.0 + ratio)

    def matches(self, q: bytes):
        """(pair position, doc, W, count, docSize) of every pair of a query term, in pair order"""
        w = Counter(tokenize(q))
        found = [t for t in w if t in self.tid]
        m = []
        for t in found:
            i = self.tid[t]
            W = float(w[t]) * self.idf(i)
            for p in self.by_term[self.first[i]:self.first[i + 1]].tolist():
                m.append((p, self.doc[p], W, self.count[p], self.docsize[p]))
        m.sort()
        return m, len(found)

    def scores(self, q: bytes, k1=1.2, b=0.75, avgdl=0.0, fuse=None):
        """doc -> score.  fuse="acc": W * sat + acc in one rounding; fuse="K": b * x + (1 - b) in
        one rounding (what a contracted kernel would compute)"""
        m, nfound = self.matches(q)
        avg = avgdl if avgdl else self.avgdl
        k1p1 = k1 + 1.0
        omb = 1.0 - b
        acc = {}
        for _, d, W, c, dsz in m:
            x = float(dsz) / avg
            if fuse == "K":
                nrm = float(Fraction(b) * Fraction(x) + Fraction(omb))
            else:
                bl = b * x
                nrm = omb + bl
            K = k1 * nrm
            num = float(c) * k1p1
            den = float(c) + K
            sat = num / den
            if fuse == "acc":
                acc[d] = float(Fraction(W) * Fraction(sat) + Fraction(acc.get(d, 0.0)))
            else:
                prod = W * sat
                acc[d] = acc.get(d, 0.0) + prod
        return acc, nfound

    def rank(self, q: bytes, k1=1.2, b=0.75, avgdl=0.0):
        acc, nfound = self.scores(q, k1, b, avgdl)
        return sorted(acc.items(), key=lambda x: (-x[1], x[0])), nfound

    def fused_differs(self, q: bytes, fuse: str, k1=1.2, b=0.75, k: int = 1024) -> bool:
        """would that contraction change the bits of a score returned for this query?"""
        plain, _ = self.scores(q, k1, b)
        fused, _ = self.scores(q, k1, b, fuse=fuse)
        top = sorted(plain.items(), key=lambda x: (-x[1], x[0]))[:k]
        return any(fused[d] != s for d, s in top)


@pytest.fixture(scope="module")
def c2():
    p = tfidf_configs.plan("c2", scale=0.002)
    data, off = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
    ora = oracle_py.run(data, off, p["doc_ids"], p["ndocs_total"])
    ref = Bm25Ref(ora, len(off) - 1, p["ndocs_total"])
    qs = make_queries(ora, np.random.default_rng(11), 200)
    return dict(p=p, data=data, off=off, ora=ora, ref=ref, qs=qs, refs=[ref.rank(q) for q in qs],
                args=(data, off, p["doc_ids"], p["ndocs_total"]))


def test_c2_bm25_vs_reference(engine, c2):
    ref, qs = c2["ref"], c2["qs"]
    # for this seed a contracted kernel cannot pass: fma(W, sat, acc) changes the bits of a
    # returned score at the default parameters, and fma(b, x, 1 - b) in K(d) at b = 0.4.  (The
    # parameter sets above cannot show the second contraction: b = 0 and b = 1 make the product
    # or the sum exact, and 0.75 * x carries only two bits more than a double, so rounding it
    # before the sum with 0.25 gives what rounding once gives for all but a sliver of document
    # lengths; no query of this corpus has a score that differs.  Hence the fifth set.)
    assert any(ref.fused_differs(q, "acc") for q in qs[:60])
    assert any(ref.fused_differs(q, "K", *K_FUSION) for q in qs[:60])
    engine.run_host(*c2["args"])
    for k1, b in PARAMS + [K_FUSION]:
        refs = c2["refs"] if (k1, b) == DEFAULT else [ref.rank(q, k1, b) for q in qs]
        for k in KS:
            res = engine.query_bm25(qs, k, k1, b)
            check(res, refs, k)
            assert bits(res["avgdl"]) == bits(ref.avgdl)
    assert any(len(h) > 10 for h, _ in c2["refs"]) and any(0 < len(h) < 1024 for h, _ in c2["refs"])
    assert all(s > 0.0 and math.isfinite(s) for h, _ in c2["refs"] for _, s in h)


@pytest.mark.parametrize("case", golden_cases())
def test_golden_bm25_vs_reference(engine, case):
    g = load_golden(case)
    ora = oracle_py.run(g["data"], g["off"])
    ref = Bm25Ref(ora, len(g["off"]) - 1)
    qs = make_queries(ora, np.random.default_rng(5), 200)
    engine.run_host(g["data"], g["off"])
    for (k1, b), ks in ((DEFAULT, KS), ((0.9, 1.0), [10])):
        refs = [ref.rank(q, k1, b) for q in qs]
        for k in ks:
            check(engine.query_bm25(qs, k, k1, b), refs, k)


def test_bm25_ties_ordered_by_numeric_id(engine):
    """byte-identical documents have the same length and counts: they tie on every score, the
    cut at k falls inside the tie, and doc9 comes before doc10 (not the strcmp order of the
    lines)"""
    docs = [b"same words in every copy copy"] * 120 + [b"other words here", b"same here once", b"nothing shared"]
    data, off = docs_to_arrays(docs)
    engine.run_host(data, off)
    ref = Bm25Ref(oracle_py.run(data, off), len(docs))
    qs = [b"copy", b"copy same", b"every words", b"here copy"]
    refs = [ref.rank(q) for q in qs]
    assert refs[0][0][8][1] == refs[0][0][9][1] and [d for d, _ in refs[0][0][8:10]] == [9, 10]
    for k in (7, 15):
        res = engine.query_bm25(qs, k)
        check(res, refs, k)
        assert res["doc"][0].tolist() == list(range(1, k + 1))
    assert bits(res["score"][0, 8]) == bits(res["score"][0, 9]) and res["doc"][0, 8:10].tolist() == [9, 10]
    assert int(res["nmatch"][0]) == 120


def test_bm25_word_of_every_document_counts(engine):
    """a word with df = N has idf log(1 + 0.5 / (N + 0.5)) > 0: every document is a hit with a
    positive score, where tfidf_query gives 0.0"""
    docs = [b"the w%d x%d" % (i, i % 5) for i in range(40)] + [b"the rare w3", b"the rare", b"unrelated text"]
    docs = [d + b" all" * (1 + i % 3) for i, d in enumerate(docs)]
    data, off = docs_to_arrays(docs)
    engine.run_host(data, off)
    ref = Bm25Ref(oracle_py.run(data, off), len(docs))
    N = len(docs)
    assert ref.df[ref.tid[b"all"]] == N
    qs = [b"all", b"all rare", b"rare the", b"all all all x1"]
    refs = [ref.rank(q) for q in qs]
    for k in (5, 1024):
        res = engine.query_bm25(qs, k)
        check(res, refs, k)
    assert int(res["nmatch"][0]) == N and int(res["nhits"][0]) == N
    assert np.all(res["score"][0, :N] > 0.0)
    plain = engine.query(qs[:1], 1024)
    assert int(plain["nmatch"][0]) == N and np.all(bits(plain["score"][0, :N]) == 0)


def test_bm25_long_documents(engine):
    """one document of 6000 distinct words (over QS_BIG pairs: a workgroup, matches in every
    256-pair tile), one over BIG_DOC bytes, one of 3000 words (many rounds of its owner wave),
    among 50 small documents; then a query batch whose table no longer fits the LDS stage"""
    rng = np.random.default_rng(3)
    word = lambda i: b"w%05d" % i
    docs = [b" ".join(word(int(j)) for j in rng.integers(0, 6000, 30)) for _ in range(50)]
    docs.insert(7, b" ".join(word(i) for i in rng.permutation(6000)))
    big = b" ".join(word(int(j)) for j in rng.integers(0, 5000, 12000))
    assert len(big) > 49152
    docs.insert(20, big)
    docs.insert(33, b" ".join(word(i) for i in range(1000, 4000)))
    data, off = docs_to_arrays(docs)
    engine.run_host(data, off)
    ora = oracle_py.run(data, off)
    ref = Bm25Ref(ora, len(docs))
    spread = [word(i) for i in range(0, 6000, 20)]                 # 300 words over the whole term range
    q = b" ".join(w for i, w in enumerate(spread) for _ in range(1 + i % 7))
    qs = [q, b" ".join(spread[::3]), word(5999) + b" " + word(0), b" ".join(word(i) for i in range(4090, 4110))]
    refs = [ref.rank(x) for x in qs]
    # document 8 is the 6000-pair one: the first query matches it in more than one tile of 256 pairs
    pos8 = [p for p, d, *_ in ref.matches(q)[0] if d == 8]
    first8 = ora["doc"].tolist().index(8)
    assert len(pos8) == 300 and len({(p - first8) // 256 for p in pos8}) > 10
    assert refs[0][1] == 300 and ref.fused_differs(q, "acc")
    for k in (3, 1024):
        check(engine.query_bm25(qs, k), refs, k)
    check(engine.query_bm25(qs, 60, 2.0, 0.3), [ref.rank(x, 2.0, 0.3) for x in qs], 60)
    # 1500 distinct query words: 2 * 1500 + 1 + 3 * 1800 words of table do not fit 4096
    wide = [b" ".join(word(i) for i in range(0, 6000, 4)), q]
    check(engine.query_bm25(wide, 60), [ref.rank(x) for x in wide], 60)


def test_bm25_vocabulary_wider_than_the_lds_filter(engine):
    """300000 terms: the LDS filter (2^18 bits over the ranks' low bits) is hashed.  Ranks 7 and
    7 + 2^18 share a bit: a pair of the other word passes the filter and the exact search must
    reject it, in a long document (workgroup path) and a short one"""
    V = 300000
    docs = [b" ".join(b"w%06d" % i for i in range(d, V, 30)) for d in range(30)]
    docs.append(b"w000007 w262151 w262152")
    data, off = docs_to_arrays(docs)
    engine.run_host(data, off)
    ora = oracle_py.run(data, off)
    by_name = sorted(ora["terms"])
    assert by_name[7] == b"w000007" and by_name[7 + (1 << 18)] == b"w262151"
    ref = Bm25Ref(ora, len(docs))
    qs = [b"w000007", b"w262151", b"w000007 w262151 w262151", b"w262152 w000008 w299999", b"w300000"]
    refs = [ref.rank(q) for q in qs]
    assert sorted(d for d, _ in refs[0][0]) == [8, 31] and sorted(d for d, _ in refs[1][0]) == [12, 31]
    check(engine.query_bm25(qs, 8), refs, 8)


def test_bm25_long_terms(engine):
    """terms of >= 16 bytes are matched by their bytes: a present one matches, one that differs
    from a vocabulary term only past byte 16 does not"""
    a = b"abcdefghijklmnop" + b"q" * 24          # 40 bytes
    b_ = b"abcdefghijklmnop" + b"r" * 24         # same first 16 bytes, present
    absent = b"abcdefghijklmnop" + b"q" * 23 + b"s"   # differs from `a` in its last byte only
    s16 = b"abcdefghijklmnop"                    # exactly 16 bytes: the shortest long term
    docs = [a + b" x", b_ + b" y " + a, b"x y z", s16 + b" " + a]
    data, off = docs_to_arrays(docs)
    engine.run_host(data, off)
    ref = Bm25Ref(oracle_py.run(data, off), len(docs))
    qs = [a, absent, b_ + b" " + absent, s16, s16[:15], a + b"\0" + absent, a * 2]
    refs = [ref.rank(q) for q in qs]
    assert refs[0][1] == 1 and refs[1] == ([], 0) and refs[4] == ([], 0) and refs[6] == ([], 0)
    res = engine.query_bm25(qs, 10)
    check(res, refs, 10)
    assert res["nmatch"].tolist()[:2] == [3, 0]


def test_bm25_groups_under_a_small_budget(engine, c2, monkeypatch):
    """TFIDF_QUERY_ACC_MB=1: the batch is cut into several groups (one pass over the pairs
    each); the bits are those of the default budget, where 64 queries are one group"""
    engine.run_host(*c2["args"])
    cases = [(c2["qs"][:64], 10), (c2["qs"][:64], 1024), (c2["qs"][:150], 10), (c2["qs"][:150], 1024)]
    want, default_groups = [], []
    for q, k in cases:
        want.append(engine.query_bm25(q, k))
        default_groups.append(engine.bm25_info()["ngroups"])
    assert default_groups == [1, 1, 3, 3]                         # 150 queries: 64 + 64 + 22
    monkeypatch.setenv("TFIDF_QUERY_ACC_MB", "1")
    with tfidf_abi.Engine(0) as e:
        e.run_host(*c2["args"])
        for (q, k), w, dg in zip(cases, want, default_groups):
            got = e.query_bm25(q, k)
            check(got, c2["refs"][:len(q)], k)
            for name in ("nhits", "nmatch", "nterms_found", "doc"):
                assert np.array_equal(got[name], w[name])
            assert np.array_equal(bits(got["score"]), bits(w["score"]))
            # the candidate lists of k = 1024 no longer fit 64 queries into 1 MiB
            assert e.bm25_info()["ngroups"] > dg if k == 1024 else e.bm25_info()["ngroups"] == dg


def test_bm25_avgdl(engine, c2):
    ref, qs = c2["ref"], c2["qs"][:80]
    engine.run_host(*c2["args"])
    own = engine.query_bm25(qs, 10)
    same = engine.query_bm25(qs, 10, avgdl=ref.avgdl)               # the default's value, passed in
    assert bits(same["avgdl"]) == bits(own["avgdl"]) == bits(ref.avgdl)
    assert np.array_equal(own["doc"], same["doc"]) and np.array_equal(bits(own["score"]), bits(same["score"]))
    other = ref.avgdl * 0.37 + 1.0
    res = engine.query_bm25(qs, 10, avgdl=other)
    assert bits(res["avgdl"]) == bits(other)
    check(res, [ref.rank(q, avgdl=other) for q in qs], 10)
    assert not np.array_equal(bits(res["score"]), bits(own["score"]))


def test_bm25_leaves_the_result_and_allocates_once(engine, c2):
    engine.run_host(*c2["args"])
    before = engine.text()
    first = engine.query_bm25(c2["qs"], 10)
    a0 = engine.alloc_counters()
    second = engine.query_bm25(c2["qs"], 10)
    assert engine.alloc_counters() == a0                          # no device allocation
    assert np.array_equal(first["doc"], second["doc"]) and np.array_equal(bits(first["score"]), bits(second["score"]))
    assert engine.text() == before
    res = engine.fetch()
    check(engine.query_bm25(c2["qs"][:20], 3), c2["refs"][:20], 3)
    assert res["output_txt"] == before
    # tfidf_query shares the accumulators and candidate lists: it still returns its own bits
    plain = Ref(c2["ora"])
    check(engine.query(c2["qs"][:60], 10), [plain.rank(q) for q in c2["qs"][:60]], 10)
    check(engine.query_bm25(c2["qs"][:20], 10), c2["refs"][:20], 10)


@pytest.mark.parametrize("K", [2, 3])
def test_group_bm25_equals_single_shard_reference(c2, K):
    ref, qs = c2["ref"], c2["qs"][:100]
    shards = []
    for r in range(K):
        p = tfidf_configs.plan("c2", scale=0.002, rank=r, nranks=K)
        d, o = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
        shards.append((d, o, p["doc_ids"], p["ndocs_total"]))
    with tfidf_abi.Group(K, devices=[0] * K, local=True) as g:
        g.run_host(shards)
        for k in (3, 1024):
            res = g.query_bm25(qs, k)                               # avgdl = 0: L and n summed over the ranks
            check(res, c2["refs"][:len(qs)], k)
            assert bits(res["avgdl"]) == bits(ref.avgdl)
        other = 123.25
        check(g.query_bm25(qs, 10, 0.9, 1.0, avgdl=other), [ref.rank(q, 0.9, 1.0, other) for q in qs], 10)
        # a rank alone normalises by its own shard's average unless it is given the corpus's
        own = set(shards[1][2].tolist())
        res = g.ranks[1].query_bm25(qs[:40], 10, avgdl=ref.avgdl)
        for q, (hits, _) in enumerate(c2["refs"][:40]):
            mine = [(d, s) for d, s in hits if d in own]
            n = min(10, len(mine))
            assert int(res["nmatch"][q]) == len(mine)
            assert res["doc"][q, :n].tolist() == [d for d, _ in mine[:n]]
            assert np.array_equal(bits(res["score"][q, :n]), bits([s for _, s in mine[:n]]))


def test_bm25_errors(c2):
    with tfidf_abi.Engine(0) as e:
        with pytest.raises(tfidf_abi.TfidfError) as ex:
            e.query_bm25([b"x"], 3)
        assert ex.value.rc == tfidf_abi.E_STATE                    # before a run
        e.run_host(*c2["args"])
        for k in (0, 1025):
            with pytest.raises(tfidf_abi.TfidfError) as ex:
                e.query_bm25([b"x"], k)
            assert ex.value.rc == tfidf_abi.E_INVAL
        for kw in (dict(k1=-0.1), dict(b=1.01), dict(b=-0.5), dict(k1=math.nan), dict(b=math.nan),
                   dict(avgdl=math.nan), dict(avgdl=-2.0), dict(k1=math.inf), dict(avgdl=math.inf)):
            with pytest.raises(tfidf_abi.TfidfError) as ex:
                e.query_bm25(c2["qs"][:3], 3, **kw)
            assert ex.value.rc == tfidf_abi.E_INVAL, kw
        res = e.query_bm25([], 4)                                  # an empty batch is valid
        assert res["doc"].shape == (0, 4)
        check(e.query_bm25(c2["qs"][:5], 1024), c2["refs"][:5], 1024)


def test_bm25_parameter_struct_on_a_live_context(engine, c2):
    """the raw C call after a run: a valid struct and a NULL one (the defaults) succeed with
    the reference's rows, a `size` below sizeof(tfidf_bm25_params) or a bad value in an
    otherwise valid struct is TFIDF_E_INVAL and leaves *out zeroed"""
    L = tfidf_abi.lib()
    engine.run_host(*c2["args"])
    qs = c2["qs"][:6]
    blob = np.frombuffer(b"".join(qs), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(q) for q in qs])]).astype(np.uint64)
    batch = tfidf_abi.Queries()
    batch.bytes, batch.nbytes, batch.q_off, batch.nqueries = blob.ctypes.data, len(blob), off.ctypes.data, len(qs)
    full = C.sizeof(tfidf_abi.Bm25Params)

    def call(p):
        h = tfidf_abi.Hits()
        rc = L.tfidf_query_bm25(engine.h, C.byref(batch), 5, None if p is None else C.byref(p), C.byref(h))
        rows = None
        if rc == 0:
            rows = [(h.doc[q * 5], h.score[q * 5]) for q in range(len(qs)) if h.nhits[q]]
        else:
            assert not h.doc and not h.score and h.nqueries == 0
        L.tfidf_hits_free(C.byref(h))
        return rc, rows

    def params(size=full, k1=1.2, b=0.75, avgdl=0.0):
        p = tfidf_abi.Bm25Params()
        p.size, p.k1, p.b, p.avgdl = size, k1, b, avgdl
        return p

    want = [(hits[0][0], hits[0][1]) for hits, _ in c2["refs"][:6] if hits]
    assert want
    for p in (params(), None, params(size=full + 16)):
        rc, rows = call(p)
        assert rc == 0 and [d for d, _ in rows] == [d for d, _ in want]
        assert np.array_equal(bits([s for _, s in rows]), bits([s for _, s in want]))
    for p in (params(size=0), params(size=8), params(size=full - 1), params(k1=-1.0), params(b=1.5),
              params(avgdl=math.nan), params(k1=2.0 ** 901), params(avgdl=2.0 ** -901)):
        assert call(p)[0] == tfidf_abi.E_INVAL, (p.size, p.k1, p.b, p.avgdl)


def test_bm25_corpus_without_a_token(engine):
    """L = 0: no document has a token, there are no pairs, avgdl is 0 and every row is empty
    (no division by it); an explicit avgdl changes nothing"""
    data, off = docs_to_arrays([b"", b"  \n\t", b"\r\n"])
    engine.run_host(data, off)
    qs = [b"x", b"", b"x y x"]
    for kw in ({}, dict(avgdl=7.5)):
        res = engine.query_bm25(qs, 5, **kw)
        assert res["nhits"].tolist() == [0, 0, 0] and res["nmatch"].tolist() == [0, 0, 0]
        assert res["nterms_found"].tolist() == [0, 0, 0] and res["avgdl"] == kw.get("avgdl", 0.0)
    plain = engine.query(qs, 5)
    assert plain["nhits"].tolist() == [0, 0, 0] and plain["nmatch"].tolist() == [0, 0, 0]


@pytest.mark.parametrize("extra", [[], ["--shards", "2"]])
def test_cli_bm25(tmp_path, extra):
    case = "g5_w3"
    g = load_golden(case)
    ora = oracle_py.run(g["data"], g["off"])
    ref, plain = Bm25Ref(ora, len(g["off"]) - 1), Ref(ora)
    qs = [q.replace(b"\n", b" ") for q in make_queries(ora, np.random.default_rng(9), 12)]
    shutil.copytree(os.path.join(GOLDEN, case, "input"), tmp_path / "input")
    (tmp_path / "q.txt").write_bytes(b"\n".join(qs))              # the last line has no newline

    def lines(rank):
        return b"".join(b"q%d\tdoc%d\t%.16f\n" % (i + 1, d, s) for i, q in enumerate(qs) for d, s in rank(q)[0][:3])

    cmd = [tfidf_abi.CLI_PATH, "--query", "q.txt", "--top", "3"] + extra
    for flags, want in ((["--bm25"], lines(ref.rank)),
                        (["--bm25", "--bm25-k1", "2.0", "--bm25-b", "0.5"], lines(lambda q: ref.rank(q, 2.0, 0.5))),
                        (["--bm25-b", "0.5"], lines(lambda q: ref.rank(q, 1.2, 0.5))),   # a parameter implies --bm25
                        ([], lines(plain.rank))):                 # without --bm25: the bytes of `tfidf --query`
        p = subprocess.run(cmd + flags, cwd=tmp_path, capture_output=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert want and (tmp_path / "hits.txt").read_bytes() == want
        assert (tmp_path / "output.txt").read_bytes() == g["output"]
