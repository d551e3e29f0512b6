"""Per-document top-k keywords (tfidf_top_terms / tfidf_group_top_terms / `tfidf --keywords`)
against a plain Python sort of the oracle's pairs.

Reference (include/tfidf.h): the keywords of a document are its pairs ordered by (score
descending, then "word\\t" ascending in strcmp order); the first k are returned, with the
run's scores bit for bit.  doc, pos, npairs, nterms, count and the words' bytes are compared
exactly, scores as u64 bits, term and pair against Engine.fetch()."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_py
import tfidf_abi
import tfidf_configs
from conftest import golden_cases, GOLDEN
from helpers import docs_to_arrays, load_golden

pytestmark = pytest.mark.gpu

KS = [1, 3, 10, 64, 65, 1024]     # 64 | 65: the wave kernel's buffers of 128 and 512 entries; 1024: of 2048


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


class Ref:
    """every document's pairs as (word, count, score), best first"""

    def __init__(self, ora, doc_ids):
        self.ids = [int(d) for d in doc_ids]
        self.order = sorted(self.ids, key=lambda d: b"doc%d@" % d)      # the lines' strcmp order (TFIDF.c:273)
        self.pos = {d: i for i, d in enumerate(self.order)}
        terms = ora["terms"]
        self.by_doc = {d: [] for d in self.ids}
        for d, t, c, s in zip(ora["doc"].tolist(), ora["term"].tolist(), ora["count"].tolist(), ora["score"].tolist()):
            self.by_doc[d].append((terms[t], c, s))
        for rows in self.by_doc.values():
            rows.sort(key=lambda x: (-x[2], x[0] + b"\t"))

    def rows(self, docs=None):
        """(doc, pos or None, pairs best first) per row"""
        if docs is None:
            return [(d, self.pos[d], self.by_doc[d]) for d in self.order]
        return [(int(d), self.pos.get(int(d)), self.by_doc.get(int(d), [])) for d in docs]

    def ties_at(self, k):
        """documents whose k-th and (k+1)-th best pairs have equal scores"""
        return sum(1 for r in self.by_doc.values() if len(r) > k and r[k - 1][2] == r[k][2])


def pair_index(fetched):
    """(doc, word) -> (pair index, term rank) of a fetched result"""
    terms = fetched["terms"]
    return {(d, terms[t]): (p, t) for p, (d, t) in enumerate(zip(fetched["doc"].tolist(), fetched["term"].tolist()))}


def check(res, rows, k, index=None, pos=True):
    assert res["k"] == k and res["term"].shape == (len(rows), k) and len(res["words"]) == len(rows)
    assert res["doc"].tolist() == [d for d, _, _ in rows], k
    if pos:
        assert res["pos"].tolist() == [tfidf_abi.NO_POS if p is None else p for _, p, _ in rows], k
    assert res["npairs"].tolist() == [len(r) for _, _, r in rows], k
    assert res["nterms"].tolist() == [min(k, len(r)) for _, _, r in rows], k
    for i, (d, _, r) in enumerate(rows):
        n = min(k, len(r))
        assert res["words"][i] == [w for w, _, _ in r[:n]], (d, k)
        assert res["count"][i, :n].tolist() == [c for _, c, _ in r[:n]], (d, k)
        assert np.array_equal(bits(res["score"][i, :n]), bits([s for _, _, s in r[:n]])), (d, k)
        if index is not None:
            want = [index[(d, w)] for w, _, _ in r[:n]]
            assert res["pair"][i, :n].tolist() == [p for p, _ in want], (d, k)
            assert res["term"][i, :n].tolist() == [t for _, t in want], (d, k)


def run_and_check(engine, data, off, ids=None, ntotal=0, ks=KS, docs=None):
    ora = oracle_py.run(data, off, ids, ntotal)
    ref = Ref(ora, range(1, len(off)) if ids is None else ids)
    engine.run_host(data, off, ids, ntotal)
    index = pair_index(engine.fetch())
    for k in ks:
        check(engine.top_terms(k, docs), ref.rows(docs), k, index)
    return ref


@pytest.fixture(scope="module")
def c2():
    p = tfidf_configs.plan("c2", scale=0.002)
    data, off = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
    ora = oracle_py.run(data, off, p["doc_ids"], p["ndocs_total"])
    return dict(p=p, data=data, off=off, ref=Ref(ora, p["doc_ids"]), args=(data, off, p["doc_ids"], p["ndocs_total"]))


def test_c2_vs_reference(engine, c2):
    ref = c2["ref"]
    # a kernel that breaks ties at the cut any other way cannot pass: most documents have one
    assert ref.ties_at(10) * 2 >= len(ref.ids)
    assert ref.ties_at(1) > 0 and ref.ties_at(3) > 0
    engine.run_host(*c2["args"])
    index = pair_index(engine.fetch())
    for k in KS:
        check(engine.top_terms(k), ref.rows(), k, index)
    info = engine.terms_info()
    assert info["ndocs"] == len(ref.ids) and info["k"] == 1024 and info["nbatches"] == 1 and info["big_docs"] == 0


@pytest.mark.parametrize("case", golden_cases())
def test_golden_vs_reference(engine, case):
    g = load_golden(case)
    ref = run_and_check(engine, g["data"], g["off"])
    if len(ref.ids) > 1 and max(len(r) for r in ref.by_doc.values()) > 10:
        assert ref.ties_at(10) > 0


def sized_doc(rng, n, lo=0, hi=6000):
    """exactly n distinct words, a third of them repeated (counts 2-4), shuffled"""
    words = rng.choice(np.arange(lo, hi), size=n, replace=False)
    toks = [int(w) for w in words for _ in range(1 + (int(w) % 3 == 0) * (1 + int(w) % 4 % 3))]
    return b" ".join(b"w%05d" % toks[i] for i in rng.permutation(len(toks)))


@pytest.mark.parametrize("k", [3, 1024])
def test_size_boundaries(engine, k):
    """documents of exactly 0, 1, k-1, k, k+1, 63, 64, 65, 4095, 4096, 4097 and 6000 distinct
    words (4096 is the cut between the wave kernel and the workgroup kernel) and one over
    BIG_DOC bytes that K1 splits across chunks, among 50 small documents"""
    rng = np.random.default_rng(7)
    docs = [b" ".join(b"w%05d" % int(j) for j in rng.integers(0, 6000, 30)) for _ in range(50)]
    sizes = [0, 1, k - 1, k, k + 1, 63, 64, 65, 4095, 4096, 4097, 6000]
    for i, n in enumerate(sizes):
        docs.insert(3 + 4 * i, sized_doc(rng, n))
    big = b" ".join(b"w%05d" % int(j) for j in rng.integers(0, 5000, 12000))
    assert len(big) > 49152
    docs.insert(20, big)
    data, off = docs_to_arrays(docs)
    ref = run_and_check(engine, data, off, ks=[k])
    assert sorted(len(r) for r in ref.by_doc.values() if len(r) in sizes) == sorted(sizes)
    nbig = sum(len(r) > 4096 for r in ref.by_doc.values())               # 4097, 6000 and the split document
    assert nbig == 3 and engine.terms_info()["big_docs"] == nbig


def test_all_tie_and_all_zero_documents(engine):
    """every word of a document occurs once there and in no other document: all its scores are
    equal and the row is its first k words in term order.  120 identical documents: every
    score is +0.0 and sorts by term alone."""
    rng = np.random.default_rng(1)
    docs = []
    for d in range(9):
        words = [b"d%dx%04d" % (d, i) for i in range(7 + 40 * d)]
        docs.append(b" ".join(words[i] for i in rng.permutation(len(words))))
    data, off = docs_to_arrays(docs)
    ref = run_and_check(engine, data, off, ks=[1, 5, 64, 65])
    res = engine.top_terms(5)
    for i, d in enumerate(ref.order):
        assert len(set(bits(res["score"][i]).tolist())) == 1
        assert res["words"][i] == [b"d%dx%04d" % (d - 1, j) for j in range(5)]
    same = b"the same nine words in every single copy copy here"
    data, off = docs_to_arrays([same] * 120)
    ref = run_and_check(engine, data, off, ks=[4, 10])
    res = engine.top_terms(4)
    assert np.all(bits(res["score"]) == 0)                              # +0.0, not -0.0
    assert res["words"] == [sorted(set(same.split()))[:4]] * 120
    assert res["npairs"].tolist() == [9] * 120


def test_long_terms(engine):
    """words of 15, 16 and 40 bytes, two sharing their first 16 bytes, and a token cut by a
    NUL: the returned bytes are the words'"""
    w15, w16 = b"abcdefghijklmno", b"abcdefghijklmnop"
    a, b_ = w16 + b"q" * 24, w16 + b"r" * 24
    docs = [a + b" x " + w15, b_ + b" y " + a + b" " + a, b"x y z ab\0cd ab", w16 + b" " + a + b" " + w15 + b" " + b_,
            b"zz " + b"L" * 300 + b" " + b"L" * 299]
    data, off = docs_to_arrays(docs)
    ref = run_and_check(engine, data, off, ks=[1, 2, 10])
    res = engine.top_terms(10)
    got = {w for row in res["words"] for w in row}
    assert {w15, w16, a, b_, b"ab", b"L" * 300, b"L" * 299} <= got and b"ab\0cd" not in got and b"cd" not in got
    assert len(ref.by_doc[4]) == 4


def test_id_lists(engine):
    """a shard with non-trivial global ids: a subset, a duplicate, absent ids, reversed order"""
    p = tfidf_configs.plan("c2", scale=0.002, rank=1, nranks=3)
    data, off = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
    ids = p["doc_ids"].tolist()
    assert ids != list(range(1, len(ids) + 1))
    absent = [d for d in range(1, p["ndocs_total"] + 1) if d not in set(ids)]
    lists = [ids[::3], [ids[5], ids[2], ids[5], ids[5]], [absent[0], ids[0], absent[-1], 0, 4000000000],
             ids[::-1], [], [absent[1]]]
    ora = oracle_py.run(data, off, p["doc_ids"], p["ndocs_total"])
    ref = Ref(ora, ids)
    engine.run_host(data, off, p["doc_ids"], p["ndocs_total"])
    index = pair_index(engine.fetch())
    for docs in lists:
        for k in (3, 65):
            res = engine.top_terms(k, docs)
            check(res, ref.rows(docs), k, index)
    assert res["pos"].tolist() == [tfidf_abi.NO_POS] and res["words"] == [[]]
    check(engine.top_terms(10), ref.rows(), 10, index)


def same_result(a, b):
    for name in ("doc", "pos", "npairs", "nterms", "term", "count", "pair"):
        assert np.array_equal(a[name], b[name]), name
    assert np.array_equal(bits(a["score"]), bits(b["score"])) and a["words"] == b["words"]


def test_batches_under_a_small_budget(engine, c2, monkeypatch):
    """TFIDF_TERMS_MB=1: 200 rows of k = 1024 (32 KiB each) are cut into batches; the results
    are the default engine's"""
    engine.run_host(*c2["args"])
    some = c2["p"]["doc_ids"][::-2]
    cases = [(1024, None), (64, None), (1024, some)]
    want = [engine.top_terms(k, d) for k, d in cases]
    assert engine.terms_info()["nbatches"] == 1
    monkeypatch.setenv("TFIDF_TERMS_MB", "1")
    with tfidf_abi.Engine(0) as e:
        e.run_host(*c2["args"])
        for (k, d), w in zip(cases, want):
            got = e.top_terms(k, d)
            same_result(got, w)
            check(got, c2["ref"].rows(d), k)
            assert (e.terms_info()["nbatches"] > 1) == (k == 1024)


def test_leaves_the_result_and_allocates_once(engine, c2):
    engine.run_host(*c2["args"])
    first = engine.top_terms(10)           # before any formatting: builds the term metadata itself
    before = engine.text()
    a0 = engine.alloc_counters()
    second = engine.top_terms(10)
    assert engine.alloc_counters() == a0                               # no device allocation
    same_result(first, second)
    check(second, c2["ref"].rows(), 10)
    assert engine.text() == before
    res = engine.fetch()
    check(engine.top_terms(3, c2["p"]["doc_ids"][:20]), c2["ref"].rows(c2["p"]["doc_ids"][:20]), 3, pair_index(res))
    assert res["output_txt"] == before


def test_group_equals_single_shard_reference(engine, c2):
    K = 3
    shards = []
    for r in range(K):
        p = tfidf_configs.plan("c2", scale=0.002, rank=r, nranks=K)
        d, o = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
        shards.append((d, o, p["doc_ids"], p["ndocs_total"]))
    engine.run_host(*c2["args"])
    index = {key: (p, None) for key, (p, _) in pair_index(engine.fetch()).items()}
    ref = c2["ref"]
    ids = c2["p"]["doc_ids"].tolist()
    some = ids[::7] + [ids[3], 999999, ids[3]] + ids[::-11]
    with tfidf_abi.Group(K, devices=[0] * K, local=True) as g:
        g.run_host(shards)
        for k in (3, 1024):
            for docs in (None, some):
                res = g.top_terms(k, docs)
                rows = ref.rows(docs)
                check(res, rows, k)
                for i, (d, _, r) in enumerate(rows):                   # pairs count over the concatenated output
                    n = min(k, len(r))
                    assert res["pair"][i, :n].tolist() == [index[(d, w)][0] for w, _, _ in r[:n]]
        # a rank alone returns its own documents only
        own = shards[1][2].tolist()
        res = g.ranks[1].top_terms(10)
        assert sorted(res["doc"].tolist()) == sorted(own)
        own_order = [d for d in ref.order if d in set(own)]
        check(res, [(d, i, ref.by_doc[d]) for i, d in enumerate(own_order)], 10)
        res = g.ranks[1].top_terms(10, [own[0], shards[0][2][0], shards[2][2][0]])
        assert [p == tfidf_abi.NO_POS for p in res["pos"].tolist()] == [False, True, True]
        assert res["nterms"].tolist()[1:] == [0, 0]


def test_errors(c2):
    with tfidf_abi.Engine(0) as e:
        with pytest.raises(tfidf_abi.TfidfError) as ex:
            e.top_terms(3)
        assert ex.value.rc == tfidf_abi.E_STATE                         # before a run
        e.run_host(*c2["args"])
        for k in (0, 1025):
            with pytest.raises(tfidf_abi.TfidfError) as ex:
                e.top_terms(k)
            assert ex.value.rc == tfidf_abi.E_INVAL
        check(e.top_terms(1024, c2["p"]["doc_ids"][:5]), c2["ref"].rows(c2["p"]["doc_ids"][:5]), 1024)


@pytest.mark.parametrize("extra", [[], ["--shards", "2"]])
def test_cli_keywords(tmp_path, extra):
    case = "g5_w3"
    g = load_golden(case)
    ref = Ref(oracle_py.run(g["data"], g["off"]), range(1, len(g["off"])))
    shutil.copytree(os.path.join(GOLDEN, case, "input"), tmp_path / "input")
    p = subprocess.run([tfidf_abi.CLI_PATH, "--keywords", "3"] + extra, cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    want = b"".join(b"doc%d\t" % d + w + b"\t%.16f\n" % s for d, _, r in ref.rows() for w, _, s in r[:3])
    assert want.count(b"\n") == 3 * len(ref.ids)
    assert (tmp_path / "keywords.txt").read_bytes() == want
    assert (tmp_path / "output.txt").read_bytes() == g["output"]
    for bad in ("0", "1025"):
        q = subprocess.run([tfidf_abi.CLI_PATH, "--keywords", bad], cwd=tmp_path, capture_output=True, timeout=120)
        assert q.returncode == 2
