"""Top-k similar documents (tfidf_similar / tfidf_group_similar / `tfidf --similar`) against a
plain Python loop over the oracle's pairs.

Reference (include/tfidf.h): document d's vector is its pairs in pair order; sq(d) is the
sequential sum of the squared scores, norm = sqrt(sq), dot(q, d) the sequential sum of the
products over the shared terms in term-table order (each product rounded before its add),
sim = dot / (norm(q) * norm(d)), +0.0 for a zero denominator.  Neighbours of q: the other
documents sharing at least one term, ordered by (sim descending, document id ascending).
nb_doc, nb_shared, nmatch, nnb, npairs and pos are compared exactly, nb_score and norm as u64
bits.  The loop runs over q's terms in order and, per term, over the term's pairs (numpy adds
one rounded product to each document's sum: the sequence of operations per (q, d) is the
definition's)."""
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import oracle_py
import tfidf_abi
import tfidf_configs
from conftest import golden_cases, GOLDEN
from helpers import docs_to_arrays, load_golden

pytestmark = pytest.mark.gpu

KS = [1, 3, 10, 1024]


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


class Ref:
    def __init__(self, ora, doc_ids):
        self.ids = [int(d) for d in doc_ids]
        self.order = sorted(self.ids, key=lambda d: b"doc%d@" % d)      # the lines' strcmp order (TFIDF.c:273)
        self.pos = {d: i for i, d in enumerate(self.order)}
        self.idx = {d: i for i, d in enumerate(self.ids)}
        self.id_arr = np.array(self.ids, dtype=np.int64)
        self.vec = {d: [] for d in self.ids}                            # (term, score) in pair order
        post = {}
        for d, t, s in zip(ora["doc"].tolist(), ora["term"].tolist(), ora["score"].tolist()):
            self.vec[d].append((t, s))
            post.setdefault(t, ([], []))
            post[t][0].append(self.idx[d])
            post[t][1].append(s)
        self.post = {t: (np.array(a, dtype=np.int64), np.array(b, dtype=np.float64)) for t, (a, b) in post.items()}
        self.sq, self.norm = {}, {}
        for d, v in self.vec.items():
            acc = 0.0
            for _, s in v:
                acc = acc + s * s
            self.sq[d] = acc
            self.norm[d] = math.sqrt(acc)
        self.norm_arr = np.array([self.norm[d] for d in self.ids], dtype=np.float64)
        self._nb = {}

    def neighbours(self, q):
        """[(doc, shared, sim)] of every neighbour of q, best first"""
        if q in self._nb:
            return self._nb[q]
        n = len(self.ids)
        acc, cnt = np.zeros(n), np.zeros(n, dtype=np.int64)
        for t, s in self.vec.get(q, []):
            di, ds = self.post[t]
            acc[di] = acc[di] + ds * s                                  # a term occurs once in a document
            cnt[di] += 1
        if q in self.idx:
            cnt[self.idx[q]] = 0
        den = self.norm_arr * self.norm.get(q, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            sim = np.where(den == 0.0, 0.0, acc / den)
        hit = np.flatnonzero(cnt)
        rows = sorted(((self.ids[i], int(cnt[i]), float(sim[i])) for i in hit.tolist()), key=lambda x: (-x[2], x[0]))
        self._nb[q] = rows
        return rows

    def rows(self, docs=None):
        """(doc, pos or None, npairs, norm, neighbours) per row"""
        ds = self.order if docs is None else [int(d) for d in docs]
        return [(d, self.pos.get(d), len(self.vec.get(d, [])), self.norm.get(d, 0.0), self.neighbours(d)) for d in ds]

    def fused_norms_differ(self):
        """would fma(s, s, acc) change the bits of any norm?"""
        for d, v in self.vec.items():
            acc = 0.0
            for _, s in v:
                acc = float(Fraction(s) * Fraction(s) + Fraction(acc))   # one rounding
            if math.sqrt(acc) != self.norm[d]:
                return True
        return False

    def fused_sims_differ(self, q, k):
        """would fma(s(q,t), s(d,t), acc) change the bits of any of q's first k similarities?"""
        nb = self.neighbours(q)[:k]
        want = {d for d, _, _ in nb}
        acc = {d: 0.0 for d in want}
        for t, s in self.vec[q]:
            di, ds = self.post[t]
            for i, x in zip(di.tolist(), ds.tolist()):
                d = self.ids[i]
                if d in want:
                    acc[d] = float(Fraction(x) * Fraction(s) + Fraction(acc[d]))
        return any(acc[d] / (self.norm[q] * self.norm[d]) != s for d, _, s in nb if self.norm[q] * self.norm[d] != 0.0)


def check(res, rows, k, pos=True):
    assert res["k"] == k and res["nb_doc"].shape == (len(rows), k)
    assert res["doc"].tolist() == [r[0] for r in rows], k
    if pos:
        assert res["pos"].tolist() == [tfidf_abi.NO_POS if r[1] is None else r[1] for r in rows], k
    assert res["npairs"].tolist() == [r[2] for r in rows], k
    assert np.array_equal(bits(res["norm"]), bits([r[3] for r in rows])), k
    assert res["nmatch"].tolist() == [len(r[4]) for r in rows], k
    assert res["nnb"].tolist() == [min(k, len(r[4])) for r in rows], k
    for i, (d, _, _, _, nb) in enumerate(rows):
        n = min(k, len(nb))
        assert res["nb_doc"][i, :n].tolist() == [x[0] for x in nb[:n]], (d, k)
        assert res["nb_shared"][i, :n].tolist() == [x[1] for x in nb[:n]], (d, k)
        assert np.array_equal(bits(res["nb_score"][i, :n]), bits([x[2] for x in nb[:n]])), (d, k)


def same_result(a, b):
    for name in ("doc", "pos", "npairs", "nmatch", "nnb", "nb_doc", "nb_shared"):
        assert np.array_equal(a[name], b[name]), name
    assert np.array_equal(bits(a["nb_score"]), bits(b["nb_score"])) and np.array_equal(bits(a["norm"]), bits(b["norm"]))


def run_and_check(engine, data, off, ids=None, ntotal=0, ks=KS, docs=None):
    ora = oracle_py.run(data, off, ids, ntotal)
    ref = Ref(ora, range(1, len(off)) if ids is None else ids)
    engine.run_host(data, off, ids, ntotal)
    for k in ks:
        check(engine.similar(k, docs), ref.rows(docs), k)
    return ref


@pytest.fixture(scope="module")
def c2():
    p = tfidf_configs.plan("c2", scale=0.002)      # seed: the plan's (fused_*_differ below hold for it)
    data, off = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
    ora = oracle_py.run(data, off, p["doc_ids"], p["ndocs_total"])
    return dict(p=p, data=data, off=off, ref=Ref(ora, p["doc_ids"]), args=(data, off, p["doc_ids"], p["ndocs_total"]))


def test_c2_vs_reference(engine, c2):
    ref = c2["ref"]
    # a kernel that fuses a product into its add cannot pass for this seed
    assert ref.fused_norms_differ()
    assert any(ref.fused_sims_differ(q, 10) for q in ref.order[:5])
    engine.run_host(*c2["args"])
    for k in KS:
        res = engine.similar(k)
        check(res, ref.rows(), k)
    info = engine.similar_info()
    assert info["rows"] == len(ref.ids) and info["k"] == 1024 and info["big_docs"] == 0
    assert info["ngroups"] == -(-len(ref.ids) // 64) and info["group_rows"] == 64
    # sim(a, b) and sim(b, a) have the same bits wherever both were returned
    sim = {}
    for i, a in enumerate(res["doc"].tolist()):
        for j in range(int(res["nnb"][i])):
            sim[(a, int(res["nb_doc"][i, j]))] = int(bits(res["nb_score"][i, j]))
    both = [(a, b) for (a, b) in sim if (b, a) in sim]
    assert len(both) > 1000 and all(sim[(a, b)] == sim[(b, a)] for a, b in both)


@pytest.mark.parametrize("case", golden_cases())
def test_golden_vs_reference(engine, case):
    g = load_golden(case)
    run_and_check(engine, g["data"], g["off"])


def test_group_boundary_and_small_budget(engine, monkeypatch):
    """65 rows cross the 64-row group.  Under the smallest budget, 1 MiB, a row of 800
    documents at k = 1024 takes 12 * 800 + 2 * (1024 * 12 + 4) + 8 = 34192 bytes: 30 rows per
    group, so the same 65 rows run in 3 groups and give the same result"""
    rng = np.random.default_rng(4)
    docs = [b" ".join(b"w%03d" % int(j) for j in rng.integers(0, 300, 15)) for _ in range(800)]
    data, off = docs_to_arrays(docs)
    ref = Ref(oracle_py.run(data, off), range(1, 801))
    engine.run_host(data, off)
    rows65 = list(range(3, 800, 12))[:65]
    assert len(rows65) == 65
    cases = [(10, rows65), (1024, rows65)]
    want = [engine.similar(k, d) for k, d in cases]
    assert engine.similar_info()["ngroups"] == 2 and engine.similar_info()["group_rows"] == 64
    for (k, d), w in zip(cases, want):
        check(w, ref.rows(d), k)
    monkeypatch.setenv("TFIDF_QUERY_ACC_MB", "1")
    with tfidf_abi.Engine(0) as e:
        e.run_host(data, off)
        for (k, d), w in zip(cases, want):
            same_result(e.similar(k, d), w)
        assert e.similar_info()["ngroups"] == 3 and e.similar_info()["group_rows"] == 30


def test_more_documents_than_a_top_k_slice(engine):
    """5000 documents: the dense accumulators are cut into two slices of 4096 and a second
    top-k round merges their lists; most neighbours tie (few distinct vectors).  The rounds beyond
    (a second round with several slices, a third launch): test_gpu_topk_rounds.py"""
    rng = np.random.default_rng(6)
    docs = [b" ".join(b"w%02d" % int(j) for j in rng.integers(0, 60, 3)) for _ in range(5000)]
    data, off = docs_to_arrays(docs)
    ref = Ref(oracle_py.run(data, off), range(1, 5001))
    engine.run_host(data, off)
    some = [4999, 1, 4097, 4096, 2500]
    for k in (3, 1024):
        check(engine.similar(k, some), ref.rows(some), k)
    assert max(len(ref.neighbours(d)) for d in some) > 200


def sized_doc(rng, n, lo=0, hi=6000):
    """exactly n distinct words, a third of them repeated (counts 2-4), shuffled"""
    words = rng.choice(np.arange(lo, hi), size=n, replace=False)
    toks = [int(w) for w in words for _ in range(1 + (int(w) % 3 == 0) * (1 + int(w) % 4 % 3))]
    return b" ".join(b"w%05d" % toks[i] for i in rng.permutation(len(toks)))


def test_wave_and_tile_boundaries(engine):
    """documents of exactly 1, 63, 64, 65, 256, 257, 4096 and 4097 pairs (64: a wave's round,
    256: its four rounds in flight and the workgroup kernel's tile, 4096: the cut between the
    wave and the workgroup kernel) among 20 small ones, every one a row and a candidate"""
    rng = np.random.default_rng(5)
    docs = [b" ".join(b"w%05d" % int(j) for j in rng.integers(0, 6000, 30)) for _ in range(20)]
    sizes = [1, 63, 64, 65, 256, 257, 4096, 4097]
    for i, n in enumerate(sizes):
        docs.insert(2 + 2 * i, sized_doc(rng, n))
    data, off = docs_to_arrays(docs)
    ref = run_and_check(engine, data, off, ks=[3, 1024])
    assert sorted(len(v) for v in ref.vec.values() if len(v) in sizes) == sizes
    assert all(len(ref.neighbours(d)) > 0 for d in ref.ids if len(ref.vec[d]) >= 63)
    assert engine.similar_info()["big_docs"] == 1                       # 4097


def test_ties_ordered_by_numeric_id(engine):
    """byte-identical documents 2, 10 and 100: their similarities to any row are equal and they
    come in numeric order (the "docN@" order is 10, 100, 2); k = 2 cuts the tie"""
    rng = np.random.default_rng(2)
    docs = [b" ".join(b"f%d_%d" % (i, int(j)) for j in rng.integers(0, 40, 12)) + b" filler" for i in range(100)]
    same = b"alpha beta gamma delta alpha"
    for d in (2, 10, 100):
        docs[d - 1] = same
    docs[49] = b"alpha beta zeta"
    docs[69] = b"gamma omega"
    data, off = docs_to_arrays(docs)
    ref = run_and_check(engine, data, off, ks=[1, 2, 3, 10])
    nb = ref.neighbours(50)
    assert [x[0] for x in nb[:3]] == [2, 10, 100] and len({x[2] for x in nb[:3]}) == 1 and nb[0][2] > 0
    assert [x[0] for x in ref.neighbours(2)[:2]] == [10, 100]
    res = engine.similar(2, [50, 70, 100])
    assert res["nb_doc"].tolist() == [[2, 10], [2, 10], [2, 10]] and res["nmatch"].tolist()[:2] == [3, 3]


def test_zero_norms(engine):
    """every term in every document: every score, norm and similarity is +0.0 and every other
    document is a neighbour, in id order.  Mixed: document 3 holds only the df = N term."""
    same = b"the same nine words in every single copy copy here"
    data, off = docs_to_arrays([same] * 70)
    ref = run_and_check(engine, data, off, ks=[4, 1024])
    res = engine.similar(1024)
    assert np.all(bits(res["nb_score"]) == 0) and np.all(bits(res["norm"]) == 0)      # +0.0, not -0.0 or NaN
    assert res["nmatch"].tolist() == [69] * 70 and res["nb_shared"][0, :69].tolist() == [9] * 69
    assert res["nb_doc"][ref.pos[5], :5].tolist() == [1, 2, 3, 4, 6]
    docs = [b"common a b c", b"common a d", b"common", b"common b c e", b"common e e a", b"common z"]
    data, off = docs_to_arrays(docs)
    ref = run_and_check(engine, data, off, ks=[1, 3, 10])
    assert ref.norm[3] == 0.0 and [x[2] for x in ref.neighbours(3)] == [0.0] * 5
    assert ref.neighbours(1)[-1][0] == 6 and ref.neighbours(1)[-1][2] == 0.0 and ref.neighbours(1)[0][2] > 0


def test_row_rules(engine):
    """non-contiguous global ids, two empty documents: every row; a caller-order list with a
    duplicate, absent ids and the empty documents; an empty list"""
    ids = np.array([7, 3, 19, 100, 42, 11, 5, 64, 28, 90, 2, 33], dtype=np.uint32)
    rng = np.random.default_rng(9)
    docs = [b" ".join(b"w%02d" % int(j) for j in rng.integers(0, 40, 15)) for _ in ids]
    docs[3], docs[8] = b"", b" \n\t "
    data, off = docs_to_arrays(docs)
    ref = run_and_check(engine, data, off, ids, 120, ks=[1, 5, 64])
    assert ref.neighbours(100) == [] and ref.neighbours(28) == [] and len(ref.neighbours(7)) > 3
    lists = [[42, 7, 42, 999, 100, 2, 42], [1, 4000000000, 0], [33, 2, 90, 28, 64, 5, 11, 42, 100, 19, 3, 7], [], [28]]
    for docs_ in lists:
        for k in (2, 64):
            res = engine.similar(k, docs_)
            check(res, ref.rows(docs_), k)
    assert res["pos"].tolist() == [ref.pos[28]] and res["nnb"].tolist() == [0] and res["npairs"].tolist() == [0]
    res = engine.similar(3, [999])
    assert res["pos"].tolist() == [tfidf_abi.NO_POS] and res["nmatch"].tolist() == [0]


def test_vocabulary_wider_than_2_18(engine):
    """300000 terms (the query pass's LDS filter covers 2^18): ranks 7 and 7 + 2^18 must not be
    taken for each other; rows of 10000 to 42858 terms (postings tables of ~10^5 entries)"""
    V = 300000
    docs = [b" ".join(b"w%06d" % i for i in range(d, V, 30)) for d in range(30)]
    docs.append(b"w000007 w262151 w262152")
    docs.append(b"w000007 w000008")
    docs.append(b"w262151 w262153")
    docs.append(b" ".join(b"w%06d" % i for i in range(0, V, 7)))
    docs.append(b" ".join(b"w%06d" % i for i in range(3, V, 11)))
    data, off = docs_to_arrays(docs)
    ora = oracle_py.run(data, off)
    by_name = sorted(ora["terms"])          # the engine's term ranks are the strcmp order
    assert by_name[7] == b"w000007" and by_name[7 + (1 << 18)] == b"w262151"
    ref = Ref(ora, range(1, len(docs) + 1))
    assert {x[0] for x in ref.neighbours(32)} == {8, 9, 31, 34} and {x[0] for x in ref.neighbours(33)} == {12, 14, 31}
    engine.run_host(data, off)
    for k in (3, 40):
        check(engine.similar(k), ref.rows(), k)
    assert engine.similar_info()["big_docs"] == 32


def long_docs():
    w15, w16 = b"abcdefghijklmno", b"abcdefghijklmnop"
    a, b_, c = w16 + b"q" * 24, w16 + b"r" * 24, b"L" * 300
    return [a + b" x " + w15 + b" " + c, b_ + b" y " + a + b" " + a, b"x y z ab\0cd ab " + b"M" * 299,
            w16 + b" " + a + b" " + w15 + b" " + b_, b"zz " + c + b" " + b"L" * 299 + b" y", b_ + b" zz " + w16 + b" " + w16]


def test_long_terms(engine):
    """terms of 16, 40 and 300 bytes shared between documents (two share their first 16 bytes)"""
    data, off = docs_to_arrays(long_docs())
    ref = run_and_check(engine, data, off, ks=[1, 2, 10])
    assert [x[0] for x in ref.neighbours(3)] and 5 in {x[0] for x in ref.neighbours(1)}
    assert sum(len(ref.neighbours(d)) for d in ref.ids) >= 20


def c2_shards(K):
    shards = []
    for r in range(K):
        p = tfidf_configs.plan("c2", scale=0.002, rank=r, nranks=K)
        d, o = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
        shards.append((d, o, p["doc_ids"], p["ndocs_total"]))
    return shards


@pytest.mark.parametrize("K", [2, 3])
def test_group_equals_single_shard_reference(c2, K):
    ref = c2["ref"]
    shards = c2_shards(K)
    ids = c2["p"]["doc_ids"].tolist()
    some = ids[::7] + [ids[3], 999999, ids[3]] + ids[::-11]
    assert all(set(s[2].tolist()) & set(some) for s in shards)          # the list's documents lie in every shard
    with tfidf_abi.Group(K, devices=[0] * K, local=True) as g:
        g.run_host(shards)
        for k in (3, 1024):
            for docs in (None, some):
                check(g.similar(k, docs), ref.rows(docs), k)
        # a rank alone searches its own documents only
        own = set(shards[1][2].tolist())
        res = g.ranks[1].similar(5, [shards[1][2][0], shards[0][2][0]])
        assert [p == tfidf_abi.NO_POS for p in res["pos"].tolist()] == [False, True] and res["nnb"].tolist()[1] == 0
        assert set(res["nb_doc"][0, :int(res["nnb"][0])].tolist()) <= own


@pytest.mark.parametrize("K", [2, 3])
def test_group_long_terms(K):
    """long terms that occur in one shard only (M * 299, L * 299) and in several"""
    docs = long_docs()
    data, off = docs_to_arrays(docs)
    ref = Ref(oracle_py.run(data, off), range(1, len(docs) + 1))
    cut = [0, 3, 6] if K == 2 else [0, 2, 4, 6]
    shards = []
    for r in range(K):
        d, o = docs_to_arrays(docs[cut[r]:cut[r + 1]])
        shards.append((d, o, np.arange(cut[r] + 1, cut[r + 1] + 1, dtype=np.uint32), len(docs)))
    with tfidf_abi.Group(K, devices=[0] * K, local=True) as g:
        g.run_host(shards)
        for k in (1, 10):
            check(g.similar(k), ref.rows(), k)
            check(g.similar(k, [6, 1, 77, 4, 1]), ref.rows([6, 1, 77, 4, 1]), k)


def test_leaves_the_result_and_allocates_once(engine, c2):
    engine.run_host(*c2["args"])
    some = c2["p"]["doc_ids"][:20]
    first = engine.similar(10)             # computes the norms
    assert engine.similar_info()["ms_norms"] > 0
    before = engine.text()
    engine.similar(10)
    engine.similar(3, some)
    a0 = engine.alloc_counters()
    second = engine.similar(10)
    third = engine.similar(3, some)
    assert engine.alloc_counters() == a0                               # no device allocation
    assert engine.similar_info()["ms_norms"] == 0                      # cached
    same_result(first, second)
    check(second, c2["ref"].rows(), 10)
    check(third, c2["ref"].rows(some), 3)
    assert engine.text() == before
    # another corpus: the norms are the new run's
    docs = [b"common a b c", b"common a d", b"b c d e", b"e e a"]
    data, off = docs_to_arrays(docs)
    run_and_check(engine, data, off, ks=[2])
    assert engine.similar_info()["ms_norms"] > 0


def test_errors(c2):
    with tfidf_abi.Engine(0) as e:
        with pytest.raises(tfidf_abi.TfidfError) as ex:
            e.similar(3)
        assert ex.value.rc == tfidf_abi.E_STATE                         # before a run
        e.run_host(*c2["args"])
        for k in (0, 1025):
            with pytest.raises(tfidf_abi.TfidfError) as ex:
                e.similar(k)
            assert ex.value.rc == tfidf_abi.E_INVAL
        some = c2["p"]["doc_ids"][:5]
        check(e.similar(1024, some), c2["ref"].rows(some), 1024)


@pytest.mark.parametrize("extra", [[], ["--shards", "2"]])
def test_cli_similar(tmp_path, extra):
    case = "g5_w3"
    g = load_golden(case)
    ref = Ref(oracle_py.run(g["data"], g["off"]), range(1, len(g["off"])))
    shutil.copytree(os.path.join(GOLDEN, case, "input"), tmp_path / "input")
    p = subprocess.run([tfidf_abi.CLI_PATH, "--similar", "3"] + extra, cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr

    def lines(rows):
        return b"".join(b"doc%d\tdoc%d\t%.16f\n" % (r[0], d, s) for r in rows for d, _, s in r[4][:3])

    want = lines(ref.rows())
    assert want.count(b"\n") > len(ref.ids)
    assert (tmp_path / "similar.txt").read_bytes() == want
    assert (tmp_path / "output.txt").read_bytes() == g["output"]
    some = [ref.order[-1], ref.order[0], 4000, ref.order[0]]
    (tmp_path / "ids.txt").write_bytes(b"".join(b"%d\n" % d for d in some))
    p = subprocess.run([tfidf_abi.CLI_PATH, "--similar", "3", "--similar-docs", "ids.txt", "--similar-file", "nb.txt"] + extra,
                       cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "nb.txt").read_bytes() == lines(ref.rows(some))
    for bad in ("0", "1025"):
        q = subprocess.run([tfidf_abi.CLI_PATH, "--similar", bad], cwd=tmp_path, capture_output=True, timeout=120)
        assert q.returncode == 2
