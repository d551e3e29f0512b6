"""Top-k retrieval (tfidf_query / tfidf_group_query / `tfidf --query`) against a plain
Python ranking of the oracle's pairs.

Reference (include/tfidf.h): a query is tokenised like a document; w = tokens per term;
score(q, d) = the sum over d's pairs, in pair order, of fl(w * s) on Python floats (never
fused); hits = documents with at least one query term, ordered by (score descending,
document id ascending).  doc rows, nhits, nmatch and nterms_found are compared exactly,
scores as u64 bits."""
import os
import shutil
import subprocess
import sys
from collections import Counter
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


def tokenize(q: bytes):
    """fscanf("%s") tokens (bytes.split() splits at exactly 0x20 and 0x09..0x0D), terms cut
    at their first NUL"""
    return [t.split(b"\0")[0] for t in q.split()]


class Ref:
    """the oracle's pairs, indexed by term; ranks a query with a plain loop"""

    def __init__(self, ora):
        self.tid = {t: i for i, t in enumerate(ora["terms"])}
        term = ora["term"]
        self.by_term = np.argsort(term, kind="stable")
        self.first = np.searchsorted(term[self.by_term], np.arange(len(ora["terms"]) + 1))
        self.doc = ora["doc"].tolist()
        self.score = ora["score"].tolist()

    def matches(self, q: bytes):
        """(pair position, doc, weight, score) of every pair of a query term, in pair order"""
        w = Counter(tokenize(q))
        found = [t for t in w if t in self.tid]
        m = []
        for t in found:
            i = self.tid[t]
            for p in self.by_term[self.first[i]:self.first[i + 1]].tolist():
                m.append((p, self.doc[p], w[t], self.score[p]))
        m.sort()
        return m, len(found)

    def rank(self, q: bytes):
        m, nfound = self.matches(q)
        acc = {}
        for _, d, w, s in m:
            acc[d] = acc.get(d, 0.0) + w * s
        return sorted(acc.items(), key=lambda x: (-x[1], x[0])), nfound

    def fused_differs(self, q: bytes) -> bool:
        """would fma(w, s, acc) change the bits of any score of this query?"""
        m, _ = self.matches(q)
        plain, fused = {}, {}
        for _, d, w, s in m:
            plain[d] = plain.get(d, 0.0) + w * s
            fused[d] = float(Fraction(w) * Fraction(s) + Fraction(fused.get(d, 0.0)))   # one rounding
        return any(plain[d] != fused[d] for d in plain)


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def check(res, refs, k):
    """res: Engine.query / Group.query output; refs: [(hits, nfound)] per query"""
    assert res["doc"].shape == (len(refs), k)
    for q, (hits, nfound) in enumerate(refs):
        n = min(k, len(hits))
        assert int(res["nhits"][q]) == n, (q, k)
        assert int(res["nmatch"][q]) == len(hits), (q, k)
        assert int(res["nterms_found"][q]) == nfound, (q, k)
        assert res["doc"][q, :n].tolist() == [d for d, _ in hits[:n]], (q, k)
        assert np.array_equal(bits(res["score"][q, :n]), bits([s for _, s in hits[:n]])), (q, k)


def make_queries(ora, rng, n):
    """n queries of 0-8 tokens drawn from the vocabulary, half of them uniformly (rare words,
    short hit lists) and half as the word of a random pair (frequent words, hit lists longer
    than k): repeats (weights 2-7), absent words, a token cut by a NUL, an empty and a
    whitespace-only query"""
    qs = [b"", b" \t\r\n \x0b\x0c "]
    terms, pair_term = ora["terms"], ora["term"]
    V = len(terms)
    while len(qs) < n:
        toks = []
        for _ in range(int(rng.integers(0, 9))):
            r = rng.random()
            if r < 0.4:
                t = terms[int(rng.integers(0, V))]
            elif r < 0.8:
                t = terms[int(pair_term[int(rng.integers(0, len(pair_term)))])]
            else:
                t = b"zz-absent-%d" % int(rng.integers(0, 50))
            if r < 0.05:
                t = t + b"\0tail"       # strcmp semantics: the term ends at the NUL
            toks += [t] * (int(rng.integers(2, 8)) if rng.random() < 0.4 else 1)
        order = rng.permutation(len(toks))
        seps = [b" ", b"\n", b"\t", b"  "]
        qs.append(b"".join(toks[i] + seps[int(rng.integers(0, 4))] for i in order))
    return qs


@pytest.fixture(scope="module")
def c2():
    p = tfidf_configs.plan("c2", scale=0.002)
    data, off = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
    ora = oracle_py.run(data, off, p["doc_ids"], p["ndocs_total"])
    ref = Ref(ora)
    qs = make_queries(ora, np.random.default_rng(11), 200)
    return dict(p=p, data=data, off=off, ref=ref, qs=qs, refs=[ref.rank(q) for q in qs])


def test_c2_queries_vs_reference(engine, c2):
    # for this seed a contracted kernel (fma(w, s, acc)) cannot pass: some returned score differs
    assert any(c2["ref"].fused_differs(q) for q in c2["qs"][:60])
    engine.run_host(c2["data"], c2["off"], c2["p"]["doc_ids"], c2["p"]["ndocs_total"])
    for k in KS:
        check(engine.query(c2["qs"], k), c2["refs"], k)
    assert any(len(h) > 10 for h, _ in c2["refs"]) and any(0 < len(h) < 1024 for h, _ in c2["refs"])


@pytest.mark.parametrize("case", golden_cases())
def test_golden_queries_vs_reference(engine, case):
    g = load_golden(case)
    ora = oracle_py.run(g["data"], g["off"])
    ref = Ref(ora)
    qs = make_queries(ora, np.random.default_rng(5), 200)
    refs = [ref.rank(q) for q in qs]
    engine.run_host(g["data"], g["off"])
    for k in KS:
        check(engine.query(qs, k), refs, k)


def test_nul_cut_token(engine):
    data, off = docs_to_arrays([b"ab x", b"cd y", b"ab ab z", b"ab\0cd q"])
    engine.run_host(data, off)
    ref = Ref(oracle_py.run(data, off))
    qs = [b"ab\0cd", b"ab\0cd cd", b"\0ab"]
    refs = [ref.rank(q) for q in qs]
    assert [d for d, _ in refs[0][0]] and 2 not in [d for d, _ in refs[0][0]]   # "cd" alone is not queried
    check(engine.query(qs, 5), refs, 5)


def test_ties_ordered_by_numeric_id(engine):
    """120 byte-identical documents tie on every score: the cut at k falls inside the tie and
    the ids come back as 1, 2, 3, ... (not the strcmp order 1, 10, 100, ... of the lines)"""
    docs = [b"same words in every copy copy"] * 120 + [b"other words here", b"same here once", b"nothing shared"]
    data, off = docs_to_arrays(docs)
    engine.run_host(data, off)
    ref = Ref(oracle_py.run(data, off))
    qs = [b"copy", b"copy same", b"every words", b"here copy"]
    refs = [ref.rank(q) for q in qs]
    for k in (7, 15):
        res = engine.query(qs, k)
        check(res, refs, k)
        assert res["doc"][0].tolist() == list(range(1, k + 1))
    assert int(engine.query(qs, 7)["nmatch"][0]) == 120


def test_zero_score_hits(engine):
    """a word of every document has idf 0: each document is a hit with score +0.0"""
    docs = [b"the w%d x%d" % (i, i % 5) for i in range(40)] + [b"the rare w3", b"the rare"]
    docs.append(b"unrelated text")          # holds neither "the" nor "rare"
    # "the" is in 42 of 43 documents (score > 0 there); "all" is in every one
    docs2 = [d + b" all" for d in docs]
    data, off = docs_to_arrays(docs2)
    engine.run_host(data, off)
    ref = Ref(oracle_py.run(data, off))
    qs = [b"all", b"all rare", b"rare the", b"all all all x1"]
    refs = [ref.rank(q) for q in qs]
    N = len(docs2)
    for k in (5, 1024):
        res = engine.query(qs, k)
        check(res, refs, k)
    assert int(res["nmatch"][0]) == N and int(res["nhits"][0]) == N
    assert np.all(bits(res["score"][0, :N]) == 0)                  # +0.0, not -0.0
    assert res["doc"][0, :N].tolist() == list(range(1, N + 1))
    assert res["doc"][1, :2].tolist() == [42, 41]                  # the rare word's documents first
    res = engine.query([b"rare the"], 1024)
    assert N not in res["doc"][0, :int(res["nhits"][0])].tolist() and int(res["nmatch"][0]) == N - 1


def test_long_documents(engine):
    """one document of 6000 distinct words (over K5_MAX_PAIRS: the workgroup-per-document
    path, many tiles), one over BIG_DOC bytes (split across chunks by K1), one of 3000 words
    (many rounds of its owner wave), among 50 small documents"""
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
    ref = Ref(oracle_py.run(data, off))
    spread = [word(i) for i in range(0, 6000, 20)]                 # 300 words over the whole term range
    q = b" ".join(w for i, w in enumerate(spread) for _ in range(1 + i % 7))
    qs = [q, b" ".join(spread[::3]), word(5999) + b" " + word(0), b" ".join(word(i) for i in range(4090, 4110))]
    refs = [ref.rank(x) for x in qs]
    assert refs[0][1] == 300 and ref.fused_differs(q)
    for k in (3, 1024):
        check(engine.query(qs, k), refs, k)
    # 1500 distinct query words: the group's term table no longer fits the kernels' LDS copy
    wide = [b" ".join(word(i) for i in range(0, 6000, 4)), q]
    check(engine.query(wide, 60), [ref.rank(x) for x in wide], 60)


def test_vocabulary_wider_than_the_lds_filter(engine):
    """300000 terms: the kernels' LDS filter (2^18 bits over the ranks' low bits) is no longer
    exact.  Ranks 7 and 7 + 2^18 share a bit: a pair of the other word passes the filter and
    the exact search must reject it, in a long document (workgroup path) and a short one"""
    V = 300000
    docs = [b" ".join(b"w%06d" % i for i in range(d, V, 30)) for d in range(30)]
    docs.append(b"w000007 w262151 w262152")
    data, off = docs_to_arrays(docs)
    engine.run_host(data, off)
    ora = oracle_py.run(data, off)
    by_name = sorted(ora["terms"])          # the engine's term ranks are the strcmp order
    assert by_name[7] == b"w000007" and by_name[7 + (1 << 18)] == b"w262151"
    ref = Ref(ora)
    qs = [b"w000007", b"w262151", b"w000007 w262151 w262151", b"w262152 w000008 w299999", b"w300000"]
    refs = [ref.rank(q) for q in qs]
    assert [d for d, _ in refs[0][0]] == [31, 8] and [d for d, _ in refs[1][0]] == [31, 12]
    check(engine.query(qs, 8), refs, 8)


def test_long_terms(engine):
    """terms of >= 16 bytes are 120-bit hashes in the table: a present one matches, an absent
    one sharing its first 16 bytes does not"""
    a = b"abcdefghijklmnop" + b"q" * 24          # 40 bytes
    b_ = b"abcdefghijklmnop" + b"r" * 24         # same first 16 bytes, present
    absent = b"abcdefghijklmnop" + b"s" * 24     # same first 16 bytes, absent
    s16 = b"abcdefghijklmnop"                    # exactly 16 bytes: the shortest long term
    docs = [a + b" x", b_ + b" y " + a, b"x y z", s16 + b" " + a]
    data, off = docs_to_arrays(docs)
    engine.run_host(data, off)
    ref = Ref(oracle_py.run(data, off))
    qs = [a, absent, b_ + b" " + absent, s16, s16[:15], a + b"\0" + absent, a * 2]
    refs = [ref.rank(q) for q in qs]
    assert refs[0][1] == 1 and refs[1] == ([], 0) and refs[4] == ([], 0) and refs[6] == ([], 0)
    res = engine.query(qs, 10)
    check(res, refs, 10)
    assert res["nmatch"].tolist()[:2] == [3, 0]


_LONGTAG_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2]); sys.path.insert(0, sys.argv[3])
import numpy as np, tfidf_abi
from helpers import docs_to_arrays
from test_gpu_query import long_key16
rng = np.random.default_rng(17)
cand = rng.integers(97, 123, (400000, 40), dtype=np.uint8)
key = long_key16(cand)
present = [bytes(cand[i]) for i in range(4)]
assert len(set(key[:4].tolist())) == 4
# an absent word whose 16-bit key equals a present word's
hit = [i for i in range(4, len(cand)) if key[i] == key[0] and bytes(cand[i]) != present[0]]
assert hit, "no collision among the candidates"
absent = bytes(cand[hit[0]])
with tfidf_abi.Engine(0) as e:
    # the CPU key is the library's: two PRESENT words sharing it are a reported collision
    data, off = docs_to_arrays([present[0] + b" x", absent + b" y"])
    try:
        e.run_host(data, off)
        print("RESULT pair merged")
    except tfidf_abi.TfidfError as ex:
        print("RESULT pair rc=%d" % ex.rc)
    data, off = docs_to_arrays([present[0] + b" x", present[1] + b" " + present[2], present[3] + b" " + present[0]])
    e.run_host(data, off)
    r = e.query([present[0], absent, absent + b" " + present[1]], 5)
    print("RESULT found", r["nterms_found"].tolist(), "nmatch", r["nmatch"].tolist(), "doc", r["doc"][0, :2].tolist())
"""


def long_key16(words: np.ndarray) -> np.ndarray:
    """make_long_key of csrc/dev_common.h with TFIDF_LONG_KEY_BITS=16 (the low 16 bits of the
    key's low word) for an [n, len] array of bytes, in wrapping u64 arithmetic"""
    u = np.uint64
    n = u(words.shape[1])

    def mix64(z):
        z = (z ^ (z >> u(30))) * u(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> u(27))) * u(0x94D049BB133111EB)
        return z ^ (z >> u(31))

    with np.errstate(over="ignore"):
        h1 = np.full(len(words), u(0x243F6A8885A308D3) ^ n, dtype=u)
        h2 = np.full(len(words), u(0x13198A2E03707344) + n * u(0x9E3779B97F4A7C15), dtype=u)
        for i in range(words.shape[1]):
            c = words[:, i].astype(u)
            h1 = (h1 ^ c) * u(0x100000001B3)
            h2 = (h2 + c + u(1)) * u(0xC2B2AE3D27D4EB4F)
            h2 ^= h2 >> u(29)
        return mix64(h1 ^ (h2 << u(1))) & u(0xFFFF)


def test_long_term_key_collision_does_not_match():
    """lib/libtfidf_hip_longtag16.so cuts long terms' keys to 16 bits.  An absent 40-byte
    word whose key equals a present word's (found by brute force on the CPU; that the CPU key
    is the library's is shown by the run that holds both words failing with
    TFIDF_E_CAPACITY) must not match: the bytes decide."""
    here = os.path.dirname(os.path.abspath(__file__))
    pydir = os.path.join(os.path.dirname(here), "parallel-systems-mpi-tfidf_amd", "python")
    env = dict(os.environ, TFIDF_LIB="longtag16")
    r = subprocess.run([sys.executable, "-c", _LONGTAG_CHILD, pydir, here, os.path.join(os.path.dirname(here), "oracle")],
                       env=env, capture_output=True, text=True, timeout=240, cwd=here)
    out = [l for l in r.stdout.splitlines() if l.startswith("RESULT")]
    assert out == ["RESULT pair rc=-9", "RESULT found [1, 0, 1] nmatch [2, 0, 1] doc [1, 3]"], r.stdout + r.stderr[-3000:]


def test_query_groups_under_a_small_budget(engine, c2, monkeypatch):
    """TFIDF_QUERY_ACC_MB=1: the batch is cut into several groups (one pass over the pairs
    each); the results are the default engine's.  64 queries at k = 10 fit one group at this
    size; k = 1024 (larger candidate lists) and 150 queries (over 64 per pass) do not."""
    args = (c2["data"], c2["off"], c2["p"]["doc_ids"], c2["p"]["ndocs_total"])
    engine.run_host(*args)
    cases = [(c2["qs"][:64], 10), (c2["qs"][:64], 1024), (c2["qs"][:150], 10)]
    want = [engine.query(q, k) for q, k in cases]
    default_groups = engine.query_info()["ngroups"]
    monkeypatch.setenv("TFIDF_QUERY_ACC_MB", "1")
    with tfidf_abi.Engine(0) as e:
        e.run_host(*args)
        for (q, k), w in zip(cases, want):
            got = e.query(q, k)
            check(got, c2["refs"][:len(q)], k)
            for name in ("nhits", "nmatch", "nterms_found", "doc"):
                assert np.array_equal(got[name], w[name])
            assert np.array_equal(bits(got["score"]), bits(w["score"]))
            groups = e.query_info()["ngroups"]
            if (len(q), k) != (64, 10):
                assert groups > 1
        assert groups == default_groups == 3     # 150 queries: 64 + 64 + 22 either way


def test_query_leaves_the_result_and_allocates_once(engine, c2):
    engine.run_host(c2["data"], c2["off"], c2["p"]["doc_ids"], c2["p"]["ndocs_total"])
    before = engine.text()
    first = engine.query(c2["qs"], 10)
    a0 = engine.alloc_counters()
    second = engine.query(c2["qs"], 10)
    assert engine.alloc_counters() == a0                          # no device allocation
    assert np.array_equal(first["doc"], second["doc"]) and np.array_equal(bits(first["score"]), bits(second["score"]))
    assert engine.text() == before
    res = engine.fetch()
    check(engine.query(c2["qs"][:20], 3), c2["refs"][:20], 3)
    assert res["output_txt"] == before


def test_group_query_equals_single_shard_reference(c2):
    K = 3
    shards = []
    for r in range(K):
        p = tfidf_configs.plan("c2", scale=0.002, rank=r, nranks=K)
        d, o = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
        shards.append((d, o, p["doc_ids"], p["ndocs_total"]))
    with tfidf_abi.Group(K, devices=[0] * K, local=True) as g:
        g.run_host(shards)
        for k in (3, 1024):
            check(g.query(c2["qs"], k), c2["refs"], k)
        # a rank alone ranks its own shard only, with the run's global-df scores
        own = set(shards[1][2].tolist())
        res = g.ranks[1].query(c2["qs"][:40], 10)
        for q, (hits, _) in enumerate(c2["refs"][:40]):
            mine = [(d, s) for d, s in hits if d in own]
            n = min(10, len(mine))
            assert int(res["nmatch"][q]) == len(mine)
            assert res["doc"][q, :n].tolist() == [d for d, _ in mine[:n]]
            assert np.array_equal(bits(res["score"][q, :n]), bits([s for _, s in mine[:n]]))


def test_query_errors(c2):
    with tfidf_abi.Engine(0) as e:
        with pytest.raises(tfidf_abi.TfidfError) as ex:
            e.query([b"x"], 3)
        assert ex.value.rc == tfidf_abi.E_STATE                    # before a run
        e.run_host(c2["data"], c2["off"], c2["p"]["doc_ids"], c2["p"]["ndocs_total"])
        for k in (0, 1025):
            with pytest.raises(tfidf_abi.TfidfError) as ex:
                e.query([b"x"], k)
            assert ex.value.rc == tfidf_abi.E_INVAL
        res = e.query([], 4)                                       # an empty batch is valid
        assert res["doc"].shape == (0, 4)
        check(e.query(c2["qs"][:5], 1024), c2["refs"][:5], 1024)


@pytest.mark.parametrize("extra", [[], ["--shards", "2"]])
def test_cli_query(tmp_path, extra):
    case = "g5_w3"
    g = load_golden(case)
    ora = oracle_py.run(g["data"], g["off"])
    ref = Ref(ora)
    qs = [q.replace(b"\n", b" ") for q in make_queries(ora, np.random.default_rng(9), 12)]
    shutil.copytree(os.path.join(GOLDEN, case, "input"), tmp_path / "input")
    (tmp_path / "q.txt").write_bytes(b"\n".join(qs))              # the last line has no newline
    p = subprocess.run([tfidf_abi.CLI_PATH, "--query", "q.txt", "--top", "3"] + extra, cwd=tmp_path,
                       capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    want = b"".join(b"q%d\tdoc%d\t%.16f\n" % (i + 1, d, s) for i, q in enumerate(qs) for d, s in ref.rank(q)[0][:3])
    assert want
    assert (tmp_path / "hits.txt").read_bytes() == want
    assert (tmp_path / "output.txt").read_bytes() == g["output"]
