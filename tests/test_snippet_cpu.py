"""Snippets on the host (no GPU): tfidf_result_snippet, the plain-C twin of the device path, against
tests/snippet_ref.py on the crafted corpus of tests/snippet_corpus.py and on every golden case, the
claim behind the candidate windows by brute force over every start, and tfidf_snippets_check's
rules.  Everything is compared exactly."""
import ctypes as C
import random

import numpy as np
import pytest

import snippet_corpus
import snippet_ref
import tfidf_abi
from conftest import golden_cases
from helpers import docs_to_arrays, load_golden


def term_table(docs):
    """a fetched result's term table: the corpus's terms in strcmp("word\\t") order"""
    return {"terms": sorted(snippet_ref.vocabulary(docs), key=lambda t: t + b"\t")}


@pytest.fixture(scope="module")
def crafted():
    docs, names = snippet_corpus.build()
    data, off = docs_to_arrays(docs)
    return {"docs": {i + 1: d for i, d in enumerate(docs)}, "data": data, "off": off, "res": term_table(docs)}


def test_abi():
    assert tfidf_abi.lib().tfidf_abi_version() == tfidf_abi.ABI_VERSION == 2
    for name in ("tfidf_snippets_check", "tfidf_snippets_free", "tfidf_snippet", "tfidf_group_snippet",
                 "tfidf_result_snippet", "tfidf_last_snippet_info"):
        assert name in tfidf_abi.EXPORTS and hasattr(tfidf_abi.lib(), name)
    assert C.sizeof(tfidf_abi.SnippetParams) == 32 and C.sizeof(tfidf_abi.SnippetInfo) == 112
    assert C.sizeof(tfidf_abi.Snippets) == 8 + 18 * 8


def test_check_bounds_and_their_neighbours():
    ok, bad = 0, tfidf_abi.E_INVAL
    assert tfidf_abi.lib().tfidf_snippets_check(None) == bad
    for w, rc in ((0, bad), (1, ok), (32, ok), (1024, ok), (1025, bad)):
        assert tfidf_abi.snippet_check(window=w) == rc, w
    for m, rc in ((0, ok), (1024, ok), (1025, bad)):
        assert tfidf_abi.snippet_check(max_marks=m) == rc, m
    assert tfidf_abi.snippet_check(size=31) == bad and tfidf_abi.snippet_check(size=24) == bad
    assert tfidf_abi.snippet_check(size=32) == ok and tfidf_abi.snippet_check(size=40) == ok
    assert tfidf_abi.snippet_check(flags=0) == ok and tfidf_abi.snippet_check(flags=1) == ok
    assert tfidf_abi.snippet_check(flags=2) == bad and tfidf_abi.snippet_check(flags=3) == bad
    for s, rc in ((0, ok), (1, bad), (65535, bad), (65536, ok), (1 << 40, ok)):
        assert tfidf_abi.snippet_check(scratch_bytes=s) == rc, s


@pytest.mark.parametrize("case", snippet_corpus.cases(), ids=lambda c: c[0])
def test_twin_on_the_crafted_corpus(crafted, case):
    name, jobs, W, M = case
    for text in (True, False):
        rows, qterms = snippet_ref.run(crafted["docs"], snippet_corpus.QUERIES, jobs, window=W, max_marks=M, text=text)
        got = tfidf_abi.result_snippets(crafted["res"], crafted["data"], crafted["off"], snippet_corpus.QUERIES, jobs,
                                        window=W, max_marks=M, text=text)
        snippet_ref.check(got, rows, qterms, name)


def test_twin_on_the_long_document(crafted):
    jobs = snippet_corpus.ones_jobs()
    rows, qterms = snippet_ref.run(crafted["docs"], snippet_corpus.QUERIES, jobs, window=32, max_marks=32)
    got = tfidf_abi.result_snippets(crafted["res"], crafted["data"], crafted["off"], snippet_corpus.QUERIES, jobs)
    snippet_ref.check(got, rows, qterms)
    assert rows[0]["nmatch"] == rows[0]["ntokens"] == 40000 and rows[0]["hits"] == 32


def test_the_crafted_corpus_holds_what_it_is_for(crafted):
    docs, names = snippet_corpus.build()
    assert [len(docs[names["edge_u%d" % s] - 1]) for s in snippet_corpus.SIZES] == list(snippet_corpus.SIZES)
    assert [len(docs[names["edge_a%d" % s] - 1]) for s in snippet_corpus.SIZES] == list(snippet_corpus.SIZES)
    off = crafted["off"]
    assert int(off[names["edge_u4096"] - 1]) % 16 == 7 and int(off[names["edge_a4096"] - 1]) % 16 == 0
    d = docs[names["edge_u8192"] - 1]
    base = int(off[names["edge_u8192"] - 1])
    starts = {p for p, _ in snippet_ref.tokens(d)}
    ends = {p + len(t) for p, t in snippet_ref.tokens(d)}
    edges = {4096 * k - x for k in (1, 2) for x in (0, base % 16)}
    assert {e - 1 for e in edges} & starts and edges & ends       # a token starts / ends in a tile's last byte
    assert any(p < e < p + len(t) for e in edges for p, t in snippet_ref.tokens(d))   # ... and one straddles
    by = {c[0]: c for c in snippet_corpus.cases()}
    rows, _ = snippet_ref.run(crafted["docs"], snippet_corpus.QUERIES, by["order"][1], window=5)
    cover, tie, clip0, clipT, _left = rows
    assert (cover["cover"], cover["hits"]) == (2, 2) and cover["win_tok"][0] > 5      # cover beats five hits
    assert tie["cover"] == 2 and tie["win_tok"] == (0, 5)                             # the earlier of two equal windows
    assert clip0["win_tok"] == (0, 5) and clipT["win_tok"] == (clipT["ntokens"] - 3, clipT["ntokens"])
    rows, _ = snippet_ref.run(crafted["docs"], snippet_corpus.QUERIES, by["t256"][1], window=8)
    assert rows[0]["flags"] == 0 and rows[0]["nmatch"] == 3                           # t255, t0, t7
    assert rows[1]["flags"] == snippet_ref.TRUNCATED and rows[1]["nmatch"] == 3       # t256 is term 257: no mark
    rows, _ = snippet_ref.run(crafted["docs"], snippet_corpus.QUERIES, by["nul"][1], window=4)
    assert rows[0]["nmatch"] == 4 and (0, 3, 0) in rows[0]["marks"] and any(m[1] == 0 for m in rows[0]["marks"])


@pytest.mark.parametrize("case", golden_cases())
def test_twin_on_the_golden_cases(case):
    g = load_golden(case)
    data, off = g["data"], g["off"]
    docs = {i + 1: bytes(data[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)}
    res = term_table(docs.values())
    rng = random.Random(len(docs))
    vocab = res["terms"]
    queries = [b" ".join(rng.sample(vocab, min(len(vocab), n)) + [b"absent%d" % n]) for n in (1, 2, 4, 7)]
    queries.append(b"absentword")
    jobs = [(q, d) for q in range(len(queries)) for d in list(docs) + [len(docs) + 1]]
    for W, M in ((3, 2), (32, 32)):
        rows, qterms = snippet_ref.run(docs, queries, jobs, window=W, max_marks=M)
        got = tfidf_abi.result_snippets(res, data, off, queries, jobs, window=W, max_marks=M)
        snippet_ref.check(got, rows, qterms, case)


def test_no_start_beats_the_match_positions():
    """the best (cover, hits) over every start s equals the best over the match positions, and after
    centring the recount finds the chosen window's own cover and hits (a match brought in on the
    left would have made a better candidate)"""
    rng = random.Random(11)
    for _ in range(300):
        T = rng.randint(1, 40)
        W = rng.randint(1, 12)
        nslots = rng.randint(1, 4)
        match = [(i, rng.randrange(nslots)) for i in range(T) if rng.random() < 0.3]
        if not match:
            continue
        s_all, best_all = snippet_ref.best_start(match, W, range(T))
        s_m, best_m = snippet_ref.best_start(match, W, [p for p, _ in match])
        assert best_all == best_m and s_m >= s_all
        doc = b" ".join(b"s%d" % dict(match)[i] if i in dict(match) else b"pad" for i in range(T))
        r = snippet_ref.snippet(doc, b" ".join(b"s%d" % s for s in range(nslots)), {b"s%d" % s for s in range(nslots)}, W, 32)
        assert (r["cover"], r["hits"]) == best_m


def test_errors():
    docs = [b"fox wolf", b"hen"]
    data, off = docs_to_arrays(docs)
    res = term_table(docs)
    for jobs in ([(1, 1)], [(0, 1), (7, 1)]):
        with pytest.raises(tfidf_abi.TfidfError) as e:
            tfidf_abi.result_snippets(res, data, off, [b"fox"], jobs)
        assert e.value.rc == tfidf_abi.E_INVAL
    with pytest.raises(tfidf_abi.TfidfError) as e:
        tfidf_abi.result_snippets(res, data, off, [b"fox"], [(0, 1)], window=0)
    assert e.value.rc == tfidf_abi.E_INVAL
    got = tfidf_abi.result_snippets(res, data, off, [b"fox"], [(0, 2), (0, 3), (0, 0), (0, 1)], doc_ids=np.array([3, 2]))
    assert got["flags"].tolist() == [0, 0, 1, 1] and got["nmatch"].tolist() == [0, 1, 0, 0]
