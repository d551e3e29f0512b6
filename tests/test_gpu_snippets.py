"""Snippets on the device (tfidf_snippet / tfidf_group_snippet) against tests/snippet_ref.py, every
field exactly: the crafted documents of tests/snippet_corpus.py (tile edges at unaligned bases,
boundary documents, NUL and long terms, the ordering rules, mark limits, query shapes, job lists),
one document of 40 000 matching tokens under the default and a small scratch budget, one of 3 MB
over hundreds of tiles and select slices, invariants
against the run's own result on config 2, the calls that change the result, the states, and
groups of shards."""
import numpy as np
import pytest

import snippet_corpus as SC
import snippet_ref as R
import tfidf_abi
import tfidf_configs
from helpers import docs_to_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crafted():
    docs, names = SC.build()
    data, off = docs_to_arrays(docs)
    return {"docs": {i + 1: d for i, d in enumerate(docs)}, "list": docs, "names": names, "data": data, "off": off}


@pytest.fixture(scope="module")
def c2():
    p = tfidf_configs.plan("c2", scale=0.002)
    data, off = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
    docs = {int(i): bytes(data[int(off[k]):int(off[k + 1])]) for k, i in enumerate(p["doc_ids"])}
    vocab = sorted(R.vocabulary(docs.values()))
    rng = np.random.default_rng(5)
    queries = [b" ".join(vocab[int(i)] for i in rng.integers(0, len(vocab), 4)) for _ in range(24)]
    return dict(p=p, args=(data, off, p["doc_ids"], p["ndocs_total"]), docs=docs, vocab=set(vocab), queries=queries)


def same(a, b):
    for k in ("flags", "ntokens", "nmatch", "nterms_matched", "win_tok", "win_byte", "cover", "hits"):
        assert np.array_equal(a[k], b[k]), k
    assert a["marks"] == b["marks"] and a["text"] == b["text"] and a["qterms"] == b["qterms"]


@pytest.mark.parametrize("case", SC.cases(), ids=lambda c: c[0])
def test_crafted_cases(engine, crafted, case):
    name, jobs, W, M = case
    engine.run_host(crafted["data"], crafted["off"])
    for text in (True, False):
        rows, qterms = R.run(crafted["docs"], SC.QUERIES, jobs, window=W, max_marks=M, text=text)
        got = engine.snippets(SC.QUERIES, jobs, window=W, max_marks=M, text=text)
        R.check(got, rows, qterms, name)
    info = engine.snippet_info()
    assert info["njobs"] == len(jobs) and info["ntokens"] == sum(r["ntokens"] for r in rows)
    assert info["nmatches"] == sum(r["nmatch"] for r in rows)


def test_long_document_batches_and_growth(engine, crafted):
    """40 000 matching one-letter tokens: the match list crosses tiles and select slices.  A budget
    of 64 KiB holds 2048 records: the list grows once to the document's 40 000, and the jobs go in
    several sub-batches; the result is the default budget's"""
    jobs = SC.ones_jobs()
    engine.run_host(crafted["data"], crafted["off"])
    rows, qterms = R.run(crafted["docs"], SC.QUERIES, jobs)
    big = engine.snippets(SC.QUERIES, jobs)
    i0 = engine.snippet_info()
    R.check(big, rows, qterms)
    assert i0["nbatches"] == 1 and i0["nsubbatches"] == 1 and i0["nbig"] == 2 and i0["scratch_bytes"] == 256 << 20
    small = engine.snippets(SC.QUERIES, jobs, scratch_bytes=tfidf_abi.SNIP_MIN_SCRATCH)
    i1 = engine.snippet_info()
    same(small, big)
    assert i1["nsubbatches"] >= 3 and i1["scratch_bytes"] == 2 * 16 * 40000
    assert i1["ntokens"] == i0["ntokens"] and i1["nmatches"] == i0["nmatches"] == sum(r["nmatch"] for r in rows) > 80000
    # ... and with a tile budget under one job's tiles: every job its own batch
    jobs2 = [(0, crafted["names"]["edge_u%d" % s]) for s in SC.SIZES] * 700
    got = engine.snippets(SC.QUERIES, jobs2, window=8, scratch_bytes=tfidf_abi.SNIP_MIN_SCRATCH)
    assert engine.snippet_info()["nbatches"] >= 3
    rows, qterms = R.run(crafted["docs"], SC.QUERIES, jobs2, window=8)
    R.check(got, rows, qterms)


def test_one_document_over_many_tiles_and_slices(engine):
    """a document of about 3 MB between two small ones: about 800 tiles whose token ordinals and
    match places come from the scans, a match list of over 50 select slices, a window deep inside"""
    rng = np.random.default_rng(2)
    words = [b"w%d" % i for i in range(8)] + [b"x" * 16 + b"%d" % i for i in range(4)]
    big = b" ".join(words[int(i)] for i in rng.integers(0, len(words), 400000))
    docs = [b"w1 lead", big + b"\nw1 w2 w3 zebra w2 w1", b"tail w3"]
    data, off = docs_to_arrays(docs)
    engine.run_host(data, off)
    qs = [b"w1 w2 w3 zebra", b"w7", words[11] + b" nothere"]
    jobs = [(0, 2), (1, 2), (2, 2), (0, 3), (0, 1)]
    got = engine.snippets(qs, jobs, window=6, max_marks=6)
    info = engine.snippet_info()
    assert info["ntiles"] > 1500 and info["nbig"] == 3 and int(got["nmatch"][0]) > 50 * 1024
    rows, qterms = R.run({i + 1: d for i, d in enumerate(docs)}, qs, jobs, window=6, max_marks=6)
    R.check(got, rows, qterms)
    assert rows[0]["cover"] == 4 and rows[0]["win_tok"][0] > 399990
    same(engine.snippets(qs, jobs, window=6, max_marks=6, scratch_bytes=1 << 20), got)   # 32 768 records: it grows


def test_invariants_against_the_run(engine, c2):
    """independent of the reference: ntokens is the fetched doc_size, nmatch the sum of the fetched
    pair counts of the query's terms in the document, and a hit matched at least one term"""
    engine.run_host(*c2["args"])
    res = engine.fetch()
    size = dict(zip(res["doc_id"].tolist(), res["doc_size"].tolist()))
    count = {(int(d), res["terms"][int(t)]): int(c) for d, t, c in zip(res["doc"], res["term"], res["count"])}
    qs = c2["queries"]
    for hits in (engine.query(qs, k=5), engine.query_bm25(qs, k=5)):
        jobs = tfidf_abi.hits_to_jobs(hits)
        assert len(jobs) > 50
        got = engine.snippets(qs, hits=hits)
        for j, (q, d) in enumerate(jobs):
            assert int(got["ntokens"][j]) == size[d]
            terms = {t for _, t in R.query_terms(qs[q])[0]}
            assert int(got["nmatch"][j]) == sum(count.get((d, t), 0) for t in terms)
            assert int(got["nterms_matched"][j]) >= 1 and int(got["cover"][j]) >= 1
        rows, qterms = R.run(c2["docs"], qs, jobs, c2["vocab"])
        R.check(got, rows, qterms)
    must = [q.split()[0] for q in qs]
    hits = engine.query_clauses(must=must, should=qs, k=5)
    jobs = tfidf_abi.hits_to_jobs(hits)
    joined = [m + b" " + q for m, q in zip(must, qs)]
    got = engine.snippets(joined, jobs)
    for j, (q, d) in enumerate(jobs):      # the must term is slot 0 of the joined text, and the document holds it
        assert count.get((d, must[q]), 0) >= 1 and int(got["nterms_matched"][j]) >= 1
    rows, qterms = R.run(c2["docs"], joined, jobs, c2["vocab"])
    R.check(got, rows, qterms)
    only = engine.snippets(must, jobs)                           # every must term's slot is among the matched ones
    assert only["nterms_matched"].tolist() == [1] * len(jobs) and int(only["nmatch"].min()) >= 1


def test_after_prune_and_reweight(engine, c2):
    engine.run_host(*c2["args"])
    qs = c2["queries"][:8]
    jobs = tfidf_abi.hits_to_jobs(engine.query(qs, k=5))
    before = engine.snippets(qs, jobs)
    engine.reweight(tf="log", idf="smooth", norm="l2")
    same(engine.snippets(qs, jobs), before)                    # scores do not move a mark
    engine.prune(min_df=3)
    kept = set(engine.fetch()["terms"])
    assert kept < c2["vocab"]
    got = engine.snippets(qs, jobs)
    rows, qterms = R.run(c2["docs"], qs, jobs, kept)            # a removed word no longer marks
    R.check(got, rows, qterms)
    assert sum(r["nmatch"] for r in rows) < int(before["nmatch"].sum())


def test_after_analyze_offsets_fit_the_original(engine):
    """the analyzer keeps offsets: the marks found in the analysed corpus cut the words out of the
    original bytes at the same positions"""
    docs = [b"The Quick, brown FOX! jumps; over (the) lazy dog. A fox?", b"Wolf & Fox: never, EVER; trust a wolf."]
    data, off = docs_to_arrays(docs)
    engine.run_corpus(engine.analyze(data, off, lower=True, punct=True))
    adata = tfidf_abi.analyze_host(data, off, lower=True, punct=True)
    adocs = {i + 1: bytes(adata[int(off[i]):int(off[i + 1])]) for i in range(2)}
    qs, jobs = [b"fox wolf ever"], [(0, 1), (0, 2)]
    got = engine.snippets(qs, jobs, window=4)
    rows, qterms = R.run(adocs, qs, jobs, window=4)
    R.check(got, rows, qterms)
    cut = [[docs[d - 1][b:b + n] for b, n, _ in got["marks"][j]] for j, (_, d) in enumerate(jobs)]
    assert cut == [[b"FOX"], [b"Wolf", b"Fox", b"EVER"]]


def test_states_errors_and_allocations(crafted):
    jobs = [(0, d) for d in range(1, 12)]
    live = tfidf_abi.alloc_live()
    with tfidf_abi.Engine(0) as e:
        with pytest.raises(tfidf_abi.TfidfError) as ex:
            e.snippets(SC.QUERIES, jobs)
        assert ex.value.rc == tfidf_abi.E_STATE                 # before a run
        e.run_host(crafted["data"], crafted["off"])
        before = e.text()
        first = e.snippets(SC.QUERIES, jobs, window=8)
        a0 = e.alloc_counters()
        second = e.snippets(SC.QUERIES, jobs, window=8)
        assert e.alloc_counters() == a0                         # no device allocation
        same(first, second)
        assert e.text() == before
        for kw in (dict(window=0), dict(window=1025), dict(max_marks=1025), dict(flags=2), dict(size=24),
                   dict(scratch_bytes=100)):
            with pytest.raises(tfidf_abi.TfidfError) as ex:
                e.snippets(SC.QUERIES, jobs, **kw)
            assert ex.value.rc == tfidf_abi.E_INVAL, kw
        with pytest.raises(tfidf_abi.TfidfError) as ex:
            e.snippets(SC.QUERIES, [(len(SC.QUERIES), 1)])
        assert ex.value.rc == tfidf_abi.E_INVAL
        got = e.snippets(SC.QUERIES, [])
        assert got["flags"].shape == (0,) and len(got["qterms"]) == len(SC.QUERIES)
        model = e.model_export()
        e.model_import(model)
        with pytest.raises(tfidf_abi.TfidfError) as ex:
            e.snippets(SC.QUERIES, jobs)
        assert ex.value.rc == tfidf_abi.E_STATE                 # a model-only context has no corpus
    assert tfidf_abi.alloc_live() == live
    with tfidf_abi.Engine(0) as e:                              # a fresh context used for snippets only
        e.run_host(crafted["data"], crafted["off"])
        e.snippets(SC.QUERIES, jobs)
    assert tfidf_abi.alloc_live() == live


@pytest.mark.parametrize("K", [2, 3])
def test_group_equals_single_shard(engine, c2, K):
    qs = c2["queries"]
    engine.run_host(*c2["args"])
    jobs = tfidf_abi.hits_to_jobs(engine.query(qs, k=4)) + [(0, 10 ** 6)]
    single = engine.snippets(qs, jobs, window=16, max_marks=5)
    shards = []
    for r in range(K):
        p = tfidf_configs.plan("c2", scale=0.002, rank=r, nranks=K)
        d, o = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
        shards.append((d, o, p["doc_ids"], p["ndocs_total"]))
    with tfidf_abi.Group(K, devices=[0] * K, local=True) as g:
        g.run_host(shards)
        same(g.snippets(qs, jobs, window=16, max_marks=5), single)
        own = g.ranks[1].snippets(qs, jobs, window=16, max_marks=5)   # a rank alone: its documents, NO_DOC elsewhere
        held = set(shards[1][2].tolist())
        assert [int(f) & 1 for f in own["flags"]] == [0 if d in held else 1 for _, d in jobs]
