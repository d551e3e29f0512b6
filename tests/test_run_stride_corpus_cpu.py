"""What test_gpu_run_stride.py relies on, established without a GPU: k_plan_chunks restated
(run_stride_corpus.plan_chunks) at both chunk sizes, every non-empty chunk of the run-stride corpus
classified with the oracle's pairs per document, and the constants of the kernels' sources.

These are conditions on the corpus, not measurements.  Which persistent workgroup claims which
chunk is not deterministic, but with W workgroups at most W chunk executions are a workgroup's
first and at most W are its last.  A class of m chunks therefore has at least m - W members that
run on the LDS table a predecessor left behind and at least m - W whose state a successor reads.
With TFIDF_GRID_CUS=1, W = 4: m >= 12 puts at least 8 members on each side, whatever the order.
When a constant changes and one of these fails, the generator is what has to follow."""
import re

import numpy as np
import pytest

import oracle_py
import run_stride_corpus as RC
from helpers import docs_to_arrays

W = RC.K1_WG_PER_CU * 1            # K1's workgroups at TFIDF_GRID_CUS=1
CLASSES = ("last_few", "multi_group", "over_budget", "partial", "long_term", "hot")
TOKEN = re.compile(rb"[^ \t\n\v\f\r]+")


@pytest.fixture(scope="module")
def rc():
    c = RC.build()
    data, off = docs_to_arrays(c["docs"])
    ora = oracle_py.run(data, off)
    pairs = np.bincount(ora["doc"], minlength=len(c["docs"]) + 1)[1:]       # by document index
    long_starts = []                                                        # tokens whose term has >= 16 bytes
    for d, o in zip(c["docs"], off[:-1].tolist()):
        long_starts += [o + m.start() for m in TOKEN.finditer(d) if len(m.group().split(b"\0")[0]) >= 16]
    return dict(c=c, data=data, off=[int(x) for x in off], ora=ora, pairs=pairs, long_starts=np.array(sorted(long_starts)))


def classify(rc, cb):
    """per chunk: None when it is empty (cs == ce), else the set of its classes (and "after_empty")"""
    off, pairs, kinds = rc["off"], rc["pairs"], rc["c"]["kinds"]
    start, doc = RC.plan_chunks(off, cb)
    out = []
    for i in range(len(start) - 1):
        cs, ce, dfirst, dlast = start[i], start[i + 1], doc[i], doc[i + 1]
        if cs >= ce:
            out.append(None)
            continue
        k = set()
        ng = dlast + 1 - dfirst                                   # the kernel's count: the document of the next grid point included
        groups = [range(g, min(g + RC.GCAP, dlast + 1)) for g in range(dfirst, dlast + 1, RC.GCAP)]
        whole = lambda d: cs <= off[d] and off[d + 1] <= ce
        if len(groups[-1]) <= RC.FEW:
            k.add("last_few")
        if ng > RC.GCAP:
            k.add("multi_group")
        if any(sum(int(pairs[d]) for d in g if whole(d)) > RC.CLAIM_BUDGET for g in groups):
            k.add("over_budget")
        if off[dfirst] < cs or (off[dlast] < ce < off[dlast + 1]):
            k.add("partial")
        a, b = np.searchsorted(rc["long_starts"], [cs, ce])
        if b > a:
            k.add("long_term")
        if any(kinds[d] == "hot" and whole(d) for d in range(dfirst, dlast + 1)):
            k.add("hot")
        if i and out[-1] is None:
            k.add("after_empty")
        out.append(k)
    return out


def test_constants_are_the_sources():
    assert (RC.CHUNK_SL, RC.CHUNK_VS) == (24576, 12288) and RC.BIG_DOC == 49152
    assert (RC.GCAP, RC.FEW, RC.CLAIM_BUDGET, RC.K1_WG_PER_CU) == (256, 8, 3008, 4)
    assert (RC.K5_SMALL_DOC, RC.K5_WAVE, RC.K5_PS_SPLIT) == (128, 1024, 4096)
    assert W == 4


def test_plan_chunks_restated(rc):
    """the restatement on a hand-made layout: a small document, one of 30 000 bytes, one over BIG_DOC"""
    off = [5, 105, 30105, 30105, 90105]
    start, doc = RC.plan_chunks(off, 12288)
    # grid points 5, 12293, 24581, 36869, ..: in documents 0, 1, 1, 3 (the empty document 2 holds none), 3, ..
    assert doc[:4] == [0, 1, 1, 3] and start[:4] == [5, 105, 105, 36869]
    assert start[-1] == 90105 and doc[-1] == 3 and len(start) == -(-90100 // 12288) + 1
    assert all(a <= b for a, b in zip(start, start[1:]))


def test_corpus_is_deterministic_and_sized(rc):
    c, ora = rc["c"], rc["ora"]
    RC.build.cache_clear()
    assert RC.build()["docs"] == c["docs"]
    nbytes = rc["off"][-1]
    print("bytes", nbytes, "documents", len(c["docs"]), "pairs", ora["npairs"], "terms", ora["nterms"])
    assert 2_000_000 <= nbytes <= 2_600_000
    assert ora["nterms"] <= 60000                                 # the retry case's growth stays within the engine's attempts
    assert {15, 16, 17, 5000} <= {len(t) for t in ora["terms"]} and b"" in ora["terms"]
    assert all(len(d) <= RC.BIG_DOC for d, k in zip(c["docs"], c["kinds"]) if k != "split")
    assert all(len(d) > RC.BIG_DOC for d, k in zip(c["docs"], c["kinds"]) if k == "split")
    many = [len(d) for d, k in zip(c["docs"], c["kinds"]) if k == "many"]
    assert 25 <= sum(many) / len(many) <= 32 and many.count(0) >= 100


@pytest.mark.parametrize("cb", [RC.CHUNK_SL, RC.CHUNK_VS])
def test_every_chunk_class_outnumbers_the_workgroups(rc, cb):
    cl = classify(rc, cb)
    nchunks = len(cl)
    m = {k: sum(1 for x in cl if x and k in x) for k in CLASSES + ("after_empty",)}
    empty = sum(1 for x in cl if x is None)
    print(cb, "chunks", nchunks, "empty", empty, m)
    assert nchunks == -(-rc["off"][-1] // cb)
    for k in CLASSES:
        assert m[k] >= 12, (k, m)                                 # m - W >= 8 run behind a predecessor, 8 before a successor
    assert empty >= 8
    assert m["after_empty"] >= 8                                  # a claimed-ahead chunk with no work, then one with
    assert nchunks >= 10 * W
    assert nchunks >= 10 * 2 * RC.K1_WG_PER_CU                    # ... and at TFIDF_GRID_CUS=2
    # the kinds alternate: a few-document flush is followed (in chunk order) by every other class
    nxt = {k: set() for k in CLASSES}
    full = [x for x in cl if x]
    for a, b in zip(full, full[1:]):
        for k in a & set(CLASSES):
            nxt[k] |= b & set(CLASSES)
    assert nxt["last_few"] == set(CLASSES) and nxt["over_budget"] >= {"multi_group", "last_few", "long_term"}


def test_documents_for_the_score_stage_and_emit(rc):
    pairs, kinds = rc["pairs"], rc["c"]["kinds"]
    assert len(pairs) > 1 * 8 * 4                                 # emit: more documents than CUs x 8 workgroups x 4 waves
    assert len(pairs) > 256 * 8 * 4                               # ... also on the device's own count
    assert int((pairs > 64).sum()) >= 40                          # emit: multi-round documents, several per wave
    assert int(((pairs > 0) & (pairs <= RC.K5_SMALL_DOC)).sum()) >= 40
    assert int(((pairs > RC.K5_SMALL_DOC) & (pairs <= RC.K5_WAVE)).sum()) >= 40
    assert int((pairs > RC.K5_PS_SPLIT).sum()) >= 2               # chunk tasks of presorted documents
    tasks = sum(-(-int(p) // RC.K5_PS_SPLIT) for p, k in zip(pairs, kinds) if k == "split" and p > RC.K5_PS_SPLIT)
    assert tasks >= 2 * 4                                         # k_emit_split's CUs x 4 workgroups: two tasks each at one CU
    assert all(pairs[d] > RC.K5_PS_SPLIT or k != "split" or pairs[d] > RC.K5_WAVE for d, k in enumerate(kinds))
    assert int((pairs == 0).sum()) >= 100                         # empty and whitespace-only documents
    odd = [int(pairs[d]) for d, k in enumerate(kinds) if k == "odd"]
    assert 65 <= min(odd) and max(odd) <= 300
