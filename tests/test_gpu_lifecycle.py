"""The context's lifecycle on the GPU (csrc/engine_ctx.h): nothing outlives a context, and a cache
kept per result is never served after the result changed.

Nothing outlives a context: tfidf_alloc_live (the engine's device allocations minus its frees,
process-wide) reads the same before a context is opened and after it is closed, whatever ran in
between.  Events, streams and pinned memory are not counted by that hook; the owning member types
cover them by construction.

A stale cache is never served: for each derivation the context caches (top-terms words: t_key /
t_len; similar: the norms; minhash: the term hashes; BM25: the length sum; the formatted text),
primed on corpus A, then one change of the result (a run of corpus B, a prune, a reweight, the
import of B's model), then the derivation again, compared with a fresh context that applied the
same change without the priming call.  A and B differ in N, V, ids and document lengths, so any of
A's cached values gives another answer.  All comparisons are exact: integers, bit patterns of
doubles, bytes."""
import numpy as np
import pytest

import tfidf_abi
from helpers import docs_to_arrays

pytestmark = pytest.mark.gpu

# six documents, non-contiguous ids, 14 distinct terms, one of 20 bytes, "the" in every document
A_DOCS = [b"the cat sat on the mat", b"the dog sat on the log", b"the cat chased the dog",
          b"the internationalization of the cat", b"the bird sang on the log log", b"the fish swam"]
A_IDS = [3, 7, 12, 20, 21, 40]
# four documents with other ids, 7 terms, other lengths
B_DOCS = [b"red green blue", b"red red yellow green pink", b"blue", b"white black red blue blue blue green"]
B_IDS = [5, 9, 100, 101]
UNSEEN = [b"red cat blue blue", b"green the pink zzz"]
QUERIES = [b"the cat", b"red blue", b"log"]
LABELS = [0, 1, 0, 1, 0, 1]


def corpus(docs, ids):
    data, off = docs_to_arrays(docs)
    return data, off, np.asarray(ids, dtype=np.uint32), len(docs)


A, B = corpus(A_DOCS, A_IDS), corpus(B_DOCS, B_IDS)


def same(got, want, what=""):
    """exact equality of two results: arrays by dtype, shape and bytes (doubles as bit patterns)"""
    if isinstance(want, dict):
        assert got.keys() == want.keys(), what
        for k in want:
            same(got[k], want[k], "%s[%s]" % (what, k))
    elif isinstance(want, np.ndarray):
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what
    else:
        assert got == want, what


def raises_state(fn, *args, **kw):
    with pytest.raises(tfidf_abi.TfidfError) as ex:
        fn(*args, **kw)
    assert ex.value.rc == tfidf_abi.E_STATE, ex.value


# ---- nothing outlives a context ----

def tour(e, tmp_path):
    """corpus A and every add-on call once; each is checked to have done something"""
    data, off, ids, n = A
    e.run_host(*A)
    assert e.query(QUERIES, 3)["nhits"].tolist()[1:] == [0, 2]          # B's words: none; "log": two documents
    assert e.query_bm25(QUERIES, 3)["nhits"].tolist()[1:] == [0, 2]
    assert sorted(e.top_terms(3)["doc"].tolist()) == A_IDS
    assert e.top_terms(2, docs=[7, 40, 999])["pos"][2] == 0xFFFFFFFF    # not held
    assert e.similar(2)["nnb"].sum() > 0 and len(e.similar(2, docs=[3, 21])["doc"]) == 2
    assert e.kmeans(2, nterms=3)["size"].sum() <= n and len(e.kmeans(2, nterms=3)["words"]) == 2
    assert e.minhash()["sig"].shape[0] == n and e.near_dups(0.3)["ndocs"] == n
    e.nb_fit(A_IDS, LABELS, 2)
    assert len(e.nb_predict()["label"]) == n and set(e.nb_predict(docs=[3, 12])["label"].tolist()) <= {0, 1}
    assert set(e.transform(*docs_to_arrays(UNSEEN))["words"]) == {b"cat", b"the"}   # B's words are unseen here
    assert e.analyze(data, off, lower=True, punct=True).ndocs == n and e.ngrams(data, off, 1, 2).ndocs == n
    model = e.model_export()
    assert len(model["terms"]) == 14
    with tfidf_abi.Engine(0) as e2:                                      # a second context beside the first
        e2.model_import(model)
        assert set(e2.transform(*docs_to_arrays(UNSEEN))["words"]) == {b"cat", b"the"}
    text = e.text()
    e.write_output(str(tmp_path / "out.txt"))
    assert text and (tmp_path / "out.txt").read_bytes() == text
    assert e.reweight(tf="log", norm="l2")["changed"] == 1
    assert e.prune(min_df=2)["nterms_after"] == 6


def test_nothing_outlives_a_context_that_ran_everything(tmp_path):
    before = tfidf_abi.alloc_live()
    with tfidf_abi.Engine(0) as e:
        tour(e, tmp_path)
        during = tfidf_abi.alloc_live()
        assert during[0] > before[0] and during[1] > before[1]
    assert tfidf_abi.alloc_live() == before


def test_nothing_outlives_a_context_that_ran_nothing():
    before = tfidf_abi.alloc_live()
    with tfidf_abi.Engine(0):
        assert tfidf_abi.alloc_live()[0] > before[0]
    assert tfidf_abi.alloc_live() == before


def test_nothing_outlives_a_group_of_two_ranks():
    before = tfidf_abi.alloc_live()
    with tfidf_abi.Group(2, devices=[0, 0], local=True) as g:
        g.run_host([corpus(A_DOCS[:3], A_IDS[:3])[:3] + (6,), corpus(A_DOCS[3:], A_IDS[3:])[:3] + (6,)])
        assert [r.info()["ndocs"] for r in g.ranks] == [3, 3] and g.ranks[0].info()["nterms_global"] == 14
        assert tfidf_abi.alloc_live()[0] > before[0]
    assert tfidf_abi.alloc_live() == before


# ---- a stale cache is never served ----

DERIVED = {
    "tmeta": lambda e: e.top_terms(3),
    "norm": lambda e: e.similar(2),
    "h0": lambda e: e.minhash(nhashes=16, seed=7),
    "bm25_L": lambda e: e.query_bm25(QUERIES, 3),
    "text": lambda e: e.text(),
}


@pytest.fixture(scope="module")
def model_b():
    with tfidf_abi.Engine(0) as e:
        e.run_host(*B)
        return e.model_export()


@pytest.fixture(scope="module")
def changes(model_b):
    return {
        "run_b": lambda e: e.run_host(*B),
        "prune": lambda e: e.prune(min_df=2),
        "reweight": lambda e: e.reweight(tf="log", idf="ref", norm="l2"),
        "import": lambda e: e.model_import(model_b),
    }


@pytest.fixture(scope="module")
def fresh(changes):
    """per change: what a context that ran A and applied the change, with nothing primed, answers"""
    want = {}
    for name, change in changes.items():
        with tfidf_abi.Engine(0) as e:
            e.run_host(*A)
            change(e)
            if name == "import":
                want[name] = e.transform(*docs_to_arrays(UNSEEN))
            else:
                want[name] = {d: fn(e) for d, fn in DERIVED.items()}
    # the changes change something: every answer differs from A's own, and B's model knows B's words
    with tfidf_abi.Engine(0) as e:
        e.run_host(*A)
        own = {d: fn(e) for d, fn in DERIVED.items()}
    differ = {"run_b": list(DERIVED), "prune": ["tmeta", "norm", "h0", "text"], "reweight": ["tmeta", "norm", "text"]}
    for name, ds in differ.items():   # (a prune and a reweight leave BM25 alone, a reweight the hashes)
        for d in ds:
            with pytest.raises(AssertionError):
                same(want[name][d], own[d])
    assert sorted(set(want["import"]["words"])) == [b"blue", b"green", b"pink", b"red"]
    return want


@pytest.mark.parametrize("change", ["run_b", "prune", "reweight", "import"])
@pytest.mark.parametrize("derived", list(DERIVED))
def test_a_primed_cache_is_not_served_after_a_change(changes, fresh, derived, change):
    with tfidf_abi.Engine(0) as e:
        e.run_host(*A)
        DERIVED[derived](e)                          # prime on A
        changes[change](e)
        if change == "import":                       # no pairs any more; the model is B's
            raises_state(DERIVED[derived], e)
            same(e.transform(*docs_to_arrays(UNSEEN)), fresh[change], "transform")
        else:
            same(DERIVED[derived](e), fresh[change][derived], derived)


@pytest.mark.parametrize("change", ["run_b", "prune", "reweight", "import"])
def test_the_classifier_after_a_change(changes, change):
    with tfidf_abi.Engine(0) as e:
        e.run_host(*A)
        e.nb_fit(A_IDS, LABELS, 2)
        before = e.nb_predict(all_scores=True)
        changes[change](e)
        if change == "reweight":                     # the counts, the ranks and the documents stay: so does the model
            same(e.nb_predict(all_scores=True), before, "nb_predict")
        else:
            raises_state(e.nb_predict)
