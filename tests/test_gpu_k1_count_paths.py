"""K1's two LDS count paths (tokcount_sl.hip): lds_count settles a key with one CAS at its
preferred slot, and a key whose preferred slot holds another key is pushed on the wave's
stack and counted by lds_count_full, 64 at a time and once more before the flush.  Every
case is compared with the oracle exactly (counts, docSize, df, score bits, text), at the
smallest shapes where the hand-over between the two paths can go wrong.

A document of at most BIG_DOC (48 KiB) is never split (k_plan_chunks moves the chunk start
to the document's start), so each single-document case below is one chunk and one group
whatever its size."""
import functools

import numpy as np
import pytest

import oracle_py
import tfidf_abi
from helpers import assert_same_result, docs_to_arrays

pytestmark = pytest.mark.gpu


def check_vs_oracle(engine, data, off, ids=None, n_total=0):
    engine.run_host(data, off, ids, n_total)
    res = engine.fetch()
    ora = oracle_py.run(data, off, ids, n_total)
    assert_same_result(res, ora)
    assert res["output_txt"] == ora["output_txt"]
    assert engine.text() == ora["output_txt"]
    return res


def _distinct_words(n, rng, lo=2, hi=12):
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    words = set()
    while len(words) < n:
        L = int(rng.integers(lo, hi + 1))
        words.add(bytes(alpha[rng.integers(0, 26, L)]))
    return sorted(words)


@functools.lru_cache(maxsize=None)
def repeated_terms_corpus(nterms, twice_only):
    """One document of `nterms` distinct 3-6-byte terms, each two (or two or three) times, in
    shuffled order: about 5.5 bytes a token, 32-40 KB, one chunk and one group."""
    rng = np.random.default_rng(nterms)
    words = _distinct_words(nterms, rng, 3, 6)
    reps = np.full(nterms, 2) if twice_only else rng.integers(2, 4, nterms)
    toks = np.repeat(np.arange(nterms), reps)
    rng.shuffle(toks)
    doc = b" ".join(words[i] for i in toks) + b"\n"
    assert len(doc) <= 49152
    return docs_to_arrays([doc])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129, 200])
def test_round_and_drain_edges(engine, n):
    """The group's last partial round, a stack below 64 at the final drain, the 64 crossing."""
    rng = np.random.default_rng(100 + n)
    words = _distinct_words(n, rng, 2, 5)
    res = check_vs_oracle(engine, *docs_to_arrays([b" ".join(words[i] for i in rng.permutation(n)) + b"\n"]))
    assert res["npairs"] == n


def test_displaced_keys_without_overflow(engine):
    """2 900 distinct terms in one group: below the 3 008-claim budget, the table up to 80 %
    full, so hundreds of keys are displaced; duplicates arrive on both paths and the same
    key is pushed more than once between drains."""
    res = check_vs_oracle(engine, *repeated_terms_corpus(2900, False))
    assert res["npairs"] == 2900


def test_overflow_mode_with_deferred_keys(engine):
    """3 400 distinct terms x 2: the waves cross WAVE_CLAIMS while keys are still deferred;
    those become partial records and are merged."""
    res = check_vs_oracle(engine, *repeated_terms_corpus(3400, True))
    assert res["npairs"] == 3400


def hot_key_corpus():
    """(data, off, tokens of the document)"""
    rng = np.random.default_rng(5)
    words = _distinct_words(501, rng, 3, 6)
    hot, others = words[250], words[:250] + words[251:]
    toks = []
    while sum(len(t) + 1 for t in toks) < 20000:
        toks += [hot, others[int(rng.integers(0, 500))]]
    return docs_to_arrays([b" ".join(toks) + b"\n"]) + (len(toks),)


def test_hot_key_from_all_waves(engine):
    """One term is every second token of a 20 KB document, between 500 distinct others: all
    four waves count it at one slot."""
    data, off, ntoks = hot_key_corpus()
    res = check_vs_oracle(engine, data, off)
    assert int(np.max(res["count"])) == ntoks // 2


def many_documents_corpus(ndocs):
    rng = np.random.default_rng(ndocs)
    pool = _distinct_words(200, rng, 1, 2)
    docs = [b" ".join(pool[i] for i in rng.integers(0, 200, int(rng.integers(28, 33)))) + b"\n" for _ in range(ndocs)]
    return docs_to_arrays(docs)


@pytest.mark.parametrize("ndocs", [9, 255, 256, 257, 600])
def test_many_documents_per_group(engine, ndocs):
    """About 30 tokens a document from a 200-word pool of 1-2-byte words (about 87 bytes a
    document): up to 257 documents are one 24 KiB chunk (the general flush, one group of GCAP
    = 256 documents and one over it), 600 are three chunks of more than GCAP documents each
    (several groups per chunk: the stack's per-group reset)."""
    check_vs_oracle(engine, *many_documents_corpus(ndocs))


def test_displaced_keys_wider_slot_field(monkeypatch):
    """The 2 900-term document over a vocabulary table of 2^24 slots: the key's slot field
    grows and its document field shrinks.  Past 2^22 slots the engine launches the kernel's
    other instance (the full count in every round, no stack), so this is that instance's
    case at the same table load."""
    monkeypatch.setenv("TFIDF_VCAP", str(1 << 24))
    monkeypatch.delenv("TFIDF_K1", raising=False)
    with tfidf_abi.Engine(0) as e:
        res = check_vs_oracle(e, *repeated_terms_corpus(2900, False))
        info = e.info()
    assert res["npairs"] == 2900
    assert info["vocab_capacity"] == 1 << 24
    assert info["flags"] & tfidf_abi.RUN_K1_SL
