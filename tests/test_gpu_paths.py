"""The engine's path switches against the oracle, each crossed by a corpus of a few MB.

engine.cpp switches code paths on V, N, the partial-record count and the table capacity
(tile sort / radix sort at SORT_TILE_MAXN = 131 072, narrow / wide K5 ranks at V = 2^21, the
full idf table up to 2^18 documents, k_tokcount_sl / k_tokcount_vs by table capacity, the
dense-merge budget).  A wrong rank on any of them still gives self-consistent output, so the
property checks of the full-size runs cannot see it; these tests compare integers, score
bits and text bytes with the oracle, and every test asserts from tfidf_last_run_info that it
took the path it is named for, so that a moved threshold fails the test instead of letting
it pass on the other side."""
import functools

import numpy as np
import pytest

import oracle_py
import tfidf_abi
import tfidf_configs
from helpers import docs_to_arrays
from test_gpu_parity import check_vs_oracle

pytestmark = pytest.mark.gpu

SORT_TILE_MAXN = 131072       # prims.h
IDF_FULL_MAX = 1 << 18        # engine.cpp
U32_MAX = 4294967295

_ALPHA = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)


def check_big_vs_oracle(engine, data, off, ids=None, n_total=0):
    """check_vs_oracle for millions of pairs: the text (which carries every pair's document,
    term and score) byte for byte, and the integer and score arrays bit for bit, on views of
    the fetched result (no per-pair Python lists)."""
    engine.run_host(data, off, ids, n_total)
    ora = oracle_py.run(data, off, ids, n_total)
    assert engine.text() == ora["output_txt"]
    with engine.fetched() as r:
        assert r["npairs"] == ora["npairs"] and r["nterms"] == ora["nterms"]
        for k in ("doc", "count", "docsize", "df"):
            assert np.array_equal(r[k], ora[k]), k
        assert np.array_equal(r["score"].view(np.uint64), ora["score"].view(np.uint64))
    return ora


def fixed_words(nums, width):
    """base-26 words of `width` letters for the integers `nums`: a (len, width) byte matrix
    whose rows order like the integers"""
    nums = np.asarray(nums, dtype=np.int64)
    m = np.empty((len(nums), width), dtype=np.uint8)
    for j in range(width - 1, -1, -1):
        m[:, j] = _ALPHA[nums % 26]
        nums = nums // 26
    return m


def corpus_of_tokens(words, tok, doc_ntok):
    """documents of fixed-width words: token t is the row words[tok[t]] followed by a blank
    (a newline at each document's end); doc_ntok[d] tokens in document d"""
    w = words.shape[1]
    m = np.empty((len(tok), w + 1), dtype=np.uint8)
    m[:, :w] = words[tok]
    m[:, w] = ord(" ")
    ends = np.cumsum(doc_ntok)
    m[ends[doc_ntok > 0] - 1, w] = ord("\n")
    off = np.zeros(len(doc_ntok) + 1, dtype=np.uint64)
    off[1:] = ends * (w + 1)
    return m.reshape(-1), off


def docs_covering(words, ndocs, rng, extra=8):
    """`ndocs` documents that together hold every word of the list at least once, a few
    random repeats in each"""
    docs = []
    for part in np.array_split(rng.permutation(len(words)), ndocs):
        toks = [words[i] for i in part] + [words[i] for i in rng.integers(0, len(words), extra)]
        rng.shuffle(toks)
        docs.append(b" ".join(toks) + b"\n")
    return docs


# ---------------------------------------------------------------- 1. vocabulary sort limit

def _tied_short_vocabulary(V, rng):
    """V distinct terms of at most 15 bytes that all start with "ab" (constant key bytes: the
    radix side's varying-byte mask), with a run of 6000 terms of 9-15 bytes tied on their
    first 8 bytes (launch_vocab_prefix_ties), a term that is its own 8-byte prefix, and a
    byte 0x01 after the shared prefix, which orders against the TAB that ends a term"""
    pre = b"abprefix"
    words = {b"abcdefg", b"abcdefgh", b"abcdefghi", pre, pre + b"\x01", pre + b"\x01a", pre + b"\x01\x01",
             pre + b"a", b"abprefi", b"ab"}
    while len(words) < 6000:
        L = int(rng.integers(1, 8))
        words.add(pre + bytes(_ALPHA[rng.integers(0, 26, L)]))
    assert sum(1 for w in words if w.startswith(pre) and 9 <= len(w) <= 15) >= 5000
    while len(words) < V:
        L = int(rng.integers(1, 12))
        words.add(b"ab" + bytes(_ALPHA[rng.integers(0, 26, L)]))
    return sorted(words)


@pytest.mark.parametrize("V", [SORT_TILE_MAXN, SORT_TILE_MAXN + 1])
def test_vocabulary_sort_limit(engine, V):
    """V = 131 072 is the last vocabulary the tile sort orders; V = 131 073 takes the u64 radix
    sort of the first 8 bytes over the varying bytes, then the prefix ties."""
    rng = np.random.default_rng(V)
    words = _tied_short_vocabulary(V, rng)
    res = check_vs_oracle(engine, *docs_to_arrays(docs_covering(words, 1500, rng)))
    assert engine.info()["nterms"] == V and res["nterms"] == V


# ----------------------------------------------------------------- 3. document ids and order

def test_document_ids_of_up_to_ten_digits(engine):
    """Ids of 1 to 10 digits up to 2^32 - 1, given in shuffled order: the "docN@" order keys
    and the emitted names (emit.hip doc_prefix)."""
    ids = np.array([1, 9, 10, 42, 99_999_999, 100_000_000, 429_496_729, 999_999_999, 1_000_000_000,
                    2_147_483_648, 4_294_967_294, 4_294_967_295], dtype=np.uint32)
    rng = np.random.default_rng(3)
    ids = ids[rng.permutation(len(ids))]
    docs = [b"id%d common w%d w%d\n" % (i, k % 3, k % 5) for k, i in enumerate(ids.tolist())]
    data, off = docs_to_arrays(docs)
    res = check_vs_oracle(engine, data, off, ids, U32_MAX)
    info = engine.info()
    assert info["ndocs"] == 12 and res["ndocs_total"] == U32_MAX
    assert res["output_txt"].startswith(b"doc1000000000@")   # strcmp order of the names, not numeric
    assert b"doc4294967295@id4294967295\t" in res["output_txt"]


@pytest.mark.parametrize("N", [SORT_TILE_MAXN, SORT_TILE_MAXN + 1])
def test_document_order_limit(engine, N):
    """N = 131 072 documents are ordered by the tile sort, 131 073 by the radix sort; the ids
    are a shuffled, non-contiguous set of 1 to 10 digits."""
    rng = np.random.default_rng(N)
    fixed = np.array([1, 9, 10, 99_999_999, 100_000_000, 999_999_999, 1_000_000_000, 2_147_483_648,
                      4_294_967_294, 4_294_967_295], dtype=np.uint64)
    pool = np.unique(np.concatenate([fixed, rng.integers(1, 10 ** 6, N // 2, dtype=np.uint64),
                                     rng.integers(10 ** 8, 10 ** 9, N // 2, dtype=np.uint64),
                                     rng.integers(10 ** 9, 1 << 32, N // 2, dtype=np.uint64)]))
    rest = np.setdiff1d(pool, fixed)
    ids = np.concatenate([fixed, rng.choice(rest, N - len(fixed), replace=False)])
    ids = ids[rng.permutation(N)].astype(np.uint32)
    assert len(np.unique(ids)) == N
    # one- or two-word documents over a small vocabulary
    words = fixed_words(np.arange(26 * 26), 2)
    two = rng.random(N) < 0.5
    ntok = 1 + two.astype(np.int64)
    tok = rng.integers(0, len(words), int(ntok.sum()))
    data, off = corpus_of_tokens(words, tok, ntok)
    res = check_vs_oracle(engine, data, off, ids, U32_MAX)
    assert engine.info()["ndocs"] == N
    assert res["npairs"] >= N


# ------------------------------------------------------------------ 4. partial-record merge

def _docs_of_many_terms(ndocs, nterms, ntok, seed):
    """documents of `ntok` 6-letter tokens over `nterms` distinct terms each"""
    rng = np.random.default_rng(seed)
    words = fixed_words(rng.choice(26 ** 6, 40000, replace=False), 6)
    toks = []
    for _ in range(ndocs):
        mine = rng.choice(len(words), nterms, replace=False)
        t = np.concatenate([mine, mine[rng.integers(0, nterms, ntok - nterms)]])
        rng.shuffle(t)
        toks.append(t)
    toks.append(np.arange(5))     # a small complete document beside them
    return corpus_of_tokens(words, np.concatenate(toks), np.array([len(t) for t in toks]))


def test_partial_merge_radix_side(engine):
    """Eight ~1 MB documents (split across chunks, below DENSE_DOC) of 20 000 distinct terms:
    more than SORT_TILE_MAXN partial records, sorted by the radix sort under the mask computed
    from N and V."""
    data, off = _docs_of_many_terms(8, 20000, 150_000, 41)
    assert np.diff(off.astype(np.int64)).max() < (4 << 20)
    check_vs_oracle(engine, data, off)
    assert engine.info()["partial_records"] > SORT_TILE_MAXN


def test_partial_merge_tile_side(engine):
    """The same shape with one 200 KB document: the partial records stay below the limit."""
    data, off = _docs_of_many_terms(1, 3000, 30_000, 42)
    check_vs_oracle(engine, data, off)
    assert 0 < engine.info()["partial_records"] <= SORT_TILE_MAXN


# ---------------------------------------------------------------------------- 5. idf table

@functools.lru_cache(maxsize=None)
def _many_df_corpus():
    """3000 documents over 400 terms whose document frequencies spread over 1..3000"""
    rng = np.random.default_rng(5)
    p = np.linspace(0.0005, 1.0, 400)
    docs = []
    for d in range(3000):
        pick = np.flatnonzero(rng.random(400) < p)
        docs.append(b" ".join(b"w%03d" % i for i in pick) + b" all\n")
    return docs_to_arrays(docs)


@pytest.mark.parametrize("n_total", [IDF_FULL_MAX, IDF_FULL_MAX + 1, 1 << 24, (1 << 24) + 1, U32_MAX])
def test_idf_table_limit(engine, n_total):
    """Up to 2^18 documents the host tabulates log(N / df) for every df; beyond, for the
    run's distinct df values only."""
    data, off = _many_df_corpus()
    res = check_vs_oracle(engine, data, off, None, n_total)
    distinct = len(np.unique(res["df"]))
    assert distinct > 300
    logs = engine.info()["idf_logs"]
    if n_total <= IDF_FULL_MAX:
        assert logs == n_total
    else:
        assert logs == distinct


# ------------------------------------------------------------------------ 6. wide-rank K5

@functools.lru_cache(maxsize=2)
def _wide_rank_corpus(V):
    """V distinct 5-letter words (row index = rank in term order) in ~3000 documents: every
    K5 class at its limits, a document of 300 consecutive ranks (one 9-bit rank bucket above
    K5_GROUP_MAX), one document split across chunks and two documents over 4 MiB."""
    rng = np.random.default_rng(V)
    words = fixed_words(np.sort(rng.choice(26 ** 5, V, replace=False)), 5)
    perm = rng.permutation(V)
    docs, at = [], 0

    def take(n):
        nonlocal at
        t = perm[at:at + n]
        at += n
        assert len(t) == n
        return t

    for _ in range(2):   # two documents over 4 MiB (6 bytes per token), some terms repeated
        t = take(700_100)
        docs.append(np.concatenate([t, t[rng.integers(0, len(t), 20_000)]]))
        assert 6 * len(docs[-1]) > (4 << 20)
    t = take(50_000)     # 360 KB: split across chunks, sorted merge
    docs.append(np.concatenate([t, t[:10_000]]))
    for n in (1, 64, 65, 1024, 1025, 2048, 4096, 4097):
        docs.append(take(n))
    r0 = int(rng.integers(0, V - 300))
    docs.append(np.concatenate([np.arange(r0, r0 + 300), perm[:40]]))   # the skewed document
    docs.extend(np.array_split(perm[at:], 3000))
    order = rng.permutation(len(docs))
    docs = [docs[i] for i in order]
    data, off = corpus_of_tokens(words, np.concatenate(docs), np.array([len(d) for d in docs]))
    return data, off, len(docs)


@pytest.mark.parametrize("V,n_total", [((1 << 21) + 1, 0), ((1 << 21) + 1, IDF_FULL_MAX + 1), (1 << 21, 0)])
def test_wide_rank_scores(V, n_total):
    """V = 2^21 + 1 is the first vocabulary whose term ranks do not fit beside K5's 11 index
    bits in a 32-bit key (k_score_wave<true, *>, the hand-off to a second k_score_large);
    with N <= 2^18 the idf comes by df, above by rank.  V = 2^21 is the last narrow one.  The
    table has 2^24 slots (k_tokcount_sl's half-size chunks).  With 4 * V * 16 bytes per dense
    document the dense budget holds one of the two documents over 4 MiB at V = 2^21 + 1, so
    the other takes the sorted merge."""
    data, off, ndocs = _wide_rank_corpus(V)
    with tfidf_abi.Engine(0) as e:
        ora = check_big_vs_oracle(e, data, off, None, n_total)
        info = e.info()
    assert info["nterms"] == V and ora["nterms"] == V
    assert info["ndocs"] == ndocs
    assert info["vocab_capacity"] == 1 << 24
    assert info["flags"] & tfidf_abi.RUN_K1_SL
    assert info["partial_records"] > SORT_TILE_MAXN
    assert info["idf_logs"] == (ndocs if n_total == 0 else len(np.unique(ora["df"])))


# ------------------------------------------------------------------- 7. table capacity

@functools.lru_cache(maxsize=None)
def _capacity_corpus():
    """c2 at scale 0.002 plus a few terms of 16 bytes or more and one document split across
    chunks"""
    p = tfidf_configs.plan("c2", scale=0.002)
    data, off = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
    rng = np.random.default_rng(9)
    split = b" ".join(bytes(_ALPHA[rng.integers(0, 26, int(rng.integers(1, 9)))]) for _ in range(40_000))
    extra = [b"internationalization supercalifragilisticexpialidocious internationalizations a\n",
             split + b"\n", b"supercalifragilisticexpialidocious z " + b"q" * 300 + b"\n"]
    assert len(split) > 3 * 49152
    x, xo = docs_to_arrays(extra)
    nid = int(p["doc_ids"].max()) + 1
    ids = np.concatenate([p["doc_ids"], np.arange(nid, nid + len(extra))]).astype(np.uint32)
    return (np.concatenate([data, x]), np.concatenate([off, off[-1] + xo[1:]]).astype(np.uint64), ids,
            p["ndocs_total"] + len(extra))


@pytest.mark.parametrize("vcap,sl_maxcap,sl", [(1 << 22, None, True), (1 << 23, None, True), (1 << 24, None, True),
                                               (1 << 25, None, True), (1 << 26, None, False),
                                               (1 << 21, 1 << 20, False)])
def test_table_capacity_switches(monkeypatch, vcap, sl_maxcap, sl):
    """k_tokcount_sl over tables of 2^22 slots (full-size chunks), 2^23 and 2^24 (half-size
    chunks; the 45 % load rule from 2^24) and 2^25 (the largest its LDS key addresses); above
    that, or above TFIDF_SL_MAXCAP, k_tokcount_vs is chosen automatically."""
    monkeypatch.setenv("TFIDF_VCAP", str(vcap))
    monkeypatch.delenv("TFIDF_K1", raising=False)
    if sl_maxcap:
        monkeypatch.setenv("TFIDF_SL_MAXCAP", str(sl_maxcap))
    data, off, ids, n_total = _capacity_corpus()
    with tfidf_abi.Engine(0) as e:
        check_vs_oracle(e, data, off, ids, n_total)
        info = e.info()
    assert info["vocab_capacity"] == vcap
    assert info["flags"] & tfidf_abi.RUN_K1_VS            # slot-keyed K1 either way
    assert bool(info["flags"] & tfidf_abi.RUN_K1_SL) == sl
    assert info["partial_records"] > 0
