"""Corpus windows (include/tfidf.h): doc_off[0] > 0, doc_off[ndocs] < nbytes, a caller-owned
device buffer at any alignment, and several ranks reading their documents from one buffer.

Every tokenize+count (K1) kernel instance masks the bytes outside [doc_off[0], doc_off[ndocs])
in its own way, k_plan_chunks starts its chunks at doc_off[0] + i * chunk bytes, the engine
takes the general kernel for a corpus base that is not 16-byte aligned, and long terms are
read back from the corpus by absolute offset (emit.hip, k_terms_words, the query lookup).

The reference everywhere is the oracle on the PACKED documents (helpers.docs_to_arrays), which
knows nothing of windows.  The bytes around a window are words of their own with a letter
touching the window on both sides (helpers.windowed), so a token extended over a boundary and
a byte counted outside the window both change counts, docSize and the text."""
import functools

import numpy as np
import pytest

import oracle_py
import tfidf_abi
from helpers import assert_k1_instance, assert_same_result, device_corpus, docs_to_arrays, k1_fixture, windowed

pytestmark = pytest.mark.gpu

k1 = k1_fixture(["sl_fast", "sl_full", "vs", "general"])

T40 = b"window_edge_term_of_exactly_forty_bytes_"
T40_FIRST = b"the_first_token_of_the_corpus_and_long__"
T40_LAST = b"the_last_token_of_the_corpus_no_blank___"
T40_ABSENT = b"a_forty_byte_term_no_document_contains__"
assert len(T40) == len(T40_FIRST) == len(T40_LAST) == len(T40_ABSENT) == 40

# lo inside the first 16-byte block (tokcount_sl's rb == 0 with lo_rel > 0), exactly on a
# block (rb == 0, the block before the chunk base is padding) and past two blocks (rb > 0)
EDGE_LEADS = [1, 3, 15, 16, 17, 33]
# hi == nbytes at varying nbytes % 16; hi one byte short of nbytes; a whole block of padding
# (and more) behind hi
EDGE_TRAILS = [0, 1, 15, 16, 17]
CHUNKS_WINDOW = (5, 7)      # every nominal chunk start lo + i * chunk bytes is odd
READBACK_WINDOW = (37, 7)
ONE_BLOCK_WINDOW = (3, 8)   # lead, b"ab cd", trail: 16 bytes in all
EMPTY_WINDOW = (5, 7)       # three empty documents: lo == hi == 5


def edge_docs(variant: str):
    """About 200 bytes in six documents: an empty first and an empty last document, a first
    token at lo, a last token ending at hi with no whitespace behind it, a NUL-cut token, and
    one 40-byte term that is the first token at lo ("long_first") or the last token at hi
    ("long_last")."""
    head = T40 if variant == "long_first" else b"ab"
    tail = T40 if variant == "long_last" else b"cd"
    docs = [b"",
            head + b" ab cd\tab q\n",
            b"ab\x00cd ef \x00zz a\x01 Qq\n",
            b"ef  gh ab",                                  # no separator before the next document
            b"xy ab cd ef\nzz Q sixteen_bytes_term " + tail,
            b""]
    assert docs[1].startswith(head) and docs[4].endswith(tail)
    return docs


EDGE_VARIANTS = ["long_first", "long_last"]


@functools.lru_cache(maxsize=None)
def chunks_docs():
    """About 160 KB: ~60 KB of 100-300-byte documents (a third without a trailing separator)
    around one 100 KB document of 1-40-byte tokens over {a, b, c}, which exceeds BIG_DOC, is
    split mid-token and gives partial records.  T40_FIRST's first occurrence is the corpus's
    first token, T40_LAST's only occurrence is its last token (nothing behind it)."""
    rng = np.random.default_rng(2024)
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    pool = sorted({bytes(alpha[rng.integers(0, 26, int(rng.integers(2, 13)))]) for _ in range(400)})
    pool += [b"a_term_of_sixteen", b"a_term_of_sixteen_and_more", T40_FIRST]

    def small():
        toks = []
        want = int(rng.integers(100, 300))
        while sum(len(t) + 1 for t in toks) < want:
            toks.append(pool[int(rng.integers(0, len(pool)))])
        sep = b"" if rng.random() < 0.33 else (b"\n" if rng.random() < 0.8 else b" \t\n")
        return b" ".join(toks) + sep

    parts, n = [], 0
    while n < 100_000:
        w = bytes(rng.integers(97, 100, int(rng.integers(1, 41)), dtype=np.uint8))
        sep = b" " if rng.random() < 0.9 else b"\n\t "
        parts.append(w + sep)
        n += len(w) + len(sep)
    before = [small() for _ in range(150)]
    after = [small() for _ in range(150)]
    docs = [T40_FIRST + b" " + before[0]] + before[1:] + [b"".join(parts)] + after + [b"closing words " + T40_LAST]
    assert 140_000 < sum(len(d) for d in docs) < 200_000
    return docs


@functools.lru_cache(maxsize=None)
def packed_oracle(name: str):
    """the oracle on the packed documents: computed once per corpus, never changed"""
    if name in EDGE_VARIANTS:
        docs = edge_docs(name)
    elif name == "one_block":
        docs = [b"ab cd"]
    elif name == "empty":
        docs = [b"", b"", b""]
    else:
        assert name == "chunks"
        docs = chunks_docs()
    return docs, oracle_py.run(*docs_to_arrays(docs))


def edge_cases():
    """(corpus name, lead, trail) of test_window_edges"""
    cases = [(v, lead, trail) for v in EDGE_VARIANTS for lead in EDGE_LEADS for trail in EDGE_TRAILS]
    return cases + [("one_block",) + ONE_BLOCK_WINDOW, ("empty",) + EMPTY_WINDOW]


def check_result(e, ora, lo, hi, what):
    res = e.fetch()
    assert_same_result(res, ora)
    assert res["output_txt"] == ora["output_txt"], what
    assert e.text() == ora["output_txt"], what
    info = e.info()
    assert info["nbytes"] == hi - lo, what
    assert info["ntokens"] == int(ora["count"].sum()), what
    return info


def test_window_edges(k1):
    instance, e = k1
    for name, lead, trail in edge_cases():
        docs, ora = packed_oracle(name)
        data, off = windowed(docs, lead, trail)
        e.run_host(data, off)
        info = check_result(e, ora, int(off[0]), int(off[-1]), (name, lead, trail))
        if name != "empty":     # an empty window launches no K1 at all
            assert_k1_instance(info, instance)
        else:
            assert info["npairs"] == 0 and int(off[0]) == int(off[-1]) > 0


def test_window_over_chunks(k1):
    instance, e = k1
    docs, ora = packed_oracle("chunks")
    data, off = windowed(docs, *CHUNKS_WINDOW)
    assert int(off[0]) % 2 == 1
    e.run_host(data, off)
    info = check_result(e, ora, int(off[0]), int(off[-1]), instance)
    assert_k1_instance(info, instance)
    assert info["nchunks"] >= (3 if instance == "sl_fast" else 5)
    assert info["partial_records"] > 0


def _run_device(monkeypatch, k1_mode, shift):
    """the chunks corpus from a caller-owned device buffer whose base is `shift` bytes past a
    16-byte boundary"""
    docs, ora = packed_oracle("chunks")
    data, off = windowed(docs, *CHUNKS_WINDOW)
    for k in ("TFIDF_K1", "TFIDF_VCAP", "TFIDF_SL_MAXCAP"):
        monkeypatch.delenv(k, raising=False)
    if k1_mode:
        monkeypatch.setenv("TFIDF_K1", k1_mode)
    with tfidf_abi.Engine(0) as e, device_corpus(data, off, shift=shift) as c:
        assert c.bytes % 16 == shift
        e.run_corpus(c)
        return check_result(e, ora, int(off[0]), int(off[-1]), (k1_mode, shift))


@pytest.mark.parametrize("shift", [0, 1, 8, 15])
def test_device_base_shift(shift, monkeypatch):
    """An aligned base takes k_tokcount_sl; any other takes the general kernel by itself."""
    info = _run_device(monkeypatch, None, shift)
    if shift == 0:
        assert_k1_instance(info, "sl_fast")
    else:
        assert info["flags"] & tfidf_abi.RUN_K1_VS == 0
        assert_k1_instance(info, "general")
    assert info["nchunks"] >= 3


def test_device_base_shift_overrides_k1_vs(monkeypatch):
    """TFIDF_K1=vs asks for a kernel that needs an aligned base: an unaligned one still takes
    the general kernel."""
    info = _run_device(monkeypatch, "vs", 1)
    assert info["flags"] & tfidf_abi.RUN_K1_VS == 0
    assert_k1_instance(info, "general")


def test_long_terms_read_back_through_a_window(engine):
    """top_terms gathers its words, and query compares its long terms, from the caller's
    buffer at absolute offsets (not offsets from doc_off[0])."""
    import test_gpu_query
    import test_gpu_terms
    docs, ora = packed_oracle("chunks")
    data, off = windowed(docs, *READBACK_WINDOW)
    with device_corpus(data, off, shift=0) as c:
        engine.run_corpus(c)
        info = check_result(engine, ora, int(off[0]), int(off[-1]), "read back")
        assert_k1_instance(info, "sl_fast")
        tref = test_gpu_terms.Ref(ora, range(1, len(docs) + 1))
        test_gpu_terms.check(engine.top_terms(3), tref.rows(), 3, test_gpu_terms.pair_index(engine.fetch()))
        assert any(len(w) >= 16 for _, _, r in tref.rows() for w, _, _ in r[:3])   # long words were gathered
        qref = test_gpu_query.Ref(ora)
        queries = [T40_FIRST, T40_LAST, T40_ABSENT, T40_LAST + b" " + T40_FIRST + b" " + T40_ABSENT]
        refs = [qref.rank(q) for q in queries]
        assert [n for _, n in refs] == [1, 1, 0, 2]
        for k in (1, 10):
            test_gpu_query.check(engine.query(queries, k), refs, k)


def shared_buffer_docs():
    """600 documents of about 30 tokens, none with a trailing separator, over 300 short words
    and a few terms of 16 bytes or more that occur on every rank"""
    rng = np.random.default_rng(600)
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    pool = sorted({bytes(alpha[rng.integers(0, 26, int(rng.integers(1, 9)))]) for _ in range(300)})
    pool += [b"exactly_16_bytes", b"seventeen_bytes_x", b"a_long_term_shared_by_every_rank", T40]
    docs = [b" ".join(pool[i] for i in rng.integers(0, len(pool), int(rng.integers(28, 33)))) for _ in range(600)]
    assert not any(d[-1:].isspace() for d in docs)
    return docs


def test_group_ranks_share_one_resident_buffer():
    """Three in-process ranks over ONE device buffer: the same bytes and nbytes, each rank's
    doc_off / doc_ids pointing at its first document in the one offsets / ids array, so rank
    r's hi is rank r+1's lo and the neighbour's bytes lie directly behind each window."""
    from test_gpu_multirank import _concat
    K, per = 3, 200
    docs = shared_buffer_docs()
    ids = np.arange(100, 100 + K * per, dtype=np.uint32)     # "doc100".."doc699": numeric = strcmp order
    ora = oracle_py.run(*docs_to_arrays(docs), ids, K * per)
    data, off = windowed(docs, *CHUNKS_WINDOW)
    with device_corpus(data, off, ids, K * per) as c:
        shards = []
        for r in range(K):
            s = tfidf_abi.Corpus()
            s.bytes, s.nbytes, s.flags, s.ndocs_total = c.bytes, c.nbytes, c.flags, K * per
            s.doc_off = c.doc_off + 8 * per * r
            s.doc_ids = c.doc_ids + 4 * per * r
            s.ndocs = per
            shards.append(s)
        with tfidf_abi.Group(K, devices=[0] * K) as g:
            g.run(shards)
            texts = [e.text() for e in g.ranks]
            res = [e.fetch() for e in g.ranks]
            infos = [e.info() for e in g.ranks]
    assert b"".join(texts) == ora["output_txt"]
    assert_same_result(_concat(res), ora)
    assert all(i["nterms_global"] == ora["nterms"] for i in infos)
    for r, i in enumerate(infos):
        assert i["nbytes"] == int(off[per * (r + 1)]) - int(off[per * r])
        assert_k1_instance(i, "sl_fast")
