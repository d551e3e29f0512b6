"""The window builder (helpers.windowed) and the oracle's reading of the corpus contract
(include/tfidf.h: document i is bytes[doc_off[i], doc_off[i+1]), bytes outside
[doc_off[0], doc_off[ndocs]) belong to no document): for every (lead, trail) pair the GPU
tests of test_gpu_corpus_windows.py use, the oracle on the windowed corpus equals the oracle
on the packed documents, and a letter touches the window on both sides."""
import numpy as np
import pytest

import oracle_py
from helpers import assert_same_result, docs_to_arrays, pad_after, pad_before, windowed
from test_gpu_corpus_windows import (CHUNKS_WINDOW, READBACK_WINDOW, edge_cases, packed_oracle, shared_buffer_docs)

WS = b" \t\n\v\f\r"


def check_window(docs, ora, lead, trail):
    data, off = windowed(docs, lead, trail)
    packed, poff = docs_to_arrays(docs)
    lo, hi = int(off[0]), int(off[-1])
    assert lo == lead and hi == lead + len(packed) and len(data) == hi + trail
    assert np.array_equal(off - np.uint64(lead), poff)
    assert data[lo:hi].tobytes() == packed.tobytes()
    # the edge bytes: a token extended over either boundary would swallow a letter
    if lead:
        assert bytes(data[lo - 1:lo]) not in WS and bytes(data[lo - 1:lo]).isalpha()
    if trail:
        assert bytes(data[hi:hi + 1]).isalpha()
    # the rest of the padding is whole words: counting it adds pairs
    assert lead < 4 or len(data[:lo].tobytes().split()) >= 2
    assert trail < 4 or len(data[hi:].tobytes().split()) >= 2
    win = oracle_py.run(data, off)
    assert_same_result(win, ora)
    assert win["output_txt"] == ora["output_txt"]


def test_padding_shapes():
    for n in range(0, 40):
        a, b = pad_before(n), pad_after(n)
        assert len(a) == n and len(b) == n
        if n:
            assert a[-1:].isalpha() and b[:1].isalpha()
        assert set(a.split()) | set(b.split()) <= {b"Qq", b"Q", b"q"}


def test_edge_windows_equal_packed():
    for name, lead, trail in edge_cases():
        docs, ora = packed_oracle(name)
        check_window(docs, ora, lead, trail)


@pytest.mark.parametrize("window", [CHUNKS_WINDOW, READBACK_WINDOW])
def test_chunk_windows_equal_packed(window):
    docs, ora = packed_oracle("chunks")
    check_window(docs, ora, *window)
    assert ora["npairs"] > 5000


def test_shared_buffer_ranks_equal_packed():
    """each rank's slice of the one windowed buffer gives its share of the packed result's text"""
    docs = shared_buffer_docs()
    ids = np.arange(100, 700, dtype=np.uint32)
    ora = oracle_py.run(*docs_to_arrays(docs), ids, 600)
    data, off = windowed(docs, *CHUNKS_WINDOW)
    texts = [oracle_py.run(data, off[200 * r:200 * (r + 1) + 1], ids[200 * r:200 * (r + 1)], 600, arrays=False)
             for r in range(3)]
    # df is per shard here (no exchange), so compare the lines' "docN@word" keys only
    keys = [ln.split(b"\t")[0] for t in texts for ln in t["output_txt"].splitlines()]
    assert keys == [ln.split(b"\t")[0] for ln in ora["output_txt"].splitlines()]
