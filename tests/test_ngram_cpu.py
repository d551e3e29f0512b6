"""tfidf_ngrams_host and tfidf_ngram_check (include/tfidf.h, section "n-grams";
csrc/ngram_host.c) against tests/ngram_ref.py, the definition in plain Python.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import ngram_ref
import oracle_py
import tfidf_abi
from helpers import load_golden, windowed


@pytest.fixture(scope="module")
def big():
    return windowed(ngram_ref.big_corpus(), 37, 21)


def test_literals():
    data, off = ngram_ref.LITERAL
    for (lo, hi), (want, want_off) in ngram_ref.LITERAL_OUT.items():
        got, got_off = tfidf_abi.ngrams_host(np.frombuffer(data, dtype=np.uint8), off, lo, hi)
        assert bytes(got) == want and got_off.tolist() == want_off
        assert ngram_ref.ngrams(data, off, lo, hi) == (want, want_off)


@pytest.mark.parametrize("rng", ngram_ref.RANGES)
def test_host_against_reference(big, rng):
    data, off = big
    want, want_off = ngram_ref.ngrams(data, off, *rng)
    got, got_off = tfidf_abi.ngrams_host(data, off, *rng)
    assert got_off.tolist() == want_off
    assert bytes(got) == want
    assert len(want) > 100_000
    # grams = sum over documents and n of max(0, m - n + 1): every gram ends in exactly one blank
    ntok, ngr = ngram_ref.counts(data, off, *rng)
    assert ntok > 20_000 and want.count(b" ") == ngr


def test_joiner(big):
    data, off = big
    for j in (0x2B, 0x01, 0xFF):
        got, got_off = tfidf_abi.ngrams_host(data[:5000], [40, 1000, 1000, 4990], 2, 3, j)
        assert (bytes(got), got_off.tolist()) == ngram_ref.ngrams(data[:5000], [40, 1000, 1000, 4990], 2, 3, j)
    a = tfidf_abi.ngrams_host(data[:5000], [40, 4990], 1, 2, 0)
    b = tfidf_abi.ngrams_host(data[:5000], [40, 4990], 1, 2, 0x5F)
    assert bytes(a[0]) == bytes(b[0])


def test_unigrams_are_the_tokens(big):
    data, off = big
    got, got_off = tfidf_abi.ngrams_host(data, off, 1, 1)
    toks = ngram_ref.tokens(data, off)
    assert ngram_ref.tokens(got, got_off) == toks
    assert bytes(got) == b"".join(t + b" " for d in toks for t in d)


def test_check_rejections():
    ok = tfidf_abi.ngram_params(1, 2)
    assert tfidf_abi.ngram_check(ok) == 0
    assert tfidf_abi.ngram_check(tfidf_abi.ngram_params(8, 8, 0x2D)) == 0
    assert tfidf_abi.lib().tfidf_ngram_check(None) == tfidf_abi.E_INVAL
    bad = []
    p = tfidf_abi.ngram_params(1, 2)
    p.size = C.sizeof(tfidf_abi.NgramParams) - 1
    bad.append(p)
    bad += [tfidf_abi.ngram_params(0, 2), tfidf_abi.ngram_params(3, 2), tfidf_abi.ngram_params(1, 9),
            tfidf_abi.ngram_params(9, 9)]
    bad += [tfidf_abi.ngram_params(1, 2, j) for j in ngram_ref.SEP]
    for i in range(7):
        p = tfidf_abi.ngram_params(1, 2)
        p.reserved[i] = 1
        bad.append(p)
    for p in bad:
        assert tfidf_abi.ngram_check(p) == tfidf_abi.E_INVAL, (p.size, p.min_n, p.max_n, p.joiner, bytes(p.reserved))
    # the host function refuses the same parameters and bad offsets, and zeroes its outputs
    data = np.frombuffer(b"a b c", dtype=np.uint8)
    ob, on, oo = C.c_void_p(1), C.c_uint64(7), C.c_void_p(1)
    for p, off in ((bad[1], [0, 5]), (ok, [0, 4, 3]), (ok, [0, 6])):
        o = np.array(off, dtype=np.uint64)
        rc = tfidf_abi.lib().tfidf_ngrams_host(C.byref(p), data.ctypes.data, len(data), o.ctypes.data, len(o) - 1,
                                              C.byref(ob), C.byref(on), C.byref(oo))
        assert rc == tfidf_abi.E_INVAL and ob.value is None and on.value == 0 and oo.value is None
        ob, on, oo = C.c_void_p(1), C.c_uint64(7), C.c_void_p(1)


def test_empty_inputs():
    z = np.zeros(0, dtype=np.uint8)
    got, off = tfidf_abi.ngrams_host(z, [0], 1, 2)
    assert len(got) == 0 and off.tolist() == [0]
    got, off = tfidf_abi.ngrams_host(z, [0, 0, 0], 1, 2)
    assert len(got) == 0 and off.tolist() == [0, 0, 0]
    got, off = tfidf_abi.ngrams_host(np.frombuffer(b"a b  \n c", dtype=np.uint8), [0, 1, 5, 5, 8], 2, 2)
    assert len(got) == 0 and off.tolist() == [0] * 5     # every document has fewer than min_n tokens


def test_unigram_counts_survive_shingling():
    g = load_golden("g5_w3")
    plain = oracle_py.run(g["data"], g["off"])
    sdata, soff = tfidf_abi.ngrams_host(g["data"], g["off"], 1, 2)
    sh = oracle_py.run(sdata, soff)
    want = {(d, plain["terms"][t]): c for d, t, c in zip(plain["doc"].tolist(), plain["term"].tolist(), plain["count"].tolist())}
    got = {(d, sh["terms"][t]): c for d, t, c in zip(sh["doc"].tolist(), sh["term"].tolist(), sh["count"].tolist())}
    assert want and all(got.get(k) == c for k, c in want.items())
    assert any(b"_" in w for _, w in got) and len(got) > len(want)
