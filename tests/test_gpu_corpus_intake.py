"""How tfidf_transform, tfidf_analyze and tfidf_ngrams take a tfidf_corpus in, host or device:
the offsets are checked before anything runs (monotone, inside the bytes, present when there
are documents), no document is a valid input, a window of empty or blank documents yields empty
rows or documents without a byte outside the window being read, and a rejected call leaves the
context ready for the next one."""
import contextlib

import numpy as np
import pytest

import analyze_ref
import ngram_ref
import tfidf_abi
import transform_ref
from helpers import device_corpus, docs_to_arrays, pad_after, pad_before, windowed

pytestmark = pytest.mark.gpu

FIT = [b"ab cd", b"cd ef ef", b"gh"]            # the run tfidf_transform scores against
DOCS = [b"ab Zz", b"", b"ef Ef cd"]             # the valid input: 3 documents in a window
LEAD, TRAIL = 5, 4


@pytest.fixture(scope="module")
def fitted():
    with tfidf_abi.Engine(0) as e:
        e.run_host(*docs_to_arrays(FIT))
        model = transform_ref.Model(*docs_to_arrays(FIT))
        model.terms = e.fetch()["terms"]
        yield e, model


@contextlib.contextmanager
def corpus(dev: bool, data, off):
    data = np.ascontiguousarray(data, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    assert len(data) < 64
    if dev:
        with device_corpus(data, off, shift=3) as c:
            yield c
    else:
        c, keep = tfidf_abi._host_corpus(data, off)
        yield c


def run(e, which: str, c):
    """the call's result, or the error code it returned"""
    try:
        if which == "transform":
            return e.transform_corpus(c)
        if which == "analyze":
            return e.analyze(c, lower=True, slot=tfidf_abi.AN_SLOT_BATCH)
        return e.ngrams(c, min_n=1, max_n=2, slot=tfidf_abi.NG_SLOT_BATCH)
    except tfidf_abi.TfidfError as ex:
        return ex.rc


def check(e, model, which: str, dev: bool, data, off):
    """a valid call against the references in plain Python"""
    off = np.asarray(off, dtype=np.uint64)
    n = len(off) - 1
    with corpus(dev, data, off) as c:
        res = run(e, which, c)
        assert not isinstance(res, int), (which, dev, res)
        if which == "transform":
            transform_ref.check(res, model.rows(transform_ref.split_docs(data, off)), off, model.terms)
            return res
        assert res.flags & tfidf_abi.TFIDF_CORPUS_DEVICE and res.ndocs == n
        got, got_off = e.corpus_bytes(res)
    if which == "analyze":
        assert res.nbytes == len(data) and np.array_equal(got_off, off)
        assert np.array_equal(got, analyze_ref.analyze(data, off, lower=True))
    else:
        want, want_off = ngram_ref.ngrams(data, off, 1, 2)
        assert bytes(got) == want and got_off.tolist() == want_off
        ntok, ngr = ngram_ref.counts(data, off, 1, 2)
        info = e.ngram_info()
        assert (info["ntokens"], info["ngrams"], info["nbytes_out"]) == (ntok, ngr, len(want))
    return res


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("which", ["transform", "analyze", "ngrams"])
def test_corpus_intake(fitted, which, dev):
    e, model = fitted
    data, off = windowed(DOCS, LEAD, TRAIL)
    n = len(data)
    assert n < 64 and off.tolist() == [5, 10, 10, 18]
    check(e, model, which, dev, data, off)

    def null_off(c):
        c.doc_off = None

    for bad_off, edit in (([5, 12, 10, 18], None),          # decreasing
                          ([18, 10, 10, 5], None),
                          ([5, 10, 10, n + 1], None),       # past the bytes
                          (off, null_off)):                 # documents without offsets
        with corpus(dev, data, bad_off) as c:
            if edit:
                edit(c)
            assert run(e, which, c) == tfidf_abi.E_INVAL, (which, dev, bad_off)
        check(e, model, which, dev, data, off)              # the context goes on

    # no document: every byte lies outside the window
    with corpus(dev, data, [LEAD]) as c:
        res = run(e, which, c)
        if which == "transform":
            assert (res["ndocs"], res["npairs"], res["ntokens"]) == (0, 0, 0) and res["words"] == []
        else:
            assert res.ndocs == 0 and res.flags & tfidf_abi.TFIDF_CORPUS_DEVICE
            if which == "analyze":
                assert res.nbytes == n and np.array_equal(e.corpus_bytes(res)[0], data)
            else:
                assert res.nbytes == 0 and e.ngram_info()["ntokens"] == 0

    # a window behind a lead whose documents are all empty, then all blank: the words that touch
    # the window on both sides are no token of it and stay as they are
    blank = np.frombuffer(pad_before(LEAD) + b" \t\n  \r " + pad_after(TRAIL), dtype=np.uint8)
    for wdata, woff in ((data, [LEAD, LEAD, LEAD, LEAD]), (blank, [LEAD, LEAD + 2, LEAD + 2, LEAD + 7])):
        res = check(e, model, which, dev, wdata, woff)
        if which == "transform":
            assert (res["npairs"], res["ntokens"]) == (0, 0) and not res["doc_size"].any() and not res["doc_oov"].any()
            assert res["row_off"].tolist() == [0, 0, 0, 0]
        elif which == "analyze":
            assert np.array_equal(e.corpus_bytes(res)[0], wdata)
        else:
            assert res.nbytes == 0 and e.corpus_bytes(res)[1].tolist() == [0, 0, 0, 0]
            assert e.ngram_info()["ngrams"] == 0
    check(e, model, which, dev, data, off)
