"""Host-only pieces of the weighting schemes (include/tfidf.h, section "weighting"): the reference
tests/weight_ref.py against every golden, tfidf_result_reweight (csrc/weight_host.c) against the
reference for every valid scheme, tfidf_weighting_check's rules one by one, and a cross-check
against scikit-learn's TfidfTransformer.  No GPU call.  Everything but the scikit-learn check is
exact: u64 bit patterns of doubles, bytes."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_py
import tfidf_abi
import weight_ref
from conftest import golden_cases
from helpers import docs_to_arrays, load_golden
from weight_ref import REFERENCE, bits


def golden(case):
    g = load_golden(case)
    ora = oracle_py.run(g["data"], g["off"])
    return g, ora, len(g["off"]) - 1


# ---- the reference itself ----

@pytest.mark.parametrize("case", golden_cases())
def test_reference_scheme_reproduces_the_golden(case):
    g, ora, N = golden(case)
    ref = weight_ref.reweight(ora, *REFERENCE, N=N)
    assert np.array_equal(bits(ref["score"]), bits(ora["score"]))
    assert ref["output_txt"] == g["output"] == ora["output_txt"]


def test_fusing_the_square_into_the_sum_would_show():
    """the corpora of these tests can tell sum + fl(w * w) from fma(w, w, sum): a device or host
    build that contracts the two passes no bit comparison below by accident"""
    g, ora, N = golden("g5_w3")
    w = weight_ref.weights(ora, "log", "smooth", N)
    runs = weight_ref.doc_runs(ora["doc"])
    differ = sum(1 for b, e in runs if weight_ref.norm_of(w[b:e], "l2") != weight_ref.norm_of(w[b:e], "l2", fused=True))
    assert differ >= 1, "no document's L2 norm depends on the rounding of the squares"


# ---- tfidf_result_reweight against the reference ----

@pytest.mark.parametrize("case", golden_cases())
def test_result_reweight_equals_reference_for_every_scheme(case):
    g, ora, N = golden(case)
    schemes = weight_ref.all_schemes(N)
    assert len(schemes) == 4 * 4 * 3 - 4
    assert {s[0] for s in schemes} == set(weight_ref.TF) and {s[1] for s in schemes} == set(weight_ref.IDF)
    for tf, idf, norm in schemes:
        want = weight_ref.reweight(ora, tf, idf, norm, N=N)
        got = tfidf_abi.result_reweight(ora, tf, idf, norm, N=N)
        assert np.array_equal(bits(got["score"]), bits(want["score"])), (tf, idf, norm)
        assert got["output_txt"] == want["output_txt"], (tf, idf, norm)
        for k in ("doc", "term", "count", "docsize", "df"):
            assert np.array_equal(got[k], ora[k])
        s = want["score"]
        assert np.all(np.isfinite(s)) and np.all(s >= 0.0) and not np.any(np.signbit(s))
        if norm != "none" and len(s):
            assert s.max() <= 1.0


def test_b_after_a_equals_b_and_reference_restores():
    g, ora, N = golden("g5_w3")
    a, b = ("log", "smooth", "l2"), ("binary", "plus1", "l1")
    ra = tfidf_abi.result_reweight(ora, *a, N=N)
    rab = tfidf_abi.result_reweight(ra, *b, N=N)
    rb = tfidf_abi.result_reweight(ora, *b, N=N)
    assert not np.array_equal(bits(ra["score"]), bits(rb["score"]))
    assert np.array_equal(bits(rab["score"]), bits(rb["score"])) and rab["output_txt"] == rb["output_txt"]
    back = tfidf_abi.result_reweight(rab, *REFERENCE, N=N)
    assert np.array_equal(bits(back["score"]), bits(ora["score"])) and back["output_txt"] == g["output"]


def test_common_word_scores_zero_only_under_the_reference_idf():
    g, ora, N = golden("g6_common_word")
    common = ora["df"] == N
    assert common.any() and not common.all()
    ref = weight_ref.reweight(ora, *REFERENCE, N=N)
    assert np.all(bits(ref["score"][common]) == 0)                              # +0.0
    for idf in ("smooth", "plus1"):
        for r in (weight_ref.reweight(ora, "ratio", idf, "none", N=N), tfidf_abi.result_reweight(ora, "ratio", idf, "none", N=N)):
            assert np.all(r["score"][common] > 0.0)
    # a document of only such words has norm 0 under the reference idf: its scores stay +0.0
    only = [(b, e) for b, e in weight_ref.doc_runs(ora["doc"]) if common[b:e].all()]
    assert only
    for norm in ("l1", "l2"):
        r = tfidf_abi.result_reweight(ora, "ratio", "ref", norm, N=N)
        assert all(np.all(bits(r["score"][b:e]) == 0) for b, e in only)
        assert weight_ref.zero_norm_docs(ora, "ratio", "ref", norm, N) == len(only)


def test_two_documents_by_hand():
    """doc1 = "a a b", doc2 = "a c"; N = 2, df(a) = 2, df(b) = df(c) = 1.  Under {log, smooth, l2}:
    idf(a) = ln(3/3) + 1 = 1, idf(b) = idf(c) = ln(3/2) + 1 = 1.4054651081081644, tf(2) = 1 + ln 2 =
    1.6931471805599454; doc1: n = sqrt(1.6931..^2 + 1.4054..^2) = 2.2004..; doc2: n = sqrt(1 + 1.4054..^2)"""
    data, off = docs_to_arrays([b"a a b", b"a c"])
    ora = oracle_py.run(data, off)
    assert [ora["terms"][t] for t in ora["term"].tolist()] == [b"a", b"b", b"a", b"c"]
    assert ora["count"].tolist() == [2, 1, 1, 1] and ora["docsize"].tolist() == [3, 3, 2, 2] and ora["df"].tolist() == [2, 1, 2, 1]
    expect = {
        ("log", "smooth", "l2"): [0.7694470729725092, 0.6387105775654869, 0.5797386715376657, 0.8148024746671689],
        ("ratio", "plus1", "l1"): [0.5415435405682275, 0.45845645943177243, 0.37131279241563214, 0.6286872075843678],
        ("ratio", "ref", "none"): [0.0, 0.23104906018664842, 0.0, 0.34657359027997264],
        ("binary", "none", "l2"): [0.7071067811865475] * 4,
        ("raw", "smooth", "l1"): [0.587291291059816, 0.4127087089401839, 0.4157200188143547, 0.5842799811856452],
    }
    assert 1.0 + math.log(2.0) == 1.6931471805599454 and math.log(3.0 / 2.0) + 1.0 == 1.4054651081081644
    for scheme, want in expect.items():
        for r in (weight_ref.reweight(ora, *scheme, N=2), tfidf_abi.result_reweight(ora, *scheme, N=2)):
            assert np.array_equal(bits(r["score"]), bits(want)), scheme
    r = tfidf_abi.result_reweight(ora, "log", "smooth", "l2", N=2)
    assert r["output_txt"] == (b"doc1@a\t0.7694470729725092\ndoc1@b\t0.6387105775654869\n"
                               b"doc2@a\t0.5797386715376657\ndoc2@c\t0.8148024746671689\n")


# ---- tfidf_weighting_check ----

def test_weighting_check_accepts_every_valid_scheme():
    for tf, idf, norm in weight_ref.all_schemes():
        assert tfidf_abi.weighting_check(tfidf_abi.weighting(tf, idf, norm)) == 0
    w = tfidf_abi.weighting("log", "smooth", "l2")
    w.size = C.sizeof(tfidf_abi.Weighting) + 64                                   # a longer struct of a later version
    assert tfidf_abi.weighting_check(w) == 0
    assert tfidf_abi.weighting_check(tfidf_abi.weighting("log", "ref", "none")) == 0   # the N limit is checked where N is known


def test_weighting_check_rejects_every_case():
    assert tfidf_abi.weighting_check(None) == tfidf_abi.E_INVAL
    w = tfidf_abi.weighting("log", "smooth", "l2")
    w.size = C.sizeof(tfidf_abi.Weighting) - 1
    assert tfidf_abi.weighting_check(w) == tfidf_abi.E_INVAL
    w.size = 0
    assert tfidf_abi.weighting_check(w) == tfidf_abi.E_INVAL
    for field, bad in (("tf", 4), ("idf", 4), ("norm", 3), ("tf", 0xFFFFFFFF), ("reserved", 1)):
        w = tfidf_abi.weighting("log", "smooth", "l2")
        setattr(w, field, bad)
        assert tfidf_abi.weighting_check(w) == tfidf_abi.E_INVAL, field
    for idf in weight_ref.IDF:
        assert tfidf_abi.weighting_check(tfidf_abi.weighting("raw", idf, "none")) == tfidf_abi.E_INVAL
        assert tfidf_abi.weighting_check(tfidf_abi.weighting("raw", idf, "l1")) == 0


def test_result_reweight_refuses_and_leaves_the_scores():
    g, ora, N = golden("g4_config1")
    for args, n in ((("raw", "ref", "none"), N), (("log", "ref", "none"), 1 << 48)):
        with pytest.raises(tfidf_abi.TfidfError) as ex:
            tfidf_abi.result_reweight(ora, *args, N=n)
        assert ex.value.rc == tfidf_abi.E_INVAL
    tfidf_abi.result_reweight(ora, "log", "ref", "l2", N=1 << 48)               # with a norm the limit does not apply
    tfidf_abi.result_reweight(ora, "log", "ref", "none", N=(1 << 48) - 1)


# ---- scikit-learn ----

def test_against_sklearn_tfidf_transformer():
    """TfidfTransformer on the count matrix of a golden (one row per document, empty ones
    included, so that its n_samples and df are the run's N and df).  Relative difference per
    element at most 4 * (n + 8) * 2^-53, n the row's pairs: one log, one product, n products and
    adds, one sqrt and one division on either side."""
    text = pytest.importorskip("sklearn.feature_extraction.text")
    g, ora, N = golden("g5_w3")
    V = ora["nterms"]
    X = np.zeros((N, V))
    X[ora["doc"].astype(np.int64) - 1, ora["term"]] = ora["count"]
    assert np.array_equal((X > 0).sum(axis=0), np.bincount(ora["term"], minlength=V))
    per_row = (X > 0).sum(axis=1)
    rows, cols = ora["doc"].astype(np.int64) - 1, ora["term"].astype(np.int64)
    checked = 0
    for tf in ("raw", "log"):
        for idf in ("smooth", "plus1"):
            for norm in ("l1", "l2", "none"):
                t = text.TfidfTransformer(norm=None if norm == "none" else norm, use_idf=True, smooth_idf=idf == "smooth",
                                          sublinear_tf=tf == "log")
                sk = np.asarray(t.fit_transform(X).todense())[rows, cols]
                ours = [weight_ref.scores(ora, tf, idf, norm, N)]
                if weight_ref.valid(tf, idf, norm, N):                          # raw + none: through the reference only
                    ours.append(tfidf_abi.result_reweight(ora, tf, idf, norm, N=N)["score"])
                bound = 4.0 * (per_row[rows] + 8) * 2.0 ** -53
                for s in ours:
                    rel = np.abs(s - sk) / np.abs(sk)
                    assert np.all(rel <= bound), (tf, idf, norm, float(rel.max()))
                    checked += len(s)
    assert checked > 10 * ora["npairs"]
