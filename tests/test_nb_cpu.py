"""Host-only pieces of Naive Bayes classification (include/tfidf.h, section "classify"):
tfidf_result_nb_fit and tfidf_nb_model_predict (plain C, csrc/nb_host.c) against the reference
tests/nb_ref.py on every golden, tfidf_nb_check's and the fit's rules one by one, a three-document
case whose weights are written out by hand, and the condition the GPU tests rely on: on the
planted corpus the reference gives every held-out document its planted class.  No GPU call.

All comparisons are exact: integers equal, doubles as u64 bit patterns."""
import ctypes as C
import math

import numpy as np
import pytest

import nb_ref as R
import oracle_py
import tfidf_abi
from conftest import golden_cases
from helpers import docs_to_arrays, load_golden

ALPHAS = [0.0, 0.5, float.fromhex("0x1p-1074"), float.fromhex("0x1p+900")]
VARIANTS = ["multinomial", "complement"]
FEATURES = ["count", "binary"]


def oracle_of(docs):
    data, off = docs_to_arrays(docs)
    return oracle_py.run(data, off), list(range(1, len(docs) + 1))


def both(ora, ids, docs, labels, K, rows=None, **kw):
    """fit and predict on the host against the reference; returns the reference's model and answer"""
    ref = R.NRef(ora, ids)
    model = ref.fit(docs, labels, K, **kw)
    assert model is not None
    got = tfidf_abi.result_nb_fit(ora, docs, labels, K, doc_ids=ids, **kw)
    R.assert_same_model(got, model)
    rows = ref.rows() if rows is None else rows
    want = R.predict(model, rows)
    fast = R.predict(model, rows, by_class=True)                         # the form the larger GPU cases use
    assert fast[0] == want[0] and R.bits(fast[1]).tolist() == R.bits(want[1]).tolist()
    assert [R.bits(s).tolist() for s in fast[2]] == [R.bits(s).tolist() for s in want[2]]
    off, term, count = R.flat_rows(rows)
    R.assert_same_labels(tfidf_abi.nb_model_predict(got, off, term, count), want, K)
    return ref, model, want


@pytest.mark.parametrize("case", golden_cases())
def test_host_equals_reference_on_goldens(case):
    g = load_golden(case)
    ora = oracle_py.run(g["data"], g["off"])
    ids = list(range(1, len(g["off"])))
    for K in (1, 2, 3):
        labels = [d % K for d in ids]
        for variant in VARIANTS:
            for feature in FEATURES:
                for uniform in (False, True):
                    for alpha in ALPHAS:
                        both(ora, ids, ids, labels, K, variant=variant, feature=feature, alpha=alpha, uniform_prior=uniform)


def test_labelled_subset_and_unseen_rows():
    """unlabelled documents take no part; rows of new documents, with words outside the vocabulary"""
    g = load_golden("g5_w3")
    ora = oracle_py.run(g["data"], g["off"])
    ids = list(range(1, len(g["off"])))
    docs = [d for d in ids if d % 3]                                     # a third stays unlabelled
    labels = [d % 2 for d in docs]
    ref = R.NRef(ora, ids)
    new = [b"zzzunknown " + ref.words[5] + b" " + ref.words[5] + b" " + ref.words[700], b"", b"qq ww", ref.words[0]]
    rows = ref.unseen(new)
    assert [len(r) for r in rows] == [2, 0, 0, 1] and rows[0][0] == (5, 2)
    for variant in VARIANTS:
        _, model, want = both(ora, ids, docs, labels, 2, rows=rows, variant=variant)
        assert want[1][1] == model["prior"][want[0][1]] and want[2][2] == model["prior"]   # no pairs: the prior
        assert sum(model["class_docs"]) == len(docs) == model["nlabelled"]
        # the counts of an unlabelled document are in no class
        assert sum(model["class_total"]) == sum(x for d in docs for _, x in ref.by_pos[ref.pos[d]])


def test_hand_computed_three_documents():
    """doc1 = "a a b" in class 0, doc2 = "b c" in class 1, doc3 = "a c c" unlabelled; V = 3, alpha = 1"""
    ora, ids = oracle_of([b"a a b", b"b c", b"a c c"])
    ln = math.log
    got = tfidf_abi.result_nb_fit(ora, [1, 2], [0, 1], 2, doc_ids=ids)
    assert got["feature_count"].tolist() == [[2, 0], [1, 1], [0, 1]]     # rows a, b, c
    assert got["class_total"].tolist() == [3, 2] and got["class_docs"].tolist() == [1, 1]
    # multinomial: log(FC + 1) - log(T + 3)
    w = [[ln(3.0) - ln(6.0), ln(1.0) - ln(5.0)], [ln(2.0) - ln(6.0), ln(2.0) - ln(5.0)], [ln(1.0) - ln(6.0), ln(2.0) - ln(5.0)]]
    prior = [ln(1.0) - ln(2.0)] * 2
    assert np.array_equal(R.bits(got["weight"]), R.bits(w)) and np.array_equal(R.bits(got["prior"]), R.bits(prior))
    # doc3: a once, c twice, in term order
    s = [(prior[c] + 1.0 * w[0][c]) + 2.0 * w[2][c] for c in range(2)]
    assert s[1] > s[0]
    out = tfidf_abi.nb_model_predict(got, [0, 2], [0, 2], [1, 2])
    assert out["label"].tolist() == [1] and np.array_equal(R.bits(out["scores"][0]), R.bits(s))
    assert R.bits(out["score"])[0] == R.bits([s[1]])[0]
    # complement: log((Ttot - T) + 3) - log((F - FC) + 1), Ttot = 5, F = 2, 2, 1; no prior
    got = tfidf_abi.result_nb_fit(ora, [1, 2], [0, 1], 2, doc_ids=ids, variant="complement")
    w = [[ln(5.0) - ln(1.0), ln(6.0) - ln(3.0)], [ln(5.0) - ln(2.0), ln(6.0) - ln(2.0)], [ln(5.0) - ln(2.0), ln(6.0) - ln(1.0)]]
    assert np.array_equal(R.bits(got["weight"]), R.bits(w)) and got["prior"].tolist() == [0.0, 0.0]
    s = [(0.0 + 1.0 * w[0][c]) + 2.0 * w[2][c] for c in range(2)]
    out = tfidf_abi.nb_model_predict(got, [0, 2], [0, 2], [1, 2])
    assert out["label"].tolist() == [1] and np.array_equal(R.bits(out["scores"][0]), R.bits(s))
    # binary features: doc1 counts a once
    got = tfidf_abi.result_nb_fit(ora, [1, 2], [0, 1], 2, doc_ids=ids, feature="binary", alpha=0.5, uniform_prior=True)
    assert got["feature_count"].tolist() == [[1, 0], [1, 1], [0, 1]] and got["class_total"].tolist() == [2, 2]
    assert got["prior"].tolist() == [0.0, 0.0]
    assert R.bits(got["weight"])[0][0] == R.bits([ln(1.5) - ln(3.5)])[0]


def test_ties_take_the_lowest_class():
    """two classes with the same documents' words score alike: the lower class wins"""
    ora, ids = oracle_of([b"x y", b"x y", b"z", b"x"])
    _, model, want = both(ora, ids, [1, 2, 3], [2, 1, 0], 3, uniform_prior=True)
    j = R.NRef(ora, ids).pos[4]
    assert want[2][j][1] == want[2][j][2] > want[2][j][0] and want[0][j] == 1


def params(**kw):
    base = dict(docs=[1, 2, 3], labels=[0, 1, 0], nclasses=2)
    base.update(kw)
    return tfidf_abi.nb_params(**base)


def test_check_rules_one_by_one():
    E = tfidf_abi.E_INVAL
    assert tfidf_abi.nb_check(params()) == 0
    assert tfidf_abi.nb_check(None) == E
    assert tfidf_abi.nb_check(params(size=C.sizeof(tfidf_abi.NbParams) - 8)) == E            # a short size
    assert tfidf_abi.nb_check(params(size=C.sizeof(tfidf_abi.NbParams) + 8)) == 0             # a newer caller's
    assert tfidf_abi.nb_check(params(nclasses=0, labels=[0, 0, 0])) == E
    assert tfidf_abi.nb_check(params(docs=list(range(1, 258)), labels=list(range(257)), nclasses=257)) == E
    assert tfidf_abi.nb_check(params(docs=list(range(1, 257)), labels=list(range(256)), nclasses=256)) == 0
    for alpha, rc in ((0.0, 0), (1.0, 0), (float.fromhex("0x1p-1074"), 0), (float.fromhex("0x1p+900"), 0),
                      (float.fromhex("0x1.0000000000001p+900"), E), (-1.0, E), (-0.5, E), (math.inf, E), (math.nan, E)):
        assert tfidf_abi.nb_check(params(alpha=alpha)) == rc, alpha
    assert tfidf_abi.nb_check(params(labels=[0, 2, 1])) == E                                  # a label >= K
    assert tfidf_abi.nb_check(params(docs=[1, 2, 1])) == E                                    # a repeated id
    assert tfidf_abi.nb_check(params(labels=[0, 0, 0])) == E                                  # class 1 has no document
    assert tfidf_abi.nb_check(params(docs=[], labels=[])) == E                                # ... nor has any
    p, keep = params()
    p.variant = 2
    assert tfidf_abi.nb_check(p) == E
    p, keep = params()
    p.feature = 2
    assert tfidf_abi.nb_check(p) == E
    p, keep = params()
    p.label = None
    assert tfidf_abi.nb_check(p) == E
    for kw in (dict(), dict(alpha=-1.0), dict(labels=[0, 2, 1]), dict(docs=[1, 2, 1]), dict(labels=[0, 0, 0])):
        assert R.check_params(kw.get("docs", [1, 2, 3]), kw.get("labels", [0, 1, 0]), 2, kw.get("alpha", 0.0)) == \
            (tfidf_abi.nb_check(params(**kw)) == 0)


def test_fit_and_predict_rules():
    ora, ids = oracle_of([b"a b", b"b c", b"c d"])
    with pytest.raises(tfidf_abi.TfidfError) as ei:                      # an id the result does not hold
        tfidf_abi.result_nb_fit(ora, [1, 9], [0, 1], 2, doc_ids=ids)
    assert ei.value.rc == tfidf_abi.E_INVAL
    assert R.NRef(ora, ids).fit([1, 9], [0, 1], 2) is None
    with pytest.raises(tfidf_abi.TfidfError) as ei:                      # parameters that fail the check
        tfidf_abi.result_nb_fit(ora, [1, 2], [0, 0], 2, doc_ids=ids)
    assert ei.value.rc == tfidf_abi.E_INVAL
    m = tfidf_abi.result_nb_fit(ora, [1, 2], [0, 1], 2, doc_ids=ids)
    assert m["nterms"] == 4
    with pytest.raises(tfidf_abi.TfidfError) as ei:                      # a term outside the model
        tfidf_abi.nb_model_predict(m, [0, 1], [4], [1])
    assert ei.value.rc == tfidf_abi.E_INVAL
    with pytest.raises(tfidf_abi.TfidfError) as ei:                      # offsets that go back
        tfidf_abi.nb_model_predict(m, [0, 2, 1], [0, 1], [1, 1])
    assert ei.value.rc == tfidf_abi.E_INVAL
    out = tfidf_abi.nb_model_predict(m, [0], [], [])                     # no rows
    assert out["ndocs"] == 0
    out = tfidf_abi.nb_model_predict(m, [0, 1], [3], [2], all_scores=False)
    assert "scores" not in out and out["ndocs"] == 1


def test_edge_corpora():
    both(*oracle_of([b"", b"solo", b"  \n"]), [1, 2, 3], [0, 1, 0], 2)                      # empty labelled documents count in n_c
    both(*oracle_of([b"", b""]), [1, 2], [0, 1], 2)                                          # no terms at all
    both(*oracle_of([b"one two"]), [1], [0], 1, variant="complement")                        # K = 1: the complement is empty
    ora, ids = oracle_of([b"w " * 70000, b"w v"])                                            # a count above 2^16
    _, model, _ = both(ora, ids, [1, 2], [0, 1], 2)
    assert max(max(r) for r in model["feature_count"]) == 70000


def test_planted_corpus_is_classified():
    """what test_gpu_nb.py relies on: 4 classes x 12 documents, half labelled; the reference gives
    every held-out document its planted class under both variants"""
    docs, planted = R.planted_corpus()
    assert len(docs) == R.PLANT_CLASSES * R.PLANT_PER_CLASS == 48
    lab, lab_classes, held = R.planted_split(planted)
    assert len(lab) == len(held) == 24 and all(lab_classes.count(c) == 6 for c in range(4))
    ora, ids = oracle_of(docs)
    for variant in VARIANTS:
        ref, model, want = both(ora, ids, lab, lab_classes, 4, variant=variant)
        for d in held:
            assert want[0][ref.pos[d]] == planted[d - 1], (variant, d)
        for d in lab:
            assert want[0][ref.pos[d]] == planted[d - 1], (variant, d)
    shared = [w for w in ref.words if w.startswith(b"sh_")]
    assert len(shared) == 20 and len(ref.words) == 20 + 4 * 30
