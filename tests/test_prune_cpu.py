"""Host-only pieces of vocabulary pruning (include/tfidf.h, section "prune"): the reference filter
tests/prune_ref.py on every golden, tfidf_prune_check's rules one by one, and tfidf_model_prune
against the reference, ties at the max_features cut included.  No GPU call."""
import ctypes as C

import numpy as np
import pytest

import oracle_py
import prune_ref
import tfidf_abi
from conftest import golden_cases
from helpers import load_golden
from test_model_cpu import golden_model, model_of

# [2, N - 1]: (terms kept, terms, documents emptied), computed on the CPU from the golden inputs
RANGE_FACTS = {"g1_whitespace": (None, None, 1), "g3_bytes": (None, None, 1), "g6_common_word": (0, 4, 4),
               "g4_config1": (11, 21, None), "g5_w3": (298, 820, None)}


def param_sets(N, V):
    return [(2, 0, 0), (0, N - 1, 0), (2, N - 1, 0), (0, 0, V // 2), (0, 0, 1), (0, 0, 0)]


@pytest.mark.parametrize("case", golden_cases())
def test_reference_filter_on_goldens(case):
    g = load_golden(case)
    ora = oracle_py.run(g["data"], g["off"])
    N, V = len(g["off"]) - 1, len(ora["terms"])
    for mn, mx, mf in param_sets(N, V):
        pr = prune_ref.prune(ora, mn, mx, mf)
        # the filtered golden lines are the lines formatted from the filtered result
        assert prune_ref.filter_lines(g["output"], set(pr["terms"])) == tfidf_abi.format_lines(pr)
        assert pr["output_txt"] == tfidf_abi.format_lines(pr)
        assert pr["npairs"] == len(pr["doc"]) == len(pr["term"]) <= ora["npairs"]
        if (mn, mx, mf) == (0, 0, 0):
            assert pr["nterms"] == V and pr["npairs"] == ora["npairs"] and pr["output_txt"] == g["output"]
        if mf:
            assert pr["nterms"] == min(mf, V)
        # the kept pairs carry the input's own bits
        words = set(pr["terms"])
        sel = np.array([ora["terms"][t] in words for t in ora["term"].tolist()], dtype=bool)
        assert np.array_equal(pr["score"].view(np.uint64), ora["score"][sel].view(np.uint64))
        assert np.array_equal(pr["count"], ora["count"][sel]) and np.array_equal(pr["docsize"], ora["docsize"][sel])
    if case in RANGE_FACTS:
        kept, total, emptied = RANGE_FACTS[case]
        pr = prune_ref.prune(ora, 2, N - 1, 0)
        if kept is not None:
            assert (pr["nterms"], V) == (kept, total)
        if emptied is not None:
            assert prune_ref.emptied_docs(ora, pr) == emptied


def test_df_one_share_of_the_goldens():
    for case, (ones, total) in {"g5_w1": (461, 785), "g5_w3": (516, 820)}.items():
        g = load_golden(case)
        df = prune_ref.term_df(oracle_py.run(g["data"], g["off"]))
        assert (int((df == 1).sum()), len(df)) == (ones, total)


# ---- tfidf_prune_check ----

def test_prune_check_accepts():
    for mn, mx, mf in [(0, 0, 0), (1, 0, 0), (2, 2, 0), (5, 0, 7), (0, 3, 1), (0xFFFFFFFF, 0, 0xFFFFFFFF)]:
        assert tfidf_abi.prune_check(tfidf_abi.prune_params(mn, mx, mf)) == 0


def test_prune_check_rejects_every_case():
    assert tfidf_abi.prune_check(None) == tfidf_abi.E_INVAL
    p = tfidf_abi.prune_params(2, 0, 0)
    p.size = C.sizeof(tfidf_abi.PruneParams) - 1
    assert tfidf_abi.prune_check(p) == tfidf_abi.E_INVAL
    p.size = 0
    assert tfidf_abi.prune_check(p) == tfidf_abi.E_INVAL
    p = tfidf_abi.prune_params(2, 0, 0)
    p.reserved = 1
    assert tfidf_abi.prune_check(p) == tfidf_abi.E_INVAL
    assert tfidf_abi.prune_check(tfidf_abi.prune_params(3, 2, 0)) == tfidf_abi.E_INVAL
    assert tfidf_abi.prune_check(tfidf_abi.prune_params(3, 0, 0)) == 0      # max_df 0: no upper bound
    p = tfidf_abi.prune_params(2, 0, 0)
    p.size = C.sizeof(tfidf_abi.PruneParams) + 64                             # a longer struct of a later version
    assert tfidf_abi.prune_check(p) == 0


# ---- tfidf_model_prune ----

def same_model(a, b):
    assert a["N"] == b["N"] and a["terms"] == b["terms"] and np.array_equal(a["df"], b["df"])


@pytest.mark.parametrize("case", golden_cases())
def test_model_prune_on_goldens(case):
    m = golden_model(case)
    N, V = m["N"], len(m["terms"])
    for mn, mx, mf in param_sets(N, V):
        got = tfidf_abi.model_prune(m, mn, mx, mf)
        same_model(got, prune_ref.prune_model(m, mn, mx, mf))
        assert tfidf_abi.model_check(got) == 0 and int(got["term_off"][0]) == 0


def test_model_prune_ties_at_the_cut():
    """many terms of equal df: the cut takes the lowest ranks among equals"""
    terms = sorted([b"w%03d" % i for i in range(200)] + [b"", b"\x80\xff", b"\xc3\xa9t\xc3\xa9", b"q" * 40],
                   key=lambda w: w + b"\t")
    V = len(terms)
    df = np.array([3 if i % 5 else 7 for i in range(V)], dtype=np.uint32)
    m = model_of(terms, df, 9)
    assert terms[0] == b"" and any(w[0] >= 0x80 for w in terms if w)
    for M in (1, 2, int((df == 7).sum()), int((df == 7).sum()) + 1, V - 1, V, V + 1):
        got = tfidf_abi.model_prune(m, 0, 0, M)
        want = prune_ref.prune_model(m, 0, 0, M)
        same_model(got, want)
        assert len(got["terms"]) == min(M, V)
    # M = 1 keeps the first df-7 term by rank; one past the df-7 terms adds the first df-3 term
    assert tfidf_abi.model_prune(m, 0, 0, 1)["terms"] == [terms[int(np.flatnonzero(df == 7)[0])]]
    n7 = int((df == 7).sum())
    extra = set(tfidf_abi.model_prune(m, 0, 0, n7 + 1)["terms"]) - set(tfidf_abi.model_prune(m, 0, 0, n7)["terms"])
    assert extra == {terms[int(np.flatnonzero(df == 3)[0])]}
    # the range test comes first: with max_df = 3 the df-7 terms are gone before the cut
    same_model(tfidf_abi.model_prune(m, 0, 3, 2), prune_ref.prune_model(m, 0, 3, 2))
    assert all(d == 3 for d in tfidf_abi.model_prune(m, 0, 3, 2)["df"].tolist())


def test_model_prune_rejects():
    m = model_of([b"a", b"b"], [1, 2], 2)
    with pytest.raises(tfidf_abi.TfidfError) as ex:
        tfidf_abi.model_prune(m, 3, 2, 0)
    assert ex.value.rc == tfidf_abi.E_INVAL
    with pytest.raises(tfidf_abi.TfidfError) as ex:
        tfidf_abi.model_prune(model_of([b"b", b"a"], [1, 2], 2), 2, 0, 0)      # fails tfidf_model_check
    assert ex.value.rc == tfidf_abi.E_INVAL
    assert tfidf_abi.model_prune(m, 3, 0, 0)["terms"] == []                    # everything pruned: a valid empty model


def test_pruned_model_save_load(tmp_path):
    m = golden_model("g5_w3")
    pr = tfidf_abi.model_prune(m, 2, m["N"] - 1, 0)
    assert 0 < len(pr["terms"]) < len(m["terms"])
    path = str(tmp_path / "pruned.model")
    tfidf_abi.model_save(pr, path)
    back = tfidf_abi.model_load(path)
    same_model(back, pr)
    same_model(back, prune_ref.prune_model(m, 2, m["N"] - 1, 0))
    # pruning the loaded model again with the same range changes nothing
    same_model(tfidf_abi.model_prune(back, 2, m["N"] - 1, 0), back)
