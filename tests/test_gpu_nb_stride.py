"""The Naive Bayes calls on the stride corpus (tests/stride_corpus.py) with TFIDF_GRID_CUS = 1, 2
and unset, as tests/test_gpu_grid_stride.py runs the other calls over the resident result: with
one or two CUs every grid-stride loop of csrc/nb.hip makes three trips and more (asserted from the
*_WG_PER_CU constants of kernels.h), so what a wave carries from one document, row or term to the
next (its column sums, a `continue` in front of an unlabelled document or a row that is not held)
is exercised.  The reference knows nothing of the grid, so equality at every setting is grid
independence.  All comparisons are exact."""
import numpy as np
import pytest

import nb_ref as R
import oracle_py
import stride_corpus as SC
import tfidf_abi
from helpers import docs_to_arrays
from test_gpu_grid_stride import device_cus
from test_gpu_nb import check, same_answer

pytestmark = pytest.mark.gpu

N = SC.NDOCS
NT = 256                                        # threads of a workgroup of nb.hip
FITS = ((20, "multinomial"), (130, "complement"))     # one and three accumulators per lane
NB_WG, NB_EL_WG = SC.kernels_h("NB_WG_PER_CU"), SC.kernels_h("NB_EL_WG_PER_CU")


def trips(ncu: int, ndocs: int, V: int, K: int) -> dict:
    """launch -> trips of its longest-working wave or thread through the grid-stride loop"""
    def waves(items):                           # a wave per item, four waves per workgroup
        grid = min(-(-items // SC.WAVES), ncu * NB_WG)
        return -(-items // (grid * SC.WAVES))

    def threads(n):                             # a thread per matrix entry
        grid = min(-(-n // NT), ncu * NB_EL_WG)
        return -(-n // (grid * NT))
    return {"k_nb_count": waves(ndocs), "k_nb_predict": waves(ndocs), "k_nb_sums": waves(V), "k_nb_argmax": threads(V * K),
            "k_nb_list": threads(V * K), "k_nb_weights": threads(V * K)}


def list_corpus():
    """40 documents over 700 words; document 1 repeats one word 70 000 times, so the fit has log
    arguments past the table and runs the list kernel"""
    docs = [b" ".join(b"q%03d" % ((17 * d + j) % 700) for j in range(60)) for d in range(40)]
    docs[0] = b"q000 " * 70000 + docs[0]
    return docs


@pytest.fixture(scope="module")
def want():
    """the corpora and the reference's models and answers, computed once for the three settings"""
    c = SC.build()
    data, off = docs_to_arrays(c["docs"])
    ids = list(range(1, N + 1))
    ref = R.NRef(oracle_py.run(data, off), ids)
    docs = [d for d in ids if d % 3]                                     # a third stays unlabelled: the count pass skips them
    w = dict(data=data, off=off, ref=ref, docs=docs)
    ldocs = list_corpus()
    ldata, loff = docs_to_arrays(ldocs)
    w["list"] = dict(data=ldata, off=loff, ref=R.NRef(oracle_py.run(ldata, loff), list(range(1, len(ldocs) + 1))))
    assert w["list"]["ref"].V == 700
    return w


@pytest.mark.parametrize("cus", ["1", "2", None])
def test_nb_at_this_cu_count(want, cus, monkeypatch):
    if cus is None:
        monkeypatch.delenv("TFIDF_GRID_CUS", raising=False)
    else:
        monkeypatch.setenv("TFIDF_GRID_CUS", cus)
    w, ref = want, want["ref"]
    with tfidf_abi.Engine(0) as e:                                              # the environment is read at tfidf_open
        assert e.grid_cus() == (int(cus) if cus else device_cus())
        e.run_host(w["data"], w["off"])
        for K, variant in FITS:
            if cus:
                t = trips(int(cus), N, ref.V, K)
                assert all(v >= 3 for v in t.values()), t
            labels = [d % K for d in w["docs"]]
            assert set(labels) == set(range(K))
            key = (K, variant)
            if key not in w:                                                    # the reference's answer, once
                model = ref.fit(w["docs"], labels, K, variant=variant)
                w[key] = (model, R.predict(model, ref.rows(), by_class=True))
            model, answer = w[key]
            e.nb_fit(w["docs"], labels, K, variant=variant)
            R.assert_same_model(e.nb_export(), model)
            got = e.nb_predict(all_scores=True)
            R.assert_same_labels(got, answer, K)
            # uploaded rows through the same kernel; a list with ids the context does not hold
            rows = e.transform(w["data"], w["off"])
            same_answer(e.nb_predict_rows(rows, all_scores=True), e.nb_predict(list(range(1, N + 1)), all_scores=True))
            listed = [d if d % 5 else 10 ** 6 + d for d in range(1, N + 1)]
            part = e.nb_predict(listed, all_scores=True)
            for r, d in enumerate(listed):
                if d > N:
                    assert part["label"][r] == tfidf_abi.NO_CLASS and part["pos"][r] == tfidf_abi.NO_POS and not part["scores"][r].any()
                else:
                    assert part["label"][r] == answer[0][ref.pos[d]]
                    assert R.bits(part["scores"][r]).tolist() == R.bits(answer[2][ref.pos[d]]).tolist()
        # the list kernel: arguments past the table
        lw, lref = w["list"], w["list"]["ref"]
        e.run_host(lw["data"], lw["off"])
        ids = list(range(1, 41))
        if cus:
            t = trips(int(cus), 40, lref.V, 20)
            assert t["k_nb_list"] >= 3 and t["k_nb_weights"] >= 3 and t["k_nb_argmax"] >= 3, t
        for variant in ("multinomial", "complement"):
            check(e, lref, ids, [d % 20 for d in ids], 20, by_class=True, variant=variant)
            assert e.nb_info()["nlisted"] >= 1
        assert e.grid_cus() == (int(cus) if cus else device_cus())
