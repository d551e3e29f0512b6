"""Every call over the resident result on the stride corpus (tests/stride_corpus.py) with
TFIDF_GRID_CUS = 1, 2 and unset, each against the plain references the calls' own tests use.

The launches take min(work, CUs x a per-kernel constant) workgroups that stride over the work
(csrc/kernels.h).  On a 256-CU device no corpus of the suite makes a wave or workgroup of them take
a second document, row, candidate or tile, so what a loop carries from one trip to the next (LDS
accumulators, a barrier before shared words are rewritten, a `continue` in front of a small
document, per-document minima) ran untested.  With one CU every loop here makes 3 to 67 trips
(test_stride_corpus_cpu.py establishes that, and the transitions a wave meets, without a GPU).
The references know nothing of the grid, so equality at every setting is grid independence.
tfidf_run's own persistent kernels follow the same count, so the result each setting starts from is
built at the small grid too (test_gpu_run_stride.py is the run's own test).

All comparisons are exact: integers, u64 bit patterns of doubles, bytes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dedup_ref
import oracle_py
import prune_ref
import stride_corpus as SC
import tfidf_abi
import weight_ref
from helpers import docs_to_arrays, hip
from kmeans_ref import KRef
from test_gpu_bm25 import Bm25Ref
from test_gpu_kmeans import check as km_check
from test_gpu_query import Ref as QRef, bits, check as q_check, make_queries
from test_gpu_similar import Ref as SRef, check as s_check
from test_gpu_terms import Ref as TRef, check as t_check
from test_gpu_weight import check_state

pytestmark = pytest.mark.gpu

N = SC.NDOCS
SCHEMES = [("ratio", "plus1", "l1"), ("ratio", "smooth", "none"), ("log", "smooth", "l2")]   # one per NORM; the flagship last
QUERY_KS = (1, 10, 1024)
TERMS_KS = (3, 100, 300)           # the register list, the 512-entry and the 2048-entry wave kernel; the big rows' kernel each time
KMEANS = ((8, 3, 10), (100, 3, 10), (130, 3, 10))     # k_km_assign<1>, <2>, <3>
MINHASH = (64, 192, 256)
NEAR_DUPS = ((64, 1), (192, 3), (128, 4))
THRESHOLDS = (0.0, 0.8)


def references() -> dict:
    """the corpus and every reference answer"""
    c = SC.build()
    data, off = docs_to_arrays(c["docs"])
    ora = oracle_py.run(data, off)
    ids = list(range(1, N + 1))
    order, n = c["order"], c["sizes"]
    w = dict(c=c, data=data, off=off, ora=ora, nbig=len(c["big"]))
    w["reweight"] = {s: (weight_ref.reweight(ora, *s, N=N), weight_ref.zero_norm_docs(ora, *s, N)) for s in SCHEMES}
    qs = make_queries(ora, np.random.default_rng(11), 80) + [SC.word(0) + b" " + SC.word(SC.NCOMMON - 1)]
    qref, bref = QRef(ora), Bm25Ref(ora, N, N)
    w["qs"], w["query"], w["bm25"] = qs, [qref.rank(q) for q in qs], [bref.rank(q) for q in qs]
    assert len(w["query"][-1][0]) >= w["nbig"]                                  # the last query hits every big document
    w["terms"] = TRef(ora, ids).rows()
    empty = next(p for p, x in enumerate(n) if x == 0)
    rows = [order[p] for p in (c["big"][0], c["big"][5], empty, c["families"][0][0])]
    rows += [d for d in order if d not in rows][:20]
    w["sim_docs"], w["similar"] = rows, SRef(ora, ids).rows(rows)
    assert len(rows) == 24
    kref = KRef(ora, ids)
    assert len(kref.clusterable) >= 130
    w["kmeans"] = {a: kref.run(*a) for a in KMEANS}
    pruned = prune_ref.prune(ora, 2)
    assert 0 < pruned["npairs"] < ora["npairs"]
    per_id = np.bincount(pruned["doc"], minlength=N + 1)
    w["pruned"], w["pruned_big"] = pruned, int((per_id > SC.RW_BIG).sum())
    assert w["pruned_big"] == w["nbig"]                                         # the blocks' words have df = 2
    w["pruned_rw"] = weight_ref.reweight(pruned, *SCHEMES[-1], N=N)
    dref = dedup_ref.DRef(ora, ids)
    w["dref"] = dref
    w["sig"] = {H: dref.signatures(H, 1) for H in MINHASH}
    w["dups"] = {(H, r, t): dref.near_dups(H, r, 1, t) for H, r in NEAR_DUPS for t in THRESHOLDS}
    return w


@pytest.fixture(scope="module")
def want():
    """computed once for the three settings"""
    return references()


def hip_attribute(name: str) -> int:
    """the value of an enumerator of hipDeviceAttribute_t, from the installed header"""
    path = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include", "hip", "hip_runtime_api.h")
    src = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(path).read(), flags=re.S)
    body = re.search(r"typedef\s+enum\s+hipDeviceAttribute_t\s*\{(.*?)\}", src, flags=re.S).group(1)
    seen, value = {}, -1
    for item in (x.strip() for x in body.split(",")):
        if not item:
            continue
        key, _, rhs = (x.strip() for x in item.partition("="))
        value = value + 1 if not rhs else seen[rhs] if rhs in seen else int(rhs, 0)
        seen[key] = value
    return seen[name]


def device_cus() -> int:
    """device 0's CU count, asked of the HIP runtime and not of the library under test"""
    n = C.c_int(0)
    assert hip().hipDeviceGetAttribute(C.byref(n), hip_attribute("hipDeviceAttributeMultiprocessorCount"), 0) == 0
    assert 1 <= n.value <= 4096
    return n.value


@pytest.mark.parametrize("cus", ["1", "2", None])
def test_every_result_call_at_this_cu_count(want, cus, monkeypatch):
    if cus is None:
        monkeypatch.delenv("TFIDF_GRID_CUS", raising=False)
    else:
        monkeypatch.setenv("TFIDF_GRID_CUS", cus)
    w, ora = want, want["ora"]
    with tfidf_abi.Engine(0) as e:                                              # the environment is read at tfidf_open
        assert e.grid_cus() == (int(cus) if cus else device_cus())
        e.run_host(w["data"], w["off"])
        check_state(e, ora)                                                     # fetch and text: the corpus is what the oracle saw
        queries(e, w)
        top_terms(e, w)
        similar_kmeans(e, w)
        dedup(e, w)
        reweight_transform(e, w)
        prune_then_reweight(e, w)
        assert e.grid_cus() == (int(cus) if cus else device_cus())


def queries(e, w):
    for k in QUERY_KS:
        q_check(e.query(w["qs"], k), w["query"], k)
        q_check(e.query_bm25(w["qs"], k), w["bm25"], k)


def top_terms(e, w):
    for k in TERMS_KS:
        t_check(e.top_terms(k), w["terms"], k)


def similar_kmeans(e, w):
    s_check(e.similar(10, w["sim_docs"]), w["similar"], 10)
    for a, ref in w["kmeans"].items():
        km_check(e.kmeans(*a), ref)


def dedup(e, w):
    dref = w["dref"]
    for H in MINHASH:
        got = e.minhash(H, 1)
        assert got["nhashes"] == H and [int(d) for d in got["doc"]] == dref.order and [int(x) for x in got["npairs"]] == dref.n
        assert np.array_equal(got["sig"], w["sig"][H]), H
        assert e.dedup_info()["big_docs"] == w["nbig"]
    for (H, r, thr), ref in w["dups"].items():
        dedup_ref.assert_same_dups(e.near_dups(thr, H, r, 1), ref)
        info = e.dedup_info()
        assert (info["ncand"], info["nedges"], info["big_docs"]) == (ref["ncand"], ref["nedges"], w["nbig"]), (H, r, thr)


def reweight_transform(e, w):
    for s in SCHEMES:
        ref, zero = w["reweight"][s]
        info = e.reweight(*s)
        check_state(e, ref)
        assert (info["big_docs"], info["zero_norm_docs"]) == (w["nbig"], zero), s
    # the corpus's own documents through tfidf_transform under the flagship scheme: the row norm's
    # two launches give the resident pairs bit for bit
    f = e.fetch()
    res = e.transform(w["data"], w["off"])
    ro = res["row_off"].tolist()
    for i in range(N):                                                          # rows in batch order, the result in name order
        sel = np.flatnonzero(f["doc"] == i + 1)
        assert np.array_equal(res["term"][ro[i]:ro[i + 1]], f["term"][sel]), i + 1
        assert np.array_equal(res["count"][ro[i]:ro[i + 1]], f["count"][sel]), i + 1
        assert np.array_equal(bits(res["score"][ro[i]:ro[i + 1]]), bits(f["score"][sel])), i + 1
    e.reweight(*weight_ref.REFERENCE)
    check_state(e, w["ora"])


def prune_then_reweight(e, w):
    e.prune(2)
    check_state(e, w["pruned"])
    info = e.reweight(*SCHEMES[-1])
    check_state(e, w["pruned_rw"])
    assert info["big_docs"] == w["pruned_big"]
