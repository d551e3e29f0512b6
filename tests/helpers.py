"""Shared test helpers: golden fixture loading and result comparison."""
from __future__ import annotations

import contextlib
import ctypes as C
import json
import os

import numpy as np

from conftest import GOLDEN


def read_dir_corpus(input_dir: str):
    """Reference input contract (TFIDF.c:98-110,130-139): N = entries, docs doc1..docN."""
    names = [n for n in os.listdir(input_dir) if n not in (".", "..")]
    n = len(names)
    docs = []
    for i in range(1, n + 1):
        with open(os.path.join(input_dir, f"doc{i}"), "rb") as f:
            docs.append(f.read())
    return docs_to_arrays(docs)


def docs_to_arrays(docs):
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
    data = np.frombuffer(b"".join(docs), dtype=np.uint8).copy()
    return data, off


def load_golden(case: str):
    d = os.path.join(GOLDEN, case)
    data, off = read_dir_corpus(os.path.join(d, "input"))
    with open(os.path.join(d, "output.txt"), "rb") as f:
        out = f.read()
    with open(os.path.join(d, "tf_jobs.txt"), "rb") as f:
        tf = f.read()
    with open(os.path.join(d, "idf_jobs.txt"), "rb") as f:
        idf = f.read()
    with open(os.path.join(d, "meta.json")) as f:
        meta = json.load(f)
    return dict(data=data, off=off, output=out, tf_jobs=tf, idf_jobs=idf, meta=meta)


def sorted_lines(b: bytes) -> bytes:
    lines = [x for x in b.split(b"\n") if x]
    return b"".join(x + b"\n" for x in sorted(lines))


def jobs_from_result(res: dict):
    """TF Job / IDF Job lines (TFIDF.c:204,239) rebuilt from a fetched GPU result."""
    terms = res["terms"]
    tf, idf = [], []
    N = res["ndocs_total"]
    for d, t, c, ds, df in zip(res["doc"].tolist(), res["term"].tolist(), res["count"].tolist(),
                               res["docsize"].tolist(), res["df"].tolist()):
        w = terms[t]
        tf.append(w + b"@doc%d\t%d/%d" % (d, c, ds))
        idf.append(w + b"@doc%d\t%d/%d" % (d, N, df))
    return b"".join(x + b"\n" for x in sorted(tf)), b"".join(x + b"\n" for x in sorted(idf))


def describe_diff(gpu: dict, ora: dict) -> str:
    """First document whose pairs differ, for the failure message."""
    def by_doc(r):
        out = {}
        for d, t, c, ds in zip(r["doc"].tolist(), r["term"].tolist(), r["count"].tolist(), r["docsize"].tolist()):
            out.setdefault(d, []).append((r["terms"][t], c, ds))
        return out
    g, o = by_doc(gpu), by_doc(ora)
    for d in sorted(set(g) | set(o)):
        if g.get(d) != o.get(d):
            gs, os_ = g.get(d, []), o.get(d, [])
            extra = sorted(set(gs) - set(os_))[:10]
            missing = sorted(set(os_) - set(gs))[:10]
            return (f"doc{d}: gpu {len(gs)} pairs, oracle {len(os_)}; gpu-only {extra}; oracle-only {missing}; "
                    f"docsize gpu {gs[0][2] if gs else None} oracle {os_[0][2] if os_ else None}")
    return "no per-document difference"


def assert_same_result(gpu: dict, ora: dict, exact_scores: bool = True):
    """Field-by-field parity: integers bit-exact, scores exact (or <= 1e-12 relative)."""
    assert gpu["npairs"] == ora["npairs"], describe_diff(gpu, ora)
    np.testing.assert_array_equal(gpu["doc"], ora["doc"])
    gterms = [gpu["terms"][t] for t in gpu["term"].tolist()]
    oterms = [ora["terms"][t] for t in ora["term"].tolist()]
    assert gterms == oterms
    np.testing.assert_array_equal(gpu["count"], ora["count"])
    np.testing.assert_array_equal(gpu["docsize"], ora["docsize"])
    np.testing.assert_array_equal(gpu["df"], ora["df"])
    if exact_scores:
        np.testing.assert_array_equal(gpu["score"].view(np.uint64), ora["score"].view(np.uint64))
    else:
        np.testing.assert_allclose(gpu["score"], ora["score"], rtol=1e-12, atol=0)


def _chunk_bounds(doc: np.ndarray, chunk: int):
    """pair ranges of about `chunk` pairs, each starting at a document's first pair"""
    P = len(doc)
    b = [0]
    for t in range(chunk, P, chunk):
        if t <= b[-1]:
            continue
        j, w = t, 1 << 16
        while j < P:
            seg = doc[j - 1:j + w]
            ch = np.flatnonzero(seg[1:] != seg[:-1])
            if len(ch):
                j += int(ch[0])
                break
            j += w
        if j < P:
            b.append(j)
    b.append(P)
    return b


def check_full_properties(r: dict, ntokens: int, threads: int = 8, chunk: int = 1 << 26):
    """Size-independent properties of a result (the views of Engine.fetched(), any size),
    checked in document-aligned chunks on a thread pool so that full-size configurations
    need no copy of the pairs:
      counts sum to the tokens; per document (a contiguous run of pairs): sum of counts =
      docSize (TFIDF.c:141-167), docSize as the run's documents report it; terms strictly
      increasing inside a document and documents strictly increasing in "docN@" strcmp
      order, each document one run (TFIDF.c:245,273); DF = pairs per term (TFIDF.c:169-234);
      score = count/docSize * log(N/df) within 1e-12 relative (TFIDF.c:202,243-244)."""
    from concurrent.futures import ThreadPoolExecutor
    import tfidf_configs
    P, V, N = r["npairs"], r["nterms"], r["ndocs_total"]
    doc, term, cnt, dsz, df, score, tdf = (r[k] for k in ("doc", "term", "count", "docsize", "df", "score", "term_df"))
    assert P > 0 and len(doc) == P
    bounds = _chunk_bounds(doc, chunk)

    def one(i):
        a, b = bounds[i], bounds[i + 1]
        d, t, c = doc[a:b], term[a:b], cnt[a:b].astype(np.int64)
        st = np.flatnonzero(np.r_[True, d[1:] != d[:-1]])
        assert np.array_equal(np.add.reduceat(c, st), dsz[a:b][st].astype(np.int64)), "per-document sums"
        same = d[1:] == d[:-1]
        assert np.all(~same | (t[1:] > t[:-1])), "term order inside a document"
        assert np.all(~same | (dsz[a + 1:b] == dsz[a:b - 1])), "docSize constant inside a document"
        assert np.array_equal(df[a:b], tdf[t]), "df = the term's df"
        ds = dsz[a:b].astype(np.float64)
        ref = (c / ds) * np.log(N / df[a:b].astype(np.float64))
        err = np.abs(score[a:b] - ref)
        assert np.all(err <= 1e-12 * np.abs(ref) + 1e-300), "scores"
        return int(c.sum()), np.bincount(t, minlength=V), d[st].copy(), dsz[a:b][st].copy()

    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(one, range(len(bounds) - 1)))
    assert sum(p[0] for p in parts) == ntokens
    dfc = np.zeros(V, dtype=np.int64)
    for p in parts:
        dfc += p[1]
    assert np.array_equal(dfc, tdf.astype(np.int64)), "DF = pairs per term"
    runs = np.concatenate([p[2] for p in parts])
    run_ds = np.concatenate([p[3] for p in parts])
    key = tfidf_configs.doc_name_key(runs)
    assert np.all(key[1:] > key[:-1]), "documents strictly increasing, one run each"
    # the run's docSize is the document's (tfidf_result doc_id/doc_size); empty documents have no run
    ids, sizes = r["doc_id"], r["doc_size"]
    o = np.argsort(ids, kind="stable")
    pos = np.searchsorted(ids[o], runs)
    assert np.array_equal(ids[o][pos], runs) and np.array_equal(sizes[o][pos], run_ds)
    assert int(sizes.astype(np.int64).sum()) == ntokens
    # term table in strcmp("word\t") order
    toff, tb = r["term_off"], r["term_bytes"]
    step = max(1, V // 200_000)
    for i in range(0, V - 1, step):
        x = bytes(tb[int(toff[i]):int(toff[i + 1])]) + b"\t"
        y = bytes(tb[int(toff[i + 1]):int(toff[i + 2])]) + b"\t"
        assert x < y, (i, x, y)


# ---- corpus windows: doc_off[0] > 0, doc_off[ndocs] < nbytes, caller-owned device buffers ----

_PAD = b"Qq "


def pad_before(n: int) -> bytes:
    """n padding bytes in front of a window: whole words "Qq" separated by blanks, the last
    byte (the one just before the window) a letter"""
    return (_PAD * (n // 3 + 2))[:-1][-n:] if n else b""


def pad_after(n: int) -> bytes:
    """n padding bytes behind a window: the first byte (the one at the window's end) a letter"""
    return (_PAD * (n // 3 + 2))[:n]


def windowed(docs, lead: int, trail: int):
    """The packed documents between `lead` and `trail` bytes that belong to no document
    (include/tfidf.h: doc_off[0] > 0, doc_off[ndocs] < nbytes).  The padding holds words of
    its own, and a letter touches the window on both sides: a token extended over a boundary
    and a byte counted outside the window both change the result."""
    data, off = docs_to_arrays(docs)
    buf = pad_before(lead) + data.tobytes() + pad_after(trail)
    return np.frombuffer(buf, dtype=np.uint8).copy(), off + np.uint64(lead)


_hip = None


def hip():
    """the HIP runtime through ctypes (test plumbing: allocation and copies only)"""
    global _hip
    if _hip is None:
        h = C.CDLL("libamdhip64.so")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipFree.argtypes = [C.c_void_p]
        _hip = h
    return _hip


def _to_device(host: np.ndarray) -> int:
    p = C.c_void_p()
    assert hip().hipMalloc(C.byref(p), max(host.nbytes, 16)) == 0
    if host.nbytes:
        assert hip().hipMemcpy(p, host.ctypes.data, host.nbytes, 1) == 0
    return p.value


@contextlib.contextmanager
def device_corpus(data, off, ids=None, n_total: int = 0, shift: int = 0):
    """A tfidf_abi.Corpus with flags = TFIDF_CORPUS_DEVICE in buffers of the caller's own.
    The bytes lie in an allocation of whole 4 KiB pages with at least 256 bytes of padding
    words (pad_before / pad_after) on both sides, the corpus base at the allocation's start
    + 256 + shift: a kernel that reads past an edge of the corpus stays inside the allocation
    and gives a wrong result.  doc_off and doc_ids are device arrays.  Everything stays
    allocated until the context exits (text(), fetch(), top_terms and query read long terms
    from the corpus bytes)."""
    import tfidf_abi
    assert 0 <= shift < 16
    data = np.ascontiguousarray(data, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32)
    front = 256 + shift
    total = (front + len(data) + 256 + 4095) & ~4095
    image = np.frombuffer(pad_before(front) + data.tobytes() + pad_after(total - front - len(data)), dtype=np.uint8)
    ptrs = []
    try:
        ptrs.append(_to_device(image))
        assert ptrs[0] % 16 == 0
        ptrs.append(_to_device(off))
        if ids is not None:
            ptrs.append(_to_device(ids))
        assert hip().hipDeviceSynchronize() == 0
        c = tfidf_abi.Corpus()
        c.bytes = ptrs[0] + front
        c.nbytes = len(data)
        c.doc_off = ptrs[1]
        c.doc_ids = None if ids is None else ptrs[2]
        c.ndocs = len(off) - 1
        c.flags = tfidf_abi.TFIDF_CORPUS_DEVICE
        c.ndocs_total = n_total
        yield c
    finally:
        hip().hipDeviceSynchronize()
        for p in ptrs:
            hip().hipFree(p)


# The four tokenize+count (K1) kernel instances and the environment that selects each
# (read by tfidf_open, so every instance has an Engine of its own).
K1_INSTANCES = {
    "sl_fast": {},                              # k_tokcount_sl<true>: the default
    "sl_full": {"TFIDF_VCAP": "8388608"},       # k_tokcount_sl<false>: past 2^22 vocabulary slots
    "vs": {"TFIDF_K1": "vs"},                   # k_tokcount_vs: what runs past 2^25 slots
    "general": {"TFIDF_K1": "general"},         # k_tokcount: what an unaligned corpus base gets
}
_K1_ENV = ("TFIDF_K1", "TFIDF_VCAP", "TFIDF_VLOAD", "TFIDF_VLOAD_BIG", "TFIDF_SL_MAXCAP")


@contextlib.contextmanager
def k1_engine(instance: str):
    """an Engine opened under the instance's environment; the environment is restored as soon
    as the engine is open"""
    import tfidf_abi
    saved = {k: os.environ.pop(k, None) for k in _K1_ENV}
    os.environ.update(K1_INSTANCES[instance])
    try:
        e = tfidf_abi.Engine(0)
    finally:
        for k in _K1_ENV:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    try:
        yield e
    finally:
        e.close()


def assert_k1_instance(info: dict, instance: str):
    """the last run (Engine.info()) took the kernel instance it is named for"""
    import tfidf_abi
    f, cap = info["flags"], info["vocab_capacity"]
    if instance == "sl_fast":
        assert f & tfidf_abi.RUN_K1_SL and cap <= 1 << 22, (f, cap)
    elif instance == "sl_full":
        assert f & tfidf_abi.RUN_K1_SL and cap == 1 << 23, (f, cap)
    elif instance == "vs":
        assert (f & 3) == 2 and not f & tfidf_abi.RUN_K1_SL, f
    else:
        assert instance == "general" and (f & 3) == 0, f


def k1_fixture(instances):
    """a module-scoped fixture over K1 instances: (instance name, its Engine)"""
    import pytest

    @pytest.fixture(scope="module", params=list(instances))
    def k1(request):
        with k1_engine(request.param) as e:
            yield request.param, e
    return k1
