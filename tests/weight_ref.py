"""Reference for the weighting schemes (include/tfidf.h, section "weighting") in plain Python:
the definition on a result dict (oracle_py.run's or Engine.fetch's) by math.log, math.sqrt,
Python floats and left folds, and the output lines by "%.16f".

Every Python float operation is one IEEE binary64 operation rounded to nearest, and nothing here
is vectorised: a sum is a loop that adds one rounded term after the other, in pair order."""
from __future__ import annotations

import math

import numpy as np

TF = {"ratio": 0, "raw": 1, "log": 2, "binary": 3}
IDF = {"ref": 0, "smooth": 1, "plus1": 2, "none": 3}
NORM = {"none": 0, "l2": 1, "l1": 2}
REFERENCE = ("ratio", "ref", "none")


def valid(tf: str, idf: str, norm: str, N: int = 1) -> bool:
    """the two static limits of the header"""
    if tf == "raw" and norm == "none":
        return False
    if tf == "log" and norm == "none" and N >= 1 << 48:
        return False
    return True


def all_schemes(N: int = 1) -> list:
    return [(t, i, n) for t in TF for i in IDF for n in NORM if valid(t, i, n, N)]


def tf_of(mode: str, c: int, ds: int) -> float:
    if mode == "ratio":
        return float(c) / float(ds)
    if mode == "raw":
        return float(c)
    if mode == "log":
        return 1.0 + math.log(float(c))
    return 1.0


def idf_of(mode: str, N: int, df: int) -> float:
    if mode == "ref":
        return math.log(1.0 * float(N) / float(df))
    if mode == "smooth":
        return math.log((float(N) + 1.0) / (float(df) + 1.0)) + 1.0
    if mode == "plus1":
        return math.log(1.0 * float(N) / float(df)) + 1.0
    return 1.0


def norm_of(ws: list, norm: str, fused: bool = False) -> float:
    """the row's divisor: sqrt of the ordered sum of rounded squares (l2), the ordered sum (l1).
    fused: what a compiler that contracts w * w + sum into one fma would compute (l2 only), for
    the tests' assertion that the corpus can tell the two apart."""
    s = 0.0
    for w in ws:
        if norm == "l2":
            s = _fma(w, w, s) if fused else s + w * w
        else:
            s = s + w
    return math.sqrt(s) if norm == "l2" else s


def _fma(a: float, b: float, c: float) -> float:
    """a * b + c rounded once, exactly (rationals)"""
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def normalize(ws: list, norm: str) -> list:
    if norm == "none":
        return list(ws)
    n = norm_of(ws, norm)
    if n == 0.0:
        return list(ws)
    return [w / n for w in ws]


def doc_runs(doc) -> list:
    """[b, e) of every maximal run of equal document ids"""
    d = np.asarray(doc)
    if len(d) == 0:
        return []
    st = np.flatnonzero(np.r_[True, d[1:] != d[:-1]]).tolist() + [len(d)]
    return list(zip(st[:-1], st[1:]))


def weights(res: dict, tf: str, idf: str, N: int) -> list:
    """w(d, t) = fl(tf * idf) per pair"""
    return [tf_of(tf, c, ds) * idf_of(idf, N, df)
            for c, ds, df in zip(res["count"].tolist(), res["docsize"].tolist(), res["df"].tolist())]


def scores(res: dict, tf: str, idf: str, norm: str, N: int) -> np.ndarray:
    w = weights(res, tf, idf, N)
    out = []
    for b, e in doc_runs(res["doc"]):
        out.extend(normalize(w[b:e], norm))
    return np.array(out, dtype=np.float64)


def lines(res: dict, score) -> bytes:
    """"docN@word\\t%.16f\\n" per pair, in pair order"""
    terms = res["terms"]
    return b"".join(b"doc%d@" % d + terms[t] + b"\t%.16f\n" % s
                    for d, t, s in zip(res["doc"].tolist(), res["term"].tolist(), np.asarray(score).tolist()))


def n_of(res: dict, N=None) -> int:
    if N:
        return int(N)
    if res.get("ndocs_total"):
        return int(res["ndocs_total"])
    raise ValueError("N is not known: pass it")


def reweight(res: dict, tf: str = "ratio", idf: str = "ref", norm: str = "none", N=None) -> dict:
    """the result dict with score and output_txt replaced; everything else is the input's"""
    N = n_of(res, N)
    assert valid(tf, idf, norm, N)
    out = {k: v for k, v in res.items() if k not in ("tf_jobs", "idf_jobs")}
    out["score"] = scores(res, tf, idf, norm, N)
    out["output_txt"] = lines(res, out["score"])
    return out


def zero_norm_docs(res: dict, tf: str, idf: str, norm: str, N: int) -> int:
    """documents that hold pairs and whose norm is 0"""
    if norm == "none":
        return 0
    w = weights(res, tf, idf, N)
    return sum(1 for b, e in doc_runs(res["doc"]) if norm_of(w[b:e], norm) == 0.0)


def rows(tr_rows: list, tf: str, idf: str, norm: str, N: int) -> list:
    """transform_ref.Model.rows() under a scheme: score replaced per row"""
    out = []
    for r in tr_rows:
        w = [tf_of(tf, c, r["doc_size"]) * idf_of(idf, N, df) for c, df in zip(r["count"], r["df"])]
        q = dict(r)
        q["score"] = normalize(w, norm)
        out.append(q)
    return out


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
