"""Reference for tfidf_prune in plain Python: a filter of a result dict (oracle_py.run's or
Engine.fetch's) and a filter of output lines.

A term survives the range test when (min_df <= 1 or df >= min_df) and (max_df == 0 or
df <= max_df); with max_features = M > 0 only the first M survivors stay, by df descending, then
by word + b"\\t" ascending (the term table's strcmp order: ranks are compared through the words,
never through an index, because the oracle numbers terms by first appearance).  Nothing that
stays is recomputed: the kept pairs are the input's own array elements."""
from __future__ import annotations

import numpy as np


def term_df(res: dict) -> np.ndarray:
    """df per term index (every term has at least one pair, which carries it)"""
    if "term_df" in res:
        return np.asarray(res["term_df"], dtype=np.uint32)
    df = np.zeros(len(res["terms"]), dtype=np.uint32)
    df[res["term"]] = res["df"]
    return df


def keep_mask(terms, df, min_df: int = 0, max_df: int = 0, max_features: int = 0) -> np.ndarray:
    df = [int(d) for d in df]
    keep = [(min_df <= 1 or d >= min_df) and (max_df == 0 or d <= max_df) for d in df]
    if max_features > 0:
        surv = sorted((i for i in range(len(df)) if keep[i]), key=lambda i: (-df[i], terms[i] + b"\t"))
        for i in surv[max_features:]:
            keep[i] = False
    return np.array(keep, dtype=bool)


def kept_words(res: dict, min_df: int = 0, max_df: int = 0, max_features: int = 0) -> set:
    k = keep_mask(res["terms"], term_df(res), min_df, max_df, max_features)
    return {w for w, f in zip(res["terms"], k.tolist()) if f}


def filter_lines(text: bytes, words: set) -> bytes:
    """the lines "docN@word\\t%.16f\\n" whose word is kept, in the same order (a word holds no TAB
    and a document name no '@')"""
    out = []
    for line in text.split(b"\n"):
        if not line:
            continue
        word = line[line.index(b"@") + 1:line.rindex(b"\t")]
        if word in words:
            out.append(line + b"\n")
    return b"".join(out)


def prune(res: dict, min_df: int = 0, max_df: int = 0, max_features: int = 0) -> dict:
    """the result dict without the pruned terms and their pairs, pair terms renumbered"""
    df = term_df(res)
    keep = keep_mask(res["terms"], df, min_df, max_df, max_features)
    new = np.cumsum(keep) - 1
    pk = keep[res["term"]] if len(res["term"]) else np.zeros(0, dtype=bool)
    out = {k: v for k, v in res.items() if k not in ("tf_jobs", "idf_jobs")}
    for name in ("doc", "count", "docsize", "df", "score"):
        out[name] = res[name][pk]
    out["term"] = new[res["term"][pk]].astype(np.uint32) if pk.any() else np.zeros(0, dtype=np.uint32)
    out["terms"] = [w for w, f in zip(res["terms"], keep.tolist()) if f]
    out["npairs"] = int(pk.sum())
    out["nterms"] = len(out["terms"])
    if "term_df" in res:
        out["term_df"] = df[keep]
    out["output_txt"] = filter_lines(res["output_txt"], set(out["terms"]))
    return out


def emptied_docs(before: dict, after: dict) -> int:
    """documents that hold pairs before and none after"""
    return len(set(before["doc"].tolist()) - set(after["doc"].tolist()))


def prune_model(model: dict, min_df: int = 0, max_df: int = 0, max_features: int = 0) -> dict:
    """a model dict (N, terms in term-table order, df) without the pruned terms"""
    keep = keep_mask(model["terms"], model["df"], min_df, max_df, max_features)
    return {"N": int(model["N"]), "terms": [w for w, f in zip(model["terms"], keep.tolist()) if f],
            "df": np.asarray(model["df"], dtype=np.uint32)[keep]}
