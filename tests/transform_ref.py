"""Reference for tfidf_transform in plain Python, over oracle_py.run of the fitted corpus.

Tokens: doc.split() (bytes.split cuts at exactly the six bytes 0x20, 0x09..0x0D); term:
tok.split(b"\\0")[0]; vocabulary and df: the oracle's; score: (c / ds) * math.log(N / df), the
reference's two operations on the host's libm (TFIDF.c:202,243-244); pairs ordered by
word + b"\\t" (TFIDF.c:245,273).  Words are compared by their bytes, never by an index: the
oracle numbers terms by first appearance, the library by rank."""
from __future__ import annotations

import math
import re

import numpy as np

import oracle_py

_TOKEN = re.compile(rb"[^ \t\n\r\x0b\x0c]+")


class Model:
    """the fitted corpus: N and the global df of every word"""

    def __init__(self, data, off, doc_ids=None, n_total: int = 0):
        ora = oracle_py.run(data, off, doc_ids, n_total)
        self.N = int(n_total) if n_total else len(off) - 1
        self.df = {}
        for t, d in zip(ora["term"].tolist(), ora["df"].tolist()):
            self.df[ora["terms"][t]] = d
        self.oracle = ora

    def row(self, doc: bytes) -> dict:
        toks = [(m.group(), m.start()) for m in _TOKEN.finditer(doc)]
        assert [t for t, _ in toks] == doc.split()
        ds = len(toks)
        count, first = {}, {}
        for tok, at in toks:
            w = tok.split(b"\0")[0]
            if w in self.df:
                count[w] = count.get(w, 0) + 1
                first.setdefault(w, at)
        words = sorted(count, key=lambda w: w + b"\t")
        return {
            "doc_size": ds, "doc_oov": ds - sum(count.values()), "words": words,
            "count": [count[w] for w in words], "df": [self.df[w] for w in words],
            "score": [(count[w] / ds) * math.log(self.N / self.df[w]) for w in words],
            "first": [first[w] for w in words],
        }

    def rows(self, docs) -> list:
        return [self.row(bytes(d)) for d in docs]


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def split_docs(data, off) -> list:
    b = np.ascontiguousarray(data, dtype=np.uint8).tobytes()
    o = [int(x) for x in off]
    return [b[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def totals(rows) -> dict:
    """tokens, out-of-vocabulary tokens, pairs, pairs scoring +0.0"""
    return {"tokens": sum(r["doc_size"] for r in rows), "oov": sum(r["doc_oov"] for r in rows),
            "pairs": sum(len(r["words"]) for r in rows),
            "zero": sum(1 for r in rows for s in r["score"] if s == 0.0)}


def check(res: dict, rows: list, off, terms=None):
    """Engine.transform's dict against the reference rows: integers exactly, scores as u64
    bits, the words and their offsets in the batch; terms: the engine's term table
    (fetch()["terms"]) to check the term ranks against, None for a group result."""
    n = len(rows)
    assert res["ndocs"] == n and len(res["row_off"]) == n + 1
    assert res["doc_size"].tolist() == [r["doc_size"] for r in rows]
    assert res["doc_oov"].tolist() == [r["doc_oov"] for r in rows]
    ro = res["row_off"].tolist()
    assert ro[0] == 0 and ro[-1] == res["npairs"] == sum(len(r["words"]) for r in rows)
    assert res["ntokens"] == sum(r["doc_size"] for r in rows)
    for i, r in enumerate(rows):
        a, b = ro[i], ro[i + 1]
        assert res["words"][a:b] == r["words"], (i, res["words"][a:b][:5], r["words"][:5])
        assert res["count"][a:b].tolist() == r["count"], i
        assert res["df"][a:b].tolist() == r["df"], i
        assert np.array_equal(bits(res["score"][a:b]), bits(r["score"])), i
        assert res["word_len"][a:b].tolist() == [len(w) for w in r["words"]], i
        assert res["word_off"][a:b].tolist() == [int(off[i]) + f for f in r["first"]], i
        if terms is not None:
            assert [terms[t] for t in res["term"][a:b].tolist()] == r["words"], i
            assert np.all(np.diff(res["term"][a:b].astype(np.int64)) > 0), i
        else:
            assert np.all(res["term"][a:b] == 0xFFFFFFFF), i
