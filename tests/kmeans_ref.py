"""Spherical k-means (include/tfidf.h, section "clusters") as plain Python floats over the
oracle's pairs: the reference of test_gpu_kmeans.py and of the CLI test.

Every product and every sum below is one IEEE binary64 operation, in the definition's order:
Python floats never fuse, numpy's elementwise product rounds each product on its own, and
np.cumsum adds strictly left to right.  A centroid is kept sparse (term -> weight); a term it
does not hold would add +0.0 to a sum that is >= +0.0, which changes no bit, so such terms are
left out of the sums.

  KRef(ora, doc_ids).run(k, max_iter, nterms, seeds) -> dict
  KRef.fused_differs(res)   would a kernel that fuses products into sums return other bits?
"""
import math
from fractions import Fraction

import numpy as np

NO_CLUSTER = 0xFFFFFFFF


class KRef:
    def __init__(self, ora, doc_ids):
        self.ids = [int(d) for d in doc_ids]
        self.order = sorted(self.ids, key=lambda d: b"doc%d@" % d)       # output order (TFIDF.c:273)
        self.pos = {d: j for j, d in enumerate(self.order)}
        # term rank: the strcmp order of "word\t", the order of the pairs inside a document
        words = ora["terms"]
        by_rank = sorted(range(len(words)), key=lambda i: words[i] + b"\t")
        rank = {i: r for r, i in enumerate(by_rank)}
        self.words = [words[i] for i in by_rank]
        vec = {d: [] for d in self.ids}
        for d, t, s in zip(ora["doc"].tolist(), ora["term"].tolist(), ora["score"].tolist()):
            vec[d].append((rank[t], s))
        self.norm, self.t, self.u = [], [], []                           # by output position
        for d in self.order:
            v = sorted(vec[d])
            acc = 0.0
            for _, s in v:
                acc = acc + s * s
            n = math.sqrt(acc)
            self.norm.append(n)
            self.t.append(np.array([t for t, _ in v], dtype=np.int64))
            self.u.append(np.array([s / n for _, s in v], dtype=np.float64) if n > 0.0 else np.zeros(len(v)))
        self.clusterable = [j for j, n in enumerate(self.norm) if n > 0.0]

    # ---- pieces of the definition ----
    def default_seeds(self, k):
        m = len(self.clusterable)
        return [self.order[self.clusterable[c * m // k]] for c in range(k)]

    def check_seeds(self, k, seeds):
        """the ids as the library would take them, or None where it answers TFIDF_E_INVAL"""
        if k < 1 or k > 256 or k > len(self.clusterable):
            return None
        if seeds is None:
            return self.default_seeds(k)
        seeds = [int(s) for s in seeds]
        if len(seeds) != k or len(set(seeds)) != k:
            return None
        if any(s not in self.pos or not self.norm[self.pos[s]] > 0.0 for s in seeds):
            return None
        return seeds

    @staticmethod
    def _dense(cent):
        """a sparse centroid as sorted arrays for the lookups of assign"""
        ts = np.array(sorted(cent), dtype=np.int64)
        return ts, np.array([cent[int(t)] for t in ts], dtype=np.float64)

    def _weights(self, j, ct, cw):
        """C[c][t] for the terms of the document at position j (+0.0 where the centroid has none)"""
        t = self.t[j]
        if not len(ct) or not len(t):
            return np.zeros(len(t))
        at = np.searchsorted(ct, t)
        at[at >= len(ct)] = 0
        return np.where(ct[at] == t, cw[at], 0.0)

    def sim(self, j, ct, cw):
        prod = self.u[j] * self._weights(j, ct, cw)                      # each product rounded
        return float(np.cumsum(prod)[-1]) if len(prod) else 0.0         # +0.0 + p1 is p1: all >= +0.0

    def assign(self, cents):
        dense = [self._dense(c) for c in cents]
        label, sim = [], []
        for j in range(len(self.order)):
            if not self.norm[j] > 0.0:
                label.append(NO_CLUSTER)
                sim.append(0.0)
                continue
            best, bc = -1.0, 0
            for c, (ct, cw) in enumerate(dense):
                x = self.sim(j, ct, cw)
                if x > best:                                             # ties: the lowest c
                    best, bc = x, c
            label.append(bc)
            sim.append(best)
        return label, sim

    def sums(self, label, c):
        S = {}
        for j, lab in enumerate(label):                                  # ascending output position
            if lab == c:
                for t, u in zip(self.t[j].tolist(), self.u[j].tolist()):
                    S[t] = S.get(t, 0.0) + u
        return S

    @staticmethod
    def normalise(S):
        sq = 0.0
        for t in sorted(S):                                              # ascending term rank
            if S[t] != 0.0:
                sq = sq + S[t] * S[t]
        nrm = math.sqrt(sq)
        return {t: S[t] / nrm for t in S}

    # ---- the loop ----
    def run(self, k, max_iter=0, nterms=10, seeds=None):
        seeds = self.check_seeds(k, seeds)
        if seeds is None or nterms > 64:
            return None
        max_iter = max_iter or 20
        cents = []
        for s in seeds:
            j = self.pos[s]
            cents.append(dict(zip(self.t[j].tolist(), self.u[j].tolist())))
        prev, last_sums = None, {}
        it, converged = 0, 0
        while True:
            it += 1
            label, sim = self.assign(cents)
            if it > 1 and label == prev:
                converged = 1
                break
            if it == max_iter:
                break
            for c in range(k):
                if c in label:
                    last_sums[c] = self.sums(label, c)
                    cents[c] = self.normalise(last_sums[c])
            prev = label
        size = [label.count(c) for c in range(k)]
        top = []
        for cent in cents:
            best = sorted(((w, t) for t, w in cent.items() if w != 0.0), key=lambda x: (-x[0], x[1]))[:nterms]
            top.append([(t, w, self.words[t]) for w, t in best])
        return dict(k=k, iterations=it, converged=converged, doc=list(self.order), label=label, sim=sim, size=size,
                    seed=seeds, top=top, cents=cents, last_sums=last_sums)

    def fused_differs(self, res):
        """Would fma(u, w, acc) in the assignment or fma(S, S, acc) in the centroid norm change
        a bit of the result?  Recomputes, with one rounding per product-and-add (exact
        Fractions), every document's sim to its own (final) centroid and every updated
        centroid's weights from the last update's sums."""
        for j, lab in enumerate(res["label"]):
            if lab == NO_CLUSTER:
                continue
            cent = res["cents"][lab]
            acc = 0.0
            for t, u in zip(self.t[j].tolist(), self.u[j].tolist()):
                w = cent.get(t, 0.0)
                if w != 0.0:
                    acc = float(Fraction(u) * Fraction(w) + Fraction(acc))
            if acc != res["sim"][j]:
                return True
        for c, S in res["last_sums"].items():
            sq = 0.0
            for t in sorted(S):
                sq = float(Fraction(S[t]) * Fraction(S[t]) + Fraction(sq))
            nrm = math.sqrt(sq)
            if any(S[t] / nrm != res["cents"][c][t] for t in S):
                return True
        return False


def cluster_lines(res):
    """clusters.txt of the CLI: a line per cluster, then a line per document in output order"""
    out = []
    for c in range(res["k"]):
        out.append(b"c%d\t%d\t" % (c, res["size"][c]) + b" ".join(b"%s:%.16f" % (w, x) for _, x, w in res["top"][c]) + b"\n")
    for d, lab, s in zip(res["doc"], res["label"], res["sim"]):
        out.append(b"doc%d\t-\t0.0000000000000000\n" % d if lab == NO_CLUSTER else b"doc%d\tc%d\t%.16f\n" % (d, lab, s))
    return b"".join(out)
