"""The reference for tfidf_query_clauses (include/tfidf.h, "clauses") over an oracle result: the
OR ranking of the text must + " " + should with one operation per statement (as
test_gpu_query.Ref and test_gpu_bm25.Bm25Ref do it), filtered by the four conditions, and the
generators of the queries the tests run.

A query is a dict: must, should, must_not (bytes), m (min_should), and what the generator knows
of it: d0 (a document that is a hit by construction, or None), d1 (a document the must_not text
removes by construction, or None), kind (the unsatisfiable family)."""
import math
from collections import Counter
from fractions import Fraction

import numpy as np

SEPS = [b" ", b"\n", b"\t", b"  "]


def tokenize(text: bytes):
    """tokens are the maximal runs outside {0x20, 0x09..0x0D} (what bytes.split() splits at), a
    term is the token up to its first NUL"""
    return [t.split(b"\0")[0] for t in text.split()]


class ClauseRef:
    def __init__(self, ora, ndocs, n_total=0):
        self.terms = ora["terms"]
        self.tid = {t: i for i, t in enumerate(ora["terms"])}
        term = ora["term"]
        self.by_term = np.argsort(term, kind="stable")
        self.first = np.searchsorted(term[self.by_term], np.arange(len(ora["terms"]) + 1))
        self.doc = ora["doc"].tolist()
        self.score = ora["score"].tolist()
        self.count = ora["count"].tolist()
        self.docsize = ora["docsize"].tolist()
        self.pair_term = term.tolist()
        self.N = int(n_total) if n_total else ndocs
        self.df = [0] * len(ora["terms"])
        for t, d in zip(self.pair_term, ora["df"].tolist()):
            self.df[t] = d
        self.L = sum(self.count)
        self.avgdl = self.L / ndocs if self.L else 0.0
        self._docs_of = {}
        self.doc_terms = {}                      # document id -> the set of its terms (bytes)
        for d, t in zip(self.doc, self.pair_term):
            self.doc_terms.setdefault(d, set()).add(self.terms[t])

    def pairs_of(self, t: bytes):
        i = self.tid.get(t)
        return [] if i is None else self.by_term[self.first[i]:self.first[i + 1]].tolist()

    def docs_of(self, t: bytes):
        """the documents that hold the term (none when the vocabulary lacks it)"""
        if t not in self._docs_of:
            self._docs_of[t] = frozenset(self.doc[p] for p in self.pairs_of(t))
        return self._docs_of[t]

    def idf(self, i: int) -> float:
        num = float(self.N - self.df[i]) + 0.5
        den = float(self.df[i]) + 0.5
        ratio = num / den
        return math.log(1.0 + ratio)

    def or_scores(self, text: bytes, ranking="tfidf", k1=1.2, b=0.75, avgdl=0.0, fuse=False):
        """doc -> score of the OR ranking of text, and the distinct terms found.  fuse: every
        product and its add in one rounding, what a contracted kernel would compute"""
        w = Counter(tokenize(text))
        found = [t for t in w if t in self.tid]
        m = []
        for t in found:
            W = float(w[t]) * self.idf(self.tid[t]) if ranking == "bm25" else w[t]
            for p in self.pairs_of(t):
                m.append((p, W))
        m.sort()                                  # pair order
        avg = avgdl if avgdl else self.avgdl
        k1p1 = k1 + 1.0
        omb = 1.0 - b
        acc = {}
        for p, W in m:
            d = self.doc[p]
            if ranking == "bm25":
                x = float(self.docsize[p]) / avg
                bl = b * x
                nrm = omb + bl
                K = k1 * nrm
                num = float(self.count[p]) * k1p1
                den = float(self.count[p]) + K
                v = num / den
            else:
                v = self.score[p]
            if fuse:
                acc[d] = float(Fraction(W) * Fraction(v) + Fraction(acc.get(d, 0.0)))
            else:
                prod = W * v
                acc[d] = acc.get(d, 0.0) + prod
        return acc, len(found)

    def explain(self, q, ranking="tfidf", k1=1.2, b=0.75, avgdl=0.0, fuse=False):
        """the hits of q, the scoring terms found, and what each condition removes from the OR
        ranking (a document may fail several)"""
        M, S, X = set(tokenize(q["must"])), set(tokenize(q["should"])), set(tokenize(q["must_not"]))
        acc, nfound = self.or_scores(q["must"] + b" " + q["should"], ranking, k1, b, avgdl, fuse)
        keep, fail = {}, {"a": 0, "b": 0, "c": 0}
        Md, Sd = [self.docs_of(t) for t in M], [self.docs_of(t) for t in S]
        Xd = [x for x in (self.docs_of(t) for t in X) if x]       # an X term outside the vocabulary is ignored
        for d, s in acc.items():                  # (d) holds for every document of the OR ranking
            a_ok = all(d in x for x in Md)
            b_ok = not any(d in x for x in Xd)
            c_ok = sum(d in x for x in Sd) >= q["m"]
            fail["a"] += not a_ok
            fail["b"] += not b_ok
            fail["c"] += not c_ok
            if a_ok and b_ok and c_ok:
                keep[d] = s
        hits = sorted(keep.items(), key=lambda x: (-x[1], x[0]))
        return dict(hits=hits, nfound=nfound, n_or=len(acc), fail=fail)

    def rank(self, q, ranking="tfidf", k1=1.2, b=0.75, avgdl=0.0):
        """(hits, nterms_found): what test_gpu_query.check compares a result row with"""
        e = self.explain(q, ranking, k1, b, avgdl)
        return e["hits"], e["nfound"]

    def fused_differs(self, q, k: int = 1024) -> bool:
        """would fma(w, s, acc) change the bits of a score returned for this query?"""
        plain = dict(self.explain(q)["hits"][:k])
        fused = dict(self.explain(q, fuse=True)["hits"])
        return any(fused[d] != s for d, s in plain.items())


def texts(qs):
    """the three lists and the min_should list Engine.query_clauses takes"""
    return ([q["must"] for q in qs], [q["should"] for q in qs], [q["must_not"] for q in qs], [q["m"] for q in qs])


def _join(toks, rng):
    order = rng.permutation(len(toks))
    return b"".join(toks[i] + SEPS[int(rng.integers(0, 4))] for i in order)


def make_clause_queries(ref: ClauseRef, rng, n):
    """n queries, each built around a seed document d0 so that d0 is a hit: must terms from d0;
    the must_not term from a document d1 that shares a must term with d0 and holds a term d0
    lacks (so d1 is removed), or an absent word, or none; should terms from d0 and from the
    vocabulary (half of those uniformly, half as the word of a random pair), with repeats, absent
    words, a token cut by a NUL and empty texts; m at most the should terms d0 holds."""
    docs = sorted(d for d, t in ref.doc_terms.items() if t)
    V = len(ref.terms)
    qs = []
    while len(qs) < n:
        d0 = docs[int(rng.integers(0, len(docs)))]
        T0 = sorted(ref.doc_terms[d0])
        pick0 = lambda: T0[int(rng.integers(0, len(T0)))]
        must = [pick0() for _ in range(int(rng.integers(0, 4)))]
        toks = []
        for t in must:
            toks += [t] * (int(rng.integers(2, 5)) if rng.random() < 0.3 else 1)
        must_text = _join(toks, rng)
        should = []
        if rng.random() < 0.85:
            for _ in range(int(rng.integers(0, 4))):
                should.append(pick0())
            for _ in range(int(rng.integers(0, 4))):
                r = rng.random()
                if r < 0.4:
                    should.append(ref.terms[int(rng.integers(0, V))])
                elif r < 0.8:
                    should.append(ref.terms[ref.pair_term[int(rng.integers(0, len(ref.pair_term)))]])
                else:
                    should.append(b"zz-absent-%d" % int(rng.integers(0, 50)))
        if not must and not any(t in ref.doc_terms[d0] for t in should):
            should.append(pick0())                # (d): d0 needs a scoring term
        toks = []
        for t in should:
            if rng.random() < 0.08:
                t = t + b"\0tail"                 # the term ends at the NUL
            toks += [t] * (int(rng.integers(2, 8)) if rng.random() < 0.4 else 1)
        should_text = _join(toks, rng)
        in_d0 = len({t for t in should if t in ref.doc_terms[d0]})
        m = int(rng.integers(0, in_d0 + 1)) if rng.random() < 0.5 else 0
        d1, x = None, []
        r = rng.random()
        if must and r < 0.7:
            t = must[int(rng.integers(0, len(must)))]
            for d in sorted(ref.docs_of(t) - {d0}):
                extra = sorted(ref.doc_terms[d] - ref.doc_terms[d0])
                if extra:
                    d1, x = d, [extra[int(rng.integers(0, len(extra)))]]
                    break
        elif r < 0.85:
            x = [b"zz-absent-%d" % int(rng.integers(0, 50))]
        if x and rng.random() < 0.3:
            x = x * 2 + [b"zz-never"]
        qs.append(dict(must=must_text, should=should_text, must_not=_join(x, rng), m=m, d0=d0, d1=d1, kind=None))
    return qs


def make_unsatisfiable_queries(ref: ClauseRef, rng, n):
    """queries without hits, most of them although their OR ranking has some: an absent must
    word, a term in both the must and the must_not text, m over |S|, a must_not text alone"""
    docs = sorted(d for d, t in ref.doc_terms.items() if t)
    qs = []
    kinds = ("absent_must", "must_and_not", "m_over_s", "not_only")
    while len(qs) < n:
        kind = kinds[len(qs) % 4]
        d0 = docs[int(rng.integers(0, len(docs)))]
        T0 = sorted(ref.doc_terms[d0])
        a, b = T0[int(rng.integers(0, len(T0)))], T0[int(rng.integers(0, len(T0)))]
        q = dict(must=b"", should=b"", must_not=b"", m=0, d0=None, d1=None, kind=kind)
        if kind == "absent_must":
            q.update(must=a + b" zz-never", should=b)
        elif kind == "must_and_not":
            q.update(must=a + b"\t" + b, should=b, must_not=b"zz-never " + a)
        elif kind == "m_over_s":
            q.update(must=a, should=a + b" " + b + b" " + b, m=len({a, b}) + 1)
        else:
            q.update(must_not=a)
        qs.append(q)
    return qs
