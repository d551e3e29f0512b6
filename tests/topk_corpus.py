"""The top-k corpus: 20000 tiny documents, on which the top-k driver that tfidf_query,
tfidf_query_bm25, tfidf_query_clauses and tfidf_similar share (topk_rounds in csrc/engine_query.cpp
over k_query_topk in csrc/query.hip) takes three launches at k = 1024 and k = 1000, and the rule
those launches follow, stated here on its own.

  rounds     round 1 cuts the N output positions into nsl0 = ceil(N / QT_SLICE) slices and leaves
             the best k of each in order; every later round takes the nsl lists of k as nsl * k
             inputs, nsl <- ceil(nsl * k / QT_SLICE), until one slice is left.  20000 documents are
             five first-round slices (the last holds 3616), then two, then one.
  documents  2 to 5 tokens of the 40 words w00 .. w39 and the word "all", which every document with
             a token holds once.  A query for it hits them all, and its score depends on the
             document's length alone (four values): the quarter of the documents with three tokens
             tie for the best, far more than k, so the ids alone order the result.  Output positions
             are in "docN@" strcmp order: the lowest ids lie in every slice.
  empty      five documents without a token: two in slice 0, one in slice 2, two in slice 4.  No
             query hits them; slices 1 and 3 stay full, so that a query for "all" has QT_SLICE hits
             there (no pad in the sort).  They make the df of "all" N - 5, so its TF-IDF score is a
             small positive number, not +0.0 (hits of +0.0 through every round: topk_test.cpp).

test_topk_corpus_cpu.py establishes on the references alone what test_gpu_topk_rounds.py relies
on."""
import numpy as np

from stride_corpus import kernels_h

QT_SLICE = kernels_h("QT_SLICE")
N = 20000
NWORDS = 40
SEED = 7
KS = (1024, 1000, 10, 1024)             # the last call repeats the first over the others' stale lists
EMPTY_POS = (5, QT_SLICE - 1, 2 * QT_SLICE + 1234, 4 * QT_SLICE, N - 1)      # output positions
ABSENT_ID = N + 5


def rounds(n: int, k: int) -> list:
    """the output slices of each launch: [nsl0, .., 1]"""
    nsl = -(-n // QT_SLICE)
    out = [nsl]
    while nsl > 1:
        nsl = -(-(nsl * k) // QT_SLICE)
        out.append(nsl)
    return out


def second_round_slice(pos: int, local_rank: int, k: int) -> int:
    """the second-round slice that reads entry local_rank of the list of pos's first-round slice"""
    return ((pos // QT_SLICE) * k + local_rank) // QT_SLICE


def first_round_slice(pos: int) -> int:
    return pos // QT_SLICE


def Q(must=b"", should=b"", must_not=b"", m=0):
    return dict(must=must, should=should, must_not=must_not, m=m)


PLAIN = [b"w00 w01 w01 w02", b"w05", b"w07 w08 w09 w10 w11 w12", b"all", b"all w05", b"zz-absent", b"",
         b"w05 zz-absent w05 w06", b"w39"]
WORD_QUERIES = (0, 1, 2)                # of PLAIN: the ones with a spread of scores
ALL_QUERY = 3
CLAUSES = [Q(must=b"w07", must_not=b"w08"),                                    # a must word with a must_not word
           Q(must=b"all w05"),                                                 # two must words
           Q(should=b"w01 w02 w03 w04 w05 w06 w07 w08", m=2),                  # should only
           Q(must=b"zz-absent", should=b"w01"),                                # unsatisfiable
           Q(must=b"all", should=b"w00 w01 w02", must_not=b"w39"),             # more than k hits in every slice
           Q(should=b"all", must_not=b"zz-absent")]
CLAUSE_SPREAD = (0, 1, 2, 4)            # of CLAUSES: more than k hits, a spread of scores


def build() -> dict:
    """docs by id (document id i is docs[i - 1]); order: the ids by output position; pos: id -> output
    position; empty: the ids of the empty documents; similar: the rows of the similar calls (one of
    every first-round slice, an empty document, an id nobody holds)"""
    rng = np.random.default_rng(SEED)
    docs = []
    for _ in range(N):
        n = int(rng.integers(2, 6))
        docs.append(b" ".join([b"w%02d" % int(w) for w in rng.integers(0, NWORDS, n)] + [b"all"]))
    order = sorted(range(1, N + 1), key=lambda i: b"doc%d@" % i)
    empty = [order[p] for p in EMPTY_POS]
    for d in empty:
        docs[d - 1] = b""
    pos = {d: p for p, d in enumerate(order)}
    similar = [order[s * QT_SLICE + 777] for s in range(-(-N // QT_SLICE))] + [empty[2], ABSENT_ID]
    return dict(docs=docs, order=order, pos=pos, empty=empty, similar=similar)


def references() -> dict:
    """the corpus, its arrays, the oracle's result and the four Python references over it (plain loops:
    Ref and Bm25Ref of the query tests, ClauseRef, Ref of the similar test), with every ranking the
    tests compare against: plain / bm25 [(hits, nfound)] per query of PLAIN, clauses[ranking] the
    same per query of CLAUSES, rows as test_gpu_similar.check takes them"""
    import oracle_py
    from clause_ref import ClauseRef
    from helpers import docs_to_arrays
    from test_gpu_bm25 import Bm25Ref
    from test_gpu_query import Ref
    from test_gpu_similar import Ref as SimilarRef
    c = build()
    data, off = docs_to_arrays(c["docs"])
    ora = oracle_py.run(data, off)
    ref, bm, cl = Ref(ora), Bm25Ref(ora, N), ClauseRef(ora, N)
    sim = SimilarRef(ora, range(1, N + 1))
    assert sim.order == c["order"]
    return dict(c, data=data, off=off, ora=ora,
                plain=[ref.rank(q) for q in PLAIN], bm25=[bm.rank(q) for q in PLAIN],
                clauses={r: [cl.rank(q, r) for q in CLAUSES] for r in ("tfidf", "bm25")},
                rows=sim.rows(c["similar"]))


def split(hits, pos, k: int) -> dict:
    """where the first k of a best-first hit list [(doc, ...)] lie: per: hits per first-round slice;
    win: winners per first-round slice; second: winners per second-round slice, each by its rank
    inside its own slice's list; ranks4: the local ranks of the last slice's winners"""
    nsl = -(-N // QT_SLICE)
    per, win, second, ranks4 = [0] * nsl, [0] * nsl, {}, []
    for i, h in enumerate(hits):
        s = first_round_slice(pos[h[0]])
        if i < k:
            r = per[s]                  # best first: the slice's hits before this one are exactly its better ones
            win[s] += 1
            s2 = second_round_slice(pos[h[0]], r, k)
            second[s2] = second.get(s2, 0) + 1
            if s == nsl - 1:
                ranks4.append(r)
        per[s] += 1
    return dict(per=per, win=win, second=second, ranks4=ranks4)
