"""Naive Bayes classification (include/tfidf.h, section "classify") in plain Python over a result
dict (oracle_py.run's, prune_ref.prune's or Engine.fetch's): the reference of test_nb_cpu.py,
test_gpu_nb.py, test_gpu_nb_stride.py and the CLI test.

Counts are Python ints (exact), every logarithm is math.log (the host's libm), and every
floating-point expression is written one operation per statement, in the definition's order; a
Python float operation is one IEEE binary64 operation, and Python never fuses a product into an add.

  NRef(res, doc_ids)                        documents in output order, their (rank, count) rows
  NRef.fit(docs, labels, K, ...)            the model as a dict, None when the parameters are refused
  predict(model, rows)                      labels, scores, all scores of (rank, count) rows
  NRef.rows(positions) / NRef.unseen(docs)  rows of resident documents / of new documents' bytes
  classes_lines(...)                        classes.txt of the CLI
"""
import math

import numpy as np

MAX_CLASSES = 256
MAX_ALPHA = float.fromhex("0x1p+900")
NO_CLASS = 0xFFFFFFFF
NO_POS = 0xFFFFFFFF


def check_params(docs, labels, K, alpha=0.0, variant="multinomial", feature="count") -> bool:
    """would tfidf_nb_check take them?"""
    if not 1 <= K <= MAX_CLASSES or variant not in ("multinomial", "complement") or feature not in ("count", "binary"):
        return False
    if not (0.0 <= alpha <= MAX_ALPHA):                                  # NaN fails both
        return False
    if len(docs) != len(labels) or any(not 0 <= c < K for c in labels):
        return False
    if len(set(docs)) != len(docs) or set(labels) != set(range(K)):
        return False
    return True


class NRef:
    def __init__(self, res: dict, doc_ids):
        self.ids = [int(d) for d in doc_ids]
        self.order = sorted(self.ids, key=lambda d: b"doc%d@" % d)      # output order
        self.pos = {d: j for j, d in enumerate(self.order)}
        words = res["terms"]
        by_rank = sorted(range(len(words)), key=lambda i: words[i] + b"\t")
        rank = {i: r for r, i in enumerate(by_rank)}
        self.words = [words[i] for i in by_rank]
        self.rank_of = {w: r for r, w in enumerate(self.words)}
        self.V = len(words)
        rows = {d: [] for d in self.ids}
        for d, t, c in zip(np.asarray(res["doc"]).tolist(), np.asarray(res["term"]).tolist(),
                           np.asarray(res["count"]).tolist()):
            rows[d].append((rank[t], c))
        self.by_pos = [sorted(rows[d]) for d in self.order]              # pair order: term-table order

    def rows(self, positions=None):
        return [self.by_pos[j] for j in (range(len(self.order)) if positions is None else positions)]

    def unseen(self, docs):
        """rows of new documents: bytes.split cuts at the six whitespace bytes; a term is the
        token up to its first NUL; words outside the vocabulary are dropped"""
        out = []
        for d in docs:
            cnt = {}
            for tok in bytes(d).split():
                r = self.rank_of.get(tok.split(b"\0")[0])
                if r is not None:
                    cnt[r] = cnt.get(r, 0) + 1
            out.append(sorted(cnt.items()))
        return out

    def fit(self, docs, labels, K, variant="multinomial", feature="count", alpha=0.0, uniform_prior=False):
        docs, labels = [int(d) for d in docs], [int(c) for c in labels]
        if not check_params(docs, labels, K, alpha, variant, feature) or any(d not in self.pos for d in docs):
            return None
        V, comp, binary = self.V, variant == "complement", feature == "binary"
        alpha = 1.0 if alpha == 0.0 else float(alpha)
        FC = [[0] * K for _ in range(V)]                                 # [t][c], Python ints
        n_c = [0] * K
        for d, c in zip(docs, labels):
            n_c[c] += 1
            for t, x in self.by_pos[self.pos[d]]:
                FC[t][c] += 1 if binary else x
        T = [sum(FC[t][c] for t in range(V)) for c in range(K)]
        F = [sum(FC[t]) for t in range(V)]
        Ttot, n = sum(T), sum(n_c)
        aV = alpha * float(V)
        W = [[0.0] * K for _ in range(V)]
        prior = [0.0] * K
        log_of = {}                                                      # math.log of an entry's argument, once per distinct count
        for c in range(K):
            if not comp and not uniform_prior:
                ln_c = math.log(float(n_c[c]))
                ln_n = math.log(float(n))
                prior[c] = ln_c - ln_n
            if not V:                                                    # no weights: the class's own logarithm has no reader
                continue
            a = float(Ttot - T[c] if comp else T[c]) + aV
            lc = math.log(a)
            for t in range(V):
                m = F[t] - FC[t][c] if comp else FC[t][c]
                la = log_of.get(m)
                if la is None:
                    a = float(m) + alpha
                    la = log_of[m] = math.log(a)
                W[t][c] = lc - la if comp else la - lc
        return dict(nclasses=K, nterms=V, variant=int(comp), feature=int(binary), uniform_prior=int(bool(uniform_prior)),
                    alpha=alpha, nlabelled=n, class_docs=n_c, class_total=T, feature_count=FC, prior=prior, weight=W)


def predict(model: dict, rows, by_class=False):
    """(labels, scores of the labels, all scores [row][class]) of rows of (rank, count).
    by_class: the same operations with numpy taking the classes of a pair at once (an elementwise
    product, then an elementwise add: one IEEE operation per element each, never fused), for the
    corpora on which the plain loops take long; test_nb_cpu.py holds the two forms equal."""
    K, W, prior, binary = model["nclasses"], model["weight"], model["prior"], model["feature"] == 1
    if by_class:
        Wn = np.array(W, dtype=np.float64).reshape(len(W), K)
        pn = np.array(prior, dtype=np.float64)
    labels, best, scores = [], [], []
    for row in rows:
        if by_class:
            acc = pn.copy()
            for t, x in row:
                prod = np.float64(1.0 if binary else float(x)) * Wn[t]
                acc = acc + prod
            s = acc.tolist()
        else:
            s = []
            for c in range(K):
                acc = prior[c]
                for t, x in row:
                    prod = (1.0 if binary else float(x)) * W[t][c]
                    acc = acc + prod
                s.append(acc)
        lab = 0
        for c in range(1, K):
            if s[c] > s[lab]:                                            # a later class only when strictly larger
                lab = c
        labels.append(lab)
        best.append(s[lab])
        scores.append(s)
    return labels, best, scores


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_model(got: dict, ref: dict):
    """a library model (tfidf_abi's dict) against NRef.fit: integers equal, doubles as u64 bits"""
    for k in ("nclasses", "nterms", "variant", "feature", "uniform_prior", "nlabelled"):
        assert int(got[k]) == int(ref[k]), k
    assert bits([got["alpha"]])[0] == bits([ref["alpha"]])[0]
    K, V = ref["nclasses"], ref["nterms"]
    assert [int(x) for x in got["class_docs"]] == ref["class_docs"]
    assert [int(x) for x in got["class_total"]] == ref["class_total"]
    want_fc = np.array(ref["feature_count"], dtype=object).reshape(V, K) if V else np.zeros((0, K), dtype=object)
    assert got["feature_count"].shape == (V, K)
    assert (got["feature_count"].astype(object) == want_fc).all()
    assert np.array_equal(bits(got["prior"]), bits(ref["prior"]))
    want_w = np.array(ref["weight"], dtype=np.float64).reshape(V, K) if V else np.zeros((0, K))
    assert np.array_equal(bits(got["weight"]), bits(want_w)), np.argwhere(bits(got["weight"]) != bits(want_w))[:5]


def assert_same_labels(got: dict, want, K: int):
    """a library answer with all scores against predict()'s triple"""
    labels, best, scores = want
    assert got["ndocs"] == len(labels) and got["nclasses"] == K
    assert [int(x) for x in got["label"]] == labels
    assert np.array_equal(bits(got["score"]), bits(best))
    if "scores" in got:
        want_s = np.array(scores, dtype=np.float64).reshape(len(labels), K)
        assert np.array_equal(bits(got["scores"]), bits(want_s))


def flat_rows(rows):
    """row_off, term, count arrays of rows of (rank, count)"""
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
    term = np.array([t for r in rows for t, _ in r], dtype=np.uint32)
    count = np.array([x for r in rows for _, x in r], dtype=np.uint32)
    return off, term, count


def classes_lines(doc_numbers, labels, best, names) -> bytes:
    """classes.txt of the CLI: a line per classified document, doc<M>\\t<name>\\t%.16f"""
    return b"".join(b"doc%d\t%s\t%.16f\n" % (d, names[c], s) for d, c, s in zip(doc_numbers, labels, best))


# ---- the planted corpus shared by the CPU, GPU and CLI tests ----

PLANT_CLASSES, PLANT_PER_CLASS = 4, 12


def _word(prefix: bytes, i: int) -> bytes:
    return prefix + b"%03d" % i


def planted_corpus():
    """4 classes x 12 documents.  Class c owns 30 words (k<c>_000 ..); 20 words are shared.  A
    document holds 14 of its class's words (a window that moves with the document), some twice,
    and 8 shared ones.  Returns (docs, planted): document id i is docs[i - 1], planted[i - 1] its
    class; documents alternate between the classes, so every class has labelled and held-out
    members under `id odd -> labelled`."""
    docs, planted = [], []
    for i in range(PLANT_CLASSES * PLANT_PER_CLASS):
        c, m = i % PLANT_CLASSES, i // PLANT_CLASSES
        own = [_word(b"k%d_" % c, (3 * m + j) % 30) for j in range(14)]
        own += own[:1 + m % 3]                                           # a few words twice
        shared = [_word(b"sh_", (5 * m + 3 * c + j) % 20) for j in range(8)]
        docs.append(b" ".join(own + shared))
        planted.append(c)
    return docs, planted


def planted_split(planted):
    """(labelled ids, their classes, held-out ids): half the documents are labelled, every
    class's members with an even index"""
    lab, held = [], []
    for i in range(len(planted)):
        m = i // PLANT_CLASSES
        (lab if m % 2 == 0 else held).append(i + 1)
    return lab, [planted[d - 1] for d in lab], held
