"""Near-duplicate detection (include/tfidf.h, section "near duplicates") in plain Python and
numpy over a result dict (oracle_py.run's, prune_ref.prune's or Engine.fetch's): the reference of
test_dedup_cpu.py, test_gpu_dedup.py and the CLI test.

Everything is integer arithmetic modulo 2^64 or 2^32 (Python ints masked, or numpy uint64 arrays,
which wrap) plus one Python float division, which is one IEEE binary64 division.

  DRef(res, doc_ids)               documents in output order, their term sets by rank, h0
  DRef.signatures(H, seed)         uint32 [N, H]
  DRef.near_dups(H, r, seed, thr)  dict: ncand, edges, group, ngroups, ...
  dups_lines(out)                  dups.txt of the CLI
"""
import numpy as np

M64 = (1 << 64) - 1
FNV_BASIS = 0xCBF29CE484222325
FNV_PRIME = 0x100000001B3
GOLDEN_GAMMA = 0x9E3779B97F4A7C15
DEFAULT_H, DEFAULT_ROWS, DEFAULT_SEED = 128, 4, 1
MAX_H = 256


def mix64(z: int) -> int:
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def fnv1a64(b: bytes) -> int:
    h = FNV_BASIS
    for c in b:
        h = ((h ^ c) * FNV_PRIME) & M64
    return h


def h0(term: bytes) -> int:
    return mix64(fnv1a64(term))


def family(H: int, seed: int):
    """(a, b): a_i odd 64-bit multipliers, b_i 32-bit offsets, in the definition's order"""
    s, a, b = seed & M64, [], []
    for _ in range(H):
        s = (s + GOLDEN_GAMMA) & M64
        a.append(mix64(s) | 1)
        s = (s + GOLDEN_GAMMA) & M64
        b.append(mix64(s) >> 32)
    return a, b


def _mix64_np(z):
    z = z.astype(np.uint64, copy=True)
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def check_params(H: int, r: int, thr: float) -> bool:
    """would the library take them?  (H = 0 stands for the defaults)"""
    if H > MAX_H or not (0.0 <= thr <= 1.0):
        return False
    return H == 0 or (r >= 1 and H % r == 0)


class DRef:
    def __init__(self, res: dict, doc_ids):
        self.ids = [int(d) for d in doc_ids]
        self.order = sorted(self.ids, key=lambda d: b"doc%d@" % d)      # output order
        self.pos = {d: j for j, d in enumerate(self.order)}
        words = res["terms"]
        by_rank = sorted(range(len(words)), key=lambda i: words[i] + b"\t")
        rank = np.zeros(len(words) + 1, dtype=np.int64)
        rank[np.array(by_rank, dtype=np.int64)] = np.arange(len(words))
        self.words = [words[i] for i in by_rank]
        self.h0 = np.array([h0(w) for w in self.words], dtype=np.uint64)
        sets = {d: [] for d in self.ids}
        for d, t in zip(np.asarray(res["doc"]).tolist(), rank[np.asarray(res["term"], dtype=np.int64)].tolist()):
            sets[d].append(t)
        self.sets = [np.array(sorted(set(sets[d])), dtype=np.int64) for d in self.order]   # by position
        self.n = [len(s) for s in self.sets]

    def signatures(self, H: int = DEFAULT_H, seed: int = DEFAULT_SEED) -> np.ndarray:
        a, b = family(H, seed)
        a = np.array(a, dtype=np.uint64)
        b = np.array(b, dtype=np.uint64)
        sig = np.full((len(self.order), H), 0xFFFFFFFF, dtype=np.uint32)
        for j, s in enumerate(self.sets):
            if not len(s):
                continue
            x = self.h0[s]
            for c in range(0, len(x), 2048):
                g = (((a[None, :] * x[c:c + 2048, None]) >> np.uint64(32)) + b[None, :]) & np.uint64(0xFFFFFFFF)
                sig[j] = np.minimum(sig[j], g.min(axis=0).astype(np.uint32))
        return sig

    @staticmethod
    def band_keys(sig: np.ndarray, r: int) -> np.ndarray:
        """uint64 [N, b]"""
        N, H = sig.shape
        nb = H // r
        keys = np.zeros((N, nb), dtype=np.uint64)
        for j in range(nb):
            k = np.full(N, mix64(j + 1), dtype=np.uint64)
            for i in range(j * r, j * r + r):
                k = _mix64_np(k ^ sig[:, i].astype(np.uint64))
            keys[:, j] = k
        return keys

    def candidates(self, keys: np.ndarray):
        """the set C as a sorted list of (pos_a, pos_b)"""
        live = np.array([j for j, n in enumerate(self.n) if n >= 1], dtype=np.int64)
        C = set()
        if len(live) < 2:
            return []
        for j in range(keys.shape[1]):
            k = keys[live, j]
            o = np.lexsort((live, k))                                    # by (band key, pos)
            ks, ps = k[o], live[o]
            for i in np.flatnonzero(ks[1:] == ks[:-1]).tolist():
                C.add((int(ps[i]), int(ps[i + 1])))
        return sorted(C)

    def verify(self, a: int, b: int, sig: np.ndarray):
        shared = len(np.intersect1d(self.sets[a], self.sets[b], assume_unique=True))
        uni = self.n[a] + self.n[b] - shared
        return shared, uni, int((sig[a] == sig[b]).sum()), float(shared) / float(uni)

    @staticmethod
    def groups(N: int, edges):
        parent = list(range(N))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for a, b in edges:
            x, y = find(a), find(b)
            if x != y:
                parent[max(x, y)] = min(x, y)
        group = [find(i) for i in range(N)]
        return group, len({g for i, g in enumerate(group) if g != i})

    def near_dups(self, H: int = 0, r: int = 0, seed: int = 0, threshold: float = 0.8):
        if not check_params(H, r, threshold):
            return None
        if H == 0:
            H, r, seed = DEFAULT_H, DEFAULT_ROWS, DEFAULT_SEED
        sig = self.signatures(H, seed)
        cand = self.candidates(self.band_keys(sig, r))
        edges = []
        for a, b in cand:
            shared, uni, same, jac = self.verify(a, b, sig)
            if jac >= threshold:
                edges.append(dict(a_pos=a, b_pos=b, a_doc=self.order[a], b_doc=self.order[b], shared=shared, uni=uni,
                                  same=same, jaccard=jac))
        group, ngroups = self.groups(len(self.order), [(e["a_pos"], e["b_pos"]) for e in edges])
        return dict(ndocs=len(self.order), doc=list(self.order), npairs=list(self.n), sig=sig, nhashes=H, rows=r,
                    ncand=len(cand), cand=cand, nedges=len(edges), edges=edges, group=group, ngroups=ngroups)

    def jaccard(self, da: int, db: int) -> float:
        """exact Jaccard of two documents by id (for planted pairs)"""
        a, b = self.pos[da], self.pos[db]
        shared = len(np.intersect1d(self.sets[a], self.sets[b], assume_unique=True))
        uni = self.n[a] + self.n[b] - shared
        return float(shared) / float(uni) if uni else 0.0


def edge_tuples(out: dict):
    """the kept edges as comparable tuples, the jaccard as its bits"""
    if "edges" in out:
        return [(e["a_pos"], e["b_pos"], e["a_doc"], e["b_doc"], e["shared"], e["uni"], e["same"],
                 int(np.float64(e["jaccard"]).view(np.uint64))) for e in out["edges"]]
    jb = np.asarray(out["jaccard"], dtype=np.float64).view(np.uint64)
    return [tuple(int(out[k][i]) for k in ("a_pos", "b_pos", "a_doc", "b_doc", "shared", "uni", "same")) + (int(jb[i]),)
            for i in range(int(out["nedges"]))]


def assert_same_dups(got: dict, ref: dict):
    """a library answer (tfidf_abi's dict) against DRef.near_dups: every integer and the jaccard bits"""
    assert got["ndocs"] == ref["ndocs"]
    assert [int(x) for x in got["doc"]] == ref["doc"]
    assert int(got["ncand"]) == ref["ncand"], (int(got["ncand"]), ref["ncand"])
    assert int(got["nedges"]) == ref["nedges"], (int(got["nedges"]), ref["nedges"])
    assert edge_tuples(got) == edge_tuples(ref)
    assert [int(x) for x in got["group"]] == ref["group"]
    assert int(got["ngroups"]) == ref["ngroups"]


def dups_lines(out: dict) -> bytes:
    """dups.txt of the CLI: a line per group of two or more (members in position order, groups by
    their lowest position), then a line per kept edge"""
    doc = [int(d) for d in out["doc"]]
    members = {}
    for pos, g in enumerate(int(x) for x in out["group"]):
        members.setdefault(g, []).append(pos)
    lines, i = [], 0
    for g in sorted(members):
        if len(members[g]) >= 2:
            lines.append(b"g%d\t%d\t" % (i, len(members[g])) + b" ".join(b"doc%d" % doc[p] for p in members[g]) + b"\n")
            i += 1
    for a_pos, b_pos, a_doc, b_doc, shared, uni, same, jb in edge_tuples(out):
        jac = float(np.uint64(jb).view(np.float64))
        lines.append(b"doc%d\tdoc%d\t%d\t%d\t%.16f\n" % (a_doc, b_doc, shared, uni, jac))
    return b"".join(lines)


# ---- crafted corpora shared by the CPU and GPU tests ----

def _word(i: int) -> bytes:
    """a distinct lowercase word per i (base 26, at least 3 letters)"""
    s = b""
    i += 26 * 26 * 3
    while i:
        s = bytes([97 + i % 26]) + s
        i //= 26
    return s


def families_corpus():
    """(a) 48 documents: 8 families, each a 60-word base plus 4 copies with 0 to 3 words replaced,
    and 8 unrelated documents.  Returns (docs, families): families = the lists of ids (1-based,
    in list order) of each family's five members.  Two members with i and j words replaced
    share at least 60 - i - j of at most 60 + i + j words."""
    docs, families, nxt = [], [], 0
    for f in range(8):
        base = [_word(nxt + i) for i in range(60)]
        nxt += 60
        first = len(docs) + 1
        docs.append(b" ".join(base))
        for k in range(4):                                               # k words replaced
            w = list(base)
            for x in range(k):
                w[(7 * f + 13 * x + k) % 60] = _word(nxt)
                nxt += 1
            docs.append(b" ".join(w))
        families.append(list(range(first, first + 5)))
    for _ in range(8):
        docs.append(b" ".join(_word(nxt + i) for i in range(60)))
        nxt += 60
    return docs, families


def planted_pairs(ref: "DRef", families, min_jaccard: float = 0.9):
    """The planted pairs the candidate stage must propose, as (pos_a, pos_b): two members of a
    family that are neighbours in output order among the family's members, with an exact Jaccard
    of at least min_jaccard.  Candidates are chains in position order (a bucket of m documents
    gives its m - 1 neighbouring pairs), so a pair with another member between them can be left
    to the groups; a neighbouring pair cannot: no family member stands between the two in any
    bucket that holds both."""
    out = []
    for fam in families:
        ps = sorted(ref.pos[d] for d in fam)
        for a, b in zip(ps, ps[1:]):
            if ref.jaccard(ref.order[a], ref.order[b]) >= min_jaccard:
                out.append((a, b))
    return out


def overlap_corpus():
    """(b) 24 documents of 30 words over a sliding window that moves by 15: neighbours share half
    their words (Jaccard 1/3)"""
    return [b" ".join(_word(15 * d + i) for i in range(30)) for d in range(24)]


def identical_corpus(n: int = 70):
    """(c) n byte-identical documents"""
    return [b" ".join(_word(i) for i in range(40))] * n


def big_corpus(nterms: int):
    """(d) two documents of `nterms` distinct terms each, 100 of which differ"""
    common = [_word(i) for i in range(nterms - 100)]
    a = common + [_word(10_000_000 + i) for i in range(100)]
    b = common + [_word(20_000_000 + i) for i in range(100)]
    return [b" ".join(a), b" ".join(b)]
