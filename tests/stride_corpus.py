"""The stride corpus: 300 documents on which, with TFIDF_GRID_CUS=1, every grid-stride loop of the
launches over the resident result (csrc/kernels.h, "grids of the launches over the resident
result") makes three trips and more, and on which a wave or workgroup meets the kinds of document
that take different paths one after the other.

Laid out by output position (the "docN@" name order), since that is what the kernels stride over:

  sizes      distinct terms per position, drawn with a fixed seed from SIZES, then overwritten by
             what is planted below
  big        NBIG documents of BIG + 1 terms, STEP positions apart: NCOMMON words they all hold plus
             two of NBIG blocks of BLOCK words (document i: blocks i and i + 1), so two of them share
             all but 100 or 200 terms and every block word has df = 2 (a prune(2) keeps them big)
  per stride S (a wave's or workgroup's step in positions: 4 x the per-CU constant of a
             wave-per-document kernel, the constant itself of a workgroup-per-row kernel)
             small -> big -> small at q - S, q, q + S; 129 terms -> none; 257 terms -> 64
  families   two families of FAMILY byte-identical small documents

A document of n terms at position p holds the words s, s + 1, .. s + n - 1 (mod NCOMMON; s drawn per
document; from 63 terms on the last is a word of the document's own, the only words with df = 1),
word k repeated 1 + (k + p) % 3 times; the words are w00000 .. with every 89th padded
to 15, 16 and 17 bytes.  test_stride_corpus_cpu.py checks the properties on the oracle's result
without a GPU; test_gpu_grid_stride.py runs every call on it."""
import os
import re

import numpy as np

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parallel-systems-mpi-tfidf_amd")


def kernels_h(name):
    """a constant of csrc/kernels.h, so that the corpus follows the kernels' thresholds and grids"""
    src = open(os.path.join(PKG, "csrc", "kernels.h")).read()
    m = re.search(r"#define\s+%s\s+\(?\s*(\d+)u?(?:\s*<<\s*(\d+))?" % name, src)
    assert m, name
    return int(m.group(1)) << int(m.group(2) or 0)


# the cuts to a workgroup per document; one value today, and the corpus needs them equal
QS_BIG, RW_BIG, DD_BIG_PAIRS = kernels_h("QS_BIG"), kernels_h("RW_BIG"), kernels_h("DD_BIG_PAIRS")
BIG = max(QS_BIG, RW_BIG, DD_BIG_PAIRS)
RW_KEEP = kernels_h("RW_KEEP")
PR_TILE = kernels_h("PR_TILE")
WAVES = 4                                     # waves of a 256-thread workgroup
# launch -> (per-CU constant, items a workgroup takes per trip, what it strides over)
WAVE_KERNELS = {"k_doc_score": "QS_WG_PER_CU", "k_sim_score": "SM_WG_PER_CU", "k_km_assign": "KM_WG_PER_CU",
                "k_rw_docs": "RW_WG_PER_CU", "k_dd_sig": "DD_WG_PER_CU"}
ROW_KERNELS = {"k_terms_select_list": "TM_LIST_WG_PER_CU", "k_terms_select<64,512>": "TM_W512_WG_PER_CU",
               "k_terms_select<64,2048>": "TM_W2048_WG_PER_CU"}
PER_CU = {n: kernels_h(n) for n in list(WAVE_KERNELS.values()) + list(ROW_KERNELS.values()) +
          ["DD_BIG_WG_PER_CU", "TM_BIG_WG_PER_CU", "PR_WG_PER_CU", "BIG_WG_PER_CU", "BIG_WG_MAX"]}

# a wave's (workgroup's) step in output positions at TFIDF_GRID_CUS=1
STRIDES = sorted({WAVES * PER_CU[c] for c in WAVE_KERNELS.values()} | {PER_CU[c] for c in ROW_KERNELS.values()})

NDOCS = 300
SIZES = (0, 1, 2, 63, 64, 65, 129, 256, 257, 1025)
SIZE_P = (0.14, 0.14, 0.14, 0.11, 0.11, 0.11, 0.10, 0.06, 0.06, 0.03)
NBIG, STEP, FIRST_BIG = 13, 22, 11
BLOCK = 100
NCOMMON = BIG + 1 - 2 * BLOCK
FAMILY = 12
FAMILIES = ((100, 64, 0), (2000, 65, 1))      # (first word, terms, the p of the counts) of the identical documents
SEED = 20


def word(k: int) -> bytes:
    w = b"w%05d" % k
    return w + b"x" * {5: 9, 6: 10, 7: 11}.get(k % 89, 0)      # 15, 16 and 17 bytes


def text(terms, p: int) -> bytes:
    return b" ".join(b" ".join([word(k)] * (1 + (k + p) % 3)) for k in terms)


def trips(ncu: int, ndocs: int, nbig: int, npairs: int, ncand: int, nbigcand: int) -> dict:
    """launch -> trips of its longest-working wave or workgroup through the grid-stride loop"""
    def n(work, per_cu, unit=1, cap=None):
        grid = min((work + unit - 1) // unit, ncu * PER_CU[per_cu], *([cap] if cap else []))
        return 0 if not work else -(-work // (grid * unit))
    out = {k: n(ndocs, c, WAVES) for k, c in WAVE_KERNELS.items()}
    out.update({k: n(ndocs, c) for k, c in ROW_KERNELS.items()})
    for k in ("k_doc_score_big", "k_sim_score_big", "k_rw_docs_big"):
        out[k] = -(-nbig // min((ndocs + WAVES - 1) // WAVES, PER_CU["BIG_WG_MAX"], ncu * PER_CU["BIG_WG_PER_CU"]))
    out["k_terms_select<256,4096,BIG>"] = -(-nbig // min(ndocs, ncu * PER_CU["TM_BIG_WG_PER_CU"]))
    out["k_dd_sig_big"] = -(-nbig // min(ndocs, ncu * PER_CU["DD_BIG_WG_PER_CU"]))
    out["k_dd_verify"] = n(ncand, "DD_WG_PER_CU", WAVES)
    out["k_dd_verify_big"] = -(-nbigcand // min(ncand, ncu * PER_CU["DD_BIG_WG_PER_CU"])) if ncand else 0
    out["k_pr_count / k_pr_write"] = n(-(-npairs // PR_TILE), "PR_WG_PER_CU")
    return out


def layout():
    """sizes by position, the big positions, the families' positions"""
    rng = np.random.default_rng(SEED)
    sizes = [int(x) for x in rng.choice(SIZES, NDOCS, p=SIZE_P)]
    big = [FIRST_BIG + STEP * i for i in range(NBIG)]
    fixed = set(big)
    for q in big:
        sizes[q] = BIG + 1

    def put(at, vals):
        assert all(0 <= a < NDOCS and a not in fixed for a in at), at
        for a, v in zip(at, vals):
            sizes[a] = v
            fixed.add(a)

    def free_run(start, S, n):
        p = start
        while any(p + i * S in fixed or p + i * S >= NDOCS for i in range(n)):
            p += 1
            assert p < NDOCS
        return [p + i * S for i in range(n)]

    for i, S in enumerate(STRIDES):
        q = big[2 + 2 * i]                                      # a big document of its own per stride
        put([q - S, q + S], [65, 2])                            # small -> big -> small
        put(free_run(40 + 50 * i, S, 2), [129, 0])              # a wave's worth of pairs -> none
        put(free_run(60 + 50 * i, S, 2), [RW_KEEP + 1, 64])     # past the register path -> inside it
    free = [p for p in range(NDOCS) if p not in fixed]
    fams = [free[2::19][:FAMILY], free[9::19][:FAMILY]]
    for f, (_, n, _) in zip(fams, FAMILIES):
        assert len(f) == FAMILY
        put(f, [n] * FAMILY)
    return sizes, big, fams, rng


def build() -> dict:
    """docs by id (document id i is docs[i - 1]), and by output position: order (ids), sizes (distinct
    terms), big (positions), families (positions)"""
    sizes, big, fams, rng = layout()
    order = sorted(range(1, NDOCS + 1), key=lambda i: b"doc%d@" % i)
    by_pos = []
    for p, n in enumerate(sizes):
        s = int(rng.integers(0, NCOMMON))                       # drawn for every position: planting moves no other document
        terms = [(s + k) % NCOMMON for k in range(n)]
        if n >= 63:
            terms[-1] = NCOMMON + BLOCK * NBIG + p               # a word of its own (df = 1): a prune(2) has pairs to remove
        by_pos.append(text(terms, p))
    for i, q in enumerate(big):
        terms = list(range(NCOMMON))
        for b in (i, (i + 1) % NBIG):
            terms += range(NCOMMON + BLOCK * b, NCOMMON + BLOCK * (b + 1))
        by_pos[q] = text(terms, q)
    for f, (w0, n, d) in zip(fams, FAMILIES):
        for p in f:
            by_pos[p] = text(range(w0, w0 + n), d)
    docs = [None] * NDOCS
    for p, d in enumerate(order):
        docs[d - 1] = by_pos[p]
    return dict(docs=docs, order=order, sizes=sizes, big=big, families=fams)
