"""The run-stride corpus: about 2 MB on which, with TFIDF_GRID_CUS=1 (four persistent K1
workgroups), every workgroup of k_tokcount_sl / k_tokcount_vs claims ten and more chunks of every
kind one after another, and every wave of the score stage and of emit.hip takes many documents.

K1 carries state from a chunk to the workgroup's next one: k_tokcount_sl clears its LDS table once
per workgroup and relies on every flush clearing what it emits, the few-document flush
(sl_flush_few, groups of <= FEW documents) is always a chunk's last, a chunk may end in overflow
mode with keys still deferred, and the next chunk is claimed ahead.  The corpus is segments of six
kinds in an order shuffled by a fixed seed, so that chunks of different kinds follow each other:

  few        one document of ~2 900 distinct terms, 2 or 3 times each (32-40 KB, <= BIG_DOC): a
             group of one under the claim budget with the table up to 80 % full: sl_flush_few
             with hundreds of displaced keys
  overflow   one document of ~3 400 distinct terms x 2: the waves cross the claim budget with
             keys still deferred: partial records, and sl_flush_few behind overflow mode
  many       2 000 documents of about 30 bytes (every 41st empty, every 59th whitespace only):
             more than GCAP of them in a chunk of either size, so several groups per chunk, the
             general flush, and a last group that is sometimes <= FEW
  hot        a 20 KB document whose every second token is one term: all waves at one slot
  split      a document of 100-120 KB of 1-40-byte tokens over {a, b, c}: above BIG_DOC, so cut
             mid-token into chunks whose first and last documents are partial; long terms; more
             than K5_PS_SPLIT pairs
  odd        eight documents of 65-300 pairs with terms of 15, 16 and 17 bytes that share their
             first 15 bytes, NUL-cut tokens, and in two of them a 5 000-byte term: emit's
             multi-round documents and its direct-write path

A document of at most BIG_DOC bytes is never split: every grid point inside it starts its chunk at
the document's start, so all but the last of them are empty chunks (cs == ce).  The 32-40 KB
documents give those at both chunk sizes; nothing pads them away.

The words of the few / overflow / hot / odd documents come from one pool, so the vocabulary stays
far below the 60 000 terms the retry case of test_gpu_run_stride.py allows.
test_run_stride_corpus_cpu.py establishes on the CPU what the GPU test relies on."""
import functools
import os
import re

import numpy as np

from test_gpu_k1_count_paths import _distinct_words

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parallel-systems-mpi-tfidf_amd")


@functools.lru_cache(maxsize=None)
def _source(name):
    return open(os.path.join(PKG, "csrc", name)).read()


def source_const(name, files=("kernels.h",)):
    """an integer constant of the kernels' sources: `#define NAME expr` or `constexpr T NAME = expr;`,
    expr over integers, shifts, + - * / and other such constants of the same files"""
    for f in files:
        m = (re.search(r"^\s*#\s*define\s+%s\s+([^\n/]+?)\s*(?:/\*|$)" % name, _source(f), flags=re.M) or
             re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, _source(f)))
        if m:
            expr = re.sub(r"\(\s*(?:uint\d+_t|int|unsigned)\s*\)", "", m.group(1))
            expr = re.sub(r"\b(\d+)(?:ull|u)\b", r"\1", expr).replace("/", "//")
            names = set(re.findall(r"[A-Za-z_]\w*", expr))
            return int(eval(expr, {"__builtins__": {}}, {n: source_const(n, files) for n in names}))
    raise AssertionError(name)


SL = ("tokcount_sl.hip", "kernels.h")
CHUNK_SL, CHUNK_VS = source_const("CHUNK_BYTES_ST"), source_const("CHUNK_BYTES")    # 24 576 and 12 288
BIG_DOC = source_const("BIG_DOC")
GCAP, FEW = source_const("GCAP", SL), source_const("FEW", SL)
CLAIM_BUDGET = source_const("WAVE_CLAIMS", SL) * source_const("NWAVE", SL)          # 3 008
K1_WG_PER_CU = source_const("WG_PER_CU", SL)
K5_SMALL_DOC, K5_WAVE, K5_PS_SPLIT = (source_const(n) for n in ("K5_SMALL_DOC", "K5_WAVE", "K5_PS_SPLIT"))
assert source_const("GCAP", ("tokcount_vs.hip", "kernels.h")) == GCAP

SEED = 31
POOL = 6500                  # 3-6-byte words the few / overflow / hot / odd documents draw from
COUNTS = dict(few=8, overflow=14, many=8, hot=15, split=4, odd=10)
MANY_DOCS = 2000
SPLIT_BYTES = (100_000, 120_000, 100_000, 120_000)
ODD_DOCS = 8
LONG_STEM = b"fifteen_bytes_x"                        # 15 bytes: itself, +1 and +2 bytes, all sharing it
LONG_TERMS = [LONG_STEM] + [LONG_STEM + bytes([c]) for c in b"abcdef"] + [LONG_STEM + bytes([c, d]) for c in b"ab" for d in b"yz"]
assert sorted({len(t) for t in LONG_TERMS}) == [15, 16, 17]


@functools.lru_cache(maxsize=None)
def pool():
    return _distinct_words(POOL, np.random.default_rng(SEED), 3, 6)


def few_doc(rep, nterms, twice_only):
    """test_gpu_k1_count_paths.repeated_terms_corpus with a seed per repetition and the words of
    the shared pool"""
    rng = np.random.default_rng([SEED, 1 + twice_only, rep])
    words = [pool()[i] for i in rng.choice(POOL, nterms, replace=False)]
    reps = np.full(nterms, 2) if twice_only else rng.integers(2, 4, nterms)
    toks = np.repeat(np.arange(nterms), reps)
    rng.shuffle(toks)
    doc = b" ".join(words[i] for i in toks) + b"\n"
    assert 32768 <= len(doc) <= min(BIG_DOC, 45056), len(doc)
    return [doc]


def many_docs(rep):
    rng = np.random.default_rng([SEED, 3, rep])
    words = _distinct_words(200, rng, 1, 2)
    docs = []
    for i in range(MANY_DOCS):
        if i % 41 == 7:
            docs.append(b"")
        elif i % 59 == 11:
            docs.append((b" \n", b"\t\n ", b"\n")[i % 3])
        else:
            docs.append(b" ".join(words[j] for j in rng.integers(0, 200, int(rng.integers(8, 14)))) + b"\n")
    return docs


def hot_doc(rep):
    """test_gpu_k1_count_paths.hot_key_corpus with a seed per repetition"""
    rng = np.random.default_rng([SEED, 4, rep])
    words = [pool()[i] for i in rng.choice(POOL, 501, replace=False)]
    hot, others = words[250], words[:250] + words[251:]
    toks, n = [], 0
    while n < 20000:
        toks += [hot, others[int(rng.integers(0, 500))]]
        n += len(hot) + len(toks[-1]) + 2
    return [b" ".join(toks) + b"\n"]


def split_doc(rep):
    """the long document of test_gpu_corpus_windows.chunks_docs"""
    rng = np.random.default_rng([SEED, 5, rep])
    parts, n = [], 0
    while n < SPLIT_BYTES[rep]:
        w = bytes(rng.integers(97, 100, int(rng.integers(1, 41)), dtype=np.uint8))
        sep = b" " if rng.random() < 0.9 else b"\n\t "
        parts.append(w + sep)
        n += len(w) + len(sep)
    return [b"".join(parts)]


def odd_docs(rep):
    rng = np.random.default_rng([SEED, 6, rep])
    huge = bytes(rng.integers(100, 110, 5000, dtype=np.uint8))      # one 5 000-byte term per segment
    docs = []
    for k in range(ODD_DOCS):
        n = int(rng.integers(60, 290))
        toks = [pool()[i] for i in rng.choice(POOL, n, replace=False)]
        toks += [LONG_TERMS[i] for i in rng.choice(len(LONG_TERMS), 5, replace=False)]
        toks += [b"nul\x00cut", b"\x00empty", toks[0] + b"\x00" + toks[1]]   # the terms nul, "" and toks[0] again
        if k in (2, 5):
            toks.append(huge)
        toks = [toks[i] for i in rng.permutation(len(toks))]
        toks += [toks[int(rng.integers(0, len(toks)))] for _ in range(int(rng.integers(0, 40)))]
        docs.append(b" ".join(toks) + (b"" if k % 3 == 0 else b"\n"))
    return docs


MAKERS = dict(few=lambda r: few_doc(r, 2900 - 7 * r, False), overflow=lambda r: few_doc(r, 3400 - 3 * r, True),
              many=many_docs, hot=hot_doc, split=split_doc, odd=odd_docs)


@functools.lru_cache(maxsize=None)
def build() -> dict:
    """docs (document id i is docs[i - 1]) and, per document, the kind of its segment"""
    segs = [(kind, r) for kind, n in COUNTS.items() for r in range(n)]
    order = np.random.default_rng(SEED).permutation(len(segs))
    docs, kinds = [], []
    for s in order:
        kind, r = segs[int(s)]
        d = MAKERS[kind](r)
        docs += d
        kinds += [kind] * len(d)
    return dict(docs=docs, kinds=kinds)


def plan_chunks(off, cb):
    """k_plan_chunks (tokcount.hip) restated: grid point i is lo + i * cb; a chunk starts at its
    grid point's document's start when that document is at most BIG_DOC bytes, else at the grid
    point.  Returns (chunk_start[n + 1], chunk_doc[n + 1])."""
    off = [int(x) for x in off]
    lo, hi, ndocs = off[0], off[-1], len(off) - 1
    n = -(-(hi - lo) // cb)
    start, doc = [], []
    oa = np.asarray(off, dtype=np.uint64)
    for i in range(n):
        b = lo + i * cb
        d = int(np.searchsorted(oa, np.uint64(b), side="right")) - 1          # doc_off[d] <= b < doc_off[d + 1]
        start.append(off[d] if off[d + 1] - off[d] <= BIG_DOC else b)
        doc.append(d)
    return start + [hi], doc + [ndocs - 1 if ndocs else 0]
