"""The crafted dictionaries of the term-matching tests (tests/match_ref.py is the reference).

  abc5    every string over {a, b, c} of length 1..5: 363 terms whose df is one of five values, so
          a pattern's matches tie heavily on (dist, df) and the cut falls inside a class
  edges   the empty term (a NUL-led token); terms of 1, 14..17 and 62..67 bytes that are 0 to 3
          edits apart at their ends and in the middle; pairs that differ by one transposition, one of
          them across bytes 14..16; the bytes 0x01, 0x7F, 0x80 and 0xFF (a signed compare shows);
          long terms whose first 16 bytes are a short term

Each is a list of documents (bytes) for a run, and dictionary() gives what a run makes of them:
the terms in term-table order with their df, computed here from the documents."""
import itertools

import numpy as np

ALPHA = b"abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"


def dictionary(docs):
    """(terms in strcmp("word\\t") order, df by rank, N) of the documents: tokens are maximal runs
    of bytes outside {0x20, 0x09..0x0D}, a term is its token up to the first NUL"""
    df = {}
    for d in docs:
        for t in {tok.split(b"\0")[0] for tok in d.split()}:
            df[t] = df.get(t, 0) + 1
    terms = sorted(df, key=lambda t: t + b"\t")
    return terms, np.array([df[t] for t in terms], dtype=np.uint32), len(docs)


def model(docs) -> dict:
    """the model dict (tfidf_abi.model_match_terms) of the documents"""
    terms, df, n = dictionary(docs)
    return {"N": n, "terms": terms, "df": df}


def spread(terms, ndocs: int = 8, classes: int = 5):
    """term i goes into the documents 0 .. i % classes, repeated 1 + (i + d) % 3 times"""
    docs = [[] for _ in range(ndocs)]
    for i, t in enumerate(terms):
        for d in range(1 + i % classes):
            docs[d] += [t] * (1 + (i + d) % 3)
    return [b" ".join(d) for d in docs]


def abc_strings(lo: int = 1, hi: int = 5):
    return [bytes(s) for n in range(lo, hi + 1) for s in itertools.product(b"abc", repeat=n)]


def abc5():
    return spread(abc_strings())


def base(n: int) -> bytes:
    return (ALPHA * 2)[:n]


def sub(s: bytes, *at) -> bytes:
    b = bytearray(s)
    for i in at:
        b[i] = ord("#") if b[i] != ord("#") else ord("%")
    return bytes(b)


def swap(s: bytes, i: int) -> bytes:
    b = bytearray(s)
    b[i], b[i + 1] = b[i + 1], b[i]
    return bytes(b)


EDGE_LENGTHS = (14, 15, 16, 17, 62, 63, 64, 65, 66, 67)


def edge_terms():
    terms = {b"a", b"b", b"\x01", b"ab", b"ba", b"abc", b"ca", b"acb"}
    for n in EDGE_LENGTHS:
        s = base(n)
        mid = n // 2
        terms |= {s, sub(s, 0), sub(s, mid), sub(s, n - 1), sub(s, 0, n - 1), sub(s, 0, mid, n - 1),
                  s[:mid] + b"+" + s[mid:], b"+" + s[:-1], swap(s, mid), swap(s, n - 2), swap(s, 0)}
    terms |= {swap(base(16), 14), swap(base(17), 15), swap(base(17), 14)}       # across the 16-byte key's end
    terms |= {b"\x01\x7f\x80\xff", b"\x01\x7f\x80\xfe", b"\x01\x7f\xff\x80", b"\x7f\x80", b"\x80\x7f", b"\xff\xff\xff",
              b"\xff\xff\x7f", b"\x80", b"\xff", b"\x7f", b"\x80" * 20, b"\x80" * 19 + b"\x7f", b"\xff" * 64}
    terms |= {base(16) + b"Q" * 24, base(16) + b"R" * 24}                     # share their first 16 bytes with a term
    return sorted(terms)


def edges():
    docs = spread(edge_terms(), ndocs=6, classes=4)
    docs[2] += b" \0zz x\0y"                 # the empty term, and a token cut at its NUL
    return docs


def edge_patterns():
    """(pattern, kind) over the edges dictionary: every term that is a legal pattern, neighbours of
    the long ones that are no term, 63- and 64-byte patterns, prefixes"""
    pats = [(t, 0) for t in edge_terms() if 1 <= len(t) <= 64]
    for n in (15, 16, 17, 62, 63, 64):
        s = base(n)
        pats += [(sub(s, 1), 0), (sub(s, n // 2 + 1, n - 2), 0), (s[1:], 0), (s[:n // 2] + s[n // 2 + 1:], 0)]
    pats += [(base(64)[:63] + b"!", 0), (b"zzzzzz", 0), (b"\xfe", 0), (b"x", 0), (b"xy", 0), (b"\x80\x80", 0)]
    pats += [(p, 1) for p in (b"a", base(14), base(15), base(16), base(17), base(62), base(64), b"\xff", b"\x80", b"\x7f",
                              b"\x01\x7f", b"nothing", sub(base(64), 63))]
    return pats


def docs_of(data, off):
    """the documents of a packed corpus as bytes objects"""
    raw = bytes(data)
    return [raw[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


def edited(rng, word: bytes, nedits: int) -> bytes:
    """the word after nedits random edits (substitute, insert, delete, transpose) with lower-case
    letters, kept within 1..64 bytes"""
    w = bytearray(word)
    for _ in range(nedits):
        op = int(rng.integers(0, 4))
        at = int(rng.integers(0, max(1, len(w))))
        c = int(rng.integers(ord("a"), ord("z") + 1))
        if op == 0 and w:
            w[at] = c
        elif op == 1 and len(w) < 64:
            w.insert(at, c)
        elif op == 2 and len(w) > 1:
            del w[at]
        elif op == 3 and len(w) > 1:
            at = min(at, len(w) - 2)
            w[at], w[at + 1] = w[at + 1], w[at]
    return bytes(w) if w else b"a"


def drawn_patterns(terms, n: int, seed: int):
    """n patterns: terms of 1..64 bytes drawn with the seed, with 0, 1 and 2 random edits in turn"""
    rng = np.random.default_rng(seed)
    legal = [t for t in terms if 1 <= len(t) <= 64]
    return [edited(rng, legal[int(rng.integers(0, len(legal)))], i % 3) for i in range(n)]
