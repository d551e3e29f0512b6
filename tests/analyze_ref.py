"""The analyzer's definition (include/tfidf.h, section "analyzer") in plain Python: the only
reference of the analyzer tests.  Also the helpers that decorate a clean corpus."""
import numpy as np

SEPARATORS = (0x20, 0x09, 0x0A, 0x0B, 0x0C, 0x0D)
PUNCT = [c for c in range(0x80) if not (chr(c).isalnum() or c in SEPARATORS)]


def byte_map(lower: bool, punct: bool) -> list:
    t = list(range(256))
    for c in range(0x80):
        if punct and c in PUNCT:
            t[c] = 0x20
        if lower and 0x41 <= c <= 0x5A:
            t[c] = c + 0x20
    return t


def analyze(data, off, lower=False, punct=False, min_len=0, stop=()) -> np.ndarray:
    """data: the bytes, off: the documents' offsets; returns the analyzed bytes"""
    t, stop = byte_map(lower, punct), set(bytes(w) for w in stop)
    out = bytearray(bytes(data))
    off = [int(x) for x in off]
    for b, e in zip(off[:-1], off[1:]):
        doc = bytearray(t[c] for c in out[b:e])
        i = 0
        while i < len(doc):
            if doc[i] in SEPARATORS:
                i += 1
                continue
            j = i
            while j < len(doc) and doc[j] not in SEPARATORS:
                j += 1
            if j - i < min_len or bytes(doc[i:j]) in stop:
                doc[i:j] = b" " * (j - i)
            i = j
        out[b:e] = doc
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()


def decorate(data, off, seed: int):
    """Upper-cases some letters and glues punctuation to the front or back of some tokens (never
    inside one); returns (data, off) of the decorated documents.  LOWER | PUNCT maps every token
    back to the clean corpus's."""
    rng = np.random.default_rng(seed)
    raw, off = bytes(data), [int(x) for x in off]
    glue = [bytes([c]) for c in PUNCT]
    docs = []
    for b, e in zip(off[:-1], off[1:]):
        doc, parts, i = raw[b:e], [], 0
        while i < len(doc):
            j = i
            if doc[i] in SEPARATORS:
                while j < len(doc) and doc[j] in SEPARATORS:
                    j += 1
                parts.append(doc[i:j])
            else:
                while j < len(doc) and doc[j] not in SEPARATORS:
                    j += 1
                w = bytearray(doc[i:j])
                for k in range(len(w)):
                    if 0x61 <= w[k] <= 0x7A and rng.random() < 0.3:
                        w[k] -= 0x20
                r = rng.random()
                front = glue[rng.integers(len(glue))] if r < 0.25 else b""
                back = glue[rng.integers(len(glue))] if 0.15 < r < 0.5 else b""
                parts.append(front + bytes(w) + back)
            i = j
        docs.append(b"".join(parts))
    o = np.zeros(len(docs) + 1, dtype=np.uint64)
    o[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
    return np.frombuffer(b"".join(docs), dtype=np.uint8).copy(), o
