"""Word n-grams in plain Python: the definition of include/tfidf.h, section "n-grams", and the
only reference of the n-gram tests."""
SEP = (0x20, 0x09, 0x0A, 0x0B, 0x0C, 0x0D)


def ngrams(data, off, min_n=1, max_n=2, joiner=0x5F):
    raw, off = bytes(data), [int(x) for x in off]
    out, out_off = bytearray(), [0]
    for b, e in zip(off[:-1], off[1:]):
        doc, toks, i = raw[b:e], [], 0
        while i < len(doc):
            if doc[i] in SEP:
                i += 1
                continue
            j = i
            while j < len(doc) and doc[j] not in SEP:
                j += 1
            toks.append(doc[i:j])
            i = j
        for p in range(len(toks)):
            for n in range(min_n, max_n + 1):
                if p + n <= len(toks):
                    out += bytes([joiner]).join(toks[p:p + n]) + b" "
        out_off.append(len(out))
    return bytes(out), out_off


def tokens(data, off):
    """the token sequence of every document"""
    raw, off = bytes(data), [int(x) for x in off]
    table = bytes.maketrans(bytes(SEP), b" " * len(SEP))
    return [[t for t in raw[b:e].translate(table).split(b" ") if t] for b, e in zip(off[:-1], off[1:])]


def counts(data, off, min_n, max_n):
    """(tokens, grams) of the documents: grams = sum over docs and n of max(0, m - n + 1)"""
    ms = [len(t) for t in tokens(data, off)]
    return sum(ms), sum(max(0, m - n + 1) for m in ms for n in range(min_n, max_n + 1))


LITERAL = (b"XXnew  york\ncityrunning onYY", [2, 16, 20, 26])
LITERAL_OUT = {
    (1, 2): (b"new new_york york york_city city runn ing ing_on on ", [0, 33, 38, 52]),
    (2, 3): (b"new_york new_york_city york_city ing_on ", [0, 33, 33, 40]),
}
RANGES = ((1, 1), (1, 2), (2, 3), (3, 8))


def big_corpus(seed=42, target=200_000):
    """docs built like test_gpu_analyze._big_corpus: tokens glued across document boundaries,
    empty documents, NUL and >= 0x80 bytes, every separator"""
    import numpy as np
    rng = np.random.default_rng(seed)
    alpha = [b"a", b"b", b"c", b"A", b"B", b"1", b".", b",", b"\x00", b"\xc3\xa9"]
    seps = [b" ", b" ", b" ", b"\n", b"\t", b"\r", b"\x0b", b"\x0c"]
    docs, total = [], 0
    while total < target:
        parts = []
        for _ in range(int(rng.integers(0, 1500))):
            r = rng.random()
            n = int(rng.integers(1, 9)) if r < 0.97 else int(rng.integers(9, 71))
            parts.append(b"".join(alpha[i] for i in rng.integers(0, len(alpha), n)))
            if rng.random() < 0.97:                       # else: glued to the next token
                parts.append(seps[int(rng.integers(len(seps)))] * int(rng.integers(1, 3)))
        docs.append(b"".join(parts))                     # often ends inside a token: the next document starts there
        total += len(docs[-1])
        if rng.random() < 0.2:
            docs.append(b"")
    return docs
