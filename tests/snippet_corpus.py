"""Crafted documents and job lists for the snippet tests (CPU twin and GPU): the smallest shapes at
which each piece of the definition, and each piece of the device's tile scan, can go wrong.  The
documents are packed back to back with no separator, so bases are unaligned and neighbours adjoin.

The device scans a document in tiles of TILE bytes that start at the 16-byte boundary at or below
the document's first byte, so a tile edge lies at the document-relative offsets TILE * k and
TILE * k - (base % 16); probe tokens are placed on both kinds of edge."""
import random

TILE = 4096
SIZES = (4096, 4097, 8192, 3 * 4096 + 5)
PROBES = (b"fox", b"wolf", b"f")          # words that end, start and lie on an edge
STRADDLE = b"straddle"
T15, T16, T17, T70 = b"a" * 14 + b"p", b"b" * 15 + b"q", b"c" * 16 + b"r", b"long" * 17 + b"st"
assert (len(T15), len(T16), len(T17), len(T70)) == (15, 16, 17, 70)


def _filled(size: int) -> bytearray:
    return bytearray((b"pad " * (size // 4 + 1))[:size])


def _place(buf: bytearray, at: int, word: bytes):
    """word at [at, at + len) with a blank on either side where the document has room for one"""
    if at < 0 or at + len(word) > len(buf):
        return
    if at > 0:
        buf[at - 1] = 0x20
    buf[at:at + len(word)] = word
    if at + len(word) < len(buf):
        buf[at + len(word)] = 0x20


def edge_doc(size: int, base: int, style: int) -> bytes:
    """a document of `size` bytes that will lie at `base`: on every tile edge of either kind a probe
    that ends in the edge's last byte, starts in it, is that byte alone, or straddles the edge"""
    buf = _filled(size)
    edges = sorted({TILE * k - d for k in range(1, size // TILE + 2) for d in (0, base % 16)})
    for i, e in enumerate(e for e in edges if 16 <= e <= size):
        kind = (i + style) % 4
        if kind == 0:
            _place(buf, e - 3, b"fox")                  # ends in the tile's last byte
        elif kind == 1:
            _place(buf, e - 1, b"wolf")                 # starts in the tile's last byte
        elif kind == 2:
            _place(buf, e - 1, b"f")                    # is the tile's last byte
        else:
            _place(buf, e - 4, STRADDLE)                # four bytes on either side
    _place(buf, size - 3, b"fox")                       # the document's last token; the next one adjoins it
    _place(buf, 0, b"fox")                              # ... with its first token
    return bytes(buf)


def build():
    """docs: the documents in corpus order (global ids 1..n); names: name -> global id"""
    docs, names = [], {}

    def add(name, b):
        docs.append(bytes(b))
        names[name] = len(docs)

    def base():
        return sum(len(d) for d in docs)

    add("lead7", b"seven b")                                    # 7 bytes: the next base is 7 mod 16
    for style, size in enumerate(SIZES):
        add("edge_u%d" % size, edge_doc(size, base(), style))   # unaligned bases
    add("align", b" " * ((-base()) % 16))                       # whitespace only; the next base is 0 mod 16
    assert base() % 16 == 0
    for style, size in enumerate(SIZES):
        add("edge_a%d" % size, edge_doc(size, base(), style + 1))   # the first two at 0 mod 16, then 1 mod 16
    add("empty", b"")
    add("blank", b" \t\n \r\v\f ")
    for n in (7, 8, 9):                                         # T = W - 1, W, W + 1 at W = 8
        add("t%d" % n, b" ".join([b"fox"] + [b"x%d" % i for i in range(n - 2)] + [b"wolf"]))
    rng = random.Random(7)
    words = [b"fox" if rng.random() < 0.02 else b"wolf" if rng.random() < 0.02 else b"n%d" % (i % 97) for i in range(1500)]
    words[3], words[1499] = b"fox", b"wolf"
    add("t1500", b"\n".join(words))
    add("nul", b"fox\0abc pad \0lead wolf\0 pad fox")
    add("lens", b" ".join([T15, b"pad", T16, T17, b"pad", T70, T16 + b"x", b"abcdefghi", b"abcdefgh", T70 + b"y"]))
    add("cover", b"fox fox fox fox fox " + b"pad " * 20 + b"fox wolf " + b"pad " * 5)
    add("tie", b"pad fox wolf " + b"pad " * 20 + b"fox wolf pad")
    add("clip0", b"pad fox " + b"pad " * 30)
    add("clipT", b"pad " * 30 + b"fox")
    add("left", b"wolf pad fox hen " + b"pad " * 3 + b"cat " + b"pad " * 12)
    add("many", b"fox wolf " * 20)
    add("t256", b" ".join([b"t255", b"pad", b"t256", b"t0", b"t7"]))
    add("ones", b"a " * 40000)                                  # 40 000 one-letter tokens, about 80 KB
    return docs, names


QUERIES = [
    b"fox wolf f straddle",                                                     # 0: the edge probes
    b"fox",                                                                     # 1
    b"wolf fox wolf fox fox",                                                   # 2: duplicates
    b"zzabsent qqabsent",                                                       # 3: no found term
    b"fox \0 wolf",                                                             # 4: the empty term
    b" ".join([T15, T16, T17, T70, b"abcdefgh"]),                               # 5: 15, 16, 17, 70 bytes
    b" ".join(b"t%d" % i for i in range(256)),                                  # 6: 256 distinct terms
    b" ".join(b"t%d" % i for i in range(257)),                                  # 7: 257: truncated
    b"a",                                                                       # 8
    b"fox wolf hen cat",                                                        # 9
    b"",                                                                        # 10: an empty query
]


def cases():
    """(name, jobs, window, max_marks) over QUERIES and build()'s documents"""
    docs, names = build()
    n = len(docs)
    every = [(q, d) for d in range(1, n) for q in (0, 2)]                        # all but `ones`
    shuffled = list(every)
    random.Random(3).shuffle(shuffled)
    edge = [(0, names[k]) for k in names if k.startswith("edge_")]
    out = [
        ("edges_w8", edge, 8, 32),
        ("edges_w1", edge, 1, 1),
        ("every_w8", every, 8, 32),
        ("shuffled_w5", shuffled[:40] + [shuffled[0], shuffled[0], (1, n + 5), (3, 0)], 5, 3),
        ("tw", [(q, names[k]) for k in ("t7", "t8", "t9", "empty", "blank") for q in (0, 1, 3)], 8, 32),
        ("w1024", [(q, names["t1500"]) for q in (0, 1, 2)] + [(0, names["t9"])], 1024, 1024),
        ("w1", [(0, names["t1500"]), (0, names["tie"]), (0, names["empty"])], 1, 32),
        ("nul", [(4, names["nul"]), (1, names["nul"]), (4, names["blank"])], 4, 32),
        ("lens", [(5, names["lens"])], 6, 32),
        ("order", [(0, names[k]) for k in ("cover", "tie", "clip0", "clipT")] + [(9, names["left"])], 5, 32),
        ("order_w8", [(0, names[k]) for k in ("cover", "tie", "clip0", "clipT")] + [(9, names["left"])], 8, 32),
        ("m0", [(0, names["many"]), (2, names["cover"])], 16, 0),
        ("m3", [(0, names["many"]), (2, names["cover"])], 16, 3),
        ("notfound", [(3, d) for d in range(1, n)] + [(10, names["tie"])], 8, 32),
        ("t256", [(6, names["t256"]), (7, names["t256"]), (6, names["tie"]), (7, names["empty"])], 8, 32),
        ("three_queries", [(0, names["tie"]), (1, names["tie"]), (9, names["tie"])], 8, 32),
        ("nojobs", [], 8, 32),
    ]
    return out


def ones_jobs():
    docs, names = build()
    return [(8, names["ones"]), (0, names["tie"]), (8, names["ones"]), (1, names["ones"]), (8, names["many"])]
