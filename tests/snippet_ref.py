"""The definition of snippets (include/tfidf.h, "snippets") in straightforward Python over bytes:
tokenise, U(q), matches, every candidate window by brute force, centring, recount, marks, text.
The reference the device path and its plain-C twin are compared with, field for field."""
import bisect
import re

MAX_TERMS = 256
NO_DOC = 1
TRUNCATED = 2
_TOKEN = re.compile(rb"[^ \t\n\v\f\r]+")


def tokens(b: bytes):
    """(byte offset, term) of every token: maximal runs of non-whitespace, the term up to the first NUL"""
    return [(m.start(), m.group().split(b"\0", 1)[0]) for m in _TOKEN.finditer(b)]


def query_terms(q: bytes):
    """U(q) cut at MAX_TERMS as (offset in q, term), and whether the query had more"""
    seen, used, more = set(), [], False
    for pos, t in tokens(q):
        if t in seen:
            continue
        if len(used) == MAX_TERMS:
            more = True
            continue
        seen.add(t)
        used.append((pos, t))
    return used, more


def best_start(match, W, starts):
    """the start among `starts` with the largest (cover, hits), the smallest on a tie, and that pair"""
    best, best_s = (-1, -1), None
    pos = [p for p, _ in match]   # ascending: only the matches of the window are looked at
    for s in starts:
        inside = [sl for _, sl in match[bisect.bisect_left(pos, s):bisect.bisect_left(pos, s + W)]]
        key = (len(set(inside)), len(inside))
        if key > best:
            best, best_s = key, s
    return best_s, best


def snippet(doc: bytes, q: bytes, vocab, W: int, M: int, text: bool = True) -> dict:
    """one job on a document this context holds; vocab: the set of resident terms"""
    used, more = query_terms(q)
    slot = {t: s for s, (_, t) in enumerate(used) if t in vocab}
    toks = tokens(doc)
    T = len(toks)
    match = [(i, slot[t]) for i, (_, t) in enumerate(toks) if t in slot]
    out = {"flags": TRUNCATED if more else 0, "ntokens": T, "nmatch": len(match),
           "nterms_matched": len({s for _, s in match}), "win_tok": (0, 0), "win_byte": (0, 0), "cover": 0, "hits": 0,
           "marks": [], "text": b"" if text else None}
    if T == 0:
        return out
    s1, e1 = 0, min(W, T)
    if match:
        s, _ = best_start(match, W, [p for p, _ in match])
        last = max(p for p, _ in match if s <= p < s + W)
        slack = W - (last - s + 1)
        s1 = s - min(s, slack // 2)
        e1 = min(s1 + W, T)
    inside = [(p, sl) for p, sl in match if s1 <= p < e1]
    out["win_tok"] = (s1, e1)
    out["win_byte"] = (toks[s1][0], toks[e1][0] if e1 < T else len(doc))
    out["cover"] = len({sl for _, sl in inside})
    out["hits"] = len(inside)
    out["marks"] = [(toks[p][0], len(toks[p][1]), sl) for p, sl in inside[:M]]
    if text:
        out["text"] = doc[out["win_byte"][0]:out["win_byte"][1]]
    return out


def no_doc(text: bool = True) -> dict:
    return {"flags": NO_DOC, "ntokens": 0, "nmatch": 0, "nterms_matched": 0, "win_tok": (0, 0), "win_byte": (0, 0),
            "cover": 0, "hits": 0, "marks": [], "text": b"" if text else None}


def vocabulary(docs):
    return {t for d in docs for _, t in tokens(d)}


def run(docs: dict, queries, jobs, vocab=None, window: int = 32, max_marks: int = 32, text: bool = True):
    """docs: global id -> bytes.  Returns (per-job dicts, per-query [(offset, length, found)])."""
    vocab = vocabulary(docs.values()) if vocab is None else vocab
    cache = {}
    rows = []
    for q, d in jobs:
        if d not in docs:
            rows.append(no_doc(text))
            continue
        if (q, d) not in cache:
            cache[(q, d)] = snippet(docs[d], queries[q], vocab, window, max_marks, text)
        rows.append(cache[(q, d)])
    qterms = [[(pos, len(t), int(t in vocab)) for pos, t in query_terms(q)[0]] for q in queries]
    return rows, qterms


def check(got: dict, rows, qterms=None, what: str = ""):
    """every field of a tfidf_abi snippets dict against the reference's rows"""
    assert len(got["flags"]) == len(rows), what
    for j, r in enumerate(rows):
        g = {"flags": int(got["flags"][j]), "ntokens": int(got["ntokens"][j]), "nmatch": int(got["nmatch"][j]),
             "nterms_matched": int(got["nterms_matched"][j]), "win_tok": tuple(int(x) for x in got["win_tok"][j]),
             "win_byte": tuple(int(x) for x in got["win_byte"][j]), "cover": int(got["cover"][j]),
             "hits": int(got["hits"][j]), "marks": [tuple(int(x) for x in m) for m in got["marks"][j]],
             "text": got["text"][j]}
        assert g == r, "%s job %d: got %r, expected %r" % (what, j, g, r)
    if qterms is not None:
        assert [[tuple(int(x) for x in t) for t in q] for q in got["qterms"]] == qterms, what


def render(q_index: int, doc_id: int, row: dict, nused: int) -> bytes:
    """the CLI's line of one hit: q<i> TAB doc<N> TAB s' TAB cover/|U| TAB text with [marks]"""
    t, base = row["text"], row["win_byte"][0]
    out, at = bytearray(), 0
    for b, n, _ in row["marks"]:
        out += t[at:b - base] + b"[" + t[b - base:b - base + n] + b"]"
        at = b - base + n
    out += t[at:]
    line = bytes(c if c >= 0x20 else 0x20 for c in out).rstrip(b" ")
    return b"q%d\tdoc%d\t%d\t%d/%d\t%s\n" % (q_index, doc_id, row["win_tok"][0], row["cover"], nused, line)
