"""Term matching as include/tfidf.h defines it ("term matching"), in plain Python: a full
dynamic-programming matrix over bytes, the optimal-string-alignment recurrence under the
transposition flag, and `sorted` with the defined key.  Nothing here comes from the implementation.

A dictionary is a list of terms (bytes) in term-table order, strcmp of word + "\\t", so a term's
rank is its index, and a list of their document frequencies."""
import functools

import numpy as np

FUZZY, PREFIX = 0, 1


class Bags:
    """The terms' byte histograms, for dictionaries too large to evaluate every (pattern, term)
    matrix in Python.  The bag distance of two strings, the larger of the two multiset
    differences of their bytes, never exceeds their edit distance: an insertion, deletion or
    substitution takes at most one byte out of each difference and a transposition none.  So a
    term whose bag distance from the pattern exceeds the budget is no match, and matches() may
    skip its matrix.  tests/test_match_cpu.py asserts that the rows with and without are equal."""

    def __init__(self, terms):
        self.h = np.zeros((len(terms), 256), dtype=np.int16)
        for i, t in enumerate(terms):
            if t:
                self.h[i] = np.bincount(np.frombuffer(t, dtype=np.uint8), minlength=256)

    def within(self, pattern: bytes, d: int):
        diff = self.h - np.bincount(np.frombuffer(pattern, dtype=np.uint8), minlength=256).astype(np.int16)
        more = np.clip(diff, 0, None).sum(axis=1)
        less = np.clip(-diff, 0, None).sum(axis=1)
        return np.flatnonzero(np.maximum(more, less) <= d).tolist()


@functools.lru_cache(maxsize=None)
def edit_distance(p: bytes, t: bytes, transpose: bool) -> int:
    """Levenshtein distance of the byte strings; with transpose the optimal-string-alignment
    distance (an adjacent transposition is one edit, no substring is edited twice)"""
    m, n = len(p), len(t)
    D = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        D[i][0] = i
    for j in range(n + 1):
        D[0][j] = j
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            v = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (p[i - 1] != t[j - 1]))
            if transpose and i > 1 and j > 1 and p[i - 1] == t[j - 2] and p[i - 2] == t[j - 1]:
                v = min(v, D[i - 2][j - 2] + 1)
            D[i][j] = v
    return D[m][n]


def matches(terms, df, pattern: bytes, kind: int, max_edits: int, transpose: bool = True, fixed_prefix: int = 0,
            bags: Bags = None):
    """every match of the pattern as (rank, dist, df), in the defined order: dist ascending, df
    descending, rank ascending"""
    out = []
    ranks = range(len(terms)) if bags is None or kind == PREFIX else bags.within(pattern, max_edits)
    for rank in ranks:
        t = terms[rank]
        if kind == PREFIX:
            if t[:len(pattern)] == pattern:
                out.append((rank, 0, int(df[rank])))
            continue
        fix = min(fixed_prefix, len(pattern))
        if t[:fix] != pattern[:fix]:
            continue
        if abs(len(t) - len(pattern)) > max_edits:      # the distance is at least the difference of the lengths
            continue
        d = edit_distance(pattern, t, bool(transpose))
        if d <= max_edits:
            out.append((rank, d, int(df[rank])))
    return sorted(out, key=lambda x: (x[1], -x[2], x[0]))


def expand(terms, df, patterns, kinds, max_edits, E: int, transpose: bool = True, fixed_prefix: int = 0,
           bags: Bags = None):
    """per pattern (nmatch, the first E matches as (rank, dist, df, word))"""
    n = len(patterns)
    kinds = [kinds] * n if isinstance(kinds, int) else list(kinds)
    max_edits = [max_edits] * n if isinstance(max_edits, int) else list(max_edits)
    rows = []
    for p, k, d in zip(patterns, kinds, max_edits):
        m = matches(terms, df, p, k, d, transpose, fixed_prefix, bags)
        rows.append((len(m), [(r, dd, f, terms[r]) for r, dd, f in m[:E]]))
    return rows


def check(res: dict, rows, E: int, term: bool = True, nmatch: bool = True):
    """a result of the binding (Engine.match_terms, model_match_terms, ..) equals the rows of expand:
    counts, ranks, distances, df and word bytes, all exactly"""
    assert res["k"] == E and len(res["words"]) == len(rows) and res["term"].shape == (len(rows), E)
    for i, (n, want) in enumerate(rows):
        k = len(want)
        if nmatch:
            assert int(res["nmatch"][i]) == n, (i, int(res["nmatch"][i]), n)
        assert int(res["nterms"][i]) == k == min(E, n), (i, int(res["nterms"][i]), k)
        assert res["words"][i] == [w for _, _, _, w in want], (i, res["words"][i][:5], want[:5])
        assert res["dist"][i, :k].tolist() == [d for _, d, _, _ in want], i
        assert res["df"][i, :k].tolist() == [f for _, _, f, _ in want], i
        if term:
            assert res["term"][i, :k].tolist() == [r for r, _, _, _ in want], i
