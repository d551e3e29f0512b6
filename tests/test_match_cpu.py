"""Term matching on the host (no GPU): tfidf_model_match_terms, the plain-C twin of the device
scan, against tests/match_ref.py on the crafted dictionaries of tests/match_corpus.py, and
tfidf_match_check's rules.  Everything is compared exactly: ranks, distances, df, counts and word
bytes."""
import ctypes as C

import pytest

import match_corpus
import match_ref
import tfidf_abi

ES = (1, 3, 50, 1024)


@pytest.fixture(scope="module")
def abc5():
    m = match_corpus.model(match_corpus.abc5())
    assert len(m["terms"]) == 363 and len(set(m["df"].tolist())) == 5
    return m


@pytest.fixture(scope="module")
def edges():
    m = match_corpus.model(match_corpus.edges())
    lens = {len(t) for t in m["terms"]}
    assert {0, 1, 14, 15, 16, 17, 62, 63, 64, 65, 66, 67} <= lens
    return m


def test_abi():
    assert tfidf_abi.lib().tfidf_abi_version() == tfidf_abi.ABI_VERSION == 2
    for name in ("tfidf_match_check", "tfidf_match_terms", "tfidf_term_matches_free", "tfidf_group_match_terms",
                 "tfidf_model_match_terms", "tfidf_last_match_info"):
        assert name in tfidf_abi.EXPORTS and hasattr(tfidf_abi.lib(), name)
    assert C.sizeof(tfidf_abi.MatchParams) == 32 and C.sizeof(tfidf_abi.MatchInfo) == 72


@pytest.mark.parametrize("transpose", [True, False])
@pytest.mark.parametrize("d", [0, 1, 2])
def test_abc5_every_pattern(abc5, transpose, d):
    pats = match_corpus.abc_strings()
    assert len(pats) == 363
    full = match_ref.expand(abc5["terms"], abc5["df"], pats, match_ref.FUZZY, d, 1 << 30, transpose)
    for E in ES:
        got = tfidf_abi.model_match_terms(abc5, pats, max_edits=d, max_expansions=E, transpose=transpose)
        match_ref.check(got, [(n, rows[:E]) for n, rows in full], E)


def test_abc5_prefix_and_fixed_prefix(abc5):
    pats = match_corpus.abc_strings(1, 4)
    rows = match_ref.expand(abc5["terms"], abc5["df"], pats, match_ref.PREFIX, 0, 50)
    assert rows[0][0] == 121                                         # "a" and everything behind it
    match_ref.check(tfidf_abi.model_match_terms(abc5, pats, kinds=tfidf_abi.MATCH_PREFIX, max_expansions=50), rows, 50)
    for fp in (1, 2, 5, 64):
        rows = match_ref.expand(abc5["terms"], abc5["df"], pats, match_ref.FUZZY, 2, 50, True, fp)
        match_ref.check(tfidf_abi.model_match_terms(abc5, pats, max_expansions=50, fixed_prefix=fp), rows, 50)


@pytest.mark.parametrize("transpose", [True, False])
def test_edges(edges, transpose):
    pk = match_corpus.edge_patterns()
    pats, kinds = [p for p, _ in pk], [k for _, k in pk]
    for d in (0, 1, 2):
        for E, fp in ((3, 0), (1024, 0), (50, 15)):
            rows = match_ref.expand(edges["terms"], edges["df"], pats, kinds, d, E, transpose, fp)
            got = tfidf_abi.model_match_terms(edges, pats, kinds=kinds, max_edits=d, max_expansions=E,
                                              transpose=transpose, fixed_prefix=fp)
            match_ref.check(got, rows, E)


def test_mixed_budgets_in_one_call(edges):
    pk = match_corpus.edge_patterns()
    pats, kinds = [p for p, _ in pk], [k for _, k in pk]
    edits = [i % 3 for i in range(len(pats))]
    rows = match_ref.expand(edges["terms"], edges["df"], pats, kinds, edits, 7)
    match_ref.check(tfidf_abi.model_match_terms(edges, pats, kinds=kinds, max_edits=edits, max_expansions=7), rows, 7)


def test_the_inputs_exercise_what_they_are_for(abc5, edges):
    """from the reference alone"""
    d = match_ref.edit_distance
    assert d(b"ab", b"ba", True) == 1 and d(b"ab", b"ba", False) == 2
    assert d(b"ca", b"abc", True) == 3 and d(b"ca", b"abc", False) == 3
    terms, df = abc5["terms"], abc5["df"]
    pats = match_corpus.abc_strings()
    # some pair within budget where the transposition counts
    assert any(d(p, t, True) != d(p, t, False) and d(p, t, True) <= 2 for p in pats[:60] for t in terms)
    # "ca" does not reach "abc" at d = 2
    ca = match_ref.matches(terms, df, b"ca", 0, 2, True)
    assert terms.index(b"abc") not in [r for r, _, _ in ca]
    # more than E matches, the cut inside a class of equal (dist, df)
    m = match_ref.matches(terms, df, b"abc", 0, 2, True)
    assert len(m) > 50 and m[49][1:] == m[50][1:]
    assert len(m) > 3 and m[2][1:] == m[3][1:]
    eterms, edf = edges["terms"], edges["df"]
    assert match_ref.matches(eterms, edf, b"zzzzzz", 0, 2) == []                       # matches nothing
    e = eterms.index(b"")                                                              # the empty term
    assert e in [r for r, _, _ in match_ref.matches(eterms, edf, b"x", 0, 1)]
    assert e not in [r for r, _, _ in match_ref.matches(eterms, edf, b"xy", 0, 1)]
    assert e in [r for r, _, _ in match_ref.matches(eterms, edf, b"xy", 0, 2)]
    # 0x80 sorts above 0x7F, and they are one substitution apart
    assert d(b"\x80" * 20, b"\x80" * 19 + b"\x7f", True) == 1
    assert eterms.index(b"\x7f") < eterms.index(b"\x80") < eterms.index(b"\xff")


def test_match_check_rules():
    ok = tfidf_abi.match_check
    P = tfidf_abi.match_params
    assert ok([b"a", b"x" * 64], max_edits=[0, 2]) == 0
    assert ok([]) == 0                                                             # no patterns is valid
    assert ok([b""]) == tfidf_abi.E_INVAL and ok([b"a", b""]) == tfidf_abi.E_INVAL  # length 0
    assert ok([b"x" * 65]) == tfidf_abi.E_INVAL and ok([b"x" * 65], kinds=1) == tfidf_abi.E_INVAL
    assert ok([b"ab"], max_edits=3) == tfidf_abi.E_INVAL and ok([b"ab"], max_edits=2) == 0
    assert ok([b"ab"], kinds=1, max_edits=3) == 0                                   # ignored for a prefix pattern
    assert ok([b"ab"], kinds=2) == tfidf_abi.E_INVAL
    for E, rc in ((0, tfidf_abi.E_INVAL), (1, 0), (1024, 0), (1025, tfidf_abi.E_INVAL)):
        assert ok([b"ab"], max_expansions=E) == rc
    assert ok([b"ab"], fixed_prefix=64) == 0 and ok([b"ab"], fixed_prefix=65) == tfidf_abi.E_INVAL
    assert ok([b"ab"], list_records=1023) == tfidf_abi.E_INVAL and ok([b"ab"], list_records=1) == tfidf_abi.E_INVAL
    assert ok([b"ab"], list_records=1024) == 0 and ok([b"ab"], list_records=0) == 0
    assert ok([b"ab"], flags=2) == tfidf_abi.E_INVAL and ok([b"ab"], flags=1) == 0 and ok([b"ab"], flags=0) == 0
    assert ok([b"ab"], size=C.sizeof(tfidf_abi.MatchParams) - 8) == tfidf_abi.E_INVAL
    assert ok([b"ab"], size=C.sizeof(tfidf_abi.MatchParams) + 8) == 0
    lib = tfidf_abi.lib()
    ps, keep = tfidf_abi.make_patterns([b"ab", b"cd"])
    assert lib.tfidf_match_check(None, C.byref(P())) == tfidf_abi.E_INVAL
    assert lib.tfidf_match_check(C.byref(ps), None) == tfidf_abi.E_INVAL
    ps.nbytes = 3                                                                  # p_off[npatterns] > nbytes
    assert ok(ps) == tfidf_abi.E_INVAL
    ps.nbytes = 4
    assert ok(ps) == 0
    keep[1][1] = 5                                                                 # non-monotone
    assert ok(ps) == tfidf_abi.E_INVAL
    keep[1][1] = 2
    ps.kind = None
    assert ok(ps) == tfidf_abi.E_INVAL
    ps.npatterns = tfidf_abi.MATCH_MAX_PATTERNS + 1
    assert ok(ps) == tfidf_abi.E_INVAL


def test_model_match_errors(abc5):
    with pytest.raises(tfidf_abi.TfidfError) as ex:
        tfidf_abi.model_match_terms(abc5, [b"ab"], max_edits=3)
    assert ex.value.rc == tfidf_abi.E_INVAL
    bad = dict(abc5, terms=abc5["terms"][::-1])                                     # not in term-table order
    with pytest.raises(tfidf_abi.TfidfError) as ex:
        tfidf_abi.model_match_terms(bad, [b"ab"])
    assert ex.value.rc == tfidf_abi.E_INVAL
    got = tfidf_abi.model_match_terms(abc5, [])
    assert got["nmatch"].shape == (0,) and got["words"] == []
    empty = {"N": 3, "terms": [], "df": []}
    got = tfidf_abi.model_match_terms(empty, [b"ab", b"c"], kinds=[0, 1])
    assert got["nmatch"].tolist() == [0, 0] and got["words"] == [[], []]


def test_the_bag_filter_of_the_reference_changes_no_row(abc5, edges):
    """match_ref.Bags skips matrices for large dictionaries: the rows are the unfiltered ones"""
    for m, pats in ((abc5, match_corpus.abc_strings(1, 4)), (edges, [p for p, k in match_corpus.edge_patterns() if k == 0])):
        bags = match_ref.Bags(m["terms"])
        for d in (0, 1, 2):
            for transpose in (True, False):
                assert match_ref.expand(m["terms"], m["df"], pats, 0, d, 1024, transpose, 0, bags) == \
                    match_ref.expand(m["terms"], m["df"], pats, 0, d, 1024, transpose, 0)
