"""What test_gpu_topk_rounds.py relies on, established without a GPU on the references alone (the
oracle's result on tests/topk_corpus.py, ranked by the plain Python loops of the query, BM25, clause
and similar tests): the round schedule, and that the rankings really spread their winners over every
first-round slice and both second-round slices, cut inside a slice, leave short lists, and tie at
the cut.  These are conditions on the corpus, not measurements: if QT_SLICE or the generator changes
and one of them fails, the seed is what has to follow, not the threshold.

Measured with seed 7 (hits; winners per first-round slice at k = 1024 / 1000; winners in second-round
slice 1 at k = 1024 / 1000), TF-IDF:
  w00 w01 w01 w02           4697   196 213 229 207 179 / 194 206 214 207 179   179 /  83
  w05                       1690   198 232 172 223 199 / 198 211 169 223 199   199 / 103
  w07 w08 w09 w10 w11 w12   8562   229 194 214 201 186 / 226 190 213 193 178   186 /  82
  all                      19995   101  85 357 386  95 / 101  85 357 362  95    95 /   0
BM25: the same hit counts, 171 to 240 winners per slice, 173 to 199 / 77 to 103 in second-round
slice 1.  Clause queries 0, 1, 2, 4: 1604, 1690, 2669 and 18311 hits, 150 to 230 winners per slice,
88 to 216 in second-round slice 1.  Similar rows: 19994 neighbours each, 172 to 232 winners per
slice, 76 to 198 in second-round slice 1."""
import pytest

import topk_corpus as TC

NSL = 5


@pytest.fixture(scope="module")
def tc():
    return TC.references()


def test_round_schedule():
    assert TC.QT_SLICE == 4096
    assert TC.rounds(20000, 1024) == [5, 2, 1]
    assert TC.rounds(20000, 1000) == [5, 2, 1]
    assert TC.rounds(20000, 10) == [5, 1]
    assert TC.rounds(5000, 1024) == [2, 1]                          # what the suite had before
    assert TC.rounds(16384, 1024) == [4, 1] and TC.rounds(16385, 1024) == [5, 2, 1]     # the threshold itself
    assert TC.rounds(4096, 1024) == [1] and TC.rounds(4097, 1024) == [2, 1]
    assert TC.rounds(65536, 1024) == [16, 4, 1] and TC.rounds(65537, 1024) == [17, 5, 2, 1]
    assert TC.rounds(70001, 1024) == [18, 5, 2, 1] and TC.rounds(1, 1) == [1]
    assert TC.second_round_slice(4 * 4096, 95, 1000) == 0 and TC.second_round_slice(4 * 4096, 96, 1000) == 1
    assert TC.second_round_slice(4 * 4096 - 1, 1023, 1024) == 0 and TC.second_round_slice(4 * 4096, 0, 1024) == 1


def test_the_corpus_is_what_the_generator_says(tc):
    assert len(tc["docs"]) == TC.N == 20000 and -(-TC.N // TC.QT_SLICE) == NSL
    assert 300000 < len(tc["data"]) < 450000
    assert sorted(tc["docs"][d - 1] for d in tc["empty"]) == [b""] * 5 and tc["docs"].count(b"") == 5
    assert [tc["pos"][d] // TC.QT_SLICE for d in tc["empty"]] == [0, 0, 2, 4, 4]      # slices 1 and 3 stay full
    assert tc["ora"]["nterms"] == TC.NWORDS + 1
    assert [tc["pos"].get(d, -1) // TC.QT_SLICE for d in tc["similar"][:NSL]] == list(range(NSL))
    assert tc["similar"][NSL] in tc["empty"] and tc["similar"][NSL + 1] > TC.N
    # ids 1 .. 1024 are scattered over every slice: the winners of a tie interleave across slices
    assert {tc["pos"][d] // TC.QT_SLICE for d in range(1, 1025)} == set(range(NSL))


def rankings(tc):
    """(name, best-first hits [(doc, score)]) of every ranking that must spread its winners"""
    out = []
    for name in ("plain", "bm25"):
        out += [("%s %r" % (name, TC.PLAIN[q]), tc[name][q][0]) for q in TC.WORD_QUERIES]
    for r in ("tfidf", "bm25"):
        out += [("clauses %s %d" % (r, q), tc["clauses"][r][q][0]) for q in TC.CLAUSE_SPREAD]
    out += [("similar %d" % row[0], [(d, s) for d, _, s in row[4]]) for row in tc["rows"][:NSL]]
    return out


@pytest.mark.parametrize("k", [1024, 1000])
def test_winners_in_every_first_and_second_round_slice(tc, k):
    names = rankings(tc)
    assert len(names) == 6 + 8 + NSL
    for name, hits in names:
        s = TC.split(hits, tc["pos"], k)
        print(name, k, len(hits), s["per"], s["win"], s["second"])
        assert len(hits) > k and sum(s["win"]) == k, name
        assert min(s["win"]) >= 50, name                            # every first-round slice
        assert set(s["second"]) == {0, 1} and s["second"][1] >= 50, name
        if k == 1000:                                               # the last slice's list straddles the boundary, live on both sides
            assert any(r < 96 for r in s["ranks4"]) and sum(r >= 96 for r in s["ranks4"]) >= 50, name
            assert s["second"][1] == sum(r >= 96 for r in s["ranks4"]), name
        else:
            assert s["second"][1] == s["win"][NSL - 1], name


@pytest.mark.parametrize("k", [1024, 1000])
def test_cuts_short_lists_and_ties(tc, k):
    pos = tc["pos"]
    for name in ("plain", "bm25"):
        per = [TC.split(h, pos, k)["per"] for h, _ in tc[name]]
        assert any(max(p) > k for p in per), name                   # a slice that really cuts
        assert any(all(1 <= x <= k - 1 for x in p) for p in per), name      # in_n < kk in every list of round 2
        for q in TC.WORD_QUERIES:                                   # the id decides the cut
            h = tc[name][q][0]
            assert h[k - 1][1] == h[k][1] and h[k - 1][0] < h[k][0], (name, q)
    for r in ("tfidf", "bm25"):
        per = [TC.split(h, pos, k)["per"] for h, _ in tc["clauses"][r]]
        assert any(max(p) > k for p in per) and any(all(1 <= x <= k - 1 for x in p) for p in per), r
        assert any(len(h) > k and h[k - 1][1] == h[k][1] for h, _ in tc["clauses"][r]), r
        assert tc["clauses"][r][3] == ([], 1)                       # the unsatisfiable one: its should word is found
    nbs = [row[4] for row in tc["rows"]]
    assert all(max(TC.split(nb, pos, k)["per"]) > k for nb in nbs[:NSL])
    assert any(nb[k - 1][2] == nb[k][2] for nb in nbs[:NSL])
    assert nbs[NSL] == [] and nbs[NSL + 1] == [] and tc["rows"][NSL + 1][1] is None


def test_the_word_of_every_document(tc):
    """b"all": every document but the empty ones is a hit.  The five empty documents leave its df at
    N - 5, so the score is (1 / tokens) * log(N / (N - 5)): four values, and the three-token documents,
    more than 4 * 1024 of them, tie for the best.  The ids alone order the top k."""
    hits, nfound = tc["plain"][TC.ALL_QUERY]
    assert nfound == 1 and len(hits) == TC.N - 5
    empty = set(tc["empty"])
    assert sorted(d for d, _ in hits) == [d for d in range(1, TC.N + 1) if d not in empty]
    assert len({s for _, s in hits}) == 4 and all(0.0 < s < 1e-4 for _, s in hits)
    best = [d for d, s in hits if s == hits[0][1]]
    assert len(best) > 4 * 1024 and best == sorted(d for d in range(1, TC.N + 1) if len(tc["docs"][d - 1].split()) == 3)
    assert [d for d, _ in hits[:1024]] == best[:1024]               # ids in ascending numeric order
    for ranking in ("bm25",):                                       # BM25 orders them the same way
        assert [d for d, _ in tc[ranking][TC.ALL_QUERY][0][:1024]] == best[:1024]
    for k in (1024, 1000):
        s = TC.split(hits, tc["pos"], k)
        assert min(s["win"]) >= 50 and s["win"][NSL - 1] < 96       # at k = 1000 they all stay in second-round slice 0
    full = [sl for sl in range(NSL - 1) if sl not in {tc["pos"][d] // TC.QT_SLICE for d in empty}]
    assert full == [1, 3] and all(s["per"][sl] == TC.QT_SLICE for sl in full)         # no pad in the sort
    assert s["per"] == [4094, 4096, 4095, 4096, 3614]
    # with a second word the same hits, the word's documents first
    both = tc["plain"][4][0]
    w05 = tc["plain"][1][0]
    assert len(both) == TC.N - 5 and {d for d, _ in both[:len(w05)]} == {d for d, _ in w05}
    assert tc["plain"][5] == ([], 0) and tc["plain"][6] == ([], 0)  # the absent word, the empty query
