"""tfidf_query_clauses on the GPU against tests/clause_ref.py: the OR ranking with one operation
per statement, filtered by the four conditions of include/tfidf.h ("clauses").  Everything is
compared exactly: ids, counts, and the u64 bit patterns of the scores."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_py
import prune_ref
import tfidf_abi
import tfidf_configs
import weight_ref
from clause_ref import ClauseRef, make_clause_queries, make_unsatisfiable_queries, texts
from conftest import GOLDEN, golden_cases
from helpers import docs_to_arrays, load_golden
from stride_corpus import kernels_h
from test_gpu_query import bits, check, make_queries

pytestmark = pytest.mark.gpu

KS = [1, 3, 10, 1024]
RANKINGS = ("tfidf", "bm25")
QT_SLICE, QS_BIG, QG_MAX, QTAB_WORDS = (kernels_h(n) for n in ("QT_SLICE", "QS_BIG", "QG_MAX", "QTAB_WORDS"))
T, X = tfidf_abi.CLAUSE_MAX_TERMS, tfidf_abi.CLAUSE_MAX_NOT


def Q(must=b"", should=b"", must_not=b"", m=0):
    return dict(must=must, should=should, must_not=must_not, m=m)


def run(e, qs, k, ranking="tfidf"):
    """the clause call of an Engine or a Group for a list of query dicts"""
    must, should, must_not, m = texts(qs)
    return e.query_clauses(must, should, must_not, k, m, True if ranking == "bm25" else None)


def same(a, b):
    for name in ("nhits", "nmatch", "nterms_found", "doc"):
        assert np.array_equal(a[name], b[name]), name
    assert np.array_equal(bits(a["score"]), bits(b["score"]))


def generated(ref, seed, n=200):
    rng = np.random.default_rng(seed)
    return make_clause_queries(ref, rng, n - n // 5) + make_unsatisfiable_queries(ref, rng, n // 5)


@pytest.fixture(scope="module")
def c2():
    p = tfidf_configs.plan("c2", scale=0.002)
    data, off = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
    ora = oracle_py.run(data, off, p["doc_ids"], p["ndocs_total"])
    ref = ClauseRef(ora, len(off) - 1, p["ndocs_total"])
    qs = generated(ref, 11)
    return dict(p=p, data=data, off=off, ora=ora, ref=ref, qs=qs, args=(data, off, p["doc_ids"], p["ndocs_total"]),
                refs={r: [ref.rank(q, r) for q in qs] for r in RANKINGS})


def test_c2_clauses_vs_reference(engine, c2):
    """200 queries (160 built around a seed document, 40 unsatisfiable), both rankings, every k.
    Of the 200 OR rankings here, from the reference alone: the must texts remove a document in
    146 queries, the must_not texts in 76, min_should in 36; 48 queries keep more than 10 hits;
    30 end with no hit although their OR ranking has some; fma(w, s, acc) would change a
    returned score of 12 queries."""
    ref, qs, refs = c2["ref"], c2["qs"], c2["refs"]
    ex = [ref.explain(q) for q in qs]
    for kind in "abc":                                              # each clause kind removes a hit somewhere
        assert any(e["fail"][kind] for e in ex), kind
    assert any(len(e["hits"]) > 10 for e in ex)
    assert any(not e["hits"] and e["n_or"] for e in ex)
    assert any(ref.fused_differs(q) for q in qs)                    # a contracted kernel cannot pass
    assert all(q["d0"] in dict(e["hits"]) for q, e in zip(qs, ex) if q["kind"] is None)
    assert all(q["d1"] not in dict(e["hits"]) for q, e in zip(qs, ex) if q["d1"] is not None)
    engine.run_host(*c2["args"])
    for r in RANKINGS:
        for k in KS:
            check(run(engine, qs, k, r), refs[r], k)
        info = engine.clause_info()
        assert info["nqueries"] == len(qs) and info["k"] == KS[-1] and info["ngroups"] == 4
        assert info["nq_unsatisfiable"] == sum(q["kind"] in ("absent_must", "must_and_not", "m_over_s") for q in qs) == 30
        assert info["avgdl"] == (ref.avgdl if r == "bm25" else 0.0)


def test_bm25_parameters(engine, c2):
    ref, qs = c2["ref"], c2["qs"][:60]
    engine.run_host(*c2["args"])
    must, should, must_not, m = texts(qs)
    for k1, b in ((0.0, 0.75), (2.0, 0.0), (1.5, 0.4)):
        res = engine.query_clauses(must, should, must_not, 10, m, dict(k1=k1, b=b))
        check(res, [ref.rank(q, "bm25", k1, b) for q in qs], 10)
    res = engine.query_clauses(must, should, must_not, 10, m, dict(avgdl=123.5))
    check(res, [ref.rank(q, "bm25", avgdl=123.5) for q in qs], 10)
    assert engine.clause_info()["avgdl"] == 123.5


@pytest.mark.parametrize("case", golden_cases())
def test_golden_clauses_vs_reference(engine, case):
    g = load_golden(case)
    ora = oracle_py.run(g["data"], g["off"])
    ref = ClauseRef(ora, len(g["off"]) - 1)
    qs = generated(ref, 5)
    engine.run_host(g["data"], g["off"])
    for r in RANKINGS:
        refs = [ref.rank(q, r) for q in qs]
        for k in KS:
            check(run(engine, qs, k, r), refs, k)


def test_should_text_alone_is_the_plain_query(engine, c2):
    """consequence 1, against engine.query and engine.query_bm25 themselves; and the plain calls'
    counters are not disturbed"""
    qs = make_queries(c2["ora"], np.random.default_rng(11), 200)
    engine.run_host(*c2["args"])
    for k in (3, 1024):
        plain, bm = engine.query(qs, k), engine.query_bm25(qs, k, 0.9, 0.6)
        qi, bi = engine.query_info(), engine.bm25_info()
        same(engine.query_clauses(should=qs, k=k), plain)
        same(engine.query_clauses(None, qs, None, k, [0] * len(qs), dict(k1=0.9, b=0.6)), bm)
        same(engine.query_clauses([b""] * len(qs), qs, [b""] * len(qs), k), plain)
        assert engine.query_info() == qi and engine.bm25_info() == bi
        assert engine.clause_info()["nq_unsatisfiable"] == 0


# ------------------------------------------------------------------ path switches ----

NSMALL = 4200


def bw(i):
    return b"b%x" % i


@pytest.fixture(scope="module")
def crafted():
    """4200 documents of one to three words that all hold the word c (every third one x3 too),
    and three documents of 4095, 4096 and 4097 distinct terms b0 ..: the last one is over QS_BIG"""
    docs = [b" ".join([b"c"] + ([b"x3"] if i % 3 == 0 else []) + ([b"s%d" % (i % 7)] if i % 2 else []))
            for i in range(NSMALL)]
    docs += [b" ".join(bw(i) for i in range(n)) for n in (T, T + 1, T + 2)]
    data, off = docs_to_arrays(docs)
    assert T + 1 == QS_BIG and len(docs) > QT_SLICE and len(data) < 100000
    ora = oracle_py.run(data, off)
    return dict(data=data, off=off, ref=ClauseRef(ora, len(docs)), A=NSMALL + 1, B=NSMALL + 2, C=NSMALL + 3)


def check_crafted(engine, crafted, qs, ks=(10,)):
    """both rankings against the reference; returns the reference rows and the counters of the last call"""
    for r in RANKINGS:
        refs = [crafted["ref"].rank(q, r) for q in qs]
        for k in ks:
            check(run(engine, qs, k, r), refs, k)
    return refs, engine.clause_info()


def test_first_round_predicate_across_slices(engine, crafted):
    """a must word in more than QT_SLICE documents, a must_not that removes every third one: the
    predicate in both slices of the first round, then a second round"""
    engine.run_host(crafted["data"], crafted["off"])
    qs = [Q(must=b"c", must_not=b"x3"), Q(must=b"c", should=b"s1 s2", must_not=b"x3", m=1), Q(must=b"c x3")]
    assert -(-(NSMALL + 3) // QT_SLICE) == 2
    refs, info = check_crafted(engine, crafted, qs, (1, 10, 1024))
    some = sum(1 for i in range(NSMALL) if i % 3 and i % 2 and i % 7 in (1, 2))
    assert [len(h) for h, _ in refs] == [NSMALL - NSMALL // 3, some, NSMALL // 3] and some > 10
    assert info["ngroups"] == 1 and info["ngroups_tab_lds"] == 1 and info["nq_unsatisfiable"] == 0


def test_big_document_required_and_excluded(engine, crafted):
    """the 4097-term document (k_doc_score_big) required, and the same document excluded"""
    engine.run_host(crafted["data"], crafted["off"])
    A, B, C = crafted["A"], crafted["B"], crafted["C"]
    qs = [Q(must=bw(T + 1), should=bw(0)), Q(should=bw(0) + b" " + bw(5), must_not=bw(T + 1)),
          Q(must=bw(T), should=bw(1) + b" c"), Q(must=bw(3), must_not=bw(T))]
    refs, _ = check_crafted(engine, crafted, qs)
    assert [sorted(d for d, _ in h) for h, _ in refs] == [[C], [A, B], [B, C], [A]]


def test_count_fields_at_their_maximum(engine, crafted):
    """4095 should terms at m = 4095 (the low field full, no carry into the must field), the same
    with one term absent; 4095 must terms; 255 must_not terms, all absent, one present, all
    present (the high field full)"""
    engine.run_host(crafted["data"], crafted["off"])
    A, B, C = crafted["A"], crafted["B"], crafted["C"]
    all_s = b" ".join(bw(i) for i in range(T))
    one_absent = b" ".join([bw(i) for i in range(T - 1)] + [b"zz"])
    absent_x = b" ".join(b"zz%d" % i for i in range(X))
    qs = [Q(should=all_s, m=T), Q(should=one_absent, m=T), Q(should=one_absent, m=T - 1),
          Q(must=all_s), Q(must=one_absent), Q(must=all_s, should=all_s, m=T),
          Q(must=bw(T - 1), should=all_s, m=T),
          Q(should=b"c", must_not=absent_x), Q(should=b"c", must_not=b" ".join([b"zz%d" % i for i in range(X - 1)] + [b"x3"])),
          Q(should=bw(0) + b" c", must_not=b" ".join(bw(i) for i in range(X)))]
    refs, info = check_crafted(engine, crafted, qs, (10, 1024))
    n = [len(h) for h, _ in refs]
    assert n == [3, 0, 3, 3, 0, 3, 3, NSMALL, NSMALL - NSMALL // 3, NSMALL]
    assert sorted(d for d, _ in refs[0][0]) == [A, B, C]
    assert info["nq_unsatisfiable"] == 1 and info["ngroups_tab_lds"] == 0     # the absent must word; the table is too wide


def test_groups_and_the_table_in_lds(engine, crafted, monkeypatch):
    """a 64-query group whose table fits QTAB_WORDS and one whose table does not; 65 queries are
    two groups; under TFIDF_QUERY_ACC_MB=1 a fresh engine makes more groups of fewer queries"""
    engine.run_host(crafted["data"], crafted["off"])
    small = [Q(must=b"c", should=b"s%d s%d" % (q % 7, (q + 3) % 7), must_not=b"x3" if q % 2 else b"", m=q % 3)
             for q in range(QG_MAX)]
    _, info = check_crafted(engine, crafted, small)
    assert (info["ngroups"], info["ngroups_tab_lds"], info["group_queries"]) == (1, 1, QG_MAX)
    wide = small[:-1] + [Q(should=b" ".join(bw(i) for i in range(QTAB_WORDS // 4 + 1)), m=2)]
    _, info = check_crafted(engine, crafted, wide)
    assert (info["ngroups"], info["ngroups_tab_lds"]) == (1, 0)
    more = small + [Q(must=bw(T + 1))]
    _, info = check_crafted(engine, crafted, more)
    assert (info["ngroups"], info["ngroups_tab_lds"]) == (2, 2)
    want = {r: run(engine, more, 10, r) for r in RANKINGS}
    monkeypatch.setenv("TFIDF_QUERY_ACC_MB", "1")
    with tfidf_abi.Engine(0) as e:
        e.run_host(crafted["data"], crafted["off"])
        for r in RANKINGS:
            same(run(e, more, 10, r), want[r])
            info = e.clause_info()
            assert info["group_queries"] < QG_MAX and info["ngroups"] == -(-len(more) // info["group_queries"]) >= 3


def test_vocabulary_wider_than_the_lds_filter(engine):
    """2^18 + 16 terms: ranks 7 and 7 + 2^18 share a bit of the kernels' LDS filter.  A must term
    absent from a document that holds the alias gives no hit there; the alias as a must_not does
    not exclude it.  In a short document and in one over QS_BIG."""
    V = (1 << 18) + 16
    docs = [b" ".join(b"w%06d" % i for i in range(d, V, 30)) for d in range(30)]
    docs.append(b"w000007 w000100")
    data, off = docs_to_arrays(docs)
    ora = oracle_py.run(data, off)
    by_name = sorted(ora["terms"])
    hi = b"w%06d" % (7 + (1 << 18))
    assert len(by_name) == V and by_name[7] == b"w000007" and by_name[7 + (1 << 18)] == hi
    ref = ClauseRef(ora, len(docs))
    qs = [Q(must=hi, should=b"w000100 w000007"), Q(should=b"w000100 w000007", must_not=hi),
          Q(must=b"w000007", should=hi), Q(must=b"w000007", must_not=hi), Q(must=hi, must_not=b"w000007")]
    refs = [ref.rank(q) for q in qs]
    long7, longhi = 8, (7 + (1 << 18)) % 30 + 1                     # the striding documents that hold the two words
    assert [sorted(d for d, _ in h) for h, _ in refs] == [[longhi], sorted({31, long7, 100 % 30 + 1}), [long7, 31],
                                                           [long7, 31], [longhi]]
    engine.run_host(data, off)
    for r in RANKINGS:
        check(run(engine, qs, 8, r), refs if r == "tfidf" else [ref.rank(q, r) for q in qs], 8)


# ------------------------------------------------------------------ other cases ----

@pytest.mark.parametrize("K", [2, 3])
def test_group_clauses_equal_the_single_shard_reference(c2, K):
    shards = []
    for r in range(K):
        p = tfidf_configs.plan("c2", scale=0.002, rank=r, nranks=K)
        d, o = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
        shards.append((d, o, p["doc_ids"], p["ndocs_total"]))
    # a must word that one shard's vocabulary lacks: a word of a single document
    ref, ora = c2["ref"], c2["ora"]
    rare = next(t for t in ora["terms"] if len(ref.docs_of(t)) == 1)
    qs = c2["qs"] + [Q(must=rare), Q(must=rare, should=ora["terms"][0]), Q(should=ora["terms"][0], must_not=rare)]
    refs = {r: c2["refs"][r] + [ref.rank(q, r) for q in qs[-3:]] for r in RANKINGS}
    assert len(refs["tfidf"][-3][0]) == 1
    with tfidf_abi.Group(K, devices=[0] * K, local=True) as g:
        g.run_host(shards)
        for r in RANKINGS:
            for k in (3, 1024):
                check(run(g, qs, k, r), refs[r], k)
        dropped = [rank.clause_info()["nq_unsatisfiable"] for rank in g.ranks]
        assert min(dropped) >= 30 and max(dropped) >= 32            # the rare must word: dropped where it is unknown
        # a rank alone ranks its own shard only
        own = set(shards[1][2].tolist())
        res = run(g.ranks[1], qs[:40], 10)
        for q, (hits, _) in enumerate(refs["tfidf"][:40]):
            mine = [(d, s) for d, s in hits if d in own]
            n = min(10, len(mine))
            assert int(res["nmatch"][q]) == len(mine)
            assert res["doc"][q, :n].tolist() == [d for d, _ in mine[:n]]
            assert np.array_equal(bits(res["score"][q, :n]), bits([s for _, s in mine[:n]]))


def test_clauses_follow_prune_and_reweight(engine, c2):
    ora, qs, n = c2["ora"], c2["qs"][:80], len(c2["off"]) - 1
    N = c2["p"]["ndocs_total"]
    engine.run_host(*c2["args"])
    engine.reweight("log", "smooth", "l2")
    ref = ClauseRef(weight_ref.reweight(ora, "log", "smooth", "l2", N=N), n, N)
    check(run(engine, qs, 10), [ref.rank(q) for q in qs], 10)
    check(run(engine, qs, 10, "bm25"), c2["refs"]["bm25"][:80], 10)           # BM25 reads no score
    engine.run_host(*c2["args"])
    engine.prune(2)
    want = prune_ref.prune(ora, 2)
    pruned_words = set(ora["terms"]) - set(want["terms"])
    assert any(t in pruned_words for q in qs for t in q["must"].split())      # a pruned must word: no hit any more
    ref = ClauseRef(want, n, N)
    ref.L, ref.avgdl = c2["ref"].L, c2["ref"].avgdl                           # docSize is unchanged, so L and avgdl are
    for r in RANKINGS:
        for k in (1, 1024):
            check(run(engine, qs, k, r), [ref.rank(q, r) for q in qs], k)


def test_clauses_leave_the_result_and_allocate_once(engine, c2):
    engine.run_host(*c2["args"])
    before = engine.text()
    first = {r: run(engine, c2["qs"], 10, r) for r in RANKINGS}
    a0 = engine.alloc_counters()
    for r in RANKINGS:
        same(run(engine, c2["qs"], 10, r), first[r])
    assert engine.alloc_counters() == a0                          # no device allocation
    assert engine.text() == before
    res = engine.fetch()
    check(run(engine, c2["qs"][:20], 3), c2["refs"]["tfidf"][:20], 3)
    assert res["output_txt"] == before and engine.text() == before


def test_clause_errors_and_lifecycle(c2):
    live = tfidf_abi.alloc_live()
    with tfidf_abi.Engine(0) as e:
        with pytest.raises(tfidf_abi.TfidfError) as ex:
            e.query_clauses(should=[b"x"], k=3)
        assert ex.value.rc == tfidf_abi.E_STATE                    # before a run
        e.run_host(*c2["args"])
        for kw in (dict(k=0), dict(k=1025), dict(min_should=[T + 1]), dict(bm25=dict(b=2.0)),
                   dict(must=[b"a", b"b"])):
            with pytest.raises(tfidf_abi.TfidfError) as ex:
                e.query_clauses(**{**dict(should=[b"x"], k=3), **kw})
            assert ex.value.rc == tfidf_abi.E_INVAL, kw
        res = e.query_clauses(should=[], k=4)                      # an empty batch is valid
        assert res["doc"].shape == (0, 4)
        check(run(e, c2["qs"][:5], 1024), c2["refs"]["tfidf"][:5], 1024)
        model = e.model_export()
    with tfidf_abi.Engine(0) as e:                                 # a model-only context has no pairs to rank
        e.model_import(model)
        with pytest.raises(tfidf_abi.TfidfError) as ex:
            e.query_clauses(should=[b"x"], k=3)
        assert ex.value.rc == tfidf_abi.E_STATE
    assert tfidf_abi.alloc_live() == live                          # the same before open and after close


# ------------------------------------------------------------------ the CLI ----

def split_ops(line: bytes, ops=True, all_must=False):
    """host/query_ops.h in Python: the three texts of a line"""
    out = ([], [], [])
    for t in line.split():
        if ops and len(t) >= 2 and t[:1] in (b"+", b"-"):
            out[0 if t[:1] == b"+" else 2].append(t[1:])
        else:
            out[0 if all_must else 1].append(t)
    return [b" ".join(x) for x in out]


CLI_DOCS = [b"The quick brown Fox, jumps over new york", b"a lazy dog in New York sleeps", b"new cars in old york, quick!",
            b"the fox and the dog", b"york new quick brown", b"Fox fox FOX dog."]
CLI_LINES = [b"+quick brown -dog", b"+Fox, the", b"+new +york quick", b"quick dog fox", b"-york the fox", b"+ - +brown",
             b"", b"+absent quick", b"new york -cars", b"the dog", b"new york"]


@pytest.mark.parametrize("flags", [["--query-ops"], ["--query-ops", "--lower", "--strip-punct"], ["--query-ops", "--ngrams", "2"],
                                   ["--query-all"], ["--query-ops", "--query-all"], ["--min-match", "2"],
                                   ["--query-ops", "--min-match", "2", "--bm25"], ["--query-ops", "--bm25"],
                                   ["--query-ops", "--shards", "2"]])
def test_cli_clauses(tmp_path, flags):
    """hits.txt byte for byte: the lines are split as host/query_ops.h splits them, the three texts
    and the documents go through the host analyzer and n-grams of the binding, and the reference
    ranks the result"""
    (tmp_path / "input").mkdir()
    for i, d in enumerate(CLI_DOCS):
        (tmp_path / "input" / ("doc%d" % (i + 1))).write_bytes(d)
    (tmp_path / "q.txt").write_bytes(b"\n".join(CLI_LINES))        # the last line has no newline
    an = dict(lower="--lower" in flags, punct="--strip-punct" in flags)
    ngrams = 2 if "--ngrams" in flags else 0

    def prepare(text_list):
        data, off = docs_to_arrays(text_list)
        if any(an.values()):
            data = tfidf_abi.analyze_host(data, off, **an)
        if ngrams:
            data, off = tfidf_abi.ngrams_host(data, off, 1, ngrams)
        return [bytes(data[int(off[i]):int(off[i + 1])]) for i in range(len(text_list))]

    docs = prepare(CLI_DOCS)
    data, off = docs_to_arrays(docs)
    ref = ClauseRef(oracle_py.run(data, off), len(docs))
    parts = [split_ops(l, "--query-ops" in flags, "--query-all" in flags) for l in CLI_LINES]
    must, should, must_not = (prepare([p[c] for p in parts]) for c in range(3))
    m = 2 if "--min-match" in flags else 0
    qs = [Q(a, b, c, m) for a, b, c in zip(must, should, must_not)]
    ranking = "bm25" if "--bm25" in flags else "tfidf"
    want = b"".join(b"q%d\tdoc%d\t%.16f\n" % (i + 1, d, s) for i, q in enumerate(qs) for d, s in ref.rank(q, ranking)[0][:3])
    assert want
    p = subprocess.run([tfidf_abi.CLI_PATH, "--query", "q.txt", "--top", "3"] + flags, cwd=tmp_path, capture_output=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "hits.txt").read_bytes() == want
    if flags == ["--query-ops", "--lower", "--strip-punct"]:
        assert b"fox" in must[1] and b"+" not in must[1] + should[1]           # "+Fox," requires fox
        assert b"q2\tdoc1\t" in want and b"q2\tdoc2\t" not in want
    if ngrams:
        assert b"new_york" in must[2].split()                                   # a phrase: doc5 holds both words, not the phrase
        assert b"q3\tdoc1\t" in want and b"q3\tdoc5\t" not in want


def test_cli_without_the_options_writes_the_old_bytes(tmp_path):
    """lines full of operators, without --query-ops: the plain call, every byte a word's"""
    case = "g5_w3"
    g = load_golden(case)
    ora = oracle_py.run(g["data"], g["off"])
    ref = ClauseRef(ora, len(g["off"]) - 1)
    words = ora["terms"]
    qs = [b"+" + words[3] + b" -" + words[5] + b" " + words[8], words[1] + b" + - " + words[2]]
    shutil.copytree(os.path.join(GOLDEN, case, "input"), tmp_path / "input")
    (tmp_path / "q.txt").write_bytes(b"\n".join(qs))
    p = subprocess.run([tfidf_abi.CLI_PATH, "--query", "q.txt", "--top", "3"], cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    want = b"".join(b"q%d\tdoc%d\t%.16f\n" % (i + 1, d, s) for i, q in enumerate(qs) for d, s in ref.rank(Q(should=q))[0][:3])
    assert want and (tmp_path / "hits.txt").read_bytes() == want
    assert (tmp_path / "output.txt").read_bytes() == g["output"]
