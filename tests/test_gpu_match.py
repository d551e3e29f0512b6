"""Fuzzy and prefix term matching on the device (tfidf_match_terms / tfidf_group_match_terms /
the `tfidf` options built on them) against tests/match_ref.py: the crafted dictionaries of
tests/match_corpus.py, config 2 with patterns drawn from its vocabulary, every golden case; after a
prune, on an imported model, over groups of shards; the list capacity's batches and growth.
Everything is compared exactly: ranks, distances, df, counts and word bytes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import match_corpus as MC
import match_ref as R
import tfidf_abi
import tfidf_configs
from conftest import GOLDEN, golden_cases
from helpers import docs_to_arrays, load_golden

pytestmark = pytest.mark.gpu

NO_TERM = 0xFFFFFFFF


def same_rows(a, b, term=True, nmatch=True):
    for name in ("nterms", "dist", "df") + (("term",) if term else ()) + (("nmatch",) if nmatch else ()):
        assert np.array_equal(a[name], b[name]), name
    assert a["words"] == b["words"] and a["k"] == b["k"]


@pytest.fixture(scope="module")
def abc5():
    docs = MC.abc5()
    terms, df, _ = MC.dictionary(docs)
    return dict(docs=docs, arrays=docs_to_arrays(docs), terms=terms, df=df)


@pytest.fixture(scope="module")
def edges():
    docs = MC.edges()
    terms, df, _ = MC.dictionary(docs)
    return dict(docs=docs, arrays=docs_to_arrays(docs), terms=terms, df=df)


@pytest.fixture(scope="module")
def c2():
    """config 2 at scale 0.002 and 200 patterns drawn from its vocabulary with 0, 1 and 2 edits; the
    reference's rows, once"""
    p = tfidf_configs.plan("c2", scale=0.002)
    data, off = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
    terms, df, _ = MC.dictionary(MC.docs_of(data, off))
    pats = MC.drawn_patterns(terms, 200, seed=11)
    edits = [2 if len(w) > 5 else 1 if len(w) > 2 else 0 for w in pats]          # the `auto` budgets
    bags = R.Bags(terms)
    rows = R.expand(terms, df, pats, R.FUZZY, edits, 50, True, 0, bags)
    rows2 = R.expand(terms, df, pats, R.FUZZY, 2, 50, True, 0, bags)            # and with d = 2 throughout
    return dict(p=p, args=(data, off, p["doc_ids"], p["ndocs_total"]), terms=terms, df=df, pats=pats, edits=edits,
                bags=bags, rows=rows, rows2=rows2)


def test_abc5_vs_reference(engine, abc5):
    engine.run_host(*abc5["arrays"])
    pats = MC.abc_strings()
    for transpose in (True, False):
        for d in (0, 1, 2):
            full = R.expand(abc5["terms"], abc5["df"], pats, R.FUZZY, d, 1 << 30, transpose)
            for E in (50,) if d < 2 else (1, 3, 50, 1024):
                got = engine.match_terms(pats, max_edits=d, max_expansions=E, transpose=transpose)
                R.check(got, [(n, rows[:E]) for n, rows in full], E)
    info = engine.match_info()
    assert info["npatterns"] == 363 and info["k"] == 1024 and info["ngroups"] == 6 and info["nbatches"] == 6
    assert info["list_records"] == tfidf_abi.MATCH_DEFAULT_RECORDS
    # prefixes, and a fixed prefix on the fuzzy patterns
    pre = MC.abc_strings(1, 4)
    R.check(engine.match_terms(pre, kinds=tfidf_abi.MATCH_PREFIX, max_expansions=50),
            R.expand(abc5["terms"], abc5["df"], pre, R.PREFIX, 0, 50), 50)
    for fp in (1, 2, 64):
        R.check(engine.match_terms(pre, max_expansions=50, fixed_prefix=fp),
                R.expand(abc5["terms"], abc5["df"], pre, R.FUZZY, 2, 50, True, fp), 50)


def test_edges_vs_reference(engine, edges):
    engine.run_host(*edges["arrays"])
    pk = MC.edge_patterns()
    pats, kinds = [p for p, _ in pk], [k for _, k in pk]
    for transpose in (True, False):
        for d, E, fp in ((0, 50, 0), (1, 3, 0), (2, 1024, 0), (2, 50, 15)):
            rows = R.expand(edges["terms"], edges["df"], pats, kinds, d, E, transpose, fp)
            got = engine.match_terms(pats, kinds=kinds, max_edits=d, max_expansions=E, transpose=transpose, fixed_prefix=fp)
            R.check(got, rows, E)
    edits = [i % 3 for i in range(len(pats))]                        # every budget inside one group
    R.check(engine.match_terms(pats, kinds=kinds, max_edits=edits, max_expansions=7),
            R.expand(edges["terms"], edges["df"], pats, kinds, edits, 7), 7)
    # the device and its plain-C twin
    same_rows(engine.match_terms(pats, kinds=kinds, max_expansions=50),
              tfidf_abi.model_match_terms(MC.model(edges["docs"]), pats, kinds=kinds, max_expansions=50))


def test_c2_vs_reference(engine, c2):
    assert sum(n > 50 for n, _ in c2["rows2"]) > 5 and sum(n == 0 for n, _ in c2["rows"]) > 0
    engine.run_host(*c2["args"])
    for edits, rows in ((c2["edits"], c2["rows"]), (2, c2["rows2"])):
        got = engine.match_terms(c2["pats"], max_edits=edits, max_expansions=50)
        R.check(got, rows, 50)
        info = engine.match_info()
        assert info["ngroups"] == 4 and info["nbatches"] == 4 and info["nrecords"] == sum(n for n, _ in rows)


@pytest.mark.parametrize("case", golden_cases())
def test_golden_vs_reference(engine, case):
    g = load_golden(case)
    terms, df, _ = MC.dictionary(MC.docs_of(g["data"], g["off"]))
    engine.run_host(g["data"], g["off"])
    pats = MC.drawn_patterns(terms, 40, seed=3)
    bags = R.Bags(terms)
    R.check(engine.match_terms(pats, max_expansions=10), R.expand(terms, df, pats, R.FUZZY, 2, 10, True, 0, bags), 10)
    pre = sorted({t[:1] for t in terms if t})[:20]
    R.check(engine.match_terms(pre, kinds=1, max_expansions=10), R.expand(terms, df, pre, R.PREFIX, 0, 10), 10)


def test_list_capacity_batches_and_growth(engine, c2):
    """list_records = 1024: a group whose matches sum to more is cut into batches, one pattern with
    more matches than that makes the list grow; 65 patterns are two groups; duplicates; a group of
    nothing but patterns without a match.  Every result equals the one at the default capacity."""
    engine.run_host(*c2["args"])
    terms, df, bags = c2["terms"], c2["df"], c2["bags"]
    big = [p for p, (n, _) in zip(c2["pats"], c2["rows2"]) if n > 50][:6]
    pats = (big + [b"a", big[0], b"a"] + c2["pats"][:55])[:64] + [b"qqqqqqqqqqqq%d" % i for i in range(64)] + [b"zz"]
    kinds = [1 if p in (b"a", b"zz") else 0 for p in pats]
    assert len(pats) == 129
    rows = R.expand(terms, df, pats, kinds, 2, 50, True, 0, bags)
    assert rows[6][0] > 1024 and sum(n for n, _ in rows[:64]) > 2 * 1024 and all(n == 0 for n, _ in rows[64:128])
    want = engine.match_terms(pats, kinds=kinds, max_expansions=50)
    R.check(want, rows, 50)
    assert engine.match_info()["ngroups"] == 3 and engine.match_info()["nbatches"] == 3
    got = engine.match_terms(pats, kinds=kinds, max_expansions=50, list_records=1024)
    same_rows(got, want)
    info = engine.match_info()
    assert info["ngroups"] > 4 and info["nbatches"] > 3 and info["list_records"] == rows[6][0]
    # the same call again: the same rows, the same counters
    same_rows(engine.match_terms(pats, kinds=kinds, max_expansions=50, list_records=1024), want)
    again = engine.match_info()
    assert {k: v for k, v in again.items() if not k.startswith("ms_")} == {k: v for k, v in info.items() if not k.startswith("ms_")}
    # E = 1024 with a prefix that has more matches than E
    R.check(engine.match_terms([b"a", b"b"], kinds=1, max_expansions=1024, list_records=1024),
            R.expand(terms, df, [b"a", b"b"], R.PREFIX, 0, 1024), 1024)


def test_after_prune(engine, c2):
    engine.run_host(*c2["args"])
    engine.prune(min_df=2)
    keep = [i for i, d in enumerate(c2["df"].tolist()) if d >= 2]
    terms, df = [c2["terms"][i] for i in keep], c2["df"][keep]
    assert 0 < len(terms) < len(c2["terms"])
    rows = R.expand(terms, df, c2["pats"][:64], R.FUZZY, 2, 50, True, 0, R.Bags(terms))
    R.check(engine.match_terms(c2["pats"][:64], max_expansions=50), rows, 50)


def test_imported_model_gives_the_fitted_rows(engine, edges, c2):
    pk = MC.edge_patterns()
    cases = [(edges["arrays"], [p for p, _ in pk], [k for _, k in pk]), (c2["args"], c2["pats"][:64] + [b"ab", b"zz"], [0] * 64 + [1, 1])]
    for args, pats, kinds in cases:
        engine.run_host(*args)
        fitted = engine.match_terms(pats, kinds=kinds, max_expansions=50)
        model = engine.model_export()
        with tfidf_abi.Engine(0) as e:
            e.model_import(model)
            same_rows(e.match_terms(pats, kinds=kinds, max_expansions=50), fitted)
            same_rows(e.match_terms(pats, kinds=kinds, max_expansions=50, list_records=1024), fitted)
        same_rows(tfidf_abi.model_match_terms(model, pats, kinds=kinds, max_expansions=50), fitted)


@pytest.mark.parametrize("K", [2, 3])
def test_group_equals_single_shard(engine, c2, K):
    shards = []
    for r in range(K):
        p = tfidf_configs.plan("c2", scale=0.002, rank=r, nranks=K)
        d, o = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
        shards.append((d, o, p["doc_ids"], p["ndocs_total"]))
    pats = c2["pats"] + [b"a", b"zz", b"qq"]
    kinds = [0] * 200 + [1, 1, 1]
    edits = c2["edits"] + [0, 0, 0]
    rows = c2["rows"] + R.expand(c2["terms"], c2["df"], pats[200:], R.PREFIX, 0, 50)
    with tfidf_abi.Group(K, devices=[0] * K, local=True) as g:
        g.run_host(shards)
        got = g.match_terms(pats, kinds=kinds, max_edits=edits, max_expansions=50)
        R.check(got, rows, 50, term=False, nmatch=False)
        for i, (n, want) in enumerate(rows):
            assert got["term"][i, :len(want)].tolist() == [NO_TERM] * len(want)
            assert int(got["nmatch"][i]) <= n                              # a lower bound of the corpus-wide count
        # ... namely the largest shard's count, from the shards' own dictionaries
        tables = [MC.dictionary(MC.docs_of(d, o))[0] for d, o, _, _ in shards]
        bags = [R.Bags(t) for t in tables]
        for i in list(range(30)) + [200, 201, 202]:
            counts = [len(R.matches(t, [0] * len(t), pats[i], kinds[i], edits[i], True, 0, b)) for t, b in zip(tables, bags)]
            assert int(got["nmatch"][i]) == max(counts), (i, counts)
        # a rank alone answers from its own table with the global df
        own = g.ranks[1].match_terms(pats[:20], max_edits=edits[:20], max_expansions=50)
        gdf = dict(zip(c2["terms"], c2["df"].tolist()))
        for words, dfs in zip(own["words"], own["df"]):
            assert [gdf[w] for w in words] == dfs[:len(words)].tolist()
    with tfidf_abi.Group(1, devices=[0]) as g:                             # one shard: nmatch is exact
        g.run_host([c2["args"]])
        R.check(g.match_terms(pats, kinds=kinds, max_edits=edits, max_expansions=50), rows, 50, term=False)


def test_leaves_the_result_and_allocates_once(engine, c2):
    live = tfidf_abi.alloc_live()
    with tfidf_abi.Engine(0) as e:
        e.run_host(*c2["args"])
        before = e.text()
        first = e.match_terms(c2["pats"], max_edits=c2["edits"], max_expansions=50)
        a0 = e.alloc_counters()
        second = e.match_terms(c2["pats"], max_edits=c2["edits"], max_expansions=50)
        assert e.alloc_counters() == a0                                    # no device allocation
        same_rows(first, second)
        R.check(second, c2["rows"], 50)
        assert e.text() == before and e.fetch()["output_txt"] == before
        assert tfidf_abi.alloc_live()[0] > live[0]
    assert tfidf_abi.alloc_live() == live                                  # the same before open and after close


def test_errors_and_states(c2):
    with tfidf_abi.Engine(0) as e:
        with pytest.raises(tfidf_abi.TfidfError) as ex:
            e.match_terms([b"ab"])
        assert ex.value.rc == tfidf_abi.E_STATE                            # neither a result nor a model
        e.run_host(*c2["args"])
        for kw in (dict(max_edits=3), dict(max_expansions=0), dict(max_expansions=1025), dict(fixed_prefix=65),
                   dict(list_records=1023), dict(flags=2), dict(size=24)):
            with pytest.raises(tfidf_abi.TfidfError) as ex:
                e.match_terms([b"ab"], **kw)
            assert ex.value.rc == tfidf_abi.E_INVAL, kw
        for bad in ([b""], [b"x" * 65]):
            with pytest.raises(tfidf_abi.TfidfError) as ex:
                e.match_terms(bad)
            assert ex.value.rc == tfidf_abi.E_INVAL
        got = e.match_terms([])                                            # no patterns is valid
        assert got["nmatch"].shape == (0,) and got["words"] == [] and e.match_info()["ngroups"] == 0
        R.check(e.match_terms(c2["pats"][:3], max_edits=c2["edits"][:3], max_expansions=50), c2["rows"][:3], 50)
        # an empty corpus has an empty dictionary
        e.run_host(*docs_to_arrays([b"", b""]))
        got = e.match_terms([b"ab", b"a"], kinds=[0, 1])
        assert got["nmatch"].tolist() == [0, 0] and got["words"] == [[], []]


# ---- the command-line tool ----

def auto_budget(n):
    return 0 if n <= 2 else 1 if n <= 5 else 2


def cli_expand(terms, df, lines, E=50, fuzzy="auto", prefix_ops=False):
    """what `tfidf --fuzzy` makes of query lines, from the reference: per line the (token shown,
    matches) of its patterns in the tool's order (the plain tokens, then the prefix tokens) and the
    rewritten line"""
    bags = R.Bags(terms)
    out = []
    for line in lines:
        toks = line.split()
        pre = [t[:-1] for t in toks if prefix_ops and len(t) >= 2 and t.endswith(b"*")]
        plain = [t for t in toks if not (prefix_ops and len(t) >= 2 and t.endswith(b"*"))]
        shown, words = [], []
        for kind, group in ((R.FUZZY, plain), (R.PREFIX, pre)):
            for t in group:
                term = t.split(b"\0")[0]
                if not 1 <= len(term) <= 64 or (kind == R.FUZZY and fuzzy is None):
                    words.append(t)                                    # it stays as it is
                    continue
                d = auto_budget(len(term)) if fuzzy == "auto" else (fuzzy or 0)
                m = R.matches(terms, df, term, kind, d, True, 0, bags)[:E]
                words += [terms[r] for r, _, _ in m]
                label = term + (b"*" if kind == R.PREFIX else b"")
                if label not in [s for s, _ in shown]:
                    shown.append((label, [(terms[r], dd, f) for r, dd, f in m]))
        out.append((shown, b" ".join(words)))
    return out


def suggest_bytes(expanded):
    return b"".join(b"q%d\t%s\t%s\t%d\t%d\n" % (i + 1, tok, w, d, f)
                    for i, (shown, _) in enumerate(expanded) for tok, ms in shown for w, d, f in ms)


def hits_bytes(res):
    return b"".join(b"q%d\tdoc%d\t%.16f\n" % (q + 1, res["doc"][q, i], res["score"][q, i])
                    for q in range(len(res["nhits"])) for i in range(int(res["nhits"][q])))


@pytest.fixture(scope="module")
def cli_case():
    case = "g5_w3"
    g = load_golden(case)
    terms, df, _ = MC.dictionary(MC.docs_of(g["data"], g["off"]))
    pats = MC.drawn_patterns(terms, 36, seed=5)
    lines = [b" ".join(pats[3 * i:3 * i + 3]) for i in range(12)]
    lines += [b"", pats[0] + b" " + pats[0] + b" " + b"k" * 65 + b" " + pats[1], b"zzzzzzzzzz", terms[5] + b"\0tail " + terms[6]]
    return dict(case=case, g=g, terms=terms, df=df, lines=lines, expanded=cli_expand(terms, df, lines))


def run_cli(cwd, *args):
    return subprocess.run([tfidf_abi.CLI_PATH] + list(args), cwd=cwd, capture_output=True, timeout=120)


@pytest.mark.parametrize("bm25", [False, True])
@pytest.mark.parametrize("shards", ["1", "3"])
def test_cli_fuzzy_query(engine, cli_case, tmp_path, bm25, shards):
    c = cli_case
    shutil.copytree(os.path.join(GOLDEN, c["case"], "input"), tmp_path / "input")
    (tmp_path / "q.txt").write_bytes(b"\n".join(c["lines"]) + b"\n")
    p = run_cli(tmp_path, "--query", "q.txt", "--fuzzy", "auto", "--shards", shards, *(["--bm25"] if bm25 else []))
    assert p.returncode == 0, p.stderr
    rewritten = [line for _, line in c["expanded"]]
    assert sum(len(r.split()) > len(l.split()) for r, l in zip(rewritten, c["lines"])) >= 3     # tokens did expand
    engine.run_host(c["g"]["data"], c["g"]["off"])
    want = engine.query_bm25(rewritten, 10) if bm25 else engine.query(rewritten, 10)
    assert want["nhits"].sum() > 20
    assert (tmp_path / "hits.txt").read_bytes() == hits_bytes(want)
    assert (tmp_path / "output.txt").read_bytes() == c["g"]["output"]


def test_cli_suggest_and_model(cli_case, tmp_path):
    c = cli_case
    shutil.copytree(os.path.join(GOLDEN, c["case"], "input"), tmp_path / "input")
    (tmp_path / "q.txt").write_bytes(b"\n".join(c["lines"]))              # the last line without its newline
    want = suggest_bytes(c["expanded"])
    assert want.count(b"\n") > 40
    p = run_cli(tmp_path, "--suggest", "q.txt", "--fuzzy", "auto", "--save-model", "m.bin")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "suggest.txt").read_bytes() == want
    p = run_cli(tmp_path, "--suggest", "q.txt", "--fuzzy", "auto", "--shards", "2", "--suggest-file", "s2.txt")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "s2.txt").read_bytes() == want
    # a smaller E and a fixed budget
    small = cli_expand(c["terms"], c["df"], c["lines"], E=2, fuzzy=1)
    p = run_cli(tmp_path, "--suggest", "q.txt", "--fuzzy", "1", "--max-expansions", "2", "--suggest-file", "s3.txt")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "s3.txt").read_bytes() == suggest_bytes(small)
    # the model alone: no input/, no output.txt
    served = tmp_path / "served"
    served.mkdir()
    shutil.copy(tmp_path / "m.bin", served / "m.bin")
    shutil.copy(tmp_path / "q.txt", served / "q.txt")
    p = run_cli(served, "--model", "m.bin", "--suggest", "q.txt", "--fuzzy", "auto")
    assert p.returncode == 0, p.stderr
    assert (served / "suggest.txt").read_bytes() == want
    assert sorted(os.listdir(served)) == ["m.bin", "q.txt", "suggest.txt"]
    assert run_cli(served, "--model", "m.bin").returncode == 2             # as before: it needs something to do


def test_cli_prefix_ops_behind_the_analyzer(engine, tmp_path):
    docs = [b"Connect the CONNECTION, now.", b"connected; Conn? connector connect", b"nothing here to see", b"a connect-ion (conn)"]
    (tmp_path / "input").mkdir()
    for i, d in enumerate(docs):
        (tmp_path / "input" / ("doc%d" % (i + 1))).write_bytes(d)
    lines = [b"Conn*", b"Conn*, Nothing", b"see* CONNECT"]
    (tmp_path / "q.txt").write_bytes(b"\n".join(lines) + b"\n")
    data, off = docs_to_arrays(docs)
    analyzed = tfidf_abi.analyze_host(data, off, lower=True, punct=True)
    terms, df, _ = MC.dictionary(MC.docs_of(analyzed, off))
    assert b"connection" in terms and b"conn" in terms
    # the operator is read before the analyzer, the pattern is what the analyzer makes of the rest
    behind = [b"conn*", b"conn   nothing", b"see* connect"]
    exp = cli_expand(terms, df, behind, fuzzy=None, prefix_ops=True)
    assert exp[0][0][0][0] == b"conn*" and len(exp[0][0][0][1]) >= 5 and exp[1][0] == []
    p = run_cli(tmp_path, "--lower", "--strip-punct", "--prefix-ops", "--query", "q.txt", "--suggest", "q.txt")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "suggest.txt").read_bytes() == suggest_bytes(exp)
    engine.run_host(analyzed, off)
    assert (tmp_path / "hits.txt").read_bytes() == hits_bytes(engine.query([line for _, line in exp], 10))
    # with a budget the plain tokens are patterns too
    exp = cli_expand(terms, df, behind, fuzzy="auto", prefix_ops=True)
    p = run_cli(tmp_path, "--lower", "--strip-punct", "--prefix-ops", "--fuzzy", "auto", "--suggest", "q.txt")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "suggest.txt").read_bytes() == suggest_bytes(exp)


def test_cli_refused_combinations(tmp_path):
    (tmp_path / "input").mkdir()
    (tmp_path / "input" / "doc1").write_bytes(b"one two")
    (tmp_path / "q.txt").write_bytes(b"one\n")
    for args in (["--suggest", "q.txt"], ["--fuzzy", "auto"], ["--prefix-ops"], ["--query", "q.txt", "--fuzzy", "3"],
                 ["--query", "q.txt", "--fuzzy", "auto", "--query-ops"], ["--query", "q.txt", "--prefix-ops", "--query-all"],
                 ["--query", "q.txt", "--fuzzy", "1", "--min-match", "1"], ["--query", "q.txt", "--max-expansions", "5"],
                 ["--query", "q.txt", "--fuzzy", "1", "--max-expansions", "1025"], ["--query", "q.txt", "--fuzzy", "1", "--fuzzy-prefix", "65"],
                 ["--query", "q.txt", "--fuzzy-no-transpose"]):
        p = run_cli(tmp_path, *args)
        assert p.returncode == 2, (args, p.stderr)
        assert not (tmp_path / "output.txt").exists()
