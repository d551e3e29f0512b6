"""Vocabulary pruning on the GPU (include/tfidf.h, section "prune"): tfidf_prune against the
plain-Python filter tests/prune_ref.py of the oracle's result, and every call after it against
its own reference built on the filtered result.  All comparisons are exact: integers, u64 bit
patterns of doubles, bytes."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle_py
import prune_ref
import tfidf_abi
import tfidf_configs
from conftest import GOLDEN, PKG, golden_cases
from helpers import assert_same_result, device_corpus, docs_to_arrays, load_golden
from kmeans_ref import KRef
from test_gpu_bm25 import Bm25Ref
from test_gpu_kmeans import check as km_check
from test_gpu_query import Ref as QRef, bits, check as q_check, make_queries
from test_gpu_similar import Ref as SRef, check as s_check
from test_gpu_terms import Ref as TRef, check as t_check
from transform_ref import Model, check as tr_check, split_docs

pytestmark = pytest.mark.gpu


def kernels_h(name):
    """a constant of csrc/kernels.h, so that the cases follow the kernel's tile and threshold"""
    src = open(os.path.join(PKG, "csrc", "kernels.h")).read()
    m = re.search(r"#define\s+%s\s+\(?\s*(\d+)u?(?:\s*<<\s*(\d+))?" % name, src)
    assert m, name
    return int(m.group(1)) << int(m.group(2) or 0)


PR_TILE = kernels_h("PR_TILE")
PR_LDS_TERMS = kernels_h("PR_LDS_TERMS")


def raises(rc, fn, *args, **kw):
    with pytest.raises(tfidf_abi.TfidfError) as ex:
        fn(*args, **kw)
    assert ex.value.rc == rc, ex.value


def check_state(e, want, ids=None):
    """the engine's resident result is `want` (a prune_ref.prune dict): pairs, terms, df, text"""
    got = e.fetch()
    assert (got["npairs"], got["nterms"]) == (want["npairs"], want["nterms"])
    assert_same_result(got, want)
    assert got["terms"] == sorted(want["terms"], key=lambda w: w + b"\t")
    wdf = dict(zip(want["terms"], prune_ref.term_df(want).tolist())) if want["npairs"] else {}
    assert dict(zip(got["terms"], got["term_df"].tolist())) == wdf
    if got["npairs"]:
        assert np.all(got["term"] < got["nterms"])
    assert e.text() == want["output_txt"]
    return got


def not_vacuous(ora, want):
    assert 0 < want["nterms"] < ora["nterms"] and want["npairs"] < ora["npairs"]


# ---- goldens ----

@pytest.mark.parametrize("case", golden_cases())
def test_goldens_vs_reference(engine, case):
    g = load_golden(case)
    ora = oracle_py.run(g["data"], g["off"])
    N, V = len(g["off"]) - 1, ora["nterms"]
    for mn, mx, mf in [(2, 0, 0), (0, N - 1, 0), (2, N - 1, 0), (0, 0, V // 2), (0, 0, 1), (0, 0, 0)]:
        want = prune_ref.prune(ora, mn, mx, mf)
        assert want["output_txt"] == prune_ref.filter_lines(g["output"], set(want["terms"]))
        engine.run_host(g["data"], g["off"])
        info = engine.prune(mn, mx, mf)
        check_state(engine, want)
        assert (info["nterms_before"], info["nterms_after"]) == (V, want["nterms"])
        assert (info["npairs_before"], info["npairs_after"]) == (ora["npairs"], want["npairs"])
        assert info["docs_emptied"] == prune_ref.emptied_docs(ora, want)
        if case == "g6_common_word" and (mn, mx) == (2, N - 1):
            assert (want["nterms"], want["npairs"], engine.text(), info["docs_emptied"]) == (0, 0, b"", 4)
            assert engine.query([b"the a"], 3)["nhits"].tolist() == [0]
        ri = engine.info()                       # tfidf_last_run_info still describes the run
        assert (ri["npairs"], ri["nterms"]) == (ora["npairs"], V)
    engine.run_host(g["data"], g["off"])         # a run after a prune: the full result again
    f = engine.fetch()
    assert_same_result(f, ora)
    assert engine.text() == g["output"] and f["nterms"] == V


# ---- synthetic c2 at scale 0.002: every call after the prune ----

@pytest.fixture(scope="module")
def c2():
    p = tfidf_configs.plan("c2", scale=0.002)
    data, off = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
    ora = oracle_py.run(data, off, p["doc_ids"], p["ndocs_total"])
    want = prune_ref.prune(ora, 2)
    return dict(p=p, data=data, off=off, ora=ora, want=want, args=(data, off, p["doc_ids"], p["ndocs_total"]))


def test_c2_fetch_and_model(engine, c2):
    ora, want = c2["ora"], c2["want"]
    assert (len(c2["off"]) - 1, ora["nterms"], ora["npairs"]) == (200, 27478, 122839)
    not_vacuous(ora, want)
    engine.run_host(*c2["args"])
    before = engine.model_export()
    info = engine.prune(2)
    check_state(engine, want)
    assert info["ms_select"] > 0 and info["ms_terms"] > 0 and info["ms_pairs"] > 0 and info["cut_df"] == 0
    after = engine.model_export()
    host = tfidf_abi.model_prune(before, 2)
    assert after["N"] == host["N"] and after["terms"] == host["terms"] and np.array_equal(after["df"], host["df"])
    assert np.array_equal(after["term_off"], host["term_off"]) and np.array_equal(after["term_bytes"], host["term_bytes"])


def test_c2_query_bm25_terms(engine, c2):
    ora, want, ids = c2["ora"], c2["want"], c2["p"]["doc_ids"]
    qs = make_queries(ora, np.random.default_rng(11), 80)        # words of the unpruned vocabulary: pruned ones must miss
    pruned_words = set(ora["terms"]) - set(want["terms"])
    assert any(t in pruned_words for q in qs for t in q.split())
    engine.run_host(*c2["args"])
    engine.prune(2)
    ref = QRef(want)
    for k in (1, 10, 1024):
        q_check(engine.query(qs, k), [ref.rank(q) for q in qs], k)
    b = Bm25Ref(want, len(c2["off"]) - 1, c2["p"]["ndocs_total"])
    full = Bm25Ref(ora, len(c2["off"]) - 1, c2["p"]["ndocs_total"])
    b.L, b.avgdl = full.L, full.avgdl                             # docSize is unchanged, so L and avgdl are
    res = engine.query_bm25(qs, 10)
    q_check(res, [b.rank(q) for q in qs], 10)
    assert bits(res["avgdl"]) == bits(full.avgdl)
    tref = TRef(want, ids)
    for k in (3, 64):
        t_check(engine.top_terms(k), tref.rows(), k)


def test_c2_similar_kmeans(engine, c2):
    want, ids = c2["want"], c2["p"]["doc_ids"]
    engine.run_host(*c2["args"])
    engine.similar(3, [int(ids[0])])                              # norms of the unpruned result: must be recomputed
    engine.prune(2)
    sref = SRef(want, ids)
    docs = [int(d) for d in sref.order[:24]]
    s_check(engine.similar(10, docs), sref.rows(docs), 10)
    kref = KRef(want, ids)
    km_check(engine.kmeans(8, 20, 10), kref.run(8, 20, 10))
    assert engine.kmeans_info()["matrix_bytes"] == 8 * want["nterms"] * 8


def test_c2_transform(engine, c2):
    ora, want = c2["ora"], c2["want"]
    p = c2["p"]
    m = Model(c2["data"], c2["off"], p["doc_ids"], p["ndocs_total"])
    kept = set(want["terms"])
    m.df = {w: d for w, d in m.df.items() if w in kept}          # a pruned word is out of vocabulary
    own = split_docs(c2["data"], c2["off"])[:40]
    gone = sorted(set(ora["terms"]) - kept)[:6]
    held = [b" ".join(gone) + b" " + own[0][:200], b" ".join(want["terms"][:5]) + b" zz-never-seen " + gone[0]]
    engine.run_host(*c2["args"])
    engine.prune(2)
    terms = engine.fetch()["terms"]
    for docs in (own, held):
        data, off = docs_to_arrays(docs)
        rows = m.rows(docs)
        res = engine.transform(data, off)
        tr_check(res, rows, off, terms)
    assert sum(r["doc_oov"] for r in m.rows(own)) > 0 and m.rows(held)[0]["doc_oov"] >= 6
    # the run's own documents get the pruned pairs bit for bit
    f = engine.fetch()
    data, off = docs_to_arrays(own)
    res = engine.transform(data, off)
    order = sorted(p["doc_ids"].tolist(), key=lambda d: b"doc%d@" % d)
    by_doc = {d: np.flatnonzero(f["doc"] == d) for d in p["doc_ids"].tolist()[:40]}
    ro = res["row_off"].tolist()
    for i, d in enumerate(p["doc_ids"].tolist()[:40]):
        sel = by_doc[d]
        assert np.array_equal(res["term"][ro[i]:ro[i + 1]], f["term"][sel]), d
        assert np.array_equal(bits(res["score"][ro[i]:ro[i + 1]]), bits(f["score"][sel])), d
    assert len(order) == 200


# ---- tile and document boundaries ----

def boundary_docs():
    """doc1: PR_TILE + 1 words of its own (everything pruned; pruned pairs at a tile's first and
    last position); documents of exactly 1, 63, 64, 65, 256, 257, 4096 and 4097 pairs in which a
    shared word (kept) alternates with a word of the document's own (pruned); a last document
    with every shared word (it loses nothing)"""
    sizes = [1, 63, 64, 65, 256, 257, 4096, 4097]
    docs = [b" ".join(b"u%05d" % i for i in range(PR_TILE + 1))]
    for d, n in enumerate(sizes):
        w = []
        for k in range(n):
            w.append(b"w%05d0" % (k // 2) if k % 2 == 0 else b"w%05d1d%d" % (k // 2, d))
        docs.append(b" ".join(w))
    docs.append(b" ".join(b"w%05d0" % k for k in range((max(sizes) + 1) // 2)))
    return docs, sizes


def test_tile_and_document_boundaries(engine):
    docs, sizes = boundary_docs()
    data, off = docs_to_arrays(docs)
    ora = oracle_py.run(data, off)
    want = prune_ref.prune(ora, 2)
    not_vacuous(ora, want)
    per_doc = {d: int((ora["doc"] == d).sum()) for d in range(1, len(docs) + 1)}
    assert [per_doc[d + 2] for d in range(len(sizes))] == sizes
    kept_pairs = np.array([ora["terms"][t] in set(want["terms"]) for t in ora["term"].tolist()])
    gone = np.flatnonzero(~kept_pairs)
    assert ora["npairs"] > 2 * PR_TILE                                        # more than two tiles
    assert (gone % PR_TILE == 0).any() and (gone % PR_TILE == PR_TILE - 1).any()
    after = {d: int((want["doc"] == d).sum()) for d in per_doc}
    assert after[1] == 0 and after[len(docs)] == per_doc[len(docs)]           # one loses all, one nothing
    assert [after[d + 2] for d in range(len(sizes))] == [(n + 1) // 2 for n in sizes]
    engine.run_host(data, off)
    info = engine.prune(2)
    check_state(engine, want)
    assert info["docs_emptied"] == 1
    tref = TRef(want, range(1, len(docs) + 1))
    t_check(engine.top_terms(3), tref.rows(), 3)                              # the new document offsets, empty rows included


# ---- a vocabulary wider than the bitmap's LDS threshold ----

def test_wide_vocabulary(engine):
    V = 300000
    assert V > PR_LDS_TERMS == 1 << 18
    docs = [b" ".join(b"w%06d" % i for i in range(d, V, 6)) for d in range(6)]
    docs.append(b"w000007 w000008 w262152")
    data, off = docs_to_arrays(docs)
    ora = oracle_py.run(data, off)
    want = prune_ref.prune(ora, 2)
    not_vacuous(ora, want)
    words = sorted(ora["terms"], key=lambda w: w + b"\t")
    assert words[7] == b"w000007" and words[7 + (1 << 18)] == b"w262151" and len(words) == V
    assert sorted(want["terms"]) == [b"w000007", b"w000008", b"w262152"]      # rank 7 kept, rank 7 + 2^18 pruned
    engine.run_host(data, off)
    engine.prune(2)
    check_state(engine, want)
    res = engine.query([b"w262151", b"w000007", b"w262152"], 5)
    assert res["nterms_found"].tolist() == [0, 1, 1] and res["nhits"].tolist() == [0, 2, 2]
    # a max_features cut over the same width: the sort's ties resolve by rank
    engine.run_host(data, off)
    info = engine.prune(0, 0, 100000)
    check_state(engine, prune_ref.prune(ora, 0, 0, 100000))
    assert info["cut_df"] == 1 and info["nterms_after"] == 100000


# ---- long terms ----

def test_long_terms(engine):
    w16 = b"abcdefghijklmnop"
    a, b_, c = w16 + b"q" * 24, w16 + b"r" * 24, b"L" * 300                   # a and b_ share their first 16 bytes
    docs = [a + b" x " + w16 + b" " + c, b_ + b" y " + a, b"x y z " + c, w16 + b" zz"]
    data, off = docs_to_arrays(docs)
    ora = oracle_py.run(data, off)
    want = prune_ref.prune(ora, 2)
    not_vacuous(ora, want)
    assert a in want["terms"] and b_ not in want["terms"] and c in want["terms"] and w16 in want["terms"]
    assert sorted(len(w) for w in want["terms"] if len(w) >= 16) == [16, 40, 300]
    engine.run_host(data, off)
    engine.prune(2)
    got = check_state(engine, want)                                           # text(): long words still format from the corpus
    res = engine.query([a, b_, c, w16], 4)
    assert res["nterms_found"].tolist() == [1, 0, 1, 1] and res["nhits"].tolist() == [2, 0, 2, 2]
    m = Model(data, off)
    m.df = {w: d for w, d in m.df.items() if w in set(want["terms"])}
    batch = [a + b" " + b_ + b" " + c, b_ + b" " + b_]
    bd, bo = docs_to_arrays(batch)
    r = engine.transform(bd, bo)
    tr_check(r, m.rows(batch), bo, got["terms"])
    assert r["doc_oov"].tolist() == [1, 2]


# ---- a device corpus at an unaligned base ----

def test_device_corpus_unaligned(engine):
    g = load_golden("g5_w3")
    ora = oracle_py.run(g["data"], g["off"])
    want = prune_ref.prune(ora, 2, len(g["off"]) - 2)
    not_vacuous(ora, want)
    with device_corpus(g["data"], g["off"], shift=5) as c:
        engine.run_corpus(c)
        engine.prune(2, len(g["off"]) - 2)
        check_state(engine, want)


# ---- the max_features tie rule ----

def test_max_features_ties(engine):
    words = [b"t%03d" % i for i in range(40)]
    docs = [b" ".join(words), b" ".join(words[::2]), b" ".join(words[::4]), b"t001 t003"]
    data, off = docs_to_arrays(docs)
    ora = oracle_py.run(data, off)
    df = dict(zip(ora["terms"], prune_ref.term_df(ora).tolist()))
    assert sorted(set(df.values())) == [1, 2, 3] and list(df.values()).count(2) > 5
    V = ora["nterms"]
    for M in (1, 5, 10, 11, 15, V - 1, V, V + 1):
        want = prune_ref.prune(ora, 0, 0, M)
        assert want["nterms"] == min(M, V)
        engine.run_host(data, off)
        info = engine.prune(0, 0, M)
        check_state(engine, want)
        kept_df = sorted(prune_ref.term_df(want).tolist())
        assert info["cut_df"] == (kept_df[0] if M < V else 0)
    want = prune_ref.prune(ora, 0, 2, 4)                                      # the range test first, then the cut
    engine.run_host(data, off)
    engine.prune(0, 2, 4)
    check_state(engine, want)
    assert all(d == 2 for d in prune_ref.term_df(want).tolist())


# ---- composition, identity ----

def test_composition_and_identity(engine):
    g = load_golden("g5_w3")
    N = len(g["off"]) - 1
    ora = oracle_py.run(g["data"], g["off"])
    want = prune_ref.prune(ora, 3, N - 2)
    not_vacuous(ora, want)
    engine.run_host(g["data"], g["off"])
    engine.prune(2, N - 2)
    engine.prune(3, N - 1)
    two = check_state(engine, want)
    engine.run_host(g["data"], g["off"])
    engine.prune(3, N - 2)
    one = check_state(engine, want)
    assert two["output_txt"] == one["output_txt"]
    # the identity prune leaves every byte, the formatted text and the norms included
    engine.run_host(g["data"], g["off"])
    text = engine.text()
    sim = engine.similar(3)
    info = engine.prune(0, 0, 0)
    assert (info["nterms_after"], info["npairs_after"]) == (ora["nterms"], ora["npairs"])
    assert engine.text() == text == g["output"]
    assert_same_result(engine.fetch(), ora)
    assert np.array_equal(bits(engine.similar(3)["nb_score"]), bits(sim["nb_score"]))
    info = engine.prune(1, N, ora["nterms"])
    assert info["nterms_after"] == ora["nterms"] and engine.text() == text


# ---- errors, state, allocation ----

def test_errors_and_state():
    g = load_golden("g5_w3")
    with tfidf_abi.Engine(0) as e:
        raises(tfidf_abi.E_STATE, e.prune, 2)                                 # before a run
        e.run_host(g["data"], g["off"])
        text = e.text()
        raises(tfidf_abi.E_INVAL, e.prune, 3, 2)
        p = tfidf_abi.prune_params(2)
        p.reserved = 1
        raises(tfidf_abi.E_INVAL, e.prune, params=p)
        p = tfidf_abi.prune_params(2)
        p.size = 8
        raises(tfidf_abi.E_INVAL, e.prune, params=p)
        assert e.text() == text == g["output"]                                # a failed call leaves the result
        assert_same_result(e.fetch(), oracle_py.run(g["data"], g["off"]))
        mod = e.model_export()
        e.model_import(mod)
        raises(tfidf_abi.E_STATE, e.prune, 2)                                 # a model-only context
        assert e.model_export()["terms"] == mod["terms"]


def test_second_run_and_prune_allocate_nothing(c2):
    with tfidf_abi.Engine(0) as e:
        for _ in range(2):
            e.run_host(*c2["args"])
            e.prune(2)
            e.run_host(*c2["args"])
            e.prune(0, 0, 5000)
        a0 = e.alloc_counters()
        for _ in range(2):
            e.run_host(*c2["args"])
            e.prune(2)
            e.run_host(*c2["args"])
            e.prune(0, 0, 5000)
        assert e.alloc_counters() == a0
        assert e.fetch()["nterms"] == 5000


# ---- groups ----

def c2_shards(K):
    out = []
    for r in range(K):
        p = tfidf_configs.plan("c2", scale=0.002, rank=r, nranks=K)
        data, off = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
        out.append((data, off, p["doc_ids"], p["ndocs_total"]))
    return out


@pytest.mark.parametrize("K", [2, 3])
def test_group_equals_single_shard_reference(c2, K, tmp_path):
    ora, want, ids = c2["ora"], c2["want"], c2["p"]["doc_ids"]
    with tfidf_abi.Group(K, devices=[0] * K) as g:
        g.run_host(c2_shards(K))
        with pytest.raises(tfidf_abi.TfidfError) as ex:
            g.prune(0, 0, 10)
        assert ex.value.rc == tfidf_abi.E_INVAL
        g.prune(2)
        g.write_output(str(tmp_path / "out.txt"))
        assert (tmp_path / "out.txt").read_bytes() == want["output_txt"]
        qs = make_queries(ora, np.random.default_rng(3), 40)
        ref = QRef(want)
        q_check(g.query(qs, 10), [ref.rank(q) for q in qs], 10)
        sref = SRef(want, ids)
        docs = [int(d) for d in sref.order[:8]]
        s_check(g.similar(5, docs), sref.rows(docs), 5, pos=True)
        m = Model(c2["data"], c2["off"], ids, c2["p"]["ndocs_total"])
        m.df = {w: d for w, d in m.df.items() if w in set(want["terms"])}
        batch = split_docs(c2["data"], c2["off"])[:10]
        bd, bo = docs_to_arrays(batch)
        tr_check(g.transform(bd, bo), m.rows(batch), bo, None)
        mod = g.model_export()
        df = dict(zip(ora["terms"], prune_ref.term_df(ora).tolist()))
        words = sorted(ora["terms"], key=lambda w: w + b"\t")
        host = prune_ref.prune_model({"N": c2["p"]["ndocs_total"], "terms": words, "df": [df[w] for w in words]}, 2)
        assert mod["N"] == host["N"] == 200
        assert mod["terms"] == host["terms"] and np.array_equal(mod["df"], host["df"])


# ---- CLI ----

@pytest.mark.parametrize("extra", [[], ["--shards", "2"]])
def test_cli_prune(tmp_path, extra):
    case = "g5_w3"
    g = load_golden(case)
    N = len(g["off"]) - 1
    ora = oracle_py.run(g["data"], g["off"])
    want = prune_ref.prune(ora, 2, int(np.floor(0.9 * N)))
    not_vacuous(ora, want)
    shutil.copytree(os.path.join(GOLDEN, case, "input"), tmp_path / "input")
    model = str(tmp_path / "m.bin")
    p = subprocess.run([tfidf_abi.CLI_PATH, "--min-df", "2", "--max-df", "0.9", "--save-model", model] + extra,
                       cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    out = (tmp_path / "output.txt").read_bytes()
    assert out == want["output_txt"] == prune_ref.filter_lines(g["output"], set(want["terms"]))
    p = subprocess.run([tfidf_abi.CLI_PATH, "--model", model, "--transform", "input"], cwd=tmp_path, capture_output=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "transform.txt").read_bytes() == out
    if not extra:
        p = subprocess.run([tfidf_abi.CLI_PATH, "--max-features", "50"], cwd=tmp_path, capture_output=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert (tmp_path / "output.txt").read_bytes() == prune_ref.prune(ora, 0, 0, 50)["output_txt"]
        p = subprocess.run([tfidf_abi.CLI_PATH, "--min-df", "0.5"], cwd=tmp_path, capture_output=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert (tmp_path / "output.txt").read_bytes() == prune_ref.prune(ora, int(np.ceil(0.5 * N)))["output_txt"]
    else:
        p = subprocess.run([tfidf_abi.CLI_PATH, "--max-features", "50"] + extra, cwd=tmp_path, capture_output=True, timeout=120)
        assert p.returncode == 2
    for bad in (["--min-df", "x"], ["--max-df", "1.5"], ["--min-df", "0.0"], ["--min-df", "5", "--max-df", "3"],
                ["--max-features", "0"]):
        q = subprocess.run([tfidf_abi.CLI_PATH] + bad, cwd=tmp_path, capture_output=True, timeout=120)
        assert q.returncode == 2, bad
