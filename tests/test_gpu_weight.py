"""Weighting schemes on the GPU (include/tfidf.h, section "weighting"): tfidf_reweight against the
plain-Python definition tests/weight_ref.py on the oracle's result, and every call after it
against its own reference built on the reweighted result.  All comparisons are exact: integers,
u64 bit patterns of doubles, bytes."""
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
import weight_ref
from conftest import GOLDEN, PKG, golden_cases
from helpers import assert_same_result, docs_to_arrays, load_golden
from kmeans_ref import KRef
from test_gpu_bm25 import Bm25Ref
from test_gpu_kmeans import check as km_check
from test_gpu_query import Ref as QRef, bits, check as q_check, make_queries
from test_gpu_similar import Ref as SRef, check as s_check
from test_gpu_terms import Ref as TRef, check as t_check
from transform_ref import Model, check as tr_check, split_docs

pytestmark = pytest.mark.gpu

REFERENCE = weight_ref.REFERENCE
FLAGSHIP = ("log", "smooth", "l2")
# every enum value, and every norm with every tf (raw without a norm is refused)
SCHEMES = [("log", "smooth", "l2"), ("log", "plus1", "l1"), ("log", "ref", "none"), ("raw", "smooth", "l2"),
           ("raw", "none", "l1"), ("ratio", "ref", "l2"), ("ratio", "plus1", "l1"), ("ratio", "smooth", "none"),
           ("binary", "none", "l2"), ("binary", "ref", "l1"), ("binary", "plus1", "none")]


def kernels_h(name):
    """a constant of csrc/kernels.h, so that the cases follow the kernel's thresholds"""
    src = open(os.path.join(PKG, "csrc", "kernels.h")).read()
    m = re.search(r"#define\s+%s\s+\(?\s*(\d+)u?(?:\s*<<\s*(\d+))?" % name, src)
    assert m, name
    return int(m.group(1)) << int(m.group(2) or 0)


RW_LUT_MAX = kernels_h("RW_LUT_MAX")
RW_BIG = kernels_h("RW_BIG")
RW_KEEP = kernels_h("RW_KEEP")


def raises(rc, fn, *args, **kw):
    with pytest.raises(tfidf_abi.TfidfError) as ex:
        fn(*args, **kw)
    assert ex.value.rc == rc, ex.value


def check_state(e, want):
    """the engine's resident result is `want` (a weight_ref.reweight dict): pairs, scores, text"""
    got = e.fetch()
    assert_same_result(got, want)
    assert e.text() == want["output_txt"]
    return got


def test_scheme_set_covers_the_enums():
    assert {s[0] for s in SCHEMES} == set(weight_ref.TF) and {s[1] for s in SCHEMES} == set(weight_ref.IDF)
    assert {(s[0], s[2]) for s in SCHEMES} == {(t, n) for t in weight_ref.TF for n in weight_ref.NORM} - {("raw", "none")}


# ---- goldens ----

@pytest.mark.parametrize("case", golden_cases())
def test_goldens_vs_reference(engine, case):
    g = load_golden(case)
    ora = oracle_py.run(g["data"], g["off"])
    N = len(g["off"]) - 1
    engine.run_host(g["data"], g["off"])
    assert engine.weighting() == dict(zip(("tf", "idf", "norm"), REFERENCE))
    for scheme in SCHEMES:                                                     # each from the integers, whatever was active
        want = weight_ref.reweight(ora, *scheme, N=N)
        info = engine.reweight(*scheme)
        check_state(engine, want)
        assert engine.weighting() == dict(zip(("tf", "idf", "norm"), scheme))
        assert (info["changed"], info["npairs"]) == (1, ora["npairs"])
        assert info["zero_norm_docs"] == weight_ref.zero_norm_docs(ora, *scheme, N)
        if scheme[0] == "log" and ora["npairs"]:
            assert info["max_count"] == int(ora["count"].max()) and info["listed_counts"] == 0
    engine.reweight(*REFERENCE)                                                # the run's bits again
    assert_same_result(engine.fetch(), ora)
    assert engine.text() == g["output"]
    engine.reweight(*FLAGSHIP)
    engine.run_host(g["data"], g["off"])                                       # a run resets the scheme
    assert engine.text() == g["output"] and engine.weighting() == dict(zip(("tf", "idf", "norm"), REFERENCE))
    assert_same_result(engine.fetch(), ora)


def test_common_word_is_visible_under_smooth_idf(engine):
    g = load_golden("g6_common_word")
    engine.run_host(g["data"], g["off"])
    word = [w for w, d in zip(engine.fetch()["terms"], engine.fetch()["term_df"].tolist()) if d == len(g["off"]) - 1][0]
    assert engine.query([word], 3)["score"].max() == 0.0                       # df = N: log(N / df) = +0.0
    engine.reweight("ratio", "smooth", "none")
    res = engine.query([word], 3)
    assert res["nhits"].tolist() == [3] and res["score"].min() > 0.0


# ---- path switches ----

def path_docs(long_count):
    """documents of 0, 1, 63, 64, 65, 129, RW_KEEP, RW_KEEP + 1, RW_BIG and RW_BIG + 1 pairs (document d
    holds the words w0 .. w(n-1), word k repeated 1 + (k + d) % 3 times), and a document whose one word
    repeats `long_count` times"""
    sizes = [0, 1, 63, 64, 65, 129, RW_KEEP, RW_KEEP + 1, RW_BIG, RW_BIG + 1]
    docs = []
    for d, n in enumerate(sizes):
        docs.append(b" ".join(b" ".join([b"w%05d" % k] * (1 + (k + d) % 3)) for k in range(n)))
    docs.append(b" ".join([b"rep"] * long_count))
    return docs, sizes


@pytest.mark.parametrize("long_count", [RW_LUT_MAX, RW_LUT_MAX + 1])
def test_document_sizes_and_count_table(engine, long_count):
    docs, sizes = path_docs(long_count)
    data, off = docs_to_arrays(docs)
    ora = oracle_py.run(data, off)
    N = len(docs)
    per_doc = [int((ora["doc"] == d + 1).sum()) for d in range(N)]
    assert per_doc == sizes + [1]
    engine.run_host(data, off)
    for scheme in (FLAGSHIP, ("log", "plus1", "l1"), ("log", "ref", "none"), ("ratio", "ref", "l2")):
        want = weight_ref.reweight(ora, *scheme, N=N)
        info = engine.reweight(*scheme)
        check_state(engine, want)
        assert info["big_docs"] == 1                                           # RW_BIG + 1 pairs; RW_BIG itself stays with a wave
        if scheme[0] == "log":
            assert info["max_count"] == long_count
            assert info["listed_counts"] == (1 if long_count > RW_LUT_MAX else 0)
    tref = TRef(weight_ref.reweight(ora, "ratio", "ref", "l2", N=N), range(1, N + 1))
    t_check(engine.top_terms(3), tref.rows(), 3)
    # transform of the same documents: the rows' norm takes the same two launches
    engine.reweight(*FLAGSHIP)
    f = engine.fetch()
    res = engine.transform(data, off)
    ro = res["row_off"].tolist()
    assert ro == np.r_[0, np.cumsum(per_doc)].tolist()
    for d in range(N):                                                         # rows in batch order, the result in name order
        sel = np.flatnonzero(f["doc"] == d + 1)
        assert np.array_equal(res["count"][ro[d]:ro[d + 1]], f["count"][sel]), d
        assert np.array_equal(bits(res["score"][ro[d]:ro[d + 1]]), bits(f["score"][sel])), d


@pytest.mark.parametrize("extra", [0, 1])
def test_both_idf_table_layouts(engine, extra):
    """ndocs_total = 2^18 (the idf table by df) and 2^18 + 1 (through the run's index of distinct df)"""
    Nt = (1 << 18) + extra
    docs = [b"a b c c", b"a b d", b"a e e e f", b"g"]
    ids = np.array([7, 70000, 131072, 262144], dtype=np.uint32)
    data, off = docs_to_arrays(docs)
    ora = oracle_py.run(data, off, ids, Nt)
    engine.run_host(data, off, ids, Nt)
    assert_same_result(engine.fetch(), ora)
    ndf = len(set(ora["df"].tolist()))
    for scheme in (("ratio", "smooth", "l2"), ("ratio", "plus1", "none"), ("binary", "ref", "l1")):
        info = engine.reweight(*scheme)
        check_state(engine, weight_ref.reweight(ora, *scheme, N=Nt))
        if scheme[1] != "ref":
            assert info["nlogs"] == (ndf if extra else Nt), info                # the layout the table took
    m = Model(data, off, ids, Nt)
    engine.reweight("ratio", "smooth", "l2")
    batch = [b"a c zz", b"", b"g g b"]
    bd, bo = docs_to_arrays(batch)
    rows = weight_ref.rows(m.rows(batch), "ratio", "smooth", "l2", Nt)
    tr_check(engine.transform(bd, bo), rows, bo, engine.fetch()["terms"])


# ---- synthetic c2 at scale 0.002: every call after the reweight ----

@pytest.fixture(scope="module")
def c2():
    p = tfidf_configs.plan("c2", scale=0.002)
    data, off = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
    ora = oracle_py.run(data, off, p["doc_ids"], p["ndocs_total"])
    want = weight_ref.reweight(ora, *FLAGSHIP, N=p["ndocs_total"])
    return dict(p=p, data=data, off=off, ora=ora, want=want, N=p["ndocs_total"],
                args=(data, off, p["doc_ids"], p["ndocs_total"]))


def test_c2_fetch_query_terms_model(engine, c2):
    ora, want, ids = c2["ora"], c2["want"], c2["p"]["doc_ids"]
    assert (len(c2["off"]) - 1, ora["nterms"], ora["npairs"]) == (200, 27478, 122839)
    engine.run_host(*c2["args"])
    qs = make_queries(ora, np.random.default_rng(11), 80)
    bm_before = engine.query_bm25(qs, 10)
    model_before = engine.model_export()
    info = engine.reweight(*FLAGSHIP)
    check_state(engine, want)
    assert info["ms_pairs"] > 0 and info["zero_norm_docs"] == 0 and info["max_count"] == int(ora["count"].max())
    ref = QRef(want)
    for k in (1, 10, 1024):
        q_check(engine.query(qs, k), [ref.rank(q) for q in qs], k)
    bm_after = engine.query_bm25(qs, 10)                                       # BM25 reads no score
    assert np.array_equal(bm_after["score"].view(np.uint64), bm_before["score"].view(np.uint64))
    assert np.array_equal(bm_after["doc"], bm_before["doc"]) and np.array_equal(bm_after["nhits"], bm_before["nhits"])
    b = Bm25Ref(ora, len(c2["off"]) - 1, c2["N"])
    q_check(bm_after, [b.rank(q) for q in qs], 10)
    tref = TRef(want, ids)
    for k in (3, 64):
        t_check(engine.top_terms(k), tref.rows(), k)
    after = engine.model_export()                                              # the model records no scheme
    assert after["N"] == model_before["N"] and after["terms"] == model_before["terms"]
    assert np.array_equal(after["df"], model_before["df"])


def test_c2_similar_kmeans(engine, c2):
    want, ids = c2["want"], c2["p"]["doc_ids"]
    engine.run_host(*c2["args"])
    engine.similar(3, [int(ids[0])])                                           # norms of the reference scores: must be recomputed
    engine.reweight(*FLAGSHIP)
    sref = SRef(want, ids)
    docs = [int(d) for d in sref.order[:24]]
    s_check(engine.similar(10, docs), sref.rows(docs), 10)
    kref = KRef(want, ids)
    km_check(engine.kmeans(8, 20, 10), kref.run(8, 20, 10))


def test_c2_transform(engine, c2):
    ora, p, N = c2["ora"], c2["p"], c2["N"]
    m = Model(c2["data"], c2["off"], p["doc_ids"], N)
    own = split_docs(c2["data"], c2["off"])[:40]
    held = [b"zz-never-seen " + own[0][:200] + b" qq-neither", b"", b" ".join(ora["terms"][:5]) + b" zz-never-seen"]
    engine.run_host(*c2["args"])
    engine.reweight(*FLAGSHIP)
    f = engine.fetch()
    for docs in (own, held):
        data, off = docs_to_arrays(docs)
        rows = weight_ref.rows(m.rows(docs), *FLAGSHIP, N)
        tr_check(engine.transform(data, off), rows, off, f["terms"])
    assert m.rows(held)[0]["doc_oov"] >= 2 and m.rows(held)[1]["doc_size"] == 0
    # the run's own documents get the resident pairs bit for bit
    data, off = docs_to_arrays(own)
    res = engine.transform(data, off)
    ro = res["row_off"].tolist()
    for i, d in enumerate(p["doc_ids"].tolist()[:40]):
        sel = np.flatnonzero(f["doc"] == d)
        assert np.array_equal(res["term"][ro[i]:ro[i + 1]], f["term"][sel]), d
        assert np.array_equal(bits(res["score"][ro[i]:ro[i + 1]]), bits(f["score"][sel])), d
    # every other scheme through the same path, on a few rows
    for scheme in SCHEMES[1:]:
        engine.reweight(*scheme)
        data, off = docs_to_arrays(held + own[:3])
        tr_check(engine.transform(data, off), weight_ref.rows(m.rows(held + own[:3]), *scheme, N), off, f["terms"])


def test_c2_prune_order(engine, c2):
    ora, N = c2["ora"], c2["N"]
    pruned = prune_ref.prune(ora, 2)
    a = weight_ref.reweight(pruned, *FLAGSHIP, N=N)                            # prune, then reweight: the norm over the kept words
    b = prune_ref.prune(c2["want"], 2)                                         # reweight, then prune: the unpruned norm's bits
    assert a["npairs"] == b["npairs"] and not np.array_equal(bits(a["score"]), bits(b["score"]))
    engine.run_host(*c2["args"])
    engine.prune(2)
    engine.reweight(*FLAGSHIP)
    check_state(engine, a)
    engine.run_host(*c2["args"])
    engine.reweight(*FLAGSHIP)
    engine.prune(2)
    check_state(engine, b)
    assert engine.weighting()["norm"] == "l2"
    engine.reweight(*REFERENCE)
    check_state(engine, pruned)


# ---- a model-only context ----

def test_model_only_context(c2):
    N, p = c2["N"], c2["p"]
    docs = split_docs(c2["data"], c2["off"])[:12] + [b"zz-never-seen " + c2["ora"]["terms"][0], b""]
    data, off = docs_to_arrays(docs)
    with tfidf_abi.Engine(0) as e:
        e.run_host(*c2["args"])
        e.reweight(*FLAGSHIP)
        fitted = e.transform(data, off)
        mod = e.model_export()
        e.model_import(mod)
        assert e.weighting() == dict(zip(("tf", "idf", "norm"), REFERENCE))    # the model file records no scheme
        plain = e.transform(data, off)
        info = e.reweight(*FLAGSHIP)
        assert (info["changed"], info["npairs"]) == (1, 0)
        served = e.transform(data, off)
        raises(tfidf_abi.E_STATE, e.fetch)
    m = Model(c2["data"], c2["off"], p["doc_ids"], N)
    tr_check(plain, m.rows(docs), off, mod["terms"])
    for key in ("row_off", "term", "count", "df", "doc_size", "doc_oov"):
        assert np.array_equal(served[key], fitted[key]), key
    assert np.array_equal(bits(served["score"]), bits(fitted["score"]))
    assert not np.array_equal(bits(served["score"]), bits(plain["score"]))


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
    ora, want, ids, N = c2["ora"], c2["want"], c2["p"]["doc_ids"], c2["N"]
    with tfidf_abi.Group(K, devices=[0] * K) as g:
        g.run_host(c2_shards(K))
        with pytest.raises(tfidf_abi.TfidfError) as ex:
            g.reweight("raw", "ref", "none")
        assert ex.value.rc == tfidf_abi.E_INVAL
        g.reweight(*FLAGSHIP)
        g.write_output(str(tmp_path / "out.txt"))
        assert (tmp_path / "out.txt").read_bytes() == want["output_txt"]
        qs = make_queries(ora, np.random.default_rng(3), 40)
        ref = QRef(want)
        q_check(g.query(qs, 10), [ref.rank(q) for q in qs], 10)
        sref = SRef(want, ids)
        docs = [int(d) for d in sref.order[:8]]
        s_check(g.similar(5, docs), sref.rows(docs), 5, pos=True)
        m = Model(c2["data"], c2["off"], ids, N)
        own = split_docs(c2["data"], c2["off"])[:10]
        for batch in (own, [b"zz-never-seen " + own[0][:300] + b" qq-neither", b"", own[1]]):
            bd, bo = docs_to_arrays(batch)
            tr_check(g.transform(bd, bo), weight_ref.rows(m.rows(batch), *FLAGSHIP, N), bo, None)
        g.reweight("ratio", "plus1", "none")                                   # no norm: the ranks' scores are final
        bd, bo = docs_to_arrays(own)
        tr_check(g.transform(bd, bo), weight_ref.rows(m.rows(own), "ratio", "plus1", "none", N), bo, None)


# ---- errors, state, allocation ----

def test_errors_and_state():
    g = load_golden("g5_w3")
    ora = oracle_py.run(g["data"], g["off"])
    with tfidf_abi.Engine(0) as e:
        raises(tfidf_abi.E_STATE, e.reweight, *FLAGSHIP)                       # neither a run nor a model
        e.run_host(g["data"], g["off"])
        text = e.text()
        raises(tfidf_abi.E_INVAL, e.reweight, "raw", "smooth", "none")
        for field, bad in (("tf", 4), ("idf", 7), ("norm", 3), ("reserved", 1), ("size", 8)):
            w = tfidf_abi.weighting(*FLAGSHIP)
            setattr(w, field, bad)
            raises(tfidf_abi.E_INVAL, e.reweight, params=w)
        assert e.text() == text == g["output"]                                 # a failed call leaves the result
        assert_same_result(e.fetch(), ora)
        assert e.weighting() == dict(zip(("tf", "idf", "norm"), REFERENCE))
        # a call with the active scheme changes no byte and leaves the formatted text valid
        assert e.reweight(*REFERENCE)["changed"] == 0 and e.text() == text
        e.reweight(*FLAGSHIP)
        want = weight_ref.reweight(ora, *FLAGSHIP, N=len(g["off"]) - 1)
        assert e.text() == want["output_txt"]
        info = e.reweight(*FLAGSHIP)
        assert (info["changed"], info["ms_pairs"]) == (0, 0.0) and e.text() == want["output_txt"]
        assert_same_result(e.fetch(), want)


def test_second_run_and_reweight_allocate_nothing(c2):
    with tfidf_abi.Engine(0) as e:
        for _ in range(2):
            e.run_host(*c2["args"])
            e.reweight(*FLAGSHIP)
            e.run_host(*c2["args"])
            e.prune(2)
            e.reweight("ratio", "plus1", "l1")
        a0 = e.alloc_counters()
        for _ in range(2):
            e.run_host(*c2["args"])
            e.reweight(*FLAGSHIP)
            e.run_host(*c2["args"])
            e.prune(2)
            e.reweight("ratio", "plus1", "l1")
        assert e.alloc_counters() == a0
        assert e.weighting() == {"tf": "ratio", "idf": "plus1", "norm": "l1"}


# ---- CLI ----

def test_cli_weighting(tmp_path):
    case = "g5_w3"
    g = load_golden(case)
    ora = oracle_py.run(g["data"], g["off"])
    want = weight_ref.reweight(ora, *FLAGSHIP, N=len(g["off"]) - 1)
    shutil.copytree(os.path.join(GOLDEN, case, "input"), tmp_path / "input")
    flags = ["--tf", "log", "--idf", "smooth", "--norm", "l2"]
    model = str(tmp_path / "m.bin")
    p = subprocess.run([tfidf_abi.CLI_PATH] + flags + ["--save-model", model, "--transform", "input"], cwd=tmp_path,
                       capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    out = (tmp_path / "output.txt").read_bytes()
    assert out == want["output_txt"] and out != g["output"]
    assert (tmp_path / "transform.txt").read_bytes() == out
    os.remove(tmp_path / "transform.txt")
    p = subprocess.run([tfidf_abi.CLI_PATH, "--model", model, "--transform", "input"] + flags, cwd=tmp_path,
                       capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "transform.txt").read_bytes() == out
    p = subprocess.run([tfidf_abi.CLI_PATH, "--sublinear-tf", "--idf", "smooth", "--norm", "l2"], cwd=tmp_path,
                       capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "output.txt").read_bytes() == out
    p = subprocess.run([tfidf_abi.CLI_PATH, "--debug-jobs", "--norm", "l2"], cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode != 0
    for bad in (["--tf", "x"], ["--idf", "bm25"], ["--norm", "l3"], ["--tf", "raw"]):
        q = subprocess.run([tfidf_abi.CLI_PATH] + bad, cwd=tmp_path, capture_output=True, timeout=120)
        assert q.returncode == 2, bad
