"""Spherical k-means over the resident result (tfidf_kmeans, `tfidf --clusters`) against the
plain Python loops of kmeans_ref.py over the oracle's pairs.

Everything is compared exactly: iterations, converged, doc, label, size, seed, nterms and term
as integers, sim and weight as u64 bits, the clusters' words as bytes.  No tolerance anywhere."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_py
import tfidf_abi
import tfidf_configs
from conftest import golden_cases, GOLDEN
from helpers import docs_to_arrays, load_golden
from kmeans_ref import KRef, NO_CLUSTER, cluster_lines

pytestmark = pytest.mark.gpu


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def check(res, want):
    assert want is not None
    assert (res["k"], res["iterations"], res["converged"]) == (want["k"], want["iterations"], want["converged"])
    assert res["doc"].tolist() == want["doc"]
    assert res["label"].tolist() == want["label"]
    assert np.array_equal(bits(res["sim"]), bits(want["sim"]))
    assert res["size"].tolist() == want["size"] and res["seed"].tolist() == want["seed"]
    assert res["nterms"].tolist() == [len(t) for t in want["top"]]
    for c, top in enumerate(want["top"]):
        n = len(top)
        assert res["term"][c, :n].tolist() == [t for t, _, _ in top], c
        assert np.array_equal(bits(res["weight"][c, :n]), bits([w for _, w, _ in top])), c
        assert res["words"][c] == [w for _, _, w in top], c
        assert np.all(res["term"][c, n:] == 0xFFFFFFFF) and np.all(bits(res["weight"][c, n:]) == 0), c


def same_result(a, b):
    for name in ("k", "iterations", "converged", "words"):
        assert a[name] == b[name], name
    for name in ("doc", "label", "size", "seed", "nterms", "term"):
        assert np.array_equal(a[name], b[name]), name
    assert np.array_equal(bits(a["sim"]), bits(b["sim"])) and np.array_equal(bits(a["weight"]), bits(b["weight"]))


def make_ref(data, off, ids=None, ntotal=0):
    return KRef(oracle_py.run(data, off, ids, ntotal), range(1, len(off)) if ids is None else ids)


def rc_of(fn, *a, **kw):
    with pytest.raises(tfidf_abi.TfidfError) as ex:
        fn(*a, **kw)
    return ex.value.rc


# ------------------------------------------------------------------ corpora --

@pytest.fixture(scope="module")
def c2():
    p = tfidf_configs.plan("c2", scale=0.002)
    data, off = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
    args = (data, off, p["doc_ids"], p["ndocs_total"])
    return dict(p=p, args=args, ref=make_ref(*args))


def topical_docs(n=300, seed=3):
    """short documents over six topics of 30 words (eight words of one topic, four of another,
    four of 400 noise words): clusters that take several updates to settle"""
    rng = np.random.default_rng(seed)
    docs = []
    for _ in range(n):
        a, b = rng.integers(0, 6, 2)
        w = [b"t%d_%02d" % (a, int(x)) for x in rng.integers(0, 30, 8)] + [b"t%d_%02d" % (b, int(x)) for x in rng.integers(0, 30, 4)]
        w += [b"n%03d" % int(x) for x in rng.integers(0, 400, 4)]
        docs.append(b" ".join(w))
    return docs


@pytest.fixture(scope="module")
def topical():
    data, off = docs_to_arrays(topical_docs())
    return dict(args=(data, off), ref=make_ref(data, off))


# -------------------------------------------------------------------- tests --

def test_c2_vs_reference(engine, c2):
    """Config 2 at scale 0.002 (200 documents, 122839 pairs, 27478 terms): K = 8, the default
    seeds, max_iter = 20, T = 10.  A kernel that fuses a product into its add cannot pass.

    This corpus cannot carry the `iterations >= 3` assertion: its documents are nearly orthogonal
    (pairwise similarities of 0.02 to 0.14), so after the first update every document's share of
    its own centroid, about 1 / sqrt(members), outweighs any other centroid and the labels of
    pass 2 equal those of pass 1.  The default seeds and 1200 random sets of 8 seed ids all stop
    converged after 2 passes in the reference.  The assertion is made on a corpus with structure,
    test_several_updates_vs_reference below."""
    ref = c2["ref"]
    want = ref.run(8, 20, 10)
    assert ref.fused_differs(want)
    assert (want["iterations"], want["converged"]) == (2, 1)
    engine.run_host(*c2["args"])
    check(engine.kmeans(8, 20, 10), want)
    info = engine.kmeans_info()
    assert (info["ndocs"], info["k"], info["passes"], info["updates"]) == (200, 8, 2, 1)
    assert info["clusterable"] == len(ref.clusterable) and info["matrix_bytes"] == 8 * len(ref.words) * 8
    assert info["ms_assign"] > 0 and info["ms_update"] > 0 and info["ms_terms"] > 0
    # max_iter = 0 is the default 20; other seeds by id
    check(engine.kmeans(8, 0, 10), want)
    seeds = [4, 9, 15, 53, 61, 100, 124, 165]
    check(engine.kmeans(8, 20, 64, seeds), ref.run(8, 20, 64, seeds))


@pytest.mark.parametrize("k", [2, 4, 6])
def test_several_updates_vs_reference(engine, topical, k):
    """the update more than once: 6 to 10 passes until the labels settle"""
    ref = topical["ref"]
    want = ref.run(k, 20, 10)
    assert ref.fused_differs(want)
    assert want["iterations"] >= 3 and want["converged"] == 1
    engine.run_host(*topical["args"])
    check(engine.kmeans(k, 20, 10), want)
    assert engine.kmeans_info()["updates"] == want["iterations"] - 1


@pytest.mark.parametrize("case", golden_cases())
def test_golden_vs_reference(engine, case):
    g = load_golden(case)
    ref = make_ref(g["data"], g["off"])
    engine.run_host(g["data"], g["off"])
    m = len(ref.clusterable)
    for k in sorted({1, 2, min(m, 3)}):
        if 1 <= k <= m:
            check(engine.kmeans(k, 20, 10), ref.run(k, 20, 10))
    assert rc_of(engine.kmeans, m + 1) == tfidf_abi.E_INVAL


def sized_doc(rng, n, lo=0, hi=6000):
    """exactly n distinct words, a third of them repeated (counts 2-4), shuffled"""
    words = rng.choice(np.arange(lo, hi), size=n, replace=False)
    toks = [int(w) for w in words for _ in range(1 + (int(w) % 3 == 0) * (1 + int(w) % 4 % 3))]
    return b" ".join(b"w%05d" % toks[i] for i in rng.permutation(len(toks)))


def test_pair_count_boundaries(engine):
    """documents of exactly 0, 1, 63, 64, 65, 255, 256, 257, 4096 and 4097 pairs (64: one round
    of a wave's loads, 256: the update's workgroup, 4096: other passes' cut to a second kernel,
    which this one does not have) among 20 small ones; several as seeds"""
    rng = np.random.default_rng(5)
    docs = [b" ".join(b"w%05d" % int(j) for j in rng.integers(0, 6000, 30)) for _ in range(20)]
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, 4096, 4097]
    where = {}
    for i, n in enumerate(sizes):
        docs.insert(2 + 2 * i, sized_doc(rng, n) if n else b"")
    data, off = docs_to_arrays(docs)
    ref = make_ref(data, off)
    for j, t in enumerate(ref.t):
        where.setdefault(len(t), ref.order[j])
    assert all(n in where for n in sizes)
    engine.run_host(data, off)
    for k, seeds in ((3, None), (5, [where[n] for n in (1, 64, 257, 4096, 4097)]), (4, [where[n] for n in (63, 65, 255, 256)])):
        want = ref.run(k, 20, 8, seeds)
        check(engine.kmeans(k, 20, 8, seeds), want)
        assert want["label"][ref.pos[where[0]]] == NO_CLUSTER
    assert rc_of(engine.kmeans, 2, seeds=[where[0], where[1]]) == tfidf_abi.E_INVAL


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 100, 128, 129, 130, 256])
def test_k_boundaries(engine, topical, k):
    """lane ownership (K against the 64 lanes) and one to four accumulators per lane"""
    ref = topical["ref"]
    engine.run_host(*topical["args"])
    check(engine.kmeans(k, 4, 6), ref.run(k, 4, 6))


def test_k_out_of_range(engine, topical):
    ref = topical["ref"]
    engine.run_host(*topical["args"])
    m = len(ref.clusterable)
    assert m == 300
    assert rc_of(engine.kmeans, 257) == tfidf_abi.E_INVAL and rc_of(engine.kmeans, 0) == tfidf_abi.E_INVAL
    data, off = docs_to_arrays(topical_docs(40))
    engine.run_host(data, off)
    assert rc_of(engine.kmeans, 41) == tfidf_abi.E_INVAL
    check(engine.kmeans(40, 3, 2), make_ref(data, off).run(40, 3, 2))


def test_ties_and_an_empty_cluster(engine):
    """byte-equal documents 3 and 7 as seeds 0 and 1: their centroids are equal, so in the first
    pass both documents and every tie go to cluster 0 and cluster 1 has no member.  The update
    then leaves cluster 1 its seed's centroid: after two passes it still reports the seed's
    terms (the second pass, against the moved centroid 0, may hand it members)."""
    rng = np.random.default_rng(2)
    docs = [b" ".join(b"f%d" % int(j) for j in rng.integers(0, 40, 12)) for _ in range(30)]
    docs[2] = docs[6] = b"alpha beta gamma delta alpha f1 f2"
    data, off = docs_to_arrays(docs)
    ref = make_ref(data, off)
    engine.run_host(data, off)
    seed_top = ref.run(3, 1, 5, [3, 7, 12])["top"][1]
    for it in (1, 2, 20):
        want = ref.run(3, it, 5, [3, 7, 12])
        res = engine.kmeans(3, it, 5, [3, 7, 12])
        check(res, want)
        if it == 1:
            assert want["size"][1] == 0 and want["label"][ref.pos[3]] == want["label"][ref.pos[7]] == 0
        if it <= 2:
            assert want["top"][1] == seed_top and len(res["words"][1]) == 5
    # two equal documents and nothing else to cluster: the empty cluster through every pass
    data2, off2 = docs_to_arrays([b"alpha beta beta", b"", b"alpha beta beta", b" "])
    ref2 = make_ref(data2, off2)
    engine.run_host(data2, off2)
    for it in (1, 2, 20):
        check(engine.kmeans(2, it, 5, [1, 3]), ref2.run(2, it, 5, [1, 3]))
    assert ref2.run(2, 1, 5, [1, 3])["size"] == [2, 0]
    engine.run_host(data, off)
    assert rc_of(engine.kmeans, 2, seeds=[3, 3]) == tfidf_abi.E_INVAL           # a repeated id
    assert rc_of(engine.kmeans, 2, seeds=[3, 31]) == tfidf_abi.E_INVAL          # no such document


def test_unclustered_documents(engine):
    """a document made only of the word every document holds (every score +0.0), and empty
    documents: no label, sim +0.0, in no size, not a seed"""
    common = [b"common a b c", b"common a d", b"common b c e", b"common common", b"common e e a", b"common z a"]
    empty = [b"q a b c", b"r a d", b"", b"s b c e", b"t e e a", b"u z a", b" \n"]
    for docs, out in ((common, [4]), (empty, [3, 7])):
        data, off = docs_to_arrays(docs)
        ref = make_ref(data, off)
        assert sorted(ref.order[j] for j in range(len(docs)) if j not in ref.clusterable) == out
        engine.run_host(data, off)
        for k in (1, 2, 5):
            want = ref.run(k, 20, 4)
            res = engine.kmeans(k, 20, 4)
            check(res, want)
            for d in out:
                assert res["label"][ref.pos[d]] == NO_CLUSTER and bits(res["sim"])[ref.pos[d]] == 0
            assert int(res["size"].sum()) == 5
        assert rc_of(engine.kmeans, 6) == tfidf_abi.E_INVAL
        assert rc_of(engine.kmeans, 2, seeds=[1, out[0]]) == tfidf_abi.E_INVAL
    # every document unclustered: no K fits
    data, off = docs_to_arrays([b"the same words"] * 5)
    engine.run_host(data, off)
    assert rc_of(engine.kmeans, 1) == tfidf_abi.E_INVAL


def test_max_iter(engine, topical):
    ref = topical["ref"]
    engine.run_host(*topical["args"])
    full = ref.run(4, 20, 3)
    for it in (1, 2, full["iterations"] - 1, full["iterations"], 1000):
        want = ref.run(4, it, 3)
        check(engine.kmeans(4, it, 3), want)
        assert want["iterations"] == min(it, full["iterations"])
        assert want["converged"] == (1 if it >= full["iterations"] else 0)
    one = engine.kmeans(4, 1, 3)
    assert one["converged"] == 0 and one["seed"].tolist() == ref.default_seeds(4)
    # K = M: every document its own seed, nothing to move
    data, off = docs_to_arrays([b"a b", b"c d", b"e a"])
    engine.run_host(data, off)
    check(engine.kmeans(3, 1, 2), make_ref(data, off).run(3, 1, 2))
    check(engine.kmeans(3, 5, 2), make_ref(data, off).run(3, 5, 2))


def wide_docs(V=300000, nbig=6, nshort=270):
    rng = np.random.default_rng(8)
    docs = [b" ".join(b"w%06d" % i for i in range(d, V, nbig)) for d in range(nbig)]
    docs.append(b"w000007 w262151 w262152")
    docs.append(b"w000007 w000008")
    docs.append(b"w262151 w262153")
    docs += [b" ".join(b"w%06d" % int(i) for i in rng.integers(0, V, 6)) for _ in range(nshort)]
    return docs


@pytest.fixture(scope="module")
def wide():
    data, off = docs_to_arrays(wide_docs())
    return dict(args=(data, off), ref=make_ref(data, off))


def test_vocabulary_wider_than_2_18(engine, wide):
    """300000 terms: ranks 7 and 7 + 2^18 must not be taken for each other"""
    ref = wide["ref"]
    assert ref.words[7] == b"w000007" and ref.words[7 + (1 << 18)] == b"w262151" and len(ref.words) == 300000
    engine.run_host(*wide["args"])
    seeds = [8, 9]                                  # "w000007 w000008" against "w262151 w262153"
    want = ref.run(2, 3, 4, seeds)
    check(engine.kmeans(2, 3, 4, seeds), want)
    assert want["label"][ref.pos[7]] in (0, 1) and want["iterations"] == 3
    check(engine.kmeans(2, 20, 3), ref.run(2, 20, 3))


def test_wide_matrix(engine, wide):
    """V = 300000 and K = 256: a matrix of 614 MB under the default budget of 1024, the widest
    this suite allocates.  Element and byte offsets stay below 2^32 here (a matrix past 2^32
    bytes is over the default budget); the kernels compute them in 64 bits throughout."""
    ref = wide["ref"]
    engine.run_host(*wide["args"])
    seeds = ref.order[9:9 + 256]                    # short documents: the first pass's centroids are small
    want = ref.run(256, 2, 2, seeds)
    check(engine.kmeans(256, 2, 2, seeds), want)
    assert engine.kmeans_info()["matrix_bytes"] == 300000 * 256 * 8
    assert sum(1 for c in want["size"] if c > 1) > 3


def long_docs():
    w15, w16 = b"abcdefghijklmno", b"abcdefghijklmnop"
    a, b_, c = w16 + b"q" * 24, w16 + b"r" * 24, b"L" * 300
    return [a + b" x " + w15 + b" " + c, b_ + b" y " + a + b" " + a, b"x y z ab\0cd ab " + b"M" * 299,
            w16 + b" " + a + b" " + w15 + b" " + b_, b"zz " + c + b" " + b"L" * 299 + b" y", b_ + b" zz " + w16 + b" " + w16]


def test_long_terms(engine):
    """terms of 16, 40, 299 and 300 bytes among the centroids' best terms (two share their
    first 16 bytes): the words byte for byte"""
    data, off = docs_to_arrays(long_docs())
    ref = make_ref(data, off)
    engine.run_host(data, off)
    for k in (1, 2, 3):
        want = ref.run(k, 20, 64)
        res = engine.kmeans(k, 20, 64)
        check(res, want)
        assert any(len(w) >= 16 for ws in res["words"] for w in ws)
    assert max(len(w) for ws in res["words"] for w in ws) == 300


def test_budget(c2, monkeypatch):
    """1 MiB: K * V * 8 = 8 * 27478 * 8 is over it, K = 2 is under; the refusal leaves the
    context as it was"""
    monkeypatch.setenv("TFIDF_KMEANS_MB", "1")
    with tfidf_abi.Engine(0) as e:
        e.run_host(*c2["args"])
        before = e.similar(10)
        a0 = e.alloc_counters()
        assert rc_of(e.kmeans, 8) == tfidf_abi.E_CAPACITY
        assert e.alloc_counters() == a0                                 # before any device work
        after = e.similar(10)
        for name in ("doc", "nnb", "nb_doc", "nb_shared"):
            assert np.array_equal(before[name], after[name])
        assert np.array_equal(bits(before["nb_score"]), bits(after["nb_score"]))
        check(e.kmeans(2, 20, 10), c2["ref"].run(2, 20, 10))


def test_state_and_arguments(c2):
    with tfidf_abi.Engine(0) as e:
        assert rc_of(e.kmeans, 2) == tfidf_abi.E_STATE                  # before a run
        e.run_host(*c2["args"])
        lib = tfidf_abi.lib()
        p, c = tfidf_abi.KmeansParams(), tfidf_abi.Clusters()
        p.size, p.k, p.nterms = C.sizeof(p), 2, 3
        assert lib.tfidf_kmeans(e.h, None, C.byref(c)) == tfidf_abi.E_INVAL
        assert lib.tfidf_kmeans(e.h, C.byref(p), None) == tfidf_abi.E_INVAL
        p.size = C.sizeof(p) - 8
        assert lib.tfidf_kmeans(e.h, C.byref(p), C.byref(c)) == tfidf_abi.E_INVAL
        p.size = C.sizeof(p)
        assert rc_of(e.kmeans, 2, seeds=[1]) == tfidf_abi.E_INVAL       # nseeds != k
        assert rc_of(e.kmeans, 2, seeds=[1, 2, 3]) == tfidf_abi.E_INVAL
        assert rc_of(e.kmeans, 2, nterms=65) == tfidf_abi.E_INVAL
        assert lib.tfidf_kmeans(e.h, C.byref(p), C.byref(c)) == 0 and c.k == 2 and c.t == 3
        lib.tfidf_clusters_free(C.byref(c))
        model = e.model_export()
        e.model_import(model)
        assert rc_of(e.kmeans, 2) == tfidf_abi.E_STATE                  # a model holds no documents


def test_leaves_the_result_and_allocates_once(engine, c2):
    engine.run_host(*c2["args"])
    text, nb = engine.text(), engine.similar(10)
    first = engine.kmeans(8, 20, 10)
    engine.kmeans(3, 2, 64, [5, 6, 7])
    engine.kmeans(8, 20, 10)
    a0 = engine.alloc_counters()
    second = engine.kmeans(8, 20, 10)
    third = engine.kmeans(3, 2, 64, [5, 6, 7])
    assert engine.alloc_counters() == a0                                # no device allocation
    same_result(first, second)
    check(third, c2["ref"].run(3, 2, 64, [5, 6, 7]))
    assert engine.text() == text
    nb2 = engine.similar(10)
    for name in ("doc", "nnb", "nb_doc", "nb_shared"):
        assert np.array_equal(nb[name], nb2[name])
    assert np.array_equal(bits(nb["nb_score"]), bits(nb2["nb_score"])) and np.array_equal(bits(nb["norm"]), bits(nb2["norm"]))


@pytest.mark.parametrize("split", ["1", "7", "1024"])
def test_result_does_not_depend_on_the_launch_shape(topical, split, monkeypatch):
    """TFIDF_KMEANS_SPLIT: 1, 7 or 1024 update workgroups per cluster (term ranges of all, a
    seventh or none to one of the 496 terms) give the reference's bits"""
    monkeypatch.setenv("TFIDF_KMEANS_SPLIT", split)
    with tfidf_abi.Engine(0) as e:
        e.run_host(*topical["args"])
        check(e.kmeans(6, 20, 10), topical["ref"].run(6, 20, 10))
        assert e.kmeans_info()["split"] == int(split)


def test_cli_clusters(tmp_path):
    case = "g5_w3"
    g = load_golden(case)
    ref = make_ref(g["data"], g["off"])
    shutil.copytree(os.path.join(GOLDEN, case, "input"), tmp_path / "input")
    p = subprocess.run([tfidf_abi.CLI_PATH, "--clusters", "3"], cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    want = cluster_lines(ref.run(3, 20, 10))
    assert want.count(b"\n") == 3 + len(ref.order)
    assert (tmp_path / "clusters.txt").read_bytes() == want
    assert (tmp_path / "output.txt").read_bytes() == g["output"]
    seeds = [ref.order[-1], ref.order[0], ref.order[3]]
    (tmp_path / "seeds.txt").write_bytes(b"".join(b"%d\n" % d for d in seeds))
    p = subprocess.run([tfidf_abi.CLI_PATH, "--clusters", "3", "--clusters-iter", "2", "--clusters-seeds", "seeds.txt",
                        "--clusters-terms", "4", "--clusters-file", "c.txt"], cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "c.txt").read_bytes() == cluster_lines(ref.run(3, 2, 4, seeds))
    os.remove(tmp_path / "clusters.txt")
    q = subprocess.run([tfidf_abi.CLI_PATH, "--shards", "2", "--clusters", "3"], cwd=tmp_path, capture_output=True, timeout=120)
    assert q.returncode != 0 and b"one shard only" in q.stderr and not (tmp_path / "clusters.txt").exists()
    for bad in ("0", "257"):
        q = subprocess.run([tfidf_abi.CLI_PATH, "--clusters", bad], cwd=tmp_path, capture_output=True, timeout=120)
        assert q.returncode == 2
