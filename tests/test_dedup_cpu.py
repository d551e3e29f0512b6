"""Host-only pieces of near-duplicate detection (include/tfidf.h, section "near duplicates"): the
pinned constants of the hashes, tfidf_result_minhash and tfidf_result_near_dups (plain C,
csrc/dedup_host.c) against the reference tests/dedup_ref.py on every golden and on the crafted
corpora, tfidf_dedup_check's rules one by one, and the condition the GPU tests rely on: on the
families corpus the reference proposes and keeps every planted pair.  No GPU call."""
import ctypes as C
import math

import numpy as np
import pytest

import dedup_ref as R
import oracle_py
import prune_ref
import tfidf_abi
from conftest import golden_cases
from helpers import docs_to_arrays, load_golden

SHAPES = [(1, 1), (64, 1), (128, 4), (256, 8), (96, 96)]
THRESHOLDS = [0.0, 0.5, 1.0]


def oracle_of(docs):
    data, off = docs_to_arrays(docs)
    return oracle_py.run(data, off), list(range(1, len(docs) + 1))


def both(ora, ids, H, r, seed, thr):
    ref = R.DRef(ora, ids).near_dups(H, r, seed, thr)
    got = tfidf_abi.result_near_dups(ora, ids, H, r, seed, thr)
    R.assert_same_dups(got, ref)
    return ref


def test_pinned_constants():
    assert R.fnv1a64(b"") == 0xCBF29CE484222325
    assert R.fnv1a64(b"a") == 0xAF63DC4C8601EC8C
    # mix64(1) step by step, so that no helper is trusted: 1 ^ (1 >> 30) = 1; times the first
    # constant is the constant itself; then the second xor-shift, multiply and the last xor-shift
    z = 1
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 % 2**64
    assert z == 0xBF58476D1CE4E5B9
    z ^= z >> 27
    z = z * 0x94D049BB133111EB % 2**64
    z ^= z >> 31
    assert z == 0x5692161D100B05E5 == R.mix64(1)
    assert R.mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF             # splitmix64's first output for seed 0
    assert R.mix64(0) == 0
    a, b = R.family(2, 1)
    assert a[0] == R.mix64(1 + 0x9E3779B97F4A7C15) | 1 and b[0] == R.mix64((1 + 2 * 0x9E3779B97F4A7C15) % 2**64) >> 32
    assert all(x & 1 for x in a) and all(0 <= x < 2**32 for x in b)


@pytest.mark.parametrize("case", golden_cases())
def test_host_equals_reference_on_goldens(case):
    g = load_golden(case)
    ora = oracle_py.run(g["data"], g["off"])
    ids = list(range(1, len(g["off"])))
    ref = R.DRef(ora, ids)
    for H, r in SHAPES:
        sig = ref.signatures(H, 1)
        got = tfidf_abi.result_minhash(ora, ids, H, 1)
        assert got["nhashes"] == H and got["ndocs"] == len(ids)
        assert [int(d) for d in got["doc"]] == ref.order and [int(n) for n in got["npairs"]] == ref.n
        assert np.array_equal(got["sig"], sig)
        for thr in THRESHOLDS:
            both(ora, ids, H, r, 1, thr)
    both(ora, ids, 0, 0, 0, 0.8)                                         # the defaults


def test_families_every_planted_pair_is_found():
    """what test_gpu_dedup.py relies on: with H = 128, r = 4, seed 1 the reference proposes and
    keeps every planted pair of Jaccard >= 0.9, and the groups are the families"""
    docs, families = R.families_corpus()
    assert len(docs) == 48
    ora, ids = oracle_of(docs)
    ref = R.DRef(ora, ids)
    planted = R.planted_pairs(ref, families, 0.9)
    assert len(planted) >= 16 and all(ref.jaccard(ref.order[a], ref.order[b]) >= 0.9 for a, b in planted)
    out = both(ora, ids, 128, 4, 1, 0.8)
    kept = {(e["a_pos"], e["b_pos"]) for e in out["edges"]}
    assert set(planted) <= kept
    # every pair of one family, neighbours or not, ends in one group; the unrelated documents alone
    assert out["ngroups"] == 8
    for fam in families:
        assert len({out["group"][ref.pos[d]] for d in fam}) == 1
        assert out["group"][ref.pos[fam[0]]] == min(ref.pos[d] for d in fam)
    for d in range(41, 49):
        assert out["group"][ref.pos[d]] == ref.pos[d]
    assert all(e["jaccard"] >= 0.8 for e in out["edges"])
    assert both(ora, ids, 0, 0, 0, 0.8)["edges"] == out["edges"]         # the defaults are these parameters


def test_rejection_corpus():
    """(b): r = 1 proposes the overlapping neighbours, the exact Jaccard of 1/3 rejects them"""
    ora, ids = oracle_of(R.overlap_corpus() + R.identical_corpus(3))
    out = both(ora, ids, 64, 1, 1, 0.9)
    assert out["ncand"] > out["nedges"] > 0


def test_identical_documents():
    ora, ids = oracle_of(R.identical_corpus(70))
    out = both(ora, ids, 128, 4, 1, 1.0)
    assert out["ncand"] == out["nedges"] == 69 and out["ngroups"] == 1 and set(out["group"]) == {0}
    assert all(e["same"] == 128 and e["jaccard"] == 1.0 and e["b_pos"] == e["a_pos"] + 1 for e in out["edges"])


def test_edge_corpora_and_prune():
    docs = [b"", b"solo", b"  \n", b"aa bb cc", b"aa bb cc", b"zz"]
    ora, ids = oracle_of(docs)
    out = both(ora, ids, 128, 4, 1, 0.5)
    ref = R.DRef(ora, ids)
    assert ref.n[ref.pos[1]] == 0 and ref.n[ref.pos[3]] == 0
    assert (out["sig"][ref.pos[1]] == 0xFFFFFFFF).all()
    assert out["nedges"] == 1 and out["ngroups"] == 1
    for d in (1, 2, 3, 6):
        assert out["group"][ref.pos[d]] == ref.pos[d]
    both(*oracle_of([b"one two"]), 16, 4, 7, 0.0)                        # N = 1
    both(*oracle_of([b"", b""]), 16, 4, 7, 0.0)                          # nothing but empty documents
    # pruned results: df >= 2 empties the documents that share no word
    pr = prune_ref.prune(ora, 2, 0, 0)
    out = both(pr, ids, 128, 4, 1, 0.5)
    assert out["nedges"] == 1 and R.DRef(pr, ids).n.count(0) == 4


def test_long_and_odd_terms():
    long_a = b"x" * 16 + b"tail-one"
    long_b = b"x" * 16 + b"tail-two"
    docs = [b"a" * 15 + b" " + b"b" * 16 + b" " + b"c" * 17 + b" " + long_a + b" caf\xc3\xa9 \xff\xfe",
            b"a" * 15 + b" " + b"b" * 16 + b" " + b"c" * 17 + b" " + long_b + b" caf\xc3\xa9 \xff\xfe",
            b"a" * 15 + b" " + b"b" * 16 + b" " + b"c" * 17 + b" " + long_a + b" caf\xc3\xa9 \xff\xfe"]
    ora, ids = oracle_of(docs)
    out = both(ora, ids, 64, 2, 3, 0.0)
    assert R.h0(long_a) != R.h0(long_b)
    assert any(e["jaccard"] == 1.0 for e in out["edges"])


def test_parameter_errors():
    ok = tfidf_abi.dedup_params(128, 4, 1, 0.8)
    assert tfidf_abi.dedup_check(ok) == 0
    assert tfidf_abi.dedup_check(tfidf_abi.dedup_params()) == 0          # nhashes 0: the defaults
    assert tfidf_abi.dedup_check(None) == tfidf_abi.E_INVAL
    bad = []
    p = tfidf_abi.dedup_params(128, 4, 1, 0.8)
    p.size -= 1
    bad.append(p)
    bad.append(tfidf_abi.dedup_params(257, 1, 1, 0.8))                   # H > 256
    bad.append(tfidf_abi.dedup_params(128, 0, 1, 0.8))                   # r == 0
    bad.append(tfidf_abi.dedup_params(128, 3, 1, 0.8))                   # r does not divide H
    bad.append(tfidf_abi.dedup_params(128, 256, 1, 0.8))                 # r > H
    for thr in (-0.0001, 1.0001, math.nan, math.inf, -math.inf):
        bad.append(tfidf_abi.dedup_params(128, 4, 1, thr))
    ora, ids = oracle_of([b"aa bb", b"aa bb"])
    for p in bad:
        assert tfidf_abi.dedup_check(p) == tfidf_abi.E_INVAL
        assert R.check_params(p.nhashes, p.rows, p.threshold) is False or p.size < C.sizeof(tfidf_abi.DedupParams)
        for fn in (tfidf_abi.result_near_dups, tfidf_abi.result_minhash):
            with pytest.raises(tfidf_abi.TfidfError) as ei:
                fn(ora, ids, params=p)
            assert ei.value.rc == tfidf_abi.E_INVAL
    for H, r in ((256, 256), (256, 1), (1, 1)):                          # the limits themselves pass
        assert tfidf_abi.dedup_check(tfidf_abi.dedup_params(H, r, 0, 0.0)) == 0
    assert tfidf_abi.dedup_check(tfidf_abi.dedup_params(1, 1, 0, 1.0)) == 0
    # NULL arguments, and *out zeroed on an error
    L = tfidf_abi.lib()
    d = tfidf_abi.Dups()
    d.ndocs = 7
    assert L.tfidf_result_near_dups(None, C.byref(ok), C.byref(d)) == tfidf_abi.E_INVAL and d.ndocs == 0
    assert L.tfidf_result_near_dups(None, C.byref(ok), None) == tfidf_abi.E_INVAL
    s = tfidf_abi.Signatures()
    s.ndocs = 7
    assert L.tfidf_result_minhash(None, C.byref(ok), C.byref(s)) == tfidf_abi.E_INVAL and s.ndocs == 0
    # a pair whose document is not among doc_id
    with pytest.raises(tfidf_abi.TfidfError) as ei:
        tfidf_abi.result_near_dups(ora, [1], params=ok)
    assert ei.value.rc == tfidf_abi.E_INVAL


def test_groups_union_find():
    L = tfidf_abi.lib()
    a = np.array([5, 3, 1, 7], dtype=np.uint32)
    b = np.array([6, 5, 2, 7], dtype=np.uint32)
    group = np.zeros(9, dtype=np.uint32)
    ng = C.c_uint32(99)
    assert L.tfidf_dedup_groups(9, a.ctypes.data, b.ctypes.data, 4, group.ctypes.data, C.byref(ng)) == 0
    assert group.tolist() == [0, 1, 1, 3, 4, 3, 3, 7, 8] and ng.value == 2
    assert (group.tolist(), 2) == R.DRef.groups(9, list(zip(a.tolist(), b.tolist())))
    bad = np.array([9], dtype=np.uint32)
    assert L.tfidf_dedup_groups(9, bad.ctypes.data, bad.ctypes.data, 1, group.ctypes.data, C.byref(ng)) == tfidf_abi.E_INVAL


def test_dups_lines_rendering():
    ora, ids = oracle_of([b"aa bb cc", b"dd", b"aa bb cc", b"aa bb cc dd"])
    out = both(ora, ids, 64, 1, 1, 0.7)
    txt = R.dups_lines(out)
    assert txt == R.dups_lines(tfidf_abi.result_near_dups(ora, ids, 64, 1, 1, 0.7))
    assert txt.startswith(b"g0\t") and b"doc1\tdoc3\t3\t3\t1.0000000000000000\n" in txt
