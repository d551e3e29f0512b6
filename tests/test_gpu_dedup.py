"""tfidf_minhash / tfidf_near_dups on the GPU (csrc/dedup.hip, csrc/engine_dedup.cpp) against the
plain-Python reference tests/dedup_ref.py: every integer, every u32 of the signatures and the u64
bits of every jaccard are equal.  The reference's own agreement with the plain-C host twin, and
that it finds the planted pairs of the families corpus, is established without a GPU in
test_dedup_cpu.py."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import dedup_ref as R
import oracle_py
import prune_ref
import tfidf_abi
import tfidf_configs
from conftest import GOLDEN, PKG, REPO, golden_cases
from helpers import device_corpus, docs_to_arrays, load_golden

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (64, 1), (128, 4), (256, 8), (96, 96), (192, 3), (129, 1), (160, 5)]   # one to four hashes per lane
THRESHOLDS = [0.0, 0.5, 1.0]


def big_pairs() -> int:
    with open(os.path.join(PKG, "csrc", "kernels.h")) as f:
        return int(re.search(r"#define\s+DD_BIG_PAIRS\s+(\d+)u", f.read()).group(1))


def raises(rc, fn, *a, **kw):
    with pytest.raises(tfidf_abi.TfidfError) as ei:
        fn(*a, **kw)
    assert ei.value.rc == rc, ei.value


def check(engine, ref: R.DRef, H, r, seed, thr, want=None):
    """near_dups and minhash of the resident result against the reference; returns the reference's answer"""
    want = want if want is not None else ref.near_dups(H, r, seed, thr)
    got = engine.near_dups(thr, H, r, seed)
    R.assert_same_dups(got, want)
    info = engine.dedup_info()
    assert (info["ndocs"], info["nhashes"], info["rows"]) == (want["ndocs"], want["nhashes"], want["rows"])
    assert (info["ncand"], info["nedges"], info["ngroups"]) == (want["ncand"], want["nedges"], want["ngroups"])
    assert info["clusterable"] == sum(1 for n in ref.n if n) and info["sig_bytes"] == want["ndocs"] * want["nhashes"] * 4
    return want


def check_sig(engine, ref: R.DRef, H, seed, sig=None):
    got = engine.minhash(H, seed)
    assert got["nhashes"] == H and [int(d) for d in got["doc"]] == ref.order and [int(n) for n in got["npairs"]] == ref.n
    assert np.array_equal(got["sig"], sig if sig is not None else ref.signatures(H, seed))


def run_docs(engine, docs):
    data, off = docs_to_arrays(docs)
    engine.run_host(data, off)
    ids = list(range(1, len(docs) + 1))
    return R.DRef(oracle_py.run(data, off), ids)


@pytest.mark.parametrize("case", golden_cases())
def test_goldens_vs_reference(engine, case):
    g = load_golden(case)
    engine.run_host(g["data"], g["off"])
    ref = R.DRef(oracle_py.run(g["data"], g["off"]), list(range(1, len(g["off"]))))
    for H, r in SHAPES:
        sig = ref.signatures(H, 1)
        check_sig(engine, ref, H, 1, sig)
        for thr in THRESHOLDS:
            check(engine, ref, H, r, 1, thr)
    check(engine, ref, 0, 0, 0, 0.8)                                      # the defaults


def test_families(engine):
    """(a): equality, planted within kept, and the groups are the families"""
    docs, families = R.families_corpus()
    ref = run_docs(engine, docs)
    planted = R.planted_pairs(ref, families, 0.9)
    assert len(planted) >= 16
    want = check(engine, ref, 128, 4, 1, 0.8)
    got = engine.near_dups(0.8, 128, 4, 1)
    kept = set(zip(got["a_pos"].tolist(), got["b_pos"].tolist()))
    assert set(planted) <= kept
    assert got["ngroups"] == 8
    for fam in families:
        assert {int(got["group"][ref.pos[d]]) for d in fam} == {min(ref.pos[d] for d in fam)}
    for d in range(41, 49):
        assert int(got["group"][ref.pos[d]]) == ref.pos[d]
    check_sig(engine, ref, 128, 1, want["sig"])


def test_rejection_is_exercised(engine):
    """(b): r = 1 proposes the overlapping neighbours, verification discards them"""
    ref = run_docs(engine, R.overlap_corpus() + R.identical_corpus(3))
    want = check(engine, ref, 64, 1, 1, 0.9)
    assert want["ncand"] > want["nedges"] > 0
    info = engine.dedup_info()
    assert info["ncand"] > info["nedges"] > 0


def test_identical_documents(engine):
    """(c): 70 identical documents, more than a wave"""
    ref = run_docs(engine, R.identical_corpus(70))
    check(engine, ref, 128, 4, 1, 1.0)
    got = engine.near_dups(1.0, 128, 4, 1)
    assert got["nedges"] == 69 and got["ngroups"] == 1 and set(got["group"].tolist()) == {0}
    assert np.array_equal(got["jaccard"].view(np.uint64), np.full(69, np.float64(1.0).view(np.uint64)))
    assert (got["same"] == 128).all()


def test_both_sides_of_the_big_threshold(engine):
    """(d): two documents of DD_BIG_PAIRS - 1, DD_BIG_PAIRS and DD_BIG_PAIRS + 1 distinct terms"""
    big = big_pairs()
    for n, nbig in ((big - 1, 0), (big, 0), (big + 1, 2)):
        ref = run_docs(engine, R.big_corpus(n))
        assert ref.n == [n, n]
        want = check(engine, ref, 128, 4, 1, 0.5)
        assert engine.dedup_info()["big_docs"] == nbig, n
        check(engine, ref, 256, 256, 9, 0.0)
        assert engine.dedup_info()["big_docs"] == nbig, n
        check(engine, ref, 160, 5, 3, 0.5)                                  # three hashes per lane: k_dd_sig<3> / k_dd_sig_big<3>
        assert engine.dedup_info()["big_docs"] == nbig, n
        check_sig(engine, ref, 128, 1, want["sig"])
        assert engine.dedup_info()["big_docs"] == nbig, n
        # one candidate at r = 1 (the shared minimum of some function), verified exactly
        w1 = check(engine, ref, 64, 1, 1, 0.0)
        assert w1["nedges"] == 1 and w1["edges"][0]["shared"] == n - 100 and w1["edges"][0]["uni"] == n + 100
    # a big document against a small one: the verification's workgroup form with unequal lists
    small = b" ".join(R.big_corpus(big + 1)[0].split()[:300])
    ref = run_docs(engine, [R.big_corpus(big + 1)[0], small, small])
    w = check(engine, ref, 256, 1, 1, 0.0)
    assert engine.dedup_info()["big_docs"] == 1
    assert [(e["a_pos"], e["b_pos"], e["shared"], e["uni"]) for e in w["edges"]] == [(0, 1, 300, big + 1), (1, 2, 300, 300)]


def test_edge_cases(engine):
    """(e): empty documents, a one-term document, N = 1, documents emptied by a prune"""
    docs = [b"", b"solo", b"  \n", b"aa bb cc", b"aa bb cc", b"zz", b"solo"]
    data, off = docs_to_arrays(docs)
    ids = list(range(1, len(docs) + 1))
    ora = oracle_py.run(data, off)
    engine.run_host(data, off)
    ref = R.DRef(ora, ids)
    want = check(engine, ref, 128, 4, 1, 0.5)
    assert want["nedges"] == 2
    got = engine.minhash(128, 1)
    for d in (1, 3):
        assert (got["sig"][ref.pos[d]] == 0xFFFFFFFF).all() and got["npairs"][ref.pos[d]] == 0
    # prune: df >= 2 empties doc6; it appears in no edge and is its own group
    engine.prune(2)
    pr = prune_ref.prune(ora, 2, 0, 0)
    pref = R.DRef(pr, ids)
    assert pref.n[pref.pos[6]] == 0
    got = engine.near_dups(0.5, 128, 4, 1)
    R.assert_same_dups(got, pref.near_dups(128, 4, 1, 0.5))
    p6 = pref.pos[6]
    assert p6 not in set(got["a_pos"].tolist()) | set(got["b_pos"].tolist()) and int(got["group"][p6]) == p6
    for one in ([b"one two"], [b""]):                                       # N = 1
        ref = run_docs(engine, one)
        w = check(engine, ref, 16, 4, 7, 0.0)
        assert w["ncand"] == 0 and w["group"] == [0]
        check_sig(engine, ref, 16, 7)


def long_docs():
    long_a = b"x" * 16 + b"tail-one"
    long_b = b"x" * 16 + b"tail-two"
    head = b"a" * 15 + b" " + b"b" * 16 + b" " + b"c" * 17 + b" "
    tail = b" caf\xc3\xa9 \xff\xfe na\xefve"
    return [head + long_a + tail, head + long_b + tail, head + long_a + tail, b"L" * 300 + b" " + long_b]


def test_long_and_odd_terms(engine):
    """(f): terms of 15, 16 and 17 bytes, two long terms sharing 16 bytes, bytes >= 0x80, and a
    device corpus at an unaligned base"""
    docs = long_docs()
    data, off = docs_to_arrays(docs)
    ref = R.DRef(oracle_py.run(data, off), [1, 2, 3, 4])
    engine.run_host(data, off)
    want = check(engine, ref, 64, 2, 3, 0.0)
    assert any(e["jaccard"] == 1.0 for e in want["edges"])
    check_sig(engine, ref, 64, 3, want["sig"])
    with device_corpus(data, off, shift=3) as c:
        engine.run_corpus(c)
        check(engine, ref, 64, 2, 3, 0.0, want)
        check_sig(engine, ref, 64, 3, want["sig"])
        check(engine, ref, 256, 1, 5, 0.5)


def test_state(engine):
    """(g): the result is not disturbed; prune then near_dups; a run afterwards; allocations"""
    g = load_golden("g5_w3")
    ids = list(range(1, len(g["off"])))
    ora = oracle_py.run(g["data"], g["off"])
    ref = R.DRef(ora, ids)
    with tfidf_abi.Engine(0) as e:
        raises(tfidf_abi.E_STATE, e.near_dups, 0.5)                         # before a run
        raises(tfidf_abi.E_STATE, e.minhash)
        e.run_host(g["data"], g["off"])
        text, f0 = e.text(), e.fetch()
        want = check(e, ref, 128, 2, 1, 0.1)
        check_sig(e, ref, 128, 1, want["sig"])
        f1 = e.fetch()
        assert e.text() == text == g["output"]
        for k in ("doc", "term", "count", "docsize", "df"):
            assert np.array_equal(f0[k], f1[k])
        assert np.array_equal(f0["score"].view(np.uint64), f1["score"].view(np.uint64))
        a0 = e.alloc_counters()                                             # a repeated identical call
        check(e, ref, 128, 2, 1, 0.1, want)
        check_sig(e, ref, 128, 1, want["sig"])
        assert e.alloc_counters() == a0
        e.reweight("log", "smooth", "l2")                                   # scores play no part
        check(e, ref, 128, 2, 1, 0.1, want)
        e.prune(2)
        pref = R.DRef(prune_ref.prune(ora, 2, 0, 0), ids)
        check(e, pref, 128, 2, 1, 0.1)
        e.run_host(g["data"], g["off"])                                     # the unpruned answer again
        check(e, ref, 128, 2, 1, 0.1, want)
        # parameter errors leave *out zeroed and the state alone
        bad = tfidf_abi.dedup_params(128, 3, 1, 0.5)
        raises(tfidf_abi.E_INVAL, e.near_dups, params=bad)
        raises(tfidf_abi.E_INVAL, e.minhash, params=tfidf_abi.dedup_params(300, 1, 1, 0.5))
        d = tfidf_abi.Dups()
        d.ndocs = 5
        assert tfidf_abi.lib().tfidf_near_dups(e.h, C.byref(bad), C.byref(d)) == tfidf_abi.E_INVAL and d.ndocs == 0
        assert tfidf_abi.lib().tfidf_near_dups(e.h, None, C.byref(d)) == tfidf_abi.E_INVAL
        check(e, ref, 128, 2, 1, 0.1, want)
        e.model_import(e.model_export())
        raises(tfidf_abi.E_STATE, e.near_dups, 0.5)                         # a model-only context
        raises(tfidf_abi.E_STATE, e.minhash)


CAPACITY_CHILD = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import dedup_ref as R, tfidf_abi
from helpers import docs_to_arrays
data, off = docs_to_arrays(R.identical_corpus(70))
with tfidf_abi.Engine(0) as e:
    e.run_host(data, off)
    try:
        e.near_dups(1.0, 256, 1, 1)      # 70 * 256 * 4 + 256 * 69 * 16 = 354 304 bytes: inside 1 MiB
        small_ok = True
    except tfidf_abi.TfidfError as x:
        small_ok = False
    docs = R.identical_corpus(70) * 60   # 4200 documents: 4200 * 1024 bytes of signatures alone exceed 1 MiB
    data, off = docs_to_arrays(docs)
    e.run_host(data, off)
    rcs = []
    for fn in (lambda: e.near_dups(1.0, 256, 1, 1), lambda: e.minhash(256, 1)):
        try:
            fn()
            rcs.append(0)
        except tfidf_abi.TfidfError as x:
            rcs.append(x.rc)
    print("RESULT", small_ok, rcs[0], rcs[1])
"""


def test_capacity_in_a_fresh_process():
    """(g): TFIDF_DEDUP_MB is read at tfidf_open: corpus (c) at H = 256 under a 1 MiB budget"""
    code = CAPACITY_CHILD % (os.path.join(PKG, "python"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests"))
    env = dict(os.environ, TFIDF_DEDUP_MB="1")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr
    line = [x for x in p.stdout.splitlines() if x.startswith("RESULT")][-1].split()
    # 70 documents: 70 * 1024 + 256 * 69 * 16 = 354 304 bytes fit; 4200 documents do not
    assert line[1:] == ["True", str(tfidf_abi.E_CAPACITY), str(tfidf_abi.E_CAPACITY)], p.stdout


@pytest.fixture(scope="module")
def c2():
    p = tfidf_configs.plan("c2", scale=0.002)
    data, off = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
    ora = oracle_py.run(data, off, p["doc_ids"], p["ndocs_total"])
    return dict(p=p, ora=ora, args=(data, off, p["doc_ids"], p["ndocs_total"]))


def test_synthetic_c2(engine, c2):
    """(h): config 2 at scale 0.002 at (128, 2) and (128, 4)"""
    ora = c2["ora"]
    assert (len(c2["args"][1]) - 1, ora["npairs"]) == (200, 122839)
    engine.run_host(*c2["args"])
    ref = R.DRef(ora, c2["p"]["doc_ids"])
    sig = ref.signatures(128, 1)
    check_sig(engine, ref, 128, 1, sig)
    for r in (2, 4):
        check(engine, ref, 128, r, 1, 0.0)
    check(engine, ref, 64, 1, 1, 0.05)


def cli(tmp_path, *args):
    return subprocess.run([tfidf_abi.CLI_PATH] + list(args), cwd=tmp_path, capture_output=True, timeout=120)


def test_cli(tmp_path):
    """(i): dups.txt byte-equal to the reference's rendering on a golden directory and on (a)"""
    case = "g5_w3"
    g = load_golden(case)
    ref = R.DRef(oracle_py.run(g["data"], g["off"]), list(range(1, len(g["off"]))))
    shutil.copytree(os.path.join(GOLDEN, case, "input"), tmp_path / "input")
    p = cli(tmp_path, "--near-dups", "0.05", "--near-dups-hashes", "64", "--near-dups-rows", "1", "--near-dups-seed", "5")
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "output.txt").read_bytes() == g["output"]
    want = ref.near_dups(64, 1, 5, 0.05)
    assert want["nedges"] > 0
    assert (tmp_path / "dups.txt").read_bytes() == R.dups_lines(want)
    p = cli(tmp_path, "--near-dups", "0.05", "--shards", "2")
    assert p.returncode == 2 and b"--near-dups" in p.stderr
    for bad in (["--near-dups", "1.5"], ["--near-dups", "x"], ["--near-dups", "0.5", "--near-dups-rows", "3"],
                ["--near-dups", "0.5", "--near-dups-hashes", "257"]):
        assert cli(tmp_path, *bad).returncode == 2, bad
    # (a), the defaults, another file name
    docs, families = R.families_corpus()
    fam = tmp_path / "fam"
    (fam / "input").mkdir(parents=True)
    for i, d in enumerate(docs):
        (fam / "input" / ("doc%d" % (i + 1))).write_bytes(d)
    p = cli(fam, "--near-dups", "0.8", "--near-dups-file", "pairs.txt")
    assert p.returncode == 0, p.stderr
    data, off = docs_to_arrays(docs)
    want = R.DRef(oracle_py.run(data, off), list(range(1, 49))).near_dups(0, 0, 0, 0.8)
    txt = (fam / "pairs.txt").read_bytes()
    assert txt == R.dups_lines(want) and txt.count(b"\ng") == 7 and txt.startswith(b"g0\t5\t")


def test_info_struct_honours_a_short_size():
    """(j): tfidf_last_dedup_info in the pattern of test_gpu_info_abi.py"""
    from test_gpu_info_abi import FILL, TAIL, assert_rejected, call, filled, size_of
    name, struct = "tfidf_last_dedup_info", tfidf_abi.DedupInfo
    S = C.sizeof(struct)
    with tfidf_abi.Engine(0) as e:
        assert call(name, None, filled(S, S), struct) == tfidf_abi.E_INVAL
        assert call(name, e.h, None, struct) == tfidf_abi.E_INVAL
        for size in (0, 4):
            assert_rejected(name, e.h, struct, size)
        buf = filled(S + TAIL, 8)
        assert call(name, e.h, buf, struct) == 0
        assert size_of(buf) == 8 and bytes(buf)[8:] == bytes([FILL]) * (S + TAIL - 8)
        buf = filled(S + TAIL, S + TAIL)
        assert call(name, e.h, buf, struct) == 0
        assert size_of(buf) == S and bytes(buf)[8:S] == bytes(S - 8) and bytes(buf)[S:] == bytes([FILL]) * TAIL
        data, off = docs_to_arrays(R.identical_corpus(5))
        e.run_host(data, off)
        e.near_dups(1.0, 64, 4, 1)
        buf = filled(S + TAIL, 24)                                          # size, ndocs, nhashes, rows, clusterable
        assert call(name, e.h, buf, struct) == 0 and size_of(buf) == 24
        assert list(C.cast(buf, C.POINTER(C.c_uint32))[2:6]) == [5, 64, 4, 5]
        assert bytes(buf)[24:] == bytes([FILL]) * (S + TAIL - 24)
