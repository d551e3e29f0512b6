"""TFIDF_AN_UTF8 on the host (include/tfidf.h, section "analyzer"): the generated tables, and
tfidf_analyze_host's byte-wise sequence map against tests/utf8_ref.py, the definition in plain
Python.  No GPU call."""
import ctypes as C
import os
import subprocess
import sys
import unicodedata

import numpy as np
import pytest

import tfidf_abi
import utf8_ref
from conftest import REPO
from utf8_ref import enc, exhaustive_23, exhaustive_4

SEPS = [0x20, 0x09, 0x0A, 0x0B, 0x0C, 0x0D]
COMBOS = [(False, False), (True, False), (False, True), (True, True)]


def arr(b: bytes) -> np.ndarray:
    return np.frombuffer(b, dtype=np.uint8).copy()


def host(raw: bytes, off=None, **kw) -> bytes:
    kw.setdefault("utf8", True)
    return tfidf_abi.analyze_host(arr(raw), np.array([0, len(raw)] if off is None else off, dtype=np.uint64), **kw).tobytes()


# ---- the tables ----

def test_header_equals_the_generator():
    t = utf8_ref.tables()
    if t["version"] != unicodedata.unidata_version:
        pytest.skip("the header holds Unicode %s, this Python %s" % (t["version"], unicodedata.unidata_version))
    p = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "gen_utf8_tab.py"), "-"], capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout.decode("utf-8") == utf8_ref.header_text()


def test_table_shape():
    """what the kernel's lookup relies on: sorted, disjoint, strides 1 and 2, no range across a
    change of the UTF-8 length, same-length lowercase that has no lowercase itself, and a direct
    two-byte table that says what the ranges say"""
    t = utf8_ref.tables()
    assert t["version"] == "13.0.0" and len(t["fold"]) == 1342 and len(t["blank"]) == 8348 and len(t["runs"]) == 329
    for rows in (t["ranges"], t["runs"]):
        for a, b in zip(rows[:-1], rows[1:]):
            assert a[0] <= a[1] < b[0]
        for r in rows:
            assert r[0] >= 0x80 and utf8_ref.u8len(r[0]) == utf8_ref.u8len(r[1])
    assert all(r[2] in (1, 2) and (r[1] - r[0]) % r[2] == 0 for r in t["ranges"])
    for cp, lc in t["fold"].items():
        assert lc != cp and lc >= 0x80 and utf8_ref.u8len(lc) == utf8_ref.u8len(cp) and lc not in t["fold"]
    assert sorted(cp for cp in t["fold"] if cp in t["blank"]) == list(range(0x24B6, 0x24D0))
    assert len(t["t2"]) == 1920
    for cp in range(0x80, 0x800):
        assert t["t2"][cp - 0x80] == t["fold"].get(cp, 0) | (0x8000 if cp in t["blank"] else 0)
    by_len = lambda s: [sum(1 for cp in s if utf8_ref.u8len(cp) == k) for k in (2, 3, 4)]
    assert by_len(t["fold"]) == [440, 677, 225] and by_len(t["blank"]) == [133, 4286, 3929]


# ---- fixed expectations ----

def test_fixed_expectations():
    for up, lo in ((0xC9, 0xE9), (0x3A3, 0x3C3), (0x416, 0x436), (0x1E00, 0x1E01), (0x10A0, 0x2D00), (0x10400, 0x10428)):
        assert host(enc(up), lower=True) == enc(lo)
        assert host(enc(up), lower=True, punct=True) == enc(lo)
        assert host(enc(up), punct=True) == enc(up) and host(enc(up)) == enc(up)
        assert host(enc(up), lower=True, utf8=False) == enc(up)
        assert host(enc(lo), lower=True, punct=True) == enc(lo)
    assert len(utf8_ref.EXCLUDED) == 25
    for cp in utf8_ref.EXCLUDED:
        assert len(chr(cp).lower().encode("utf-8")) != len(enc(cp)) or len(chr(cp).lower()) != 1
        assert host(enc(cp), lower=True) == enc(cp)
    for cp in (0xA0, 0x2003, 0x201C, 0x201D, 0x2018, 0x2019, 0x2013, 0x2014, 0x2026, 0xAB, 0xBB, 0xBF, 0xA1, 0x20AC, 0xA9, 0xB0, 0x1F600):
        assert host(b"a" + enc(cp) + b"b", punct=True) == b"a" + b" " * len(enc(cp)) + b"b"
        assert host(enc(cp), lower=True) == enc(cp) and host(enc(cp), punct=True, utf8=False) == enc(cp)
    for cp in (0x200B, 0xAD, 0x301):
        assert host(b"a" + enc(cp) + b"b", lower=True, punct=True) == b"a" + enc(cp) + b"b"
    assert host(enc(0x24B6), lower=True) == enc(0x24D0)                   # in both tables: the blank wins
    assert host(enc(0x24B6), lower=True, punct=True) == b"   " and host(enc(0x24B6), punct=True) == b"   "
    assert host(enc(0x3A3, 0x3C2), lower=True) == enc(0x3C3, 0x3C2)       # no final sigma
    text = "“Running” ÜBER —the… «the» naïve cafÉ".encode("utf-8")
    got = host(text, lower=True, punct=True, stem=True, stop=["über".encode("utf-8")])
    assert got.split() == [b"run", b"the", b"the", "naïve".encode("utf-8"), "café".encode("utf-8")]
    assert len(got) == len(text)


# ---- random inputs ----

def random_case(rng):
    frags = utf8_ref.fragments()
    ascii_ = [bytes([c]) for c in b"ABCDEXYZabcdexyz0123459.,;:!?()'\"-_/\x00\x7f"] + [bytes([s]) for s in SEPS] * 4
    parts = []
    for _ in range(int(rng.integers(0, 160))):
        r = rng.random()
        pool = frags if r < 0.45 else ascii_
        parts.append(pool[int(rng.integers(len(pool)))])
    if rng.random() < 0.3:
        parts.insert(int(rng.integers(len(parts) + 1)), b"running" + enc(0x201D) + b" " + enc(0x41C) * 40)   # a long token too
    data = arr(b"".join(parts))
    n = len(data)
    lead = int(rng.integers(0, n // 4 + 1)) if rng.random() < 0.5 else 0
    trail = int(rng.integers(0, n // 4 + 1)) if rng.random() < 0.5 else 0
    ndocs = int(rng.integers(0, 7))
    cuts = np.sort(rng.integers(lead, n - trail + 1, max(ndocs - 1, 0))) if ndocs else np.zeros(0, dtype=np.int64)
    if ndocs and rng.random() < 0.5 and len(cuts) > 1:
        cuts[1] = cuts[0]               # an empty document
    off = np.array(([lead] + list(cuts) + [n - trail]) if ndocs else [lead], dtype=np.uint64)
    return data, off


STOP = [enc(0xFC) + b"ber", enc(0x44D, 0x442, 0x43E), enc(0x436), enc(0xE9), b"the", b"ab", b"e"]


@pytest.mark.parametrize("lower,punct", COMBOS)
@pytest.mark.parametrize("min_len,stem", [(0, False), (3, False), (2, True)])
def test_random_inputs(lower, punct, min_len, stem):
    rng = np.random.default_rng(2000 + 8 * min_len + 2 * lower + punct)
    changed = 0
    for _ in range(25):
        data, off = random_case(rng)
        stats = {}
        kw = dict(lower=lower, punct=punct, min_len=min_len, stop=STOP, stem=stem)
        ref = utf8_ref.analyze(data, off, stats=stats, **kw)
        got = tfidf_abi.analyze_host(data, off, utf8=True, **kw)
        assert np.array_equal(got, ref), (data.tobytes(), off.tolist())
        assert np.array_equal(tfidf_abi.analyze_host(data, off, utf8=True, in_place=True, **kw), ref)
        if not stem:
            assert np.array_equal(tfidf_abi.analyze_host(got, off, utf8=True, **kw), ref)   # idempotent
        changed += stats["utf8_changed"]
        if not (lower or punct):        # the flag alone changes nothing
            assert stats["utf8_changed"] == 0
            assert np.array_equal(got, tfidf_abi.analyze_host(data, off, utf8=False, **kw))
    assert (changed > 100) == (lower or punct)


# ---- exhaustive ----

@pytest.mark.parametrize("make", [exhaustive_23, exhaustive_4])
def test_exhaustive(make):
    raw = make()
    data, off = arr(raw), np.array([0, len(raw)], dtype=np.uint64)
    for lower, punct in COMBOS[1:]:
        stats = {}
        ref = utf8_ref.analyze(data, off, lower=lower, punct=punct, stats=stats)
        assert stats["utf8_changed"] > 200
        got = tfidf_abi.analyze_host(data, off, lower=lower, punct=punct, utf8=True)
        bad = np.flatnonzero(got != ref)
        assert len(bad) == 0, (bad[:8], raw[bad[0] - 4:bad[0] + 4])


# ---- cuts ----

def test_cuts():
    for raw, off, want, need in utf8_ref.cut_cases():
        for kw in (dict(lower=True), dict(punct=True), dict(lower=True, punct=True)):
            exp = want if kw.get(need) else raw
            assert host(raw, off, **kw) == exp, (raw, off, kw)
            assert utf8_ref.analyze(arr(raw), off, **kw).tobytes() == exp


# ---- ASCII-only input, flags ----

def test_ascii_only_input_is_unchanged_by_the_flag():
    rng = np.random.default_rng(9)
    raw = bytes(rng.integers(0, 0x80, 3000, dtype=np.uint8))
    data, off = arr(raw), np.array([5, 700, 700, 2990], dtype=np.uint64)
    for lower, punct in COMBOS:
        for min_len, stop, stem in ((0, (), False), (3, [b"the", b"ab"], False), (2, [b"ab"], True)):
            kw = dict(lower=lower, punct=punct, min_len=min_len, stop=stop, stem=stem)
            stats = {}
            ref = utf8_ref.analyze(data, off, stats=stats, **kw)
            assert stats["utf8_changed"] == 0
            assert np.array_equal(tfidf_abi.analyze_host(data, off, utf8=True, **kw), ref)
            assert np.array_equal(tfidf_abi.analyze_host(data, off, utf8=False, **kw), ref)


def test_flag_acceptance():
    assert tfidf_abi.AN_UTF8 == 16
    for flags, rc in ((16, 0), (17, 0), (18, 0), (19, 0), (4, tfidf_abi.E_INVAL), (8, tfidf_abi.E_INVAL), (32, tfidf_abi.E_INVAL),
                      (16 | 4, tfidf_abi.E_INVAL), (16 | 32, tfidf_abi.E_INVAL)):
        a, keep = tfidf_abi.analyzer()
        a.flags = flags
        assert tfidf_abi.analyzer_check(a) == rc, flags
    a, keep = tfidf_abi.analyzer(lower=True, utf8=True)
    assert a.flags == 17
    assert C.sizeof(tfidf_abi.AnalyzeInfoUtf8) == 80 and tfidf_abi.AnalyzeInfoUtf8.utf8_changed.offset == 72
