"""The analyzer on the host (include/tfidf.h, section "analyzer"): tfidf_analyze_host and
tfidf_analyzer_check against tests/analyze_ref.py, the definition in plain Python.  The host
function probes the stop-word table the device kernel probes (csrc/analyze_tab.h), so the
table's collisions are covered here.  No GPU call."""
import ctypes as C

import numpy as np
import pytest

import analyze_ref
import oracle_py
import tfidf_abi
from helpers import load_golden

SEPS = list(analyze_ref.SEPARATORS)
ALPHABET = ([ord(c) for c in "ABCDEXYZabcdexyz0123459"] + SEPS * 3 + [ord(c) for c in ".,;:!?()[]{}'\"-_/@#`~^|\x7f"]
            + [0x00, 0x01, 0xC3, 0xA9, 0xC3, 0x9F])   # two-byte UTF-8: e-acute, sharp s


def tokens_of(buf, off):
    out = []
    for b, e in zip(off[:-1], off[1:]):
        w = bytes(buf[int(b):int(e)])
        for s in SEPS:
            w = w.replace(bytes([s]), b" ")
        out += [t for t in w.split(b" ") if t]
    return out


def random_case(rng):
    n = int(rng.integers(0, 401))
    data = np.array([ALPHABET[i] for i in rng.integers(0, len(ALPHABET), n)], dtype=np.uint8)
    if rng.random() < 0.3 and n > 80:   # a long token
        at = int(rng.integers(0, n - 70))
        data[at:at + 70] = ord("q")
    lead = int(rng.integers(0, n // 4 + 1)) if rng.random() < 0.5 else 0
    trail = int(rng.integers(0, n // 4 + 1)) if rng.random() < 0.5 else 0
    ndocs = int(rng.integers(0, 7))
    cuts = np.sort(rng.integers(lead, n - trail + 1, max(ndocs - 1, 0))) if ndocs else np.zeros(0, dtype=np.int64)
    if ndocs and rng.random() < 0.5 and len(cuts) > 1:
        cuts[1] = cuts[0]               # an empty document
    off = np.array(([lead] + list(cuts) + [n - trail]) if ndocs else [lead], dtype=np.uint64)
    return data, off


@pytest.mark.parametrize("lower,punct", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("min_len", [0, 1, 2, 3, 64])
def test_random_inputs(lower, punct, min_len):
    rng = np.random.default_rng(1000 + 8 * min_len + 2 * lower + punct)
    matched = 0
    for _ in range(15):
        data, off = random_case(rng)
        plain = analyze_ref.analyze(data, off, lower, punct)
        toks = sorted(set(t for t in tokens_of(plain, off) if len(t) <= 64 and 0 not in t))
        stop = [toks[i] for i in rng.permutation(len(toks))[:len(toks) // 3]] + [b"zzz", b"e", b"ab"]
        stop += stop[:2]                # duplicates are allowed
        ref = analyze_ref.analyze(data, off, lower, punct, min_len, stop)
        got = tfidf_abi.analyze_host(data, off, lower, punct, min_len, stop)
        assert np.array_equal(got, ref), (data.tobytes(), off.tolist(), stop)
        assert np.array_equal(tfidf_abi.analyze_host(data, off, lower, punct, min_len, stop, in_place=True), ref)
        assert np.array_equal(tfidf_abi.analyze_host(got, off, lower, punct, min_len, stop), ref)   # idempotent
        matched += int(np.count_nonzero(ref != plain))
    assert matched > 0                  # the list and min_len blanked something


def test_identity():
    rng = np.random.default_rng(5)
    for min_len in (0, 1):
        data, off = random_case(rng)
        assert np.array_equal(tfidf_abi.analyze_host(data, off, min_len=min_len), data)


def test_byte_map():
    data = np.arange(256, dtype=np.uint8)
    off = np.array([0, 256], dtype=np.uint64)
    for lower in (False, True):
        for punct in (False, True):
            want = np.arange(256, dtype=np.uint8)
            if punct:
                for lo, hi in ((0x00, 0x08), (0x0E, 0x1F), (0x21, 0x2F), (0x3A, 0x40), (0x5B, 0x60), (0x7B, 0x7F)):
                    want[lo:hi + 1] = 0x20
            if lower:
                want[0x41:0x5B] = np.arange(0x61, 0x7B, dtype=np.uint8)
            assert np.array_equal(tfidf_abi.analyze_host(data, off, lower, punct), want)
            assert np.array_equal(analyze_ref.analyze(data, off, lower, punct), want)


def test_boundary_cut():
    data = np.frombuffer(b"x yab" + b"cdz w", dtype=np.uint8)
    off = np.array([0, 5, 10], dtype=np.uint64)
    assert tfidf_abi.analyze_host(data, off, stop=[b"abcd", b"yabcdz"]).tobytes() == b"x yabcdz w"
    assert tfidf_abi.analyze_host(data, off, stop=[b"yab"]).tobytes() == b"x    cdz w"
    data = np.frombuffer(b"..ab" + b"cd..", dtype=np.uint8)
    off = np.array([0, 4, 8], dtype=np.uint64)
    assert tfidf_abi.analyze_host(data, off, punct=True, stop=[b"abcd"]).tobytes() == b"  abcd  "
    assert tfidf_abi.analyze_host(data, off, punct=True, stop=[b"ab"]).tobytes() == b"    cd  "


@pytest.mark.parametrize("n", [1, 15, 16, 63, 64])
def test_stop_word_lengths(n):
    w = bytes(0x61 + (i * 7) % 26 for i in range(n))
    data = np.frombuffer(b"k " + w + b" " + w + b"k " + w, dtype=np.uint8)
    off = np.array([0, len(data)], dtype=np.uint64)
    got = tfidf_abi.analyze_host(data, off, stop=[w]).tobytes()
    assert got == b"k " + b" " * n + b" " + w + b"k " + b" " * n
    assert got == analyze_ref.analyze(data, off, stop=[w]).tobytes()


def test_long_token_never_matches():
    w = bytes(0x61 + i % 26 for i in range(64))
    data = np.frombuffer(w + b"x " + w, dtype=np.uint8)   # a 65-byte token whose first 64 bytes are a stop word
    off = np.array([0, len(data)], dtype=np.uint64)
    assert tfidf_abi.analyze_host(data, off, min_len=64, stop=[w]).tobytes() == w + b"x " + b" " * 64


def _an(**kw):
    a, keep = tfidf_abi.analyzer(kw.pop("lower", False), kw.pop("punct", False), kw.pop("min_len", 0), kw.pop("stop", ()))
    return a, keep


def test_check_errors():
    E = tfidf_abi.E_INVAL
    a, keep = _an(lower=True, punct=True, min_len=64, stop=[b"the", b"a" * 64, b"the"])
    assert tfidf_abi.analyzer_check(a) == 0
    assert tfidf_abi.lib().tfidf_analyzer_check(None) == E
    a, keep = _an()
    a.size = C.sizeof(tfidf_abi.Analyzer) - 1
    assert tfidf_abi.analyzer_check(a) == E                 # a short struct
    a, keep = _an()
    a.flags = 4
    assert tfidf_abi.analyzer_check(a) == E                 # an unknown flag bit
    a, keep = _an(min_len=65)
    assert tfidf_abi.analyzer_check(a) == E                 # min_len above TFIDF_AN_MAX_WORD
    a, keep = _an(stop=[b"a" * 65])
    assert tfidf_abi.analyzer_check(a) == E                 # a stop word of 65 bytes
    a, keep = _an(stop=[b"a", b"", b"b"])
    assert tfidf_abi.analyzer_check(a) == E                 # an empty stop word
    a, keep = _an(stop=[b"a\x00b"])
    assert tfidf_abi.analyzer_check(a) == E                 # a NUL
    for s in SEPS:
        a, keep = _an(stop=[b"a" + bytes([s]) + b"b"])
        assert tfidf_abi.analyzer_check(a) == E             # a separator
    a, keep = _an(stop=[b"ab", b"cd"])
    keep[1][1] = 3
    keep[1][2] = 2
    assert tfidf_abi.analyzer_check(a) == E                 # a non-monotone stop_off
    a, keep = _an(stop=[b"ab"])
    a.stop_bytes = None
    assert tfidf_abi.analyzer_check(a) == E                 # nstop > 0 with a NULL pointer
    a, keep = _an(stop=[b"ab"])
    a.stop_off = None
    assert tfidf_abi.analyzer_check(a) == E
    a, keep = _an(stop=[b"w%d" % i for i in range(4097)])
    assert tfidf_abi.analyzer_check(a) == E                 # more than TFIDF_AN_MAX_STOP words
    a, keep = _an(stop=[b"x" * 64] * 513)
    assert tfidf_abi.analyzer_check(a) == E                 # more than TFIDF_AN_MAX_STOP_BYTES bytes


def test_maximal_list():
    stop = [b"%08d" % i for i in range(4096)]               # 4096 words, 32768 bytes
    a, keep = _an(stop=stop)
    assert tfidf_abi.analyzer_check(a) == 0
    data = np.frombuffer(b"00000000 00004095 00004096 0000409 " + b" ".join(stop[::97]), dtype=np.uint8)
    off = np.array([0, len(data)], dtype=np.uint64)
    got = tfidf_abi.analyze_host(data, off, stop=stop)
    assert np.array_equal(got, analyze_ref.analyze(data, off, stop=stop))
    assert got.tobytes().split() == [b"00004096", b"0000409"]


def test_host_bad_arguments():
    data = np.frombuffer(b"ab cd", dtype=np.uint8)
    a, keep = _an()
    out = np.empty(5, dtype=np.uint8)
    fn = tfidf_abi.lib().tfidf_analyze_host
    bad = np.array([0, 4, 3], dtype=np.uint64)
    assert fn(C.byref(a), data.ctypes.data, 5, bad.ctypes.data, 2, out.ctypes.data) == tfidf_abi.E_INVAL
    past = np.array([0, 6], dtype=np.uint64)
    assert fn(C.byref(a), data.ctypes.data, 5, past.ctypes.data, 1, out.ctypes.data) == tfidf_abi.E_INVAL
    assert fn(C.byref(a), data.ctypes.data, 5, None, 1, out.ctypes.data) == tfidf_abi.E_INVAL
    assert fn(C.byref(a), data.ctypes.data, 5, None, 0, out.ctypes.data) == 0 and out.tobytes() == b"ab cd"


@pytest.mark.parametrize("case", ["g2_twelve_docs", "g4_config1"])
def test_decorated_golden(case):
    g = load_golden(case)
    data, off = analyze_ref.decorate(g["data"], g["off"], seed=11)
    assert len(data) > len(g["data"]) and data.tobytes() != g["data"].tobytes()
    clean = tfidf_abi.analyze_host(data, off, lower=True, punct=True)
    assert np.array_equal(clean, analyze_ref.analyze(data, off, True, True))
    assert oracle_py.run(clean, off)["output_txt"] == g["output"]
