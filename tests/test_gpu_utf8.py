"""TFIDF_AN_UTF8 on the GPU (include/tfidf.h, section "analyzer"; csrc/analyze.hip,
csrc/analyze_utf8.h) against tests/utf8_ref.py, the definition in plain Python, and against
tfidf_analyze_host: a multi-byte corpus at every alignment inside windows in both forms of the
kernel, sequences and tokens placed across group and tile edges, sequences cut by boundaries, the
exhaustive two- and three-byte buffer, grids of 1 and 3 workgroups, the run of an analyzed corpus
and the CLI's --utf8."""
import subprocess

import numpy as np
import pytest

import oracle_py
import tfidf_abi
import utf8_ref
from helpers import assert_same_result, device_corpus, docs_to_arrays, windowed
from utf8_ref import enc, exhaustive_23

pytestmark = pytest.mark.gpu

UBER, ETO = "über".encode("utf-8"), "это".encode("utf-8")
STOP = [UBER, ETO, b"the", b"ab", b"cab", enc(0x436, 0x436)]
FORMS = {"map": dict(), "tile": dict(min_len=2, stop=STOP)}
FLAGS = {"LU": dict(lower=True), "PU": dict(punct=True), "LPU": dict(lower=True, punct=True), "U": dict()}


def out_bytes(e, c):
    assert c.flags & tfidf_abi.TFIDF_CORPUS_DEVICE and c.bytes % 16 == 0
    return e.corpus_bytes(c)[0]


def same(got, ref):
    bad = np.flatnonzero(got != ref)
    assert len(bad) == 0, (bad[:8], bytes(got[max(0, bad[0] - 24):bad[0] + 24]), bytes(ref[max(0, bad[0] - 24):bad[0] + 24]))


# ---- 1. the corpus ----

def _big_corpus():
    rng = np.random.default_rng(43)
    frags = utf8_ref.fragments()
    alpha = [b"a", b"b", b"c", b"A", b"B", b"1", b".", b","] + [enc(c) for c in (0xC9, 0xE9, 0x416, 0x436, 0x1E00, 0x10400, 0x201C)]
    words = ["ÜBER".encode("utf-8"), "Über".encode("utf-8"), UBER, "ЭТО".encode("utf-8"), ETO, "“The”".encode("utf-8"), b"the",
             "МОСКВА…".encode("utf-8"), "naïve—café".encode("utf-8"), "Running”".encode("utf-8")]
    seps = [b" ", b" ", b" ", b"\n", b"\t", b"\r", b"\x0b", b"\x0c", enc(0xA0), enc(0x2003)]
    docs, total = [], 0
    while total < 200_000:
        parts = []
        for _ in range(int(rng.integers(0, 1500))):
            r = rng.random()
            if r < 0.10:
                tok = words[int(rng.integers(len(words)))]
            elif r < 0.35:
                tok = b"".join(frags[i] for i in rng.integers(0, len(frags), int(rng.integers(1, 5))))
            else:
                n = int(rng.integers(1, 9)) if r < 0.97 else int(rng.integers(9, 40))
                tok = b"".join(alpha[i] for i in rng.integers(0, len(alpha), n))
            parts.append(tok)
            if rng.random() < 0.97:                       # else: glued to the next token
                parts.append(seps[int(rng.integers(len(seps)))] * int(rng.integers(1, 3)))
        docs.append(b"".join(parts))                     # often ends inside a token or a sequence
        total += len(docs[-1])
        if rng.random() < 0.2:
            docs.append(b"")
    return docs


@pytest.fixture(scope="module")
def big():
    data, off = windowed(_big_corpus(), 37, 21)
    out = {"data": data, "off": off, "ref": {}}
    for form, fkw in FORMS.items():
        for flags, kw in FLAGS.items():
            stats = {}
            ref = utf8_ref.analyze(data, off, stats=stats, **kw, **fkw)
            out["ref"][(form, flags)] = (ref, stats)
    raw = data.tobytes()
    for flags in FLAGS:                                  # tokens ÜBER and Über, folded, that the stop list blanked
        plain, ref = out["ref"][("map", flags)][0].tobytes(), out["ref"][("tile", flags)][0].tobytes()
        at, n = plain.find(b" " + UBER + b" "), 0
        while at >= 0:
            n += ref[at:at + 7] == b" " * 7 and raw[at + 1:at + 6] != UBER
            at = plain.find(b" " + UBER + b" ", at + 1)
        out["ref"][("tile", flags)][1]["stopped_uber"] = n
    return out


@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shift", [None, 0, 1, 7, 15])
def test_device_vs_host_vs_reference(engine, big, form, flags, shift):
    data, off = big["data"], big["off"]
    ref, stats = big["ref"][(form, flags)]
    kw = dict(utf8=True, **FLAGS[flags], **FORMS[form])
    # the reference alone: the case takes its path
    if flags == "U":
        assert stats["utf8_changed"] == 0
    else:
        assert stats["utf8_changed"] > 5_000           # 35 % of 25 000 tokens hold a table sequence
        for L in (2, 3, 4):
            for k in range(1, L):
                assert any(n == L and (at + k) % 16 == 0 for at, n in stats["spans"]), (L, k)
    if form == "tile" and "L" in flags:                  # the stop list met folded non-ASCII tokens: 1 % of the tokens are ÜBER or Über
        assert stats["stopped_uber"] > 20
    if shift is None:
        got = out_bytes(engine, engine.analyze(data, off, **kw))
    else:
        with device_corpus(data, off, shift=shift) as dc:
            o = engine.analyze(dc, **kw)
            assert o.nbytes == len(data) and o.ndocs == len(off) - 1
            got = out_bytes(engine, o)
    same(got, ref)
    lo, hi = int(off[0]), int(off[-1])
    assert np.array_equal(got[:lo], data[:lo]) and np.array_equal(got[hi:], data[hi:])
    info = engine.analyze_info()
    assert info["utf8_changed"] == stats["utf8_changed"]
    assert (info["lds_bytes"] > 0) == (form == "tile") and (info["grid"] > 0) == (form == "tile")
    if shift in (None, 7):
        assert np.array_equal(tfidf_abi.analyze_host(data, off, **kw), ref)


@pytest.mark.parametrize("grid", ["1", "3"])
def test_result_does_not_depend_on_the_grid(big, grid, monkeypatch):
    monkeypatch.setenv("TFIDF_AN_GRID", grid)
    data, off = big["data"], big["off"]
    with tfidf_abi.Engine(0) as e:
        for stem in (False, True):
            kw = dict(utf8=True, stem=stem, **FLAGS["LPU"], **FORMS["tile"])
            stats = {}
            ref = big["ref"][("tile", "LPU")][0] if not stem else utf8_ref.analyze(data, off, stats=stats, **kw)
            same(out_bytes(e, e.analyze(data, off, **kw)), ref)
            info = e.analyze_info()
            assert info["grid"] == int(grid) and info["utf8_changed"] == big["ref"][("tile", "LPU")][1]["utf8_changed"]
            if stem:
                assert info["stemmed_tokens"] == stats["changed"] > 0


def test_repeated_call_allocates_nothing(engine, big):
    data, off = big["data"], big["off"]
    for form in FORMS:
        kw = dict(utf8=True, **FLAGS["LPU"], **FORMS[form])
        with device_corpus(data, off, shift=9) as dc:
            engine.analyze(dc, **kw)
            engine.analyze(data, off, **kw)
            before = engine.alloc_counters()
            engine.analyze(dc, **kw)
            o = engine.analyze(data, off, **kw)
            assert engine.alloc_counters() == before
            same(out_bytes(engine, o), big["ref"][(form, "LPU")][0])


def test_flag_off_identity(engine):
    rng = np.random.default_rng(3)
    data = rng.integers(0, 0x80, 50_001, dtype=np.uint8)
    off = np.array([5, 20_000, 20_000, 49_990], dtype=np.uint64)
    for form, fkw in FORMS.items():
        for stem in ((False, True) if form == "tile" else (False,)):
            kw = dict(lower=True, punct=True, stem=stem, **fkw)
            a = out_bytes(engine, engine.analyze(data, off, utf8=True, **kw)).copy()
            assert engine.analyze_info()["utf8_changed"] == 0
            b = out_bytes(engine, engine.analyze(data, off, **kw))
            assert np.array_equal(a, b) and np.array_equal(a, utf8_ref.analyze(data, off, **kw))


# ---- 2. edges ----

FOLD_SEQ = {2: enc(0x416), 3: enc(0x1E00), 4: enc(0x10400)}
BLANK_SEQ = {2: enc(0xAB), 3: enc(0x2014), 4: enc(0x1F600)}


def filler(n):
    return np.frombuffer((b"ab " * (n // 3 + 1))[:n], dtype=np.uint8).copy()


def check_one(engine, buf, off, **kw):
    off = np.asarray(off, dtype=np.uint64)
    stats = {}
    ref = utf8_ref.analyze(buf, off, stats=stats, **kw)
    got = out_bytes(engine, engine.analyze(buf, off, utf8=True, **kw))
    same(got, ref)
    assert engine.analyze_info()["utf8_changed"] == stats["utf8_changed"]
    return ref, stats


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("L", [2, 3, 4])
def test_sequence_across_group_and_tile_edges(engine, form, L):
    T = engine_tile(engine)
    n = 2 * T + 100
    for flags, seqs in (("LU", FOLD_SEQ), ("PU", BLANK_SEQ)):
        for k in range(0, L + 1):                       # the sequence's byte k is the first behind the edge
            buf = filler(n)
            for edge in (16 * 5, T, 2 * T):
                at = edge - k
                buf[at:at + L] = np.frombuffer(seqs[L], dtype=np.uint8)
            ref, stats = check_one(engine, buf, [0, n], **FLAGS[flags], **FORMS[form])
            assert stats["utf8_changed"] == 3
            for edge in (16 * 5, T, 2 * T):
                assert bytes(ref[edge - k:edge - k + L]) != seqs[L]


def engine_tile(engine):
    engine.analyze(np.frombuffer(b"ab", dtype=np.uint8), np.array([0, 2], dtype=np.uint64), min_len=2)
    T = engine.analyze_info()["tile_bytes"]
    assert T >= 1024 and T % 16 == 0
    return T


@pytest.mark.parametrize("L", [2, 3, 4])
def test_token_with_a_sequence_across_tile_edges(engine, L):
    """a stop word of 64 bytes whose first or last character is a cased sequence, that sequence
    across the tile edge T and across T - 80 and T + 80, where the halos end"""
    T = engine_tile(engine)
    n = 2 * T + 100
    up, lo = FOLD_SEQ[L], FOLD_SEQ[L].decode("utf-8").lower().encode("utf-8")
    body = (b"qwertz" * 11)[:64 - L]
    for tok, folded, seq_at in ((up + body, lo + body, 0), (body + up, body + lo, 64 - L)):
        assert len(tok) == 64
        for edge in (T, T - 80, T + 80, 2 * T):
            for k in range(1, L):                       # the sequence's byte k is the first behind the edge
                at = edge - k - seq_at
                buf = filler(n)
                buf[at - 1] = buf[at + 64] = 0x20
                buf[at:at + 64] = np.frombuffer(tok, dtype=np.uint8)
                ref, stats = check_one(engine, buf, [0, n], lower=True, stop=[folded])
                assert bytes(ref[at:at + 64]) == b" " * 64 and stats["utf8_changed"] == 1
                ref, stats = check_one(engine, buf, [0, n], lower=True, stop=[tok])      # the unfolded form matches nothing
                assert bytes(ref[at:at + 64]) == folded


@pytest.mark.parametrize("form", list(FORMS))
def test_cuts(engine, form):
    """sequences cut by document boundaries, window edges and the buffer's end in buffers of 3 to
    25 bytes; with the padding the sequence lies across a group edge"""
    for pad in (0, 12, 13):
        for raw, off, want, need in utf8_ref.cut_cases(pad):
            buf = np.frombuffer(raw, dtype=np.uint8)
            kw = dict(lower=True, punct=True, utf8=True)
            if form == "tile":
                kw.update(min_len=1, stop=[b"zzz"])
            got = bytes(out_bytes(engine, engine.analyze(buf, np.array(off, dtype=np.uint64), **kw)))
            assert got == want, (raw, off, got)
            assert engine.analyze_info()["utf8_changed"] == (0 if want == raw else 1)
            assert (engine.analyze_info()["grid"] > 0) == (form == "tile")


@pytest.mark.parametrize("form", list(FORMS))
def test_exhaustive_two_and_three_bytes(engine, form):
    raw = exhaustive_23()
    data, off = np.frombuffer(raw, dtype=np.uint8), np.array([0, len(raw)], dtype=np.uint64)
    check_one(engine, data, off, lower=True, punct=True, **FORMS[form])


# ---- 3. end to end ----

DOCS = ["Москва — столица России.", "“The capital” of Russia is МОСКВА…", "москва, Москва и ещё раз москва",
        "«Running» in the rain: ЭТО naïve", "Санкт-Петербург is not the capital", "nothing here — just “quotes”",
        "Это the Running man", "ÜBER alles über", "café CAFÉ Café", "a b c"]
DOCS = [d.encode("utf-8") for d in DOCS]
KW = dict(lower=True, punct=True, stop=[b"the", ETO], stem=True)


def test_pipeline(engine):
    data, off = docs_to_arrays(DOCS)
    ref = utf8_ref.analyze(data, off, **KW)
    host = tfidf_abi.analyze_host(data, off, utf8=True, **KW)
    assert np.array_equal(host, ref)
    with device_corpus(data, off, shift=5) as c:
        engine.run_corpus(engine.analyze(c, utf8=True, **KW))
        res = engine.fetch()
        assert_same_result(res, oracle_py.run(ref, off))
        moskva = "москва".encode("utf-8")
        assert moskva in res["terms"] and "МОСКВА".encode("utf-8") not in res["terms"] and b"run" in res["terms"]
        q = np.frombuffer("МОСКВА".encode("utf-8"), dtype=np.uint8)
        qan = bytes(tfidf_abi.analyze_host(q, np.array([0, len(q)], dtype=np.uint64), utf8=True, **KW))
        assert qan == moskva
        hits = engine.query([qan], 10)
        assert sorted(hits["doc"][0, :int(hits["nhits"][0])].tolist()) == [1, 2, 3]
        assert int(engine.query(["МОСКВА".encode("utf-8")], 10)["nhits"][0]) == 0


@pytest.mark.parametrize("extra", [[], ["--shards", "2"]])
def test_cli(tmp_path, extra):
    qfile = "МОСКВА\n“running”\nÜBER".encode("utf-8")
    stopfile = "The ЭТО".encode("utf-8")                # folded by the same map

    def ref_of(raw, off=None):
        buf = np.frombuffer(raw, dtype=np.uint8)
        return bytes(utf8_ref.analyze(buf, [0, len(buf)] if off is None else off, **KW))

    for name in ("a", "b", "c"):                        # a: raw files and the options; b: the reference's bytes; c: raw, no --utf8
        (tmp_path / name / "input").mkdir(parents=True)
        for i, d in enumerate(DOCS):
            (tmp_path / name / "input" / ("doc%d" % (i + 1))).write_bytes(ref_of(d) if name == "b" else d)
        (tmp_path / name / "stop.txt").write_bytes(stopfile)
    qoff = [0] + [i + 1 for i, c in enumerate(qfile) if c == 0x0A] + [len(qfile)]
    for name in ("a", "c"):
        (tmp_path / name / "q.txt").write_bytes(qfile)
    (tmp_path / "b" / "q.txt").write_bytes(ref_of(qfile, qoff))
    opts = ["--lower", "--strip-punct", "--stopwords", "stop.txt", "--stem"]
    for name, o in (("a", opts + ["--utf8"]), ("b", []), ("c", opts)):
        p = subprocess.run([tfidf_abi.CLI_PATH] + o + ["--query", "q.txt"] + extra, cwd=tmp_path / name, capture_output=True, timeout=120)
        assert p.returncode == 0, p.stderr
    data, off = docs_to_arrays(DOCS)
    want = oracle_py.run(utf8_ref.analyze(data, off, **KW), off)["output_txt"]
    assert (tmp_path / "a" / "output.txt").read_bytes() == want == (tmp_path / "b" / "output.txt").read_bytes()
    hits = (tmp_path / "a" / "hits.txt").read_bytes()
    assert hits and hits == (tmp_path / "b" / "hits.txt").read_bytes()
    assert sorted(l.split(b"\t")[1] for l in hits.splitlines() if l.startswith(b"q1\t")) == [b"doc1", b"doc2", b"doc3"]
    assert b"q2\t" in hits and b"q3\t" in hits
    plain = (tmp_path / "c" / "hits.txt").read_bytes()   # without --utf8 МОСКВА stays upper case and is no term of the folded ...
    assert b"q1\t" not in plain
