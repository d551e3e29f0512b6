"""tfidf_analyze on the GPU (include/tfidf.h, section "analyzer"; csrc/analyze.hip) against
tests/analyze_ref.py, the definition in plain Python, and against tfidf_analyze_host: inputs at
every alignment inside windows, tokens placed across the kernel's tile edges, the two slots, the
run of an analyzed corpus against the oracle, three shards, and the CLI's four options."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import analyze_ref
import oracle_py
import tfidf_abi
from conftest import GOLDEN
from helpers import assert_k1_instance, assert_same_result, device_corpus, docs_to_arrays, load_golden, windowed

pytestmark = pytest.mark.gpu

LENGTHS = (1, 15, 16, 63, 64)


def word(n, salt=0):
    """a lower-case word of n bytes that no other generator here makes (it holds 'z')"""
    return bytes([0x7A] + [0x61 + (i * 7 + salt) % 25 for i in range(n - 1)])


def out_bytes(e, c):
    assert c.flags & tfidf_abi.TFIDF_CORPUS_DEVICE and c.bytes % 16 == 0
    return e.corpus_bytes(c)[0]


# ---- 1. device vs host vs reference ----

def _big_corpus():
    rng = np.random.default_rng(42)
    alpha = [b"a", b"b", b"c", b"A", b"B", b"1", b".", b",", b"\x00", b"\xc3\xa9"]
    seps = [b" ", b" ", b" ", b"\n", b"\t", b"\r", b"\x0b", b"\x0c"]
    special = [word(n) for n in LENGTHS] + [word(64) + b"q"]
    docs, total = [], 0
    while total < 200_000:
        parts = []
        for _ in range(int(rng.integers(0, 1500))):
            r = rng.random()
            if r < 0.02:
                tok = special[int(rng.integers(len(special)))]
            else:
                n = int(rng.integers(1, 9)) if r < 0.97 else int(rng.integers(9, 71))
                tok = b"".join(alpha[i] for i in rng.integers(0, len(alpha), n))
            parts.append(tok)
            if rng.random() < 0.97:                       # else: glued to the next token
                parts.append(seps[int(rng.integers(len(seps)))] * int(rng.integers(1, 3)))
        docs.append(b"".join(parts))                     # often ends inside a token: the next document starts there
        total += len(docs[-1])
        if rng.random() < 0.2:
            docs.append(b"")
    return docs


@pytest.fixture(scope="module")
def big():
    docs = _big_corpus()
    data, off = windowed(docs, 37, 21)
    out = {"data": data, "off": off, "ref": {}}
    for lower, punct in ((True, True), (False, False)):
        plain = analyze_ref.analyze(data, off, lower, punct)
        toks = {}
        for b, e in zip(off[:-1].tolist(), off[1:].tolist()):
            for t in bytes(plain[b:e]).translate(bytes.maketrans(b"\t\n\x0b\x0c\r", b"     ")).split(b" "):
                if t and len(t) <= 64 and 0 not in t:
                    toks[t] = toks.get(t, 0) + 1
        common = sorted(toks, key=lambda t: (-toks[t], t))
        stop = [word(n) for n in LENGTHS] + common[5:300]
        assert len(stop) == 300
        out["ref"][(lower, punct)] = (stop, analyze_ref.analyze(data, off, lower, punct, 2, stop))
    return out


@pytest.mark.parametrize("flags", [(True, True), (False, False)])
@pytest.mark.parametrize("shift", [None, 0, 1, 7, 15])
def test_device_vs_host_vs_reference(engine, big, flags, shift):
    data, off = big["data"], big["off"]
    stop, ref = big["ref"][flags]
    assert np.count_nonzero(ref != data) > 5_000
    kw = dict(lower=flags[0], punct=flags[1], min_len=2, stop=stop)
    if shift is None:
        got = out_bytes(engine, engine.analyze(data, off, **kw))
    else:
        with device_corpus(data, off, shift=shift) as c:
            o = engine.analyze(c, **kw)
            assert o.nbytes == len(data) and o.ndocs == len(off) - 1
            got = out_bytes(engine, o)
            assert np.array_equal(engine.corpus_bytes(o)[1], off)
    bad = np.flatnonzero(got != ref)
    assert len(bad) == 0, (bad[:8], bytes(got[max(0, bad[0] - 40):bad[0] + 40]), bytes(ref[max(0, bad[0] - 40):bad[0] + 40]))
    lo, hi = int(off[0]), int(off[-1])
    assert np.array_equal(got[:lo], data[:lo]) and np.array_equal(got[hi:], data[hi:])   # outside the window
    if shift in (None, 7):
        assert np.array_equal(tfidf_abi.analyze_host(data, off, **kw), ref)
    info = engine.analyze_info()
    assert info["nbytes"] == len(data) and info["nstop"] == 300 and info["table_slots"] == 1024
    assert info["lds_bytes"] > 0 and info["blanked_tokens"] > 1000


# ---- 2. tile edges ----

def filler(n):
    return np.frombuffer((b"ab " * (n // 3 + 1))[:n], dtype=np.uint8).copy()


def place(buf, at, tok):
    if at > 0:
        buf[at - 1] = 0x20
    buf[at:at + len(tok)] = np.frombuffer(tok, dtype=np.uint8)
    if at + len(tok) < len(buf):
        buf[at + len(tok)] = 0x20


def check_one(engine, buf, off, **kw):
    off = np.asarray(off, dtype=np.uint64)
    ref = analyze_ref.analyze(buf, off, **kw)
    got = out_bytes(engine, engine.analyze(buf, off, **kw))
    bad = np.flatnonzero(got != ref)
    assert len(bad) == 0, (bad[:8], kw.get("min_len"), off.tolist()[:4])
    return ref


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65])
def test_stop_word_across_tile_edges(engine, L):
    engine.analyze(filler(64), [0, 64], stop=[b"zz"])
    T = engine.analyze_info()["tile_bytes"]
    sw = word(min(L, 64))
    tok = sw if L <= 64 else sw + b"q"                   # 65: the stop word is a prefix only
    n, blanked = 2 * T + 100, 0
    for edge in (T, 2 * T):
        for at in range(edge - L - 1, edge + 2):
            buf = filler(n)
            place(buf, at, tok)
            ref = check_one(engine, buf, [0, n], stop=[sw, b"zzzz"])
            blanked += int(np.all(ref[at:at + L] == 0x20))
            assert engine.analyze_info()["blanked_tokens"] == (1 if L <= 64 else 0)
    assert blanked == (2 * (L + 3) if L <= 64 else 0)


def test_tile_edge_cases(engine):
    engine.analyze(filler(64), [0, 64], stop=[b"zz"])
    T = engine.analyze_info()["tile_bytes"]
    n = 3 * T + 100
    # a min_len victim of one byte as the last byte of a tile and as the first of the next
    for at in (T - 1, T, 2 * T - 1, 2 * T):
        buf = filler(n)
        place(buf, at, b"z")
        ref = check_one(engine, buf, [0, n], min_len=2)
        assert ref[at] == 0x20 and engine.analyze_info()["blanked_tokens"] > 0
    # a document boundary at T and T +- 1 cuts a stop word in two; the halves are not in the list
    sw = b"zyxwvu"
    for cut in (T - 1, T, T + 1):
        buf = filler(n)
        place(buf, T - 3, sw)
        ref = check_one(engine, buf, [0, cut, n], stop=[sw])
        assert bytes(ref[T - 3:T + 3]) == sw
        assert engine.analyze_info()["blanked_tokens"] == 0
    ref = check_one(engine, buf, [0, T - 3, T + 3, n], stop=[sw])       # boundaries at its ends: one token, blanked
    assert bytes(ref[T - 3:T + 3]) == b" " * 6
    # a token of 3 T bytes whose first and last 64 bytes are stop words
    a, b = word(64, 1), word(64, 2)
    long_tok = a + b"m" * (3 * T - 128) + b
    buf = np.frombuffer(b"ab " + long_tok + b" ab", dtype=np.uint8).copy()
    ref = check_one(engine, buf, [0, len(buf)], min_len=3, stop=[a, b])
    assert bytes(ref[3:3 + 3 * T]) == long_tok and bytes(ref[:3]) == b"   "
    # one-byte documents: every byte of two tiles starts a token
    buf = np.frombuffer((b"zyzy zy" * (2 * T // 7 + 1))[:2 * T + 40], dtype=np.uint8).copy()
    ref = check_one(engine, buf, np.arange(len(buf) + 1), min_len=1, stop=[b"z"])
    assert b"z" not in bytes(ref) and bytes(ref).count(b"y") == bytes(buf).count(b"y")
    # a stop word that ends at the corpus's last byte
    for n2 in (T, T + 5, 2 * T + 16, 100):
        buf = filler(n2)
        place(buf, n2 - 6, sw)
        ref = check_one(engine, buf, [0, n2], stop=[sw])
        assert bytes(ref[-6:]) == b" " * 6


def test_maximal_list(engine):
    """4096 words, 32768 bytes: the largest table a workgroup holds in LDS"""
    stop = [b"%08d" % i for i in range(4096)]
    rng = np.random.default_rng(3)
    toks = [b"%08d" % i for i in rng.integers(0, 8192, 3000)]
    buf = np.frombuffer(b" ".join(toks), dtype=np.uint8).copy()
    ref = check_one(engine, buf, [0, len(buf)], stop=stop)
    info = engine.analyze_info()
    assert info["table_slots"] == 8192 and info["lds_bytes"] > 65536
    assert all(int(t) >= 4096 for t in bytes(ref).split())


# ---- 3. identity, empty inputs, errors ----

def test_identity_and_byte_map(engine, big):
    data, off = big["data"], big["off"]
    for min_len in (0, 1):
        assert np.array_equal(out_bytes(engine, engine.analyze(data, off, min_len=min_len)), data)
        assert engine.analyze_info()["lds_bytes"] == 0
    every = np.tile(np.arange(256, dtype=np.uint8), 3)
    off3 = np.array([5, 700], dtype=np.uint64)
    for lower in (False, True):
        for punct in (False, True):
            with device_corpus(every, off3, shift=3) as c:
                got = out_bytes(engine, engine.analyze(c, lower=lower, punct=punct))
            assert np.array_equal(got, analyze_ref.analyze(every, off3, lower, punct)), (lower, punct)


def test_empty_inputs(engine):
    kw = dict(lower=True, punct=True, min_len=2, stop=[b"the"])
    buf = np.frombuffer(b"The the", dtype=np.uint8)
    o = engine.analyze(buf, np.zeros(1, dtype=np.uint64), **kw)          # ndocs == 0: every byte outside the window
    assert o.ndocs == 0 and bytes(out_bytes(engine, o)) == b"The the"
    o = engine.analyze(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), **kw)
    assert o.nbytes == 0 and o.ndocs == 0
    o = engine.analyze(np.zeros(0, dtype=np.uint8), np.zeros(4, dtype=np.uint64), **kw)
    assert o.nbytes == 0 and o.ndocs == 3
    o = engine.analyze(buf, np.array([3, 3, 3], dtype=np.uint64), **kw)  # only empty documents
    assert bytes(out_bytes(engine, o)) == b"The the"
    o = engine.analyze(buf, np.array([0, 0, 7, 7], dtype=np.uint64), **kw)
    assert bytes(out_bytes(engine, o)) == b"       "
    engine.run_corpus(o)
    assert engine.fetch()["npairs"] == 0


def test_slots_and_errors(engine, big):
    g = load_golden("g5_w3")
    docs = [bytes(g["data"][int(b):int(e)]) for b, e in zip(g["off"][:-1], g["off"][1:])]
    long_term = b"a" * 40
    docs[11] += b" " + long_term + b" " + long_term       # in the corpus and in the batch
    cdata, coff = analyze_ref.decorate(*docs_to_arrays(docs[:12]), seed=5)
    bdata, boff = analyze_ref.decorate(*docs_to_arrays(docs[10:]), seed=6)
    kw = dict(lower=True, punct=True, min_len=2, stop=[b"the", b"of"])
    c0 = engine.analyze(cdata, coff, slot=tfidf_abi.AN_SLOT_CORPUS, **kw)
    engine.run_corpus(c0)
    text = engine.text()
    assert b"@" + long_term + b"\t" in text
    b1 = engine.analyze(bdata, boff, slot=tfidf_abi.AN_SLOT_BATCH, **kw)
    assert b1.bytes != c0.bytes
    got = engine.transform_corpus(b1)
    want = engine.transform(tfidf_abi.analyze_host(bdata, boff, **kw), boff)
    for k in ("row_off", "doc_size", "doc_oov", "term", "count", "df", "word_off", "word_len"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["score"].view(np.uint64), want["score"].view(np.uint64)) and got["words"] == want["words"]
    assert got["npairs"] > 0 and long_term in got["words"]
    assert engine.text() == text                              # the run's corpus (slot 0) is untouched
    for bad_slot, src in ((0, c0), (2, c0), (1, b1)):
        with pytest.raises(tfidf_abi.TfidfError) as ex:
            engine.analyze(src, slot=bad_slot, **kw)
        assert ex.value.rc == tfidf_abi.E_INVAL
    again = engine.analyze(c0, slot=tfidf_abi.AN_SLOT_BATCH, **kw)   # slot 0's output into slot 1: idempotent
    assert np.array_equal(out_bytes(engine, again), out_bytes(engine, c0))
    # bad offsets and a bad analyzer
    lib, a = tfidf_abi.lib(), tfidf_abi.analyzer(True, True, 2, [b"the"])[0]
    out = tfidf_abi.Corpus()
    for off in ([0, 5, 4], [0, len(cdata) + 1]):
        c, keep = tfidf_abi._host_corpus(cdata, np.array(off, dtype=np.uint64))
        assert lib.tfidf_analyze(engine.h, a, c, 0, out) == tfidf_abi.E_INVAL
    c, keep = tfidf_abi._host_corpus(cdata, coff)
    assert lib.tfidf_analyze(engine.h, None, c, 0, out) == tfidf_abi.E_INVAL
    assert lib.tfidf_analyze(engine.h, a, None, 0, out) == tfidf_abi.E_INVAL
    assert lib.tfidf_analyze(engine.h, a, c, 0, None) == tfidf_abi.E_INVAL
    a.flags = 8
    assert lib.tfidf_analyze(engine.h, a, c, 0, out) == tfidf_abi.E_INVAL


def test_repeated_call_allocates_nothing(engine, big):
    stop, ref = big["ref"][(True, True)]
    kw = dict(lower=True, punct=True, min_len=2, stop=stop)
    with device_corpus(big["data"], big["off"], shift=9) as c:
        engine.analyze(c, **kw)
        engine.analyze(big["data"], big["off"], **kw)
        before = engine.alloc_counters()
        engine.analyze(c, **kw)
        o = engine.analyze(big["data"], big["off"], **kw)
        assert engine.alloc_counters() == before
        assert np.array_equal(out_bytes(engine, o), ref)


# ---- 4. pipelines ----

@pytest.mark.parametrize("case", ["g2_twelve_docs", "g4_config1"])
def test_pipeline_golden(engine, case):
    g = load_golden(case)
    data, off = analyze_ref.decorate(g["data"], g["off"], seed=11)
    engine.run_corpus(engine.analyze(data, off, lower=True, punct=True))
    assert engine.text() == g["output"]
    with device_corpus(data, off, shift=7) as c:
        engine.run_corpus(engine.analyze(c, lower=True, punct=True))
        assert_k1_instance(engine.info(), "sl_fast")          # an aligned output whatever the input's base
        assert engine.text() == g["output"]


def _oracle_case():
    g = load_golden("g5_w3")
    docs = [bytes(g["data"][int(b):int(e)]) for b, e in zip(g["off"][:-1], g["off"][1:])]
    docs[3] += b" " + b"w" * 40 + b" x y " + b"w" * 40
    data, off = analyze_ref.decorate(*docs_to_arrays(docs), seed=21)
    ora0 = oracle_py.run(analyze_ref.analyze(data, off, True, True), off)
    df = {}
    for t, d in zip(ora0["term"].tolist(), ora0["df"].tolist()):
        df[ora0["terms"][t]] = d
    stop = sorted(df, key=lambda w: (-df[w], w))[:20]
    return data, off, stop


def test_pipeline_oracle(engine):
    data, off, stop = _oracle_case()
    kw = dict(lower=True, punct=True, min_len=2, stop=stop)
    ref = analyze_ref.analyze(data, off, **kw)
    ora = oracle_py.run(ref, off)
    with device_corpus(data, off, shift=5) as c:
        engine.run_corpus(engine.analyze(c, **kw))
        res = engine.fetch()
        assert_same_result(res, ora)
        assert b"w" * 40 in res["terms"] and not set(stop) & set(res["terms"])
        assert all(len(t) >= 2 for t in res["terms"])
        assert engine.text() == ora["output_txt"]             # emission reads the 40-byte term from the slot's buffer


def test_three_local_shards(engine, tmp_path):
    data, off, stop = _oracle_case()
    docs = [bytes(data[int(b):int(e)]) for b, e in zip(off[:-1], off[1:])][:9]   # ids 1..9: "docN@" order is numeric
    kw = dict(lower=True, punct=True, min_len=2, stop=stop)
    d9, o9 = docs_to_arrays(docs)
    engine.run_corpus(engine.analyze(d9, o9, **kw))
    single = engine.text()
    assert single == oracle_py.run(analyze_ref.analyze(d9, o9, **kw), o9)["output_txt"]
    with tfidf_abi.Group(3, devices=[0, 0, 0]) as g:
        shards = []
        for r in range(3):
            d, o = docs_to_arrays(docs[3 * r:3 * r + 3])
            shards.append(g.ranks[r].analyze(d, o, doc_ids=[3 * r + 1, 3 * r + 2, 3 * r + 3], ndocs_total=9, **kw))
        g.run(shards)
        g.write_output(str(tmp_path / "out.txt"))
    assert (tmp_path / "out.txt").read_bytes() == single


# ---- 5. CLI ----

@pytest.mark.parametrize("extra", [[], ["--shards", "2"]])
def test_cli(tmp_path, extra):
    data, off, stop = _oracle_case()
    docs = [bytes(data[int(b):int(e)]) for b, e in zip(off[:-1], off[1:])]
    fit, held = docs[:13], docs[13:]
    (tmp_path / "input").mkdir()
    (tmp_path / "new").mkdir()
    for i, d in enumerate(fit):
        (tmp_path / "input" / ("doc%d" % (i + 1))).write_bytes(d)
    for i, d in enumerate(held):
        (tmp_path / "new" / ("doc%d" % (i + 1))).write_bytes(d)
    (tmp_path / "stop.txt").write_bytes(b"\n".join(w.upper() + b"," for w in stop) + b"\n")   # folded by the CLI
    qfile = b"GPU. " + stop[0] + b" " + fit[2][:60] + b"\n(" + fit[5][10:50] + b")\n\n" + held[0][:40]
    (tmp_path / "q.txt").write_bytes(qfile)
    p = subprocess.run([tfidf_abi.CLI_PATH, "--lower", "--strip-punct", "--min-token", "2", "--stopwords", "stop.txt",
                        "--query", "q.txt", "--transform", "new"] + extra, cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    kw = dict(lower=True, punct=True, min_len=2, stop=stop)
    fdata, foff = docs_to_arrays(fit)
    ora = oracle_py.run(analyze_ref.analyze(fdata, foff, **kw), foff)
    assert (tmp_path / "output.txt").read_bytes() == ora["output_txt"] and ora["output_txt"]
    qoff = [0] + [i + 1 for i, c in enumerate(qfile) if c == 0x0A] + [len(qfile)]
    qan = bytes(tfidf_abi.analyze_host(np.frombuffer(qfile, dtype=np.uint8), np.array(qoff, dtype=np.uint64), **kw))
    hdata, hoff = docs_to_arrays(held)
    with tfidf_abi.Engine(0) as e:
        e.run_host(analyze_ref.analyze(fdata, foff, **kw), foff)
        hits = e.query([qan[b:x] for b, x in zip(qoff[:-1], qoff[1:])], 10)
        rows = e.transform(tfidf_abi.analyze_host(hdata, hoff, **kw), hoff)
    want = b"".join(b"q%d\tdoc%d\t%.16f\n" % (q + 1, hits["doc"][q, i], hits["score"][q, i])
                    for q in range(len(qoff) - 1) for i in range(int(hits["nhits"][q])))
    assert want and (tmp_path / "hits.txt").read_bytes() == want
    ro = rows["row_off"].tolist()
    want = b"".join(b"doc%d@" % i + rows["words"][x] + b"\t%.16f\n" % rows["score"][x]
                    for i in tfidf_abi.doc_name_order(len(held)).tolist() for x in range(ro[i - 1], ro[i]))
    assert want and (tmp_path / "transform.txt").read_bytes() == want


def test_cli_without_the_options_is_unchanged(tmp_path):
    case = "g5_w3"
    shutil.copytree(os.path.join(GOLDEN, case, "input"), tmp_path / "input")
    (tmp_path / "q.txt").write_bytes(b"the of\n")
    p = subprocess.run([tfidf_abi.CLI_PATH, "--query", "q.txt", "--transform", "input"], cwd=tmp_path, capture_output=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    out = (tmp_path / "output.txt").read_bytes()
    assert out == load_golden(case)["output"] and (tmp_path / "transform.txt").read_bytes() == out
