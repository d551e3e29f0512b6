"""The analyzer's Porter stemmer on the GPU (include/tfidf.h, section "analyzer", step 3;
csrc/analyze.hip, csrc/analyze_stem.h) against tests/stem_ref.py, the definition in plain
Python, and against tfidf_analyze_host: a word corpus at every alignment inside windows, the
persistent loop at grids of 1 and 3 workgroups, tokens placed across the kernel's tile edges,
the stop list's order, the run of a stemmed corpus, and the CLI's --stem."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import analyze_ref
import oracle_py
import stem_ref
import tfidf_abi
from helpers import assert_same_result, device_corpus, docs_to_arrays, windowed

pytestmark = pytest.mark.gpu

W64 = (b"ab" * 28) + b"izations"                        # 64 letters, stem: the first 56
W65 = (b"ab" * 28) + b"oizations"                       # 65 letters: never touched


def out_bytes(e, c):
    assert c.flags & tfidf_abi.TFIDF_CORPUS_DEVICE and c.bytes % 16 == 0
    return e.corpus_bytes(c)[0]


def tokens_of(buf, off):
    out = []
    for b, e in zip(off[:-1], off[1:]):
        w = bytes(buf[int(b):int(e)]).translate(bytes.maketrans(b"\t\n\x0b\x0c\r", b"     "))
        out += [t for t in w.split(b" ") if t]
    return out


# ---- 1. the word corpus ----

def _word_corpus():
    rng = np.random.default_rng(7)
    words = stem_ref.words()
    fixed = sorted(set(s for s in (stem_ref.stem(w) for w in words[::7]) if len(s) >= 3 and stem_ref.stem(s) == s))
    odd = [b"runn1ng", b"caf\xc3\xa9s", b"b\x00ing", b"Running", b"CONNECTED", b"hopping,", b"(relational)", b"as", b"is", b"a",
           W64, W65, b"q" * 61 + b"ing", b"q" * 62 + b"ing"]
    seps = [b" ", b" ", b" ", b"\n", b"\t", b"\r", b"\x0b", b"\x0c", b"  "]
    parts, total = [], 0
    while total < 200_000:
        r = rng.random()
        if r < 0.70:
            tok = words[int(rng.integers(len(words)))]
        elif r < 0.90:
            tok = fixed[int(rng.integers(len(fixed)))]
        else:
            tok = odd[int(rng.integers(len(odd)))]
        sep = seps[int(rng.integers(len(seps)))] if rng.random() < 0.98 else b""     # else: glued to the next token
        parts.append(tok + sep)
        total += len(parts[-1])
    stream = b"".join(parts)
    cuts = sorted(set(int(x) for x in rng.integers(1, len(stream), 120)))              # most cuts fall inside a token
    docs = []
    for b, e in zip([0] + cuts, cuts + [len(stream)]):
        docs.append(stream[b:e])
        if rng.random() < 0.1:
            docs.append(b"")
    return docs


@pytest.fixture(scope="module")
def corpus():
    data, off = windowed(_word_corpus(), 37, 21)
    out = {"data": data, "off": off, "case": {}}
    plain = analyze_ref.analyze(data, off, True, True)
    count = {}
    for t in tokens_of(plain, off):
        if len(t) <= 64:
            count[t] = count.get(t, 0) + 1
    stop = sorted(count, key=lambda t: (-count[t], t))[5:305]
    assert len(stop) == 300
    for name, kw in (("full", dict(lower=True, punct=True, min_len=2, stop=stop)), ("alone", dict())):
        stats = {}
        out["case"][name] = dict(kw=kw, ref=stem_ref.analyze(data, off, stats=stats, **kw), stats=stats,
                                 unstemmed=analyze_ref.analyze(data, off, **kw))
    return out


@pytest.mark.parametrize("case", ["full", "alone"])
@pytest.mark.parametrize("shift", [None, 0, 1, 7, 15])
def test_device_vs_host_vs_reference(engine, corpus, case, shift):
    data, off, c = corpus["data"], corpus["off"], corpus["case"][case]
    kw, ref, stats = c["kw"], c["ref"], c["stats"]
    # the reference alone: the stemmer has work to do, and words to leave alone
    assert np.count_nonzero(ref != c["unstemmed"]) > 5_000
    assert stats["eligible"] - stats["changed"] > 1_000 and stats["changed"] > 1_000
    if shift is None:
        got = out_bytes(engine, engine.analyze(data, off, stem=True, **kw))
    else:
        with device_corpus(data, off, shift=shift) as dc:
            o = engine.analyze(dc, stem=True, **kw)
            assert o.nbytes == len(data) and o.ndocs == len(off) - 1
            got = out_bytes(engine, o)
    bad = np.flatnonzero(got != ref)
    assert len(bad) == 0, (bad[:8], bytes(got[max(0, bad[0] - 40):bad[0] + 40]), bytes(ref[max(0, bad[0] - 40):bad[0] + 40]))
    info = engine.analyze_info()
    assert info["stemmed_tokens"] == stats["changed"]
    assert info["lds_bytes"] > 0 and info["grid"] > 0 and info["table_slots"] == (1024 if case == "full" else 0)
    if shift in (None, 7):
        assert np.array_equal(tfidf_abi.analyze_host(data, off, stem=True, **kw), ref)
    if shift is None:                                   # the same call without the stemmer
        assert np.array_equal(out_bytes(engine, engine.analyze(data, off, **kw)), c["unstemmed"])
        assert engine.analyze_info()["stemmed_tokens"] == 0


@pytest.mark.parametrize("grid", ["1", "3", None])
def test_result_does_not_depend_on_the_grid(corpus, grid, monkeypatch):
    """TFIDF_AN_GRID: one workgroup takes every tile, three take a third each, or every tile has
    its own; with and without a stemmer"""
    if grid is None:
        monkeypatch.delenv("TFIDF_AN_GRID", raising=False)
    else:
        monkeypatch.setenv("TFIDF_AN_GRID", grid)
    data, off, c = corpus["data"], corpus["off"], corpus["case"]["full"]
    with tfidf_abi.Engine(0) as e:
        ntiles = -(-len(data) // 4096)
        for stem, want in ((True, c["ref"]), (False, c["unstemmed"])):
            got = out_bytes(e, e.analyze(data, off, stem=stem, **c["kw"]))
            assert np.array_equal(got, want), (stem, np.flatnonzero(got != want)[:8])
            info = e.analyze_info()
            assert info["tile_bytes"] == 4096 and info["grid"] == (int(grid) if grid else ntiles)
            assert info["stemmed_tokens"] == (c["stats"]["changed"] if stem else 0)


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
    stats = {}
    ref = stem_ref.analyze(buf, off, stats=stats, **kw)
    got = out_bytes(engine, engine.analyze(buf, off, stem=True, **kw))
    bad = np.flatnonzero(got != ref)
    assert len(bad) == 0, (bad[:8], off.tolist()[:4], bytes(got[max(0, bad[0] - 20):bad[0] + 20]))
    assert engine.analyze_info()["stemmed_tokens"] == stats["changed"]
    return ref


@pytest.mark.parametrize("tok,stem", [(b"relational", b"relat"), (b"hopping", b"hop"), (b"sensibilities", b"sensibl"),
                                      (b"happy", b"happi"), (b"agreed", b"agre"), (W64, W64[:56])])
def test_token_across_tile_edges(engine, tok, stem):
    """the edge before the token, inside the stem, at the cut, in front of the stem's last
    (changed) byte, inside the blanked tail and behind the token"""
    assert stem_ref.stem(tok) == stem
    L, S = len(tok), len(stem)
    T = 4096
    ks = range(0, L + 2) if L < 20 else (0, 1, 30, S - 1, S, S + 1, 60, L - 1, L, L + 1)   # L - 1: the left halo's reach
    n = 2 * T + 100
    for edge in (T, 2 * T):
        for k in ks:                                    # the token's byte k is the tile's first
            at = edge - k
            buf = filler(n)
            place(buf, at, tok)
            ref = check_one(engine, buf, [0, n])
            assert bytes(ref[at:at + L]) == stem + b" " * (L - S)


def test_tile_edge_cases(engine):
    T = 4096
    n = 3 * T + 100
    for edge in (T, 2 * T):                             # 65 letters across the edge: unchanged
        for k in (1, 33, 64):
            buf = filler(n)
            place(buf, edge - k, W65)
            ref = check_one(engine, buf, [0, n])
            assert bytes(ref[edge - k:edge - k + 65]) == W65
    for cut in (T - 1, T, T + 1):                       # a document boundary inside a word
        buf = filler(n)
        place(buf, T - 4, b"connections")
        ref = check_one(engine, buf, [0, cut, n])
        assert bytes(ref[T - 4:T + 7]) != b"connect    "
    ref = check_one(engine, buf, [0, T - 4, T + 7, n])  # boundaries at its ends: one token
    assert bytes(ref[T - 4:T + 7]) == b"connect    "
    for n2 in (T + 5, T + 100, 2 * T, 100, 7):          # a stemmable token ends the corpus, in a last partial tile
        buf = filler(n2)
        place(buf, n2 - 7, b"running")
        ref = check_one(engine, buf, [0, n2])
        assert bytes(ref[-7:]) == b"run    "
    buf = np.frombuffer((b"caresses ponies " * (2 * T // 16 + 1))[:2 * T + 40], dtype=np.uint8).copy()
    check_one(engine, buf, np.arange(0, len(buf) + 1, 4))   # four-byte documents: every token is cut
    check_one(engine, buf, [0, len(buf)], min_len=7, stop=[b"ponies"])


# ---- 3. the stop list, empty inputs, allocation ----

def test_stop_list_sees_the_unstemmed_token(engine):
    buf = np.frombuffer(b"running run Running", dtype=np.uint8)
    assert bytes(check_one(engine, buf, [0, 19], stop=[b"running"])) == b"        run Running"
    assert bytes(check_one(engine, buf, [0, 19], stop=[b"run"])) == b"run         Running"
    assert bytes(check_one(engine, buf, [0, 19], stop=[b"run"], lower=True)) == b"run         run    "
    assert bytes(check_one(engine, buf, [0, 19], min_len=4)) == b"run         Running"
    assert bytes(check_one(engine, buf, [0, 4, 19])) == b"running run Running"       # runn | ing: two tokens, both their own stems


def test_empty_inputs(engine):
    buf = np.frombuffer(b"running", dtype=np.uint8)
    o = engine.analyze(buf, np.zeros(1, dtype=np.uint64), stem=True)            # ndocs == 0
    assert o.ndocs == 0 and bytes(out_bytes(engine, o)) == b"running"
    o = engine.analyze(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), stem=True)
    assert o.nbytes == 0 and o.ndocs == 0 and engine.analyze_info()["grid"] == 0
    o = engine.analyze(np.zeros(0, dtype=np.uint8), np.zeros(4, dtype=np.uint64), stem=True)
    assert o.nbytes == 0 and o.ndocs == 3
    o = engine.analyze(buf, np.array([3, 3, 3], dtype=np.uint64), stem=True)     # only empty documents
    assert bytes(out_bytes(engine, o)) == b"running" and engine.analyze_info()["stemmed_tokens"] == 0
    o = engine.analyze(buf, np.array([0, 0, 7, 7], dtype=np.uint64), stem=True)
    assert bytes(out_bytes(engine, o)) == b"run    " and engine.analyze_info()["stemmed_tokens"] == 1
    a = tfidf_abi.analyzer(stem=True)[0]
    a.stemmer = 2
    c, keep = tfidf_abi._host_corpus(buf, np.array([0, 7], dtype=np.uint64))
    assert tfidf_abi.lib().tfidf_analyze(engine.h, a, c, 0, tfidf_abi.Corpus()) == tfidf_abi.E_INVAL


def test_info_is_size_prefixed(engine):
    """a caller built against the struct without stemmed_tokens gets its own size filled and nothing behind it"""
    engine.analyze(np.frombuffer(b"running", dtype=np.uint8), np.array([0, 7], dtype=np.uint64), stem=True)
    t = tfidf_abi.AnalyzeInfo()
    old = tfidf_abi.AnalyzeInfo.stemmed_tokens.offset
    assert old == 64 and C.sizeof(tfidf_abi.AnalyzeInfo) == 72 and C.sizeof(tfidf_abi.Analyzer) == 40
    t.size, t.stemmed_tokens = old, 0xDEADBEEF
    assert tfidf_abi.lib().tfidf_last_analyze_info(engine.h, C.byref(t)) == 0
    assert t.size == old and t.stemmed_tokens == 0xDEADBEEF and t.nbytes == 7 and t.grid == 1
    assert engine.analyze_info()["stemmed_tokens"] == 1


def test_repeated_call_allocates_nothing(engine, corpus):
    c = corpus["case"]["full"]
    with device_corpus(corpus["data"], corpus["off"], shift=9) as dc:
        engine.analyze(dc, stem=True, **c["kw"])
        engine.analyze(corpus["data"], corpus["off"], stem=True, **c["kw"])
        before = engine.alloc_counters()
        engine.analyze(dc, stem=True, **c["kw"])
        o = engine.analyze(corpus["data"], corpus["off"], stem=True, **c["kw"])
        assert engine.alloc_counters() == before
        assert np.array_equal(out_bytes(engine, o), c["ref"])


# ---- 4. pipeline ----

TWELVE = [b"The connection was lost.", b"Connected devices are running", b"a runner ran", b"Connections, relational databases",
          b"hopping and hoping", b"nothing here", b"She is connecting the wires", b"connective tissue", b"agreed; disagreed",
          b"ponies and caresses", b"sky happy", b"generalizations oscillators"]


def test_pipeline(engine):
    data, off = docs_to_arrays(TWELVE)
    kw = dict(lower=True, punct=True)
    ref = stem_ref.analyze(data, off, **kw)
    host = tfidf_abi.analyze_host(data, off, stem=True, **kw)
    assert np.array_equal(host, ref)
    with device_corpus(data, off, shift=5) as c:
        engine.run_corpus(engine.analyze(c, stem=True, **kw))
        res = engine.fetch()
        assert_same_result(res, oracle_py.run(host, off))
        assert list(res["terms"]) == sorted(set(tokens_of(ref, off)))
        assert b"connect" in res["terms"] and b"connection" not in res["terms"]
        q = np.frombuffer(b"connection\nconnected", dtype=np.uint8)
        qoff = np.array([0, 11, 20], dtype=np.uint64)
        qan = bytes(tfidf_abi.analyze_host(q, qoff, stem=True, **kw))
        assert qan == b"connect   \nconnect  "
        hits = engine.query([qan[0:11], qan[11:20]], 10)
        n = int(hits["nhits"][0])
        assert n == int(hits["nhits"][1]) == 5
        assert np.array_equal(hits["doc"][0, :n], hits["doc"][1, :n]) and np.array_equal(hits["score"][0, :n], hits["score"][1, :n])
        plain = engine.query([b"connection"], 10)          # unanalyzed: the term is not in the table
        assert int(plain["nhits"][0]) == 0


# ---- 5. CLI ----

@pytest.mark.parametrize("extra", [[], ["--shards", "2"]])
def test_cli(tmp_path, extra):
    docs = [d + b" " + TWELVE[(i + 3) % 12] for i, d in enumerate(TWELVE)]
    fit, held = docs[:9], docs[9:]                      # ids 1..9: "docN@" order is numeric
    qfile = b"Connection, running\n(ponies)\n\nhappy SKY relational"
    kw = dict(lower=True, punct=True)

    def ref_of(raw, off=None):
        buf = np.frombuffer(raw, dtype=np.uint8)
        return bytes(stem_ref.analyze(buf, [0, len(buf)] if off is None else off, **kw))

    for name in ("a", "b"):                             # a: the raw files and the options; b: the reference's bytes, no options
        (tmp_path / name / "input").mkdir(parents=True)
        (tmp_path / name / "new").mkdir()
        for sub, group in (("input", fit), ("new", held)):
            for i, d in enumerate(group):
                (tmp_path / name / sub / ("doc%d" % (i + 1))).write_bytes(d if name == "a" else ref_of(d))
    qoff = [0] + [i + 1 for i, c in enumerate(qfile) if c == 0x0A] + [len(qfile)]
    (tmp_path / "a" / "q.txt").write_bytes(qfile)
    (tmp_path / "b" / "q.txt").write_bytes(ref_of(qfile, qoff))
    opts = ["--lower", "--strip-punct", "--stem"]
    common = ["--query", "q.txt", "--transform", "new", "--save-model", "model.bin"] + extra
    for name, o in (("a", opts), ("b", [])):
        p = subprocess.run([tfidf_abi.CLI_PATH] + o + common, cwd=tmp_path / name, capture_output=True, timeout=120)
        assert p.returncode == 0, p.stderr
    for f in ("output.txt", "hits.txt", "transform.txt"):
        want = (tmp_path / "b" / f).read_bytes()
        assert want and (tmp_path / "a" / f).read_bytes() == want, f
    assert b"@connect\t" in (tmp_path / "a" / "output.txt").read_bytes()
    assert b"q1\t" in (tmp_path / "a" / "hits.txt").read_bytes()
    # serving from the model file with the same options
    p = subprocess.run([tfidf_abi.CLI_PATH, "--model", "model.bin", "--transform", "new", "--transform-file", "served.txt"] + opts,
                       cwd=tmp_path / "a", capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "a" / "served.txt").read_bytes() == (tmp_path / "b" / "transform.txt").read_bytes()
