"""tfidf_ngrams on the GPU (include/tfidf.h, section "n-grams"; csrc/ngram.hip) against
tests/ngram_ref.py, the definition in plain Python, and against tfidf_ngrams_host: inputs at
every alignment inside windows, tokens placed across the input's and the output's tile edges,
long tokens, dense and empty segments, the two slots, the run of a shingled corpus against the
oracle, three shards, serving and the CLI."""
import subprocess

import numpy as np
import pytest

import ngram_ref
import oracle_py
import tfidf_abi
from helpers import assert_k1_instance, assert_same_result, device_corpus, docs_to_arrays, load_golden, windowed

pytestmark = pytest.mark.gpu


def fetch_out(e, c):
    assert c.flags & tfidf_abi.TFIDF_CORPUS_DEVICE and c.bytes % 16 == 0
    return e.corpus_bytes(c)


def check(e, data, off, lo, hi, src=None, **kw):
    """shingles data/off (or the Corpus src that holds them) and compares bytes, offsets and
    counters with the reference; returns the reference output"""
    off = np.asarray(off, dtype=np.uint64)
    want, want_off = ngram_ref.ngrams(data, off, lo, hi, kw.get("joiner", 0) or 0x5F)
    o = e.ngrams(data, off, lo, hi, **kw) if src is None else e.ngrams(src, min_n=lo, max_n=hi, **kw)
    assert o.nbytes == len(want) and o.ndocs == len(off) - 1
    got, got_off = fetch_out(e, o)
    assert got_off.tolist() == want_off
    if bytes(got) != want:
        bad = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError((lo, hi, bad, bytes(got[max(0, bad - 40):bad + 40]), want[max(0, bad - 40):bad + 40]))
    info = e.ngram_info()
    ntok, ngr = ngram_ref.counts(data, off, lo, hi)
    assert (info["nbytes_in"], info["nbytes_out"], info["ndocs"]) == (len(data), len(want), len(off) - 1)
    assert (info["ntokens"], info["ngrams"]) == (ntok, ngr)
    assert info["grid"] == -(-len(want) // info["tile_bytes"])
    return want


def tile_bytes(e):
    e.ngrams(np.frombuffer(b"a b", dtype=np.uint8), [0, 3])
    return e.ngram_info()["tile_bytes"]


# ---- 1. device vs reference and host ----

@pytest.fixture(scope="module")
def big():
    return windowed(ngram_ref.big_corpus(), 37, 21)


@pytest.mark.parametrize("rng", ngram_ref.RANGES)
@pytest.mark.parametrize("shift", [None, 0, 1, 7, 15])
def test_device_vs_reference_and_host(engine, big, rng, shift):
    data, off = big
    if shift is None:
        want = check(engine, data, off, *rng)
    else:
        with device_corpus(data, off, shift=shift) as c:
            want = check(engine, data, off, *rng, src=c)
    assert len(want) > 100_000
    if shift in (None, 7):
        got, got_off = tfidf_abi.ngrams_host(data, off, *rng)
        assert bytes(got) == want and got_off.tolist() == ngram_ref.ngrams(data, off, *rng)[1]


# ---- 2. input tile edges ----

def filler(n):
    return np.frombuffer((b"ab " * (n // 3 + 1))[:n], dtype=np.uint8).copy()


def place(buf, at, tok):
    if at > 0:
        buf[at - 1] = 0x20
    buf[at:at + len(tok)] = np.frombuffer(tok, dtype=np.uint8)
    if at + len(tok) < len(buf):
        buf[at + len(tok)] = 0x20


@pytest.mark.parametrize("L", [1, 2, 16, 63, 200])
def test_token_across_input_tile_edges(engine, L):
    n = 2 * 4096 + 100 + L            # the filler, and room for the token placed at the last start
    tok = bytes([0x7A] + [0x61 + i % 25 for i in range(L - 1)])
    for edge in (4096, 8192):
        for at in range(edge - L - 1, edge + 2):
            buf = filler(n)
            place(buf, at, tok)
            want = check(engine, buf, [0, n], 2, 2)
            assert want.count(tok) == 2


# ---- 3. output tile edges ----

def test_output_tile_edges(engine):
    T = tile_bytes(engine)
    period, phases = 54, set()            # "ab cde f " under (1, 3): segments of 19, 19 and 16 bytes
    for lead in range(48):
        doc = (b"z" * lead + b" " if lead else b"") + b"ab cde f " * (3 * T // period + 3)
        want = check(engine, np.frombuffer(doc, dtype=np.uint8), [0, len(doc)], 1, 3)
        assert len(want) > 3 * T + 16
        first = (lead + 1) + (lead + 4) + (lead + 8) if lead else 0      # the lead token's segment
        assert want[first:first + period] == b"ab ab_cde ab_cde_f cde cde_f cde_f_ab f f_ab f_ab_cde "
        phases |= {(e - first) % period for e in (T, 2 * T, 3 * T)}
    # every byte of the period, so every joiner, blank and component start, was a tile's first byte
    assert phases == set(range(period))


# ---- 4. long tokens ----

def test_long_tokens(engine):
    T = tile_bytes(engine)
    short = b"ab cd efg "
    doc = short * 3 + b"L" * 5000 + b" " + short * 2 + b"M" * 70_000 + b" " + short + b"N" * 5000
    want = check(engine, np.frombuffer(doc, dtype=np.uint8), [0, len(doc)], 1, 2)
    assert len(want) > 3 * 70_000 and 70_000 > 16 * T      # tiles without a segment start
    check(engine, np.frombuffer(doc, dtype=np.uint8), [0, 40, 40 + 2500, len(doc)], 1, 2)   # a boundary inside the first


# ---- 5. dense segments ----

def test_dense_segments(engine):
    T = tile_bytes(engine)
    doc = np.frombuffer(b"a " * (3 * T // 2 + 50), dtype=np.uint8)
    want = check(engine, doc, [0, len(doc)], 1, 1)           # 2-byte segments: the most a tile can touch
    assert len(want) > 3 * T and want == bytes(doc)
    want = check(engine, doc, [0, len(doc)], 8, 8)
    assert want.startswith(b"a_a_a_a_a_a_a_a a_a_") and len(want) > 3 * T


# ---- 6. boundaries and empties ----

def test_boundaries_and_empties(engine):
    data, off = ngram_ref.LITERAL
    for rng, (want, want_off) in ngram_ref.LITERAL_OUT.items():
        assert check(engine, np.frombuffer(data, dtype=np.uint8), off, *rng) == want
        with device_corpus(np.frombuffer(data, dtype=np.uint8), off, shift=3) as c:
            check(engine, np.frombuffer(data, dtype=np.uint8), off, *rng, src=c)
    buf = np.frombuffer(b"Qa b  \n c ddQ", dtype=np.uint8)     # junk directly outside the window on both sides
    assert check(engine, buf, [1, 12], 1, 2) == b"a a_b b b_c c c_dd dd "
    assert check(engine, buf, [1, 2, 6, 6, 12], 2, 3) == b"c_dd "          # documents with m < min_n
    assert check(engine, buf, [1, 2, 4, 9], 2, 2) == b""                   # nothing but such documents
    assert check(engine, buf, [4, 7, 7], 1, 2) == b""                      # all-blank documents
    assert check(engine, buf, [5], 1, 2) == b""                            # ndocs == 0
    assert check(engine, buf, [3, 3, 3], 1, 2) == b""
    z = np.zeros(0, dtype=np.uint8)
    assert check(engine, z, [0], 1, 2) == b"" and check(engine, z, [0, 0, 0, 0], 2, 8) == b""   # nbytes == 0
    assert check(engine, buf, [1, 12], 1, 2, joiner=0x2B) == b"a a+b b b+c c c+dd dd "
    # thousands of documents below min_n between two others: empty segments inside one tile,
    # more than a workgroup stages
    docs = [b"x y z "] + [b"q "] * 6000 + [b"x y z"]
    d, o = docs_to_arrays(docs)
    assert check(engine, d, o, 2, 2) == b"x_y y_z x_y y_z "
    assert check(engine, d, o, 1, 2).count(b"q ") == 6000


# ---- 7. slots ----

def test_slots(engine, big):
    g = load_golden("g5_w3")
    kw = dict(lower=True, punct=True, min_len=2, stop=[b"the", b"of"])
    c = engine.ngrams(engine.analyze(g["data"], g["off"], slot=tfidf_abi.AN_SLOT_CORPUS, **kw), min_n=1, max_n=2,
                      slot=tfidf_abi.NG_SLOT_CORPUS)
    adata = tfidf_abi.analyze_host(g["data"], g["off"], **kw)
    assert bytes(fetch_out(engine, c)[0]) == ngram_ref.ngrams(adata, g["off"], 1, 2)[0]
    for bad_slot in (0, 2):                                   # its own slot's buffer as input; a slot that does not exist
        with pytest.raises(tfidf_abi.TfidfError) as ex:
            engine.ngrams(c, slot=bad_slot)
        assert ex.value.rc == tfidf_abi.E_INVAL
    engine.run_corpus(c)
    text = engine.text()
    assert b"_" in text
    data, off = big
    b1 = engine.ngrams(data, off, 1, 3, slot=tfidf_abi.NG_SLOT_BATCH)
    assert b1.bytes != c.bytes
    assert bytes(fetch_out(engine, b1)[0]) == ngram_ref.ngrams(data, off, 1, 3)[0]
    assert engine.text() == text                              # the run's corpus (slot 0) is untouched
    again = engine.ngrams(c, min_n=1, max_n=1, slot=tfidf_abi.NG_SLOT_BATCH)   # slot 0's output into slot 1
    assert bytes(fetch_out(engine, again)[0]) == bytes(fetch_out(engine, c)[0])
    lib, p, out = tfidf_abi.lib(), tfidf_abi.ngram_params(1, 2), tfidf_abi.Corpus()
    for off_bad in ([0, 5, 4], [0, len(data) + 1]):
        hc, keep = tfidf_abi._host_corpus(data, np.array(off_bad, dtype=np.uint64))
        assert lib.tfidf_ngrams(engine.h, p, hc, 0, out) == tfidf_abi.E_INVAL
    hc, keep = tfidf_abi._host_corpus(data, off)
    assert lib.tfidf_ngrams(engine.h, None, hc, 0, out) == tfidf_abi.E_INVAL
    assert lib.tfidf_ngrams(engine.h, p, None, 0, out) == tfidf_abi.E_INVAL
    assert lib.tfidf_ngrams(engine.h, p, hc, 0, None) == tfidf_abi.E_INVAL
    assert lib.tfidf_ngrams(engine.h, tfidf_abi.ngram_params(2, 1), hc, 0, out) == tfidf_abi.E_INVAL


def test_repeated_call_allocates_nothing(engine, big):
    data, off = big
    want = ngram_ref.ngrams(data, off, 1, 3)[0]
    with device_corpus(data, off, shift=9) as c:
        engine.ngrams(c, min_n=1, max_n=3)
        engine.ngrams(data, off, 1, 3)
        before = engine.alloc_counters()
        engine.ngrams(c, min_n=1, max_n=3)
        o = engine.ngrams(data, off, 1, 3)
        assert engine.alloc_counters() == before
        assert bytes(fetch_out(engine, o)[0]) == want


# ---- 8. run parity ----

@pytest.mark.parametrize("case", ["g2_twelve_docs", "g5_w3"])
def test_run_parity(engine, case):
    g = load_golden(case)
    sdata, soff = tfidf_abi.ngrams_host(g["data"], g["off"], 1, 2)
    ora = oracle_py.run(sdata, soff)
    with device_corpus(g["data"], g["off"], shift=7) as c:
        engine.run_corpus(engine.ngrams(c, min_n=1, max_n=2))
        assert_k1_instance(engine.info(), "sl_fast")          # an aligned output whatever the input's base
        res = engine.fetch()
        assert_same_result(res, ora)
        if case == "g5_w3":                                   # long terms: verified against the slot's buffer
            assert sum(len(t) >= 16 and b"_" in t for t in res["terms"]) > 100
        assert engine.text() == ora["output_txt"]


def test_three_local_shards(engine, tmp_path):
    g = load_golden("g5_w3")
    docs = [bytes(g["data"][int(b):int(e)]) for b, e in zip(g["off"][:-1], g["off"][1:])][:9]   # ids 1..9: "docN@" order is numeric
    d9, o9 = docs_to_arrays(docs)
    engine.run_corpus(engine.ngrams(d9, o9, 1, 2))
    single = engine.text()
    assert single == oracle_py.run(*tfidf_abi.ngrams_host(d9, o9, 1, 2))["output_txt"]
    with tfidf_abi.Group(3, devices=[0, 0, 0]) as grp:
        shards = []
        for r in range(3):
            d, o = docs_to_arrays(docs[3 * r:3 * r + 3])
            shards.append(grp.ranks[r].ngrams(d, o, 1, 2, doc_ids=[3 * r + 1, 3 * r + 2, 3 * r + 3], ndocs_total=9))
        grp.run(shards)
        grp.write_output(str(tmp_path / "out.txt"))
    assert (tmp_path / "out.txt").read_bytes() == single


# ---- 9. serving ----

SERVE_DOCS = [b"we flew to new york in may", b"we flew to york new in may", b"the city of york is old", b"a new day in may",
              b"nobody flew", b"an old city"]


def test_serving(engine):
    data, off = docs_to_arrays(SERVE_DOCS)
    sdata, soff = tfidf_abi.ngrams_host(data, off, 1, 2)
    q = [bytes(tfidf_abi.ngrams_host(np.frombuffer(t, dtype=np.uint8), [0, len(t)], 1, 2)[0]) for t in (b"new york", b"york new")]
    assert q[0] == b"new new_york york "
    engine.run_host(sdata, soff)
    want = engine.query(q, 6)
    c = engine.ngrams(data, off, 1, 2)
    engine.run_corpus(c)
    hits = engine.query(q, 6)
    for k in ("nhits", "nmatch", "nterms_found", "doc"):
        assert np.array_equal(hits[k], want[k]), k
    assert np.array_equal(hits["score"].view(np.uint64), want["score"].view(np.uint64))
    # documents 1 and 2 hold the same words: the bigram alone tells "new york" from "york new"
    rank = [hits["doc"][i, :int(hits["nhits"][i])].tolist() for i in range(2)]
    assert rank[0].index(1) < rank[0].index(2) and rank[1].index(2) < rank[1].index(1)
    assert hits["nterms_found"].tolist() == [3, 3]
    # the shingled corpus as a batch (slot 1) gets the run's own pairs
    rows = engine.transform_corpus(engine.ngrams(data, off, 1, 2, slot=tfidf_abi.NG_SLOT_BATCH))
    f = engine.fetch()
    assert rows["npairs"] == f["npairs"] and not rows["doc_oov"].any()
    ro = rows["row_off"].tolist()
    for r in range(len(SERVE_DOCS)):
        idx = np.flatnonzero(f["doc"] == r + 1)
        a, b = ro[r], ro[r + 1]
        assert rows["term"][a:b].tolist() == f["term"][idx].tolist() and rows["count"][a:b].tolist() == f["count"][idx].tolist()
        assert np.array_equal(rows["score"][a:b].view(np.uint64), f["score"][idx].view(np.uint64))
        assert rows["words"][a:b] == [f["terms"][t] for t in f["term"][idx].tolist()]


# ---- 10. CLI ----

@pytest.mark.parametrize("extra", [[], ["--shards", "2"]])
def test_cli(tmp_path, extra):
    docs = [d.replace(b"new", b"New,").replace(b"may", b"(May)") for d in SERVE_DOCS]
    (tmp_path / "input").mkdir()
    for i, d in enumerate(docs):
        (tmp_path / "input" / ("doc%d" % (i + 1))).write_bytes(d)
    qfile = b"NEW york!\nYork new\n"
    (tmp_path / "q.txt").write_bytes(qfile)
    p = subprocess.run([tfidf_abi.CLI_PATH, "--lower", "--strip-punct", "--ngrams", "1-2", "--query", "q.txt"] + extra,
                       cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    kw = dict(lower=True, punct=True)
    data, off = docs_to_arrays(docs)
    sdata, soff = tfidf_abi.ngrams_host(tfidf_abi.analyze_host(data, off, **kw), off, 1, 2)
    ora = oracle_py.run(sdata, soff)
    assert (tmp_path / "output.txt").read_bytes() == ora["output_txt"] and b"@new_york\t" in ora["output_txt"]
    qoff = [0, 10, len(qfile)]
    qdata, qsoff = tfidf_abi.ngrams_host(tfidf_abi.analyze_host(np.frombuffer(qfile, dtype=np.uint8), qoff, **kw), qoff, 1, 2)
    queries = [bytes(qdata[int(b):int(e)]) for b, e in zip(qsoff[:-1], qsoff[1:])]
    assert queries == [b"new new_york york ", b"york york_new new "]
    with tfidf_abi.Engine(0) as e:
        e.run_host(sdata, soff)
        hits = e.query(queries, 10)
    want = b"".join(b"q%d\tdoc%d\t%.16f\n" % (q + 1, hits["doc"][q, i], hits["score"][q, i])
                    for q in range(2) for i in range(int(hits["nhits"][q])))
    got = (tmp_path / "hits.txt").read_bytes()
    assert want and got == want
    lines = got.split(b"\n")
    assert lines.index(next(x for x in lines if x.startswith(b"q1\tdoc1\t"))) < lines.index(next(x for x in lines if x.startswith(b"q1\tdoc2\t")))


@pytest.mark.parametrize("spec", ["0", "3-2", "9", "1-"])
def test_cli_bad_spec(tmp_path, spec):
    (tmp_path / "input").mkdir()
    (tmp_path / "input" / "doc1").write_bytes(b"a b")
    p = subprocess.run([tfidf_abi.CLI_PATH, "--ngrams", spec], cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode != 0 and p.stderr.startswith(b"usage: tfidf") and b"--ngrams SPEC" in p.stderr
    assert not (tmp_path / "output.txt").exists()
