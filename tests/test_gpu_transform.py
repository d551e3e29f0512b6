"""tfidf_transform on the GPU against the plain-Python reference (transform_ref.py): unseen
documents scored with a finished run's vocabulary, df, N and idf.  Integers are compared
exactly, scores as u64 bits, words by their bytes."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import tfidf_abi
import tfidf_configs
from conftest import golden_cases, GOLDEN
from helpers import K1_INSTANCES, device_corpus, docs_to_arrays, k1_engine, load_golden, windowed
from transform_ref import Model, bits, check, split_docs, totals

pytestmark = pytest.mark.gpu


def fit(e, docs, n_total: int = 0):
    data, off = docs_to_arrays(docs)
    e.run_host(data, off, None, n_total)
    return Model(data, off, None, n_total)


def transform(e, docs):
    data, off = docs_to_arrays(docs)
    return e.transform(data, off), off


def golden_docs(case):
    g = load_golden(case)
    return split_docs(g["data"], g["off"])


# ---- 1. self-transform: a document of the run gets the run's own pairs bit for bit ----

def assert_self_transform(e, docs):
    res, off = transform(e, docs)
    f = e.fetch()
    by_doc = {}
    for i, d in enumerate(f["doc"].tolist()):
        by_doc.setdefault(d, []).append(i)
    ro = res["row_off"].tolist()
    size_of = dict(zip(f["doc_id"].tolist(), f["doc_size"].tolist()))
    assert res["npairs"] == f["npairs"]
    for r in range(len(docs)):
        idx = by_doc.get(r + 1, [])
        a, b = ro[r], ro[r + 1]
        assert b - a == len(idx), r
        assert res["term"][a:b].tolist() == f["term"][idx].tolist(), r
        assert res["count"][a:b].tolist() == f["count"][idx].tolist(), r
        assert res["df"][a:b].tolist() == f["df"][idx].tolist(), r
        assert np.array_equal(bits(res["score"][a:b]), bits(f["score"][idx])), r
        assert res["words"][a:b] == [f["terms"][t] for t in f["term"][idx].tolist()], r
        assert int(res["doc_size"][r]) == size_of[r + 1], r
    assert not res["doc_oov"].any()
    return res


@pytest.mark.parametrize("case", golden_cases())
def test_self_transform(engine, case):
    docs = golden_docs(case)
    m = fit(engine, docs)
    res = assert_self_transform(engine, docs)
    check(res, m.rows(docs), docs_to_arrays(docs)[1], engine.fetch()["terms"])


# ---- 2. held-out documents; the counts keep the case from passing vacuously ----

HELD_OUT = [   # fit on the first documents, transform the rest: tokens, OOV tokens, pairs, pairs scoring +0.0
    ("g4_config1", 5, dict(tokens=6000, oov=1494, pairs=9)),
    ("g5_w3", 13, dict(tokens=1162, oov=204, pairs=414, zero=48)),
    ("g1_whitespace", 2, dict(tokens=1, oov=1, pairs=0)),
    ("g2_twelve_docs", 8, dict(tokens=10, oov=0, pairs=8, zero=4)),
]


def assert_held_out(e, case, nfit, want, n_total: int = 0):
    docs = golden_docs(case)
    m = fit(e, docs[:nfit], n_total)
    rows = m.rows(docs[nfit:])
    got = totals(rows)
    for k, v in want.items():
        assert got[k] == v, (case, k, got)
    res, off = transform(e, docs[nfit:])
    check(res, rows, off, e.fetch()["terms"])
    return res


@pytest.mark.parametrize("case,nfit,want", HELD_OUT)
def test_held_out(engine, case, nfit, want):
    res = assert_held_out(engine, case, nfit, want)
    info = engine.transform_info()
    assert (info["ntokens"], info["noov"], info["npairs"]) == (want["tokens"], want["oov"], want["pairs"])
    assert info["nslices"] >= 1 and info["ndocs"] == res["ndocs"]


# ---- 3. N over IDF_FULL_MAX: the idf table holds the run's distinct df values only ----

def test_distinct_df_idf_table(engine):
    want = dict(tokens=1162, oov=204, pairs=414)
    assert_held_out(engine, "g5_w3", 13, want, n_total=300000)
    docs = golden_docs("g5_w3")[:13]
    m = fit(engine, docs, 300000)
    assert m.N == 300000
    res = assert_self_transform(engine, docs)
    check(res, m.rows(docs), docs_to_arrays(docs)[1], engine.fetch()["terms"])


# ---- 4. bytes ----

def test_bytes(engine):
    fitted = [b"ab cd \0zz x\0y", b"ab\0cd tail q\x01r", b"\x0bv\x0cf\rr\nn\tt s", b"\0"]
    m = fit(engine, fitted)
    assert b"" in m.df and b"ab" in m.df and b"x" in m.df
    terms = engine.fetch()["terms"]
    batch = [
        b"ab\0cd ab \0x",                       # "ab" twice (one cut at its NUL), the empty term
        b"v\x0bf\x0cr\rn\nt\ts x",              # each of the six separators
        b"  q\x01r   tail",                     # a token ending at the document's last byte
        b" \t\n\x0b\x0c\r ",                    # whitespace only
        b"", b"", b"cd",                        # two adjacent empty documents, then a token at a boundary
        b"unseen \0\0 ab",
        b"",
    ]
    rows = m.rows(batch)
    assert rows[0]["words"] == [b"", b"ab"] and rows[0]["count"] == [1, 2]
    assert rows[1]["doc_size"] == 7 and rows[1]["doc_oov"] == 0
    assert rows[3]["doc_size"] == 0 and rows[4]["words"] == []
    res, off = transform(engine, batch)
    check(res, rows, off, terms)
    res = engine.transform(np.zeros(0, np.uint8), np.zeros(1, np.uint64))       # ndocs == 0
    assert res["ndocs"] == 0 and res["npairs"] == 0 and res["row_off"].tolist() == [0]
    res, off = transform(engine, [b"", b""])
    check(res, m.rows([b"", b""]), off, terms)


# ---- 5. long terms ----

LONG = [b"l" * 14 + b"a", b"m" * 15 + b"b", b"n" * 16 + b"c", b"o" * 39 + b"d", b"p" * 299 + b"e"]   # 15, 16, 17, 40, 300 bytes


def long_cases():
    fitted = [b" ".join(LONG[:3]) + b" x", LONG[3] + b" y " + LONG[4], LONG[4] + b" x"]
    variants = [w[:-1] + b"Z" for w in LONG]
    batch = [b" ".join(LONG), b" ".join(variants), LONG[2][:16] + b" " + LONG[0][:14], LONG[4] + b" " + variants[4] + b" " + LONG[4]]
    return fitted, batch


def assert_long_terms(e):
    fitted, batch = long_cases()
    m = fit(e, fitted)
    rows = m.rows(batch)
    assert sorted(rows[0]["words"]) == sorted(LONG) and rows[0]["doc_oov"] == 0
    assert rows[1]["words"] == [] and rows[1]["doc_oov"] == 5
    assert rows[2]["words"] == [] and rows[2]["doc_oov"] == 2       # the 16-byte prefix of the 17-byte term
    assert rows[3]["count"] == [2] and rows[3]["doc_oov"] == 1
    res, off = transform(e, batch)
    check(res, rows, off, e.fetch()["terms"])
    assert sorted(res["word_len"][:5].tolist()) == [15, 16, 17, 40, 300]


def test_long_terms(engine):
    assert_long_terms(engine)


_LONGTAG_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2]); sys.path.insert(0, sys.argv[3])
import numpy as np, tfidf_abi
from helpers import docs_to_arrays
from test_gpu_query import long_key16
from transform_ref import Model, check
for n in (40, 300):
    rng = np.random.default_rng(n)
    cand = rng.integers(97, 123, (300000, n), dtype=np.uint8)
    key = long_key16(cand)
    present = bytes(cand[0])
    hit = [i for i in range(1, len(cand)) if key[i] == key[0] and bytes(cand[i]) != present]
    assert hit, "no collision among the candidates"
    absent = bytes(cand[hit[0]])
    with tfidf_abi.Engine(0) as e:
        data, off = docs_to_arrays([present + b" x", b"y x"])
        e.run_host(data, off)
        m = Model(data, off)
        bdata, boff = docs_to_arrays([absent + b" " + present + b" x", absent])
        rows = m.rows([absent + b" " + present + b" x", absent])
        res = e.transform(bdata, boff)
        check(res, rows, boff, e.fetch()["terms"])
        print("RESULT", n, res["doc_oov"].tolist(), sorted(res["word_len"].tolist()))
"""


def test_long_term_key_collision_is_out_of_vocabulary():
    """lib/libtfidf_hip_longtag16.so cuts long terms' keys to 16 bits: an unseen 40- or 300-byte
    word whose key equals a vocabulary word's (found by brute force, test_gpu_query.long_key16)
    is out of vocabulary all the same: the bytes decide."""
    here = os.path.dirname(os.path.abspath(__file__))
    pydir = os.path.join(os.path.dirname(here), "parallel-systems-mpi-tfidf_amd", "python")
    env = dict(os.environ, TFIDF_LIB="longtag16")
    r = subprocess.run([sys.executable, "-c", _LONGTAG_CHILD, pydir, here, os.path.join(os.path.dirname(here), "oracle")],
                       env=env, capture_output=True, text=True, timeout=240, cwd=here)
    out = [l for l in r.stdout.splitlines() if l.startswith("RESULT")]
    assert out == ["RESULT 40 [1, 1] [1, 40]", "RESULT 300 [1, 1] [1, 300]"], r.stdout + r.stderr[-3000:]


# ---- 6. tiles and alignment ----

SEPS = [b" ", b"\t", b"\n", b"\x0b", b"\x0c", b"\r"]


def random_word(rng):
    return bytes(rng.integers(97, 123, int(rng.integers(1, 25)), dtype=np.uint8))


@pytest.fixture(scope="module")
def tiles():
    """about 256 KiB: 300 documents of uneven size (some empty), token lengths 1-24, one to three
    separator bytes, words from a 2000-word fitted vocabulary and about 15 % unseen ones"""
    rng = np.random.default_rng(20260)
    vocab = sorted({random_word(rng) for _ in range(2200)})[:2000]
    fitted = [b" ".join(vocab[i::7]) for i in range(7)]
    ntok = rng.integers(0, 100, 300)
    ntok[rng.integers(0, 300, 20)] = 0
    ntok[[5, 150]] = [2500, 1800]
    docs = []
    for n in ntok.tolist():
        parts = []
        for _ in range(n):
            w = vocab[int(rng.integers(0, 2000))] if rng.random() >= 0.15 else random_word(rng) + b"#"
            parts.append(w + b"".join(SEPS[int(s)] for s in rng.integers(0, 6, int(rng.integers(1, 4)))))
        doc = b"".join(parts)
        docs.append(doc[:-1] if n and rng.random() < 0.5 else doc)   # half end in a token byte
    fdata, foff = docs_to_arrays(fitted)
    m = Model(fdata, foff)
    rows = m.rows(docs)
    t = totals(rows)
    assert 200_000 < sum(len(d) for d in docs) < 330_000 and 0.10 < t["oov"] / t["tokens"] < 0.20
    return dict(fdata=fdata, foff=foff, docs=docs, rows=rows)


def same(a, b, shift_off: int = 0):
    for k in ("row_off", "doc_size", "doc_oov", "term", "count", "df", "word_len"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(bits(a["score"]), bits(b["score"]))
    assert np.array_equal(a["word_off"], b["word_off"] + np.uint64(shift_off))
    assert a["words"] == b["words"]


def test_tiles_and_alignment(engine, tiles):
    engine.run_host(tiles["fdata"], tiles["foff"])
    terms = engine.fetch()["terms"]
    data, off = docs_to_arrays(tiles["docs"])
    host = engine.transform(data, off)
    check(host, tiles["rows"], off, terms)
    wdata, woff = windowed(tiles["docs"], lead=37, trail=5)
    win = engine.transform(wdata, woff)
    check(win, tiles["rows"], woff, terms)
    same(win, host, 37)
    for shift in (0, 1, 7, 15):
        with device_corpus(data, off, shift=shift) as c:
            dev = engine.transform_corpus(c)
        check(dev, tiles["rows"], off, terms)
        same(dev, host)
    with device_corpus(wdata, woff, shift=3) as c:
        same(engine.transform_corpus(c), win)


# ---- 7. counts past u16 and rows past 4096 pairs ----

def c2_host(seed_delta: int = 0):
    p = tfidf_configs.plan("c2", scale=0.002)
    data, off = tfidf_abi.synth_host(p["seed"] + seed_delta, p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
    return p, data, off


def test_counts_and_large_rows(engine):
    p, data, off = c2_host()
    engine.run_host(data, off, p["doc_ids"], p["ndocs_total"])
    m = Model(data, off, p["doc_ids"], p["ndocs_total"])
    words = sorted(m.df)
    assert len(words) > 4200
    _, data2, off2 = c2_host(1)
    batch = [(words[17] + b" ") * 70000, b"\n".join(words[:4200]) + b" nowhere#"] + split_docs(data2, off2)
    rows = m.rows(batch)
    assert rows[0]["count"] == [70000] and len(rows[1]["words"]) == 4200 and rows[1]["doc_oov"] == 1
    assert totals(rows[2:])["pairs"] > 1000
    res, boff = transform(engine, batch)
    check(res, rows, boff, engine.fetch()["terms"])


# ---- 8. every K1 instance: the table the probe reads differs per instance ----

@pytest.mark.parametrize("instance", list(K1_INSTANCES))
def test_every_k1_instance(instance):
    with k1_engine(instance) as e:
        for case, nfit, want in HELD_OUT:
            assert_held_out(e, case, nfit, want)
        assert_long_terms(e)


# ---- 9. slices ----

def test_slices_under_a_small_budget(engine, tiles, monkeypatch):
    engine.run_host(tiles["fdata"], tiles["foff"])
    data, off = docs_to_arrays(tiles["docs"])
    want = engine.transform(data, off)
    assert engine.transform_info()["nslices"] == 1
    monkeypatch.setenv("TFIDF_TRANSFORM_MB", "1")
    with tfidf_abi.Engine(0) as e:
        e.run_host(tiles["fdata"], tiles["foff"])
        got = e.transform(data, off)
        info = e.transform_info()
        check(got, tiles["rows"], off, e.fetch()["terms"])
    same(got, want)
    # the largest document (2500 tokens, ~35 KB) is a slice of its own, far under 1 MiB of records
    assert info["nslices"] > 1 and info["scratch_bytes"] <= 1 << 20
    assert info["ntokens"] == want["ntokens"]


# ---- 10. hygiene ----

def test_state_allocations_and_result(tiles):
    data, off = docs_to_arrays(tiles["docs"])
    with tfidf_abi.Engine(0) as e:
        with pytest.raises(tfidf_abi.TfidfError) as ex:
            e.transform(data, off)
        assert ex.value.rc == tfidf_abi.E_STATE                     # before a run
        e.run_host(tiles["fdata"], tiles["foff"])
        text, hits = e.text(), e.query([b"x", tiles["docs"][5][:200]], 5)
        first = e.transform(data, off)
        a0 = e.alloc_counters()
        second = e.transform(data, off)
        assert e.alloc_counters() == a0                             # no device allocation
        same(first, second)
        assert e.text() == text
        again = e.query([b"x", tiles["docs"][5][:200]], 5)
        assert np.array_equal(again["doc"], hits["doc"]) and np.array_equal(bits(again["score"]), bits(hits["score"]))
        assert e.fetch()["output_txt"] == text
        bad = off.copy()
        bad[3] = bad[2] - 1 if bad[2] else bad[4] + 1
        for o in (bad, np.array([0, len(data) + 1], dtype=np.uint64)):
            with pytest.raises(tfidf_abi.TfidfError) as ex:
                e.transform(data, o)
            assert ex.value.rc == tfidf_abi.E_INVAL
        # a second run: the transform uses the new model
        docs = golden_docs("g2_twelve_docs")
        m = fit(e, docs[:8])
        res, boff = transform(e, docs[8:])
        check(res, m.rows(docs[8:]), boff, e.fetch()["terms"])


# ---- 11. group ----

@pytest.mark.parametrize("case", ["g2_twelve_docs", "g5_w3"])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_group_equals_single_engine(engine, case, K):
    g = load_golden(case)
    docs = split_docs(g["data"], g["off"])
    N = len(docs)
    order = np.argsort(tfidf_configs.doc_name_key(np.arange(1, N + 1)), kind="stable")
    first = tfidf_configs.shard_cuts([len(docs[i]) for i in order], K)
    m = fit(engine, docs)
    held = golden_docs("g5_w2")[:3] + [b"never#seen " + docs[0][:300]]
    batch = docs + held
    # a word that one shard alone holds and a word that every shard holds
    shard_words = []
    for r in range(K):
        ws = set()
        for i in order[first[r]:first[r + 1]]:
            ws.update(t.split(b"\0")[0] for t in docs[i].split())
        shard_words.append(ws)
    only_one = sorted(w for w in shard_words[0] if not any(w in s for s in shard_words[1:]))
    everywhere = sorted(set.intersection(*shard_words))
    # g2's twelve documents share their few words across every cut: only g5_w3 has single-shard words
    assert everywhere and (only_one or case == "g2_twelve_docs")
    batch.append(b" ".join(only_one[:1] + everywhere[:1] + only_one[:1]))
    single, boff = transform(engine, batch)
    rows = m.rows(batch)
    check(single, rows, boff, engine.fetch()["terms"])
    shards = []
    for r in range(K):
        sel = order[first[r]:first[r + 1]]
        d, o = docs_to_arrays([docs[i] for i in sel])
        shards.append((d, o, (sel + 1).astype(np.uint32), N))
    bdata, _ = docs_to_arrays(batch)
    with tfidf_abi.Group(K, devices=[0] * K, local=True) as grp:
        grp.run_host(shards)
        got = grp.transform(bdata, boff)
        check(got, rows, boff)
        for k in ("row_off", "doc_size", "doc_oov", "count", "df", "word_off", "word_len"):
            assert np.array_equal(got[k], single[k]), k
        assert np.array_equal(bits(got["score"]), bits(single["score"])) and got["words"] == single["words"]
        with device_corpus(bdata, boff) as c:
            with pytest.raises(tfidf_abi.TfidfError) as ex:
                grp.transform_corpus(c)
            assert ex.value.rc == tfidf_abi.E_INVAL


# ---- 12. CLI ----

@pytest.mark.parametrize("extra", [[], ["--shards", "2"]])
@pytest.mark.parametrize("case", ["g5_w3", "g3_bytes"])
def test_cli_transform_of_the_input_is_the_output(tmp_path, case, extra):
    shutil.copytree(os.path.join(GOLDEN, case, "input"), tmp_path / "input")
    p = subprocess.run([tfidf_abi.CLI_PATH, "--transform", "input"] + extra, cwd=tmp_path, capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    out = (tmp_path / "output.txt").read_bytes()
    assert out == load_golden(case)["output"] and out
    assert (tmp_path / "transform.txt").read_bytes() == out


def test_cli_transform_held_out(tmp_path):
    docs = golden_docs("g5_w3")
    (tmp_path / "input").mkdir()
    (tmp_path / "new").mkdir()
    for i, d in enumerate(docs[:13]):
        (tmp_path / "input" / ("doc%d" % (i + 1))).write_bytes(d)
    for i, d in enumerate(docs[13:]):
        (tmp_path / "new" / ("doc%d" % (i + 1))).write_bytes(d)
    p = subprocess.run([tfidf_abi.CLI_PATH, "--transform", "new", "--transform-file", "t.txt"], cwd=tmp_path,
                       capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr
    data, off = docs_to_arrays(docs[:13])
    rows = Model(data, off).rows(docs[13:])
    ids = tfidf_abi.doc_name_order(len(rows)).tolist()
    want = b"".join(b"doc%d@" % i + w + b"\t%.16f\n" % s for i in ids for w, s in zip(rows[i - 1]["words"], rows[i - 1]["score"]))
    assert want.count(b"\n") == 414
    assert (tmp_path / "t.txt").read_bytes() == want
