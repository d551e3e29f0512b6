"""tfidf_nb_fit / tfidf_nb_predict / tfidf_nb_predict_rows / tfidf_nb_export on the GPU
(csrc/nb.hip, csrc/engine_nb.cpp) against the plain-Python reference tests/nb_ref.py: every
integer and the u64 bits of every prior, weight and score are equal.  The reference's own agreement
with the plain-C host twin, and that it classifies the planted corpus, is established without a GPU
in test_nb_cpu.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import nb_ref as R
import oracle_py
import prune_ref
import tfidf_abi
from conftest import PKG, REPO, golden_cases
from helpers import docs_to_arrays, load_golden

pytestmark = pytest.mark.gpu

ALPHAS = [0.0, 0.5, float.fromhex("0x1p-1074"), float.fromhex("0x1p+900")]
VARIANTS = ["multinomial", "complement"]
FEATURES = ["count", "binary"]


def raises(rc, fn, *a, **kw):
    with pytest.raises(tfidf_abi.TfidfError) as ei:
        fn(*a, **kw)
    assert ei.value.rc == rc, ei.value


def check(e, ref: R.NRef, docs, labels, K, by_class=False, **kw):
    """fit, export and predict every resident document against the reference; returns (model, answer)"""
    model = ref.fit(docs, labels, K, **kw)
    assert model is not None
    e.nb_fit(docs, labels, K, **kw)
    R.assert_same_model(e.nb_export(), model)
    want = R.predict(model, ref.rows(), by_class=by_class)
    got = e.nb_predict(all_scores=True)
    assert [int(d) for d in got["doc"]] == ref.order and got["pos"].tolist() == list(range(len(ref.order)))
    R.assert_same_labels(got, want, K)
    info = e.nb_info()
    assert (info["nclasses"], info["nterms"], info["nlabelled"]) == (K, ref.V, len(docs))
    assert info["matrix_bytes"] == 16 * K * ref.V and info["predict_rows"] == len(ref.order)
    return model, want


def run_docs(e, docs):
    data, off = docs_to_arrays(docs)
    e.run_host(data, off)
    return R.NRef(oracle_py.run(data, off), list(range(1, len(docs) + 1))), data, off


def same_answer(a: dict, b: dict):
    assert a["label"].tolist() == b["label"].tolist()
    assert np.array_equal(R.bits(a["score"]), R.bits(b["score"]))
    assert np.array_equal(R.bits(a["scores"]), R.bits(b["scores"]))


@pytest.mark.parametrize("case", golden_cases())
def test_goldens_vs_reference(engine, case):
    g = load_golden(case)
    engine.run_host(g["data"], g["off"])
    ids = list(range(1, len(g["off"])))
    ref = R.NRef(oracle_py.run(g["data"], g["off"]), ids)
    for K in (1, 2, 3):
        labels = [d % K for d in ids]
        for variant in VARIANTS:
            for feature in FEATURES:
                for uniform in (False, True):
                    for alpha in ALPHAS:
                        check(engine, ref, ids, labels, K, variant=variant, feature=feature, alpha=alpha, uniform_prior=uniform)
    # the rows of a transform of the run's own corpus: the resident answer bit for bit
    rows = engine.transform(g["data"], g["off"])
    got = engine.nb_predict_rows(rows, all_scores=True)
    by_id = engine.nb_predict(ids, all_scores=True)                      # batch order is id order
    assert by_id["doc"].tolist() == ids and [ref.order[p] for p in by_id["pos"].tolist()] == ids
    same_answer(got, by_id)
    assert got["doc"].tolist() == got["pos"].tolist() == list(range(len(ids)))


SIZES = (0, 1, 3, 63, 64, 65, 66, 67, 4097)     # the 64-pair tile's tail and every remainder of the rows in flight


def shapes_corpus():
    """300 documents, 291 of them not empty: one of each size of SIZES (distinct words), the rest 2 to
    40 words from a pool of 500 with counts 1 to 3"""
    rng = np.random.default_rng(7)
    docs = []
    for i in range(300):
        if i < len(SIZES):
            n = SIZES[i]
            words = [b"s%d_%05d" % (i, j) for j in range(n)] if n > 67 else [b"p%03d" % ((37 * i + j) % 500) for j in range(n)]
        elif i % 37 == 0:
            words = []
        else:
            start, n = int(rng.integers(0, 500)), int(rng.integers(2, 41))
            words = [b"p%03d" % ((start + 3 * j) % 500) for j in range(n)]
        docs.append(b" ".join(b" ".join([w] * (1 + (k + i) % 3)) for k, w in enumerate(words)))
    return docs


@pytest.fixture(scope="module")
def shapes():
    docs = shapes_corpus()
    data, off = docs_to_arrays(docs)
    ref = R.NRef(oracle_py.run(data, off), list(range(1, len(docs) + 1)))
    assert sorted(set(len(r) for r in ref.by_pos) & set(SIZES)) == list(SIZES)
    assert sum(1 for r in ref.by_pos if r) >= 256
    return dict(docs=docs, data=data, off=off, ref=ref)


@pytest.mark.parametrize("K", [1, 2, 64, 65, 129, 256])
def test_one_to_four_accumulators_per_lane(engine, shapes, K):
    """both sides of every accumulator boundary, on documents of every size of SIZES"""
    ref = shapes["ref"]
    engine.run_host(shapes["data"], shapes["off"])
    nonempty = [d for d in ref.order if ref.by_pos[ref.pos[d]]]
    docs = nonempty[:256] if K > 129 else nonempty[::2]                  # K = 256: a document per class
    labels = [(7 * i) % K for i in range(len(docs))] if K > 1 else [0] * len(docs)
    assert set(labels) == set(range(K))
    variant = "complement" if K in (2, 65) else "multinomial"
    model, want = check(engine, ref, docs, labels, K, by_class=True, variant=variant)
    assert len(set(want[0])) > min(K, 2) - 1                             # more than one class wins
    listed = [ref.order[0], 999999, ref.order[-1], ref.order[0]]        # a list: caller's order, a repeat, an id not held
    got = engine.nb_predict(listed, all_scores=True)
    assert got["pos"].tolist() == [0, tfidf_abi.NO_POS, len(ref.order) - 1, 0]
    assert got["label"].tolist() == [want[0][0], tfidf_abi.NO_CLASS, want[0][-1], want[0][0]]
    assert R.bits(got["score"]).tolist() == R.bits([want[1][0], 0.0, want[1][-1], want[1][0]]).tolist()
    assert not got["scores"][1].any() and np.array_equal(R.bits(got["scores"][2]), R.bits(want[2][-1]))
    plain = engine.nb_predict()                                          # without the score matrix
    assert "scores" not in plain and plain["label"].tolist() == want[0]


def test_count_above_the_table_takes_the_list(engine):
    """a term repeated 70 000 times: a log argument past 2^16, which the sorted list serves"""
    ref, data, off = run_docs(engine, [b"w " * 70000 + b"v", b"w v v", b"u v", b"w u u"])
    for variant in VARIANTS:
        model, _ = check(engine, ref, [1, 2, 3], [0, 1, 1], 2, variant=variant)
        assert max(max(r) for r in model["feature_count"]) == 70000
        info = engine.nb_info()
        assert info["nlisted"] >= 1 and info["nlogs"] >= 65537 + info["nlisted"] + 2
    check(engine, ref, [1, 2, 3], [0, 1, 1], 2, feature="binary")        # the same corpus inside the table
    assert engine.nb_info()["nlisted"] == 0 and engine.nb_info()["nlogs"] < 100


def test_unseen_documents(engine):
    """rows of a transform: words outside the vocabulary are no pairs; an all-OOV document and an
    empty one score the prior"""
    g = load_golden("g5_w3")
    engine.run_host(g["data"], g["off"])
    ids = list(range(1, len(g["off"])))
    ref = R.NRef(oracle_py.run(g["data"], g["off"]), ids)
    w = ref.words
    new = [b"zzzunknown " + w[5] + b" " + w[5] + b" " + w[700], b"qq ww ee", b"", w[0] + b" " + w[819] + b" never_seen",
           b" ".join(w[3 * i] for i in range(200)) + b" tail"]
    rows = ref.unseen(new)
    assert [len(r) for r in rows] == [2, 0, 0, 2, 200]
    data, off = docs_to_arrays(new)
    for variant in VARIANTS:
        labels = [d % 3 for d in ids]
        engine.nb_fit(ids, labels, 3, variant=variant)
        model = ref.fit(ids, labels, 3, variant=variant)
        want = R.predict(model, rows)
        t = engine.transform(data, off)
        assert t["doc_oov"].tolist() == [1, 3, 0, 1, 1]
        got = engine.nb_predict_rows(t, all_scores=True)
        R.assert_same_labels(got, want, 3)
        assert R.bits(got["scores"][1]).tolist() == R.bits(model["prior"]).tolist() == R.bits(got["scores"][2]).tolist()
        assert "scores" not in engine.nb_predict_rows(t)
    # rows the call refuses: a term past V (what a merged group transform carries), offsets that go back
    bad = dict(row_off=[0, 1], term=[0xFFFFFFFF], count=[1])
    raises(tfidf_abi.E_INVAL, engine.nb_predict_rows, bad)
    raises(tfidf_abi.E_INVAL, engine.nb_predict_rows, dict(row_off=[0, 1], term=[ref.V], count=[1]))
    raises(tfidf_abi.E_INVAL, engine.nb_predict_rows, dict(row_off=[0, 2, 1], term=[0, 1], count=[1, 1]))
    assert engine.nb_predict_rows(dict(row_off=[0], term=[], count=[]))["ndocs"] == 0


def test_state():
    """the model's lifetime, the untouched result, allocations, parameter errors"""
    g = load_golden("g5_w3")
    ids = list(range(1, len(g["off"])))
    ora = oracle_py.run(g["data"], g["off"])
    ref = R.NRef(ora, ids)
    labels = [d % 3 for d in ids]
    with tfidf_abi.Engine(0) as e:
        raises(tfidf_abi.E_STATE, e.nb_fit, ids, labels, 3)                 # before a run
        raises(tfidf_abi.E_STATE, e.nb_predict)
        raises(tfidf_abi.E_STATE, e.nb_export)
        e.run_host(g["data"], g["off"])
        raises(tfidf_abi.E_STATE, e.nb_predict)                             # a run, no fit yet
        raises(tfidf_abi.E_STATE, e.nb_predict_rows, dict(row_off=[0], term=[], count=[]))
        text, f0 = e.text(), e.fetch()
        model, want = check(e, ref, ids, labels, 3)
        rows = e.transform(g["data"], g["off"])
        e.nb_predict_rows(rows, all_scores=True)
        f1 = e.fetch()
        assert e.text() == text == g["output"]                              # the result is not disturbed
        for k in ("doc", "term", "count", "docsize", "df"):
            assert np.array_equal(f0[k], f1[k])
        assert np.array_equal(f0["score"].view(np.uint64), f1["score"].view(np.uint64))
        a0 = e.alloc_counters()                                             # a repeated identical fit and predict
        check(e, ref, ids, labels, 3)
        e.nb_predict_rows(rows, all_scores=True)
        assert e.alloc_counters() == a0
        e.reweight("log", "smooth", "l2")                                   # the model reads counts only
        R.assert_same_labels(e.nb_predict(all_scores=True), want, 3)
        R.assert_same_model(e.nb_export(), model)
        # parameter errors: E_INVAL, *out zeroed; a failed fit leaves no model behind
        raises(tfidf_abi.E_INVAL, e.nb_fit, ids + [10 ** 6], labels + [0], 3)        # an id the context does not hold
        raises(tfidf_abi.E_STATE, e.nb_predict)
        e.nb_fit(ids, labels, 3)
        for kw in (dict(labels=[0] * len(ids)), dict(docs=ids[:-1] + [ids[0]]), dict(alpha=-1.0), dict(alpha=float("nan")),
                   dict(labels=[3] + labels[1:]), dict(nclasses=257)):
            a = dict(docs=ids, labels=labels, nclasses=3)
            a.update(kw)
            raises(tfidf_abi.E_INVAL, e.nb_fit, a["docs"], a["labels"], a["nclasses"], alpha=a.get("alpha", 0.0))
        raises(tfidf_abi.E_INVAL, e.nb_fit, None, None, 3, params=tfidf_abi.nb_params(ids, labels, 3, size=16))
        R.assert_same_labels(e.nb_predict(all_scores=True), want, 3)        # refused by the check: the model stays
        t = tfidf_abi.NbLabels()
        t.ndocs = 5
        assert tfidf_abi.lib().tfidf_nb_predict(e.h, None, 0, 2, C.byref(t)) == tfidf_abi.E_INVAL and t.ndocs == 0  # an unknown flag
        assert tfidf_abi.lib().tfidf_nb_fit(e.h, None) == tfidf_abi.E_INVAL
        # term ranks change: the model goes
        e.prune(2)
        raises(tfidf_abi.E_STATE, e.nb_predict)
        raises(tfidf_abi.E_STATE, e.nb_predict_rows, rows)
        raises(tfidf_abi.E_STATE, e.nb_export)
        pruned = prune_ref.prune(ora, 2, 0, 0)
        pref = R.NRef(pruned, ids)
        assert pref.V < ref.V
        check(e, pref, ids, labels, 3, variant="complement")                # V is the pruned term count
        e.run_host(g["data"], g["off"])                                     # a new run
        raises(tfidf_abi.E_STATE, e.nb_predict)
        check(e, ref, ids, labels, 3)
        e.model_import(e.model_export())                                    # a model-only context
        raises(tfidf_abi.E_STATE, e.nb_fit, ids, labels, 3)
        raises(tfidf_abi.E_STATE, e.nb_predict)
        raises(tfidf_abi.E_STATE, e.nb_predict_rows, rows)


def test_edge_corpora(engine):
    ref, _, _ = run_docs(engine, [b"", b"solo", b"  \n", b"solo solo x"])
    check(engine, ref, [1, 2, 3], [0, 1, 0], 2)                             # empty labelled documents count in n_c
    check(engine, ref, [2], [0], 1, variant="complement")                  # K = 1
    ref, _, _ = run_docs(engine, [b"", b""])                                # no terms at all: the priors
    check(engine, ref, [1, 2], [0, 1], 2)
    check(engine, ref, [1], [0], 1, uniform_prior=True)


CAPACITY_CHILD = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, tfidf_abi
from helpers import docs_to_arrays
docs = [b" ".join(b"w%%05d" %% (125 * d + i) for i in range(125)) for d in range(32)]   # V = 4000
data, off = docs_to_arrays(docs)
ids = list(range(1, 33))
with tfidf_abi.Engine(0) as e:
    e.run_host(data, off)
    before = e.fetch()
    rcs = []
    for K in (8, 32):          # 16 * 8 * 4000 = 512 000 bytes fit 1 MiB; 16 * 32 * 4000 = 2 048 000 do not
        try:
            e.nb_fit(ids, [d %% K for d in ids], K)
            e.nb_predict()
            rcs.append(0)
        except tfidf_abi.TfidfError as x:
            rcs.append(x.rc)
    try:
        e.nb_predict()         # refused before any device work: the K = 8 model is still there
        after = 0
    except tfidf_abi.TfidfError as x:
        after = x.rc
    now = e.fetch()
    ok = bool(np.array_equal(before["score"].view(np.uint64), now["score"].view(np.uint64))
              and np.array_equal(before["count"], now["count"]) and now["output_txt"] == before["output_txt"])
    print("RESULT", rcs[0], rcs[1], after, ok)
"""


def test_capacity_in_a_fresh_process():
    """TFIDF_NB_MB is read at tfidf_open: V = 4000 under a 1 MiB budget at K = 8 and K = 32"""
    code = CAPACITY_CHILD % (os.path.join(PKG, "python"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests"))
    env = dict(os.environ, TFIDF_NB_MB="1")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr
    line = [x for x in p.stdout.splitlines() if x.startswith("RESULT")][-1].split()
    assert line[1:] == ["0", str(tfidf_abi.E_CAPACITY), "0", "True"], p.stdout


def cli(tmp_path, *args):
    return subprocess.run([tfidf_abi.CLI_PATH] + list(args), cwd=tmp_path, capture_output=True, timeout=120)


def name_order(ids):
    return sorted(ids, key=lambda d: b"doc%d@" % d)


NAMES = [b"Zebra", b"apple", b"apples", b"mango"]                          # in byte order: the class numbers


def test_cli_classify_dir(tmp_path):
    """the planted corpus end to end through `--labels FILE --classify DIR`: input/ holds the
    labelled half, DIR the held-out half; classes.txt equals the lines formatted from the reference"""
    docs, planted = R.planted_corpus()
    lab, lab_classes, held = R.planted_split(planted)
    assert NAMES == sorted(NAMES)
    (tmp_path / "input").mkdir()
    (tmp_path / "new").mkdir()
    for i, d in enumerate(lab):
        (tmp_path / "input" / ("doc%d" % (i + 1))).write_bytes(docs[d - 1])
    for i, d in enumerate(held):
        (tmp_path / "new" / ("doc%d" % (i + 1))).write_bytes(docs[d - 1])
    (tmp_path / "labels.txt").write_bytes(b"".join(b"doc%d\t%s\n" % (i + 1, NAMES[c]) for i, c in enumerate(lab_classes)))
    data, off = docs_to_arrays([docs[d - 1] for d in lab])
    ora = oracle_py.run(data, off)
    ids = list(range(1, len(lab) + 1))
    ref = R.NRef(ora, ids)
    new_ids = name_order(range(1, len(held) + 1))
    rows = ref.unseen([docs[held[m - 1] - 1] for m in new_ids])
    for flags, kw in (([], {}), (["--nb-binary", "--nb-uniform-prior"], dict(feature="binary", uniform_prior=True))):
        p = cli(tmp_path, "--labels", "labels.txt", "--classify", "new", *flags)
        assert p.returncode == 0, p.stderr
        assert (tmp_path / "output.txt").read_bytes() == ora["output_txt"]
        labels, best, _ = R.predict(ref.fit(ids, lab_classes, 4, **kw), rows)
        assert labels == [planted[held[m - 1] - 1] for m in new_ids]        # every held-out document: its planted class
        assert (tmp_path / "classes.txt").read_bytes() == R.classes_lines(new_ids, labels, best, NAMES)


def test_cli_classify_unlabelled(tmp_path):
    """`--labels FILE --classify-unlabelled`: input/ holds all 48 planted documents, FILE labels 24;
    the complement variant with its own alpha and file name; then a label for a document input/
    does not hold"""
    docs, planted = R.planted_corpus()
    lab, lab_classes, held = R.planted_split(planted)
    (tmp_path / "input").mkdir()
    for i, d in enumerate(docs):
        (tmp_path / "input" / ("doc%d" % (i + 1))).write_bytes(d)
    (tmp_path / "labels.txt").write_bytes(b"".join(b"doc%d\t%s\n" % (d, NAMES[c]) for d, c in zip(lab, lab_classes)))
    p = cli(tmp_path, "--labels", "labels.txt", "--classify-unlabelled", "--classify-file", "held.txt", "--nb-complement",
            "--nb-alpha", "0.5")
    assert p.returncode == 0, p.stderr
    data, off = docs_to_arrays(docs)
    ref = R.NRef(oracle_py.run(data, off), list(range(1, 49)))
    labels, best, _ = R.predict(ref.fit(lab, lab_classes, 4, variant="complement", alpha=0.5), ref.rows())
    order = [d for d in ref.order if d in set(held)]
    want = R.classes_lines(order, [labels[ref.pos[d]] for d in order], [best[ref.pos[d]] for d in order], NAMES)
    assert (tmp_path / "held.txt").read_bytes() == want and want.count(b"\n") == 24
    assert [labels[ref.pos[d]] for d in order] == [planted[d - 1] for d in order]
    (tmp_path / "labels.txt").write_bytes(b"doc1\tapple\ndoc77\tmango\n")
    p = cli(tmp_path, "--labels", "labels.txt", "--classify-unlabelled")
    assert p.returncode == 3 and b"does not hold" in p.stderr


def test_info_struct_honours_a_short_size():
    """tfidf_last_nb_info in the pattern of test_gpu_info_abi.py"""
    from test_gpu_info_abi import FILL, TAIL, assert_rejected, call, filled, size_of
    name, struct = "tfidf_last_nb_info", tfidf_abi.NbInfo
    S = C.sizeof(struct)
    with tfidf_abi.Engine(0) as e:
        assert call(name, None, filled(S, S), struct) == tfidf_abi.E_INVAL
        assert call(name, e.h, None, struct) == tfidf_abi.E_INVAL
        for size in (0, 4):
            assert_rejected(name, e.h, struct, size)
        buf = filled(S + TAIL, 8)
        assert call(name, e.h, buf, struct) == 0
        assert size_of(buf) == 8 and bytes(buf)[8:] == bytes([FILL]) * (S + TAIL - 8)
