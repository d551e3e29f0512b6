"""Packed records through the engine: k_tokcount_sl emits a complete document's record as one
word (count << sbits | slot), the DF pass rewrites it as rank << cb | count and the score
kernels sort that word.  Every corpus here is run packed and with TFIDF_REC_PACK=0
and both runs are compared with the oracle and with each other, array by array; each test reads
from tfidf_last_run_info that the run took the path it is named for.

  count limit    a table of 4M slots leaves the count 10 bits: a term 1023 times in a document
                 stays a packed record, 1024 and 1025 times send the whole document through
                 the partial-record merge with its full counts
  flags          RUN_REC_PACK / RUN_REC_PACK_KEPT set by the default run, clear with
                 TFIDF_REC_PACK=0 and with TFIDF_K1=vs
  forced unpack  70 000 distinct terms in the default 1M-slot table: V is past the LDS DF
                 histogram, so k_rec_unpack splits the records after K1
  mixed          scaled c2 and c5: packed documents beside merged (two-word) ones"""
import numpy as np
import pytest

import oracle_py
import tfidf_abi
import tfidf_configs
from helpers import assert_same_result, docs_to_arrays
from test_gpu_paths import docs_covering, fixed_words

pytestmark = pytest.mark.gpu

ARRAYS = ("doc", "term", "count", "docsize", "df")


def run_with(monkeypatch, env, data, off, ids=None, n_total=0):
    """one run in a context of its own opened under `env` (the knobs are read when a context is
    opened): the fetched result, the text and the run info"""
    for k in ("TFIDF_REC_PACK", "TFIDF_VCAP", "TFIDF_K1"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with tfidf_abi.Engine(0) as e:
        e.run_host(data, off, ids, n_total)
        return e.fetch(), e.text(), e.info()


def same_runs(a, b):
    assert a["npairs"] == b["npairs"] and a["nterms"] == b["nterms"]
    assert a["terms"] == b["terms"]
    for k in ARRAYS:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["score"].view(np.uint64), b["score"].view(np.uint64))
    assert a["output_txt"] == b["output_txt"]


def packed_and_plain(monkeypatch, env, data, off, ids=None, n_total=0):
    """the corpus packed and with TFIDF_REC_PACK=0, both against the oracle and each other"""
    ora = oracle_py.run(data, off, ids, n_total)
    res, txt, info = run_with(monkeypatch, env, data, off, ids, n_total)
    res0, txt0, info0 = run_with(monkeypatch, dict(env, TFIDF_REC_PACK="0"), data, off, ids, n_total)
    for r, t in ((res, txt), (res0, txt0)):
        assert_same_result(r, ora)
        assert r["output_txt"] == ora["output_txt"] and t == ora["output_txt"]
    same_runs(res, res0)
    assert info0["flags"] & (tfidf_abi.RUN_REC_PACK | tfidf_abi.RUN_REC_PACK_KEPT) == 0
    return res, info, info0


def count_limit_docs():
    few = b"delta epsilon zeta eta theta "
    docs = [b"alpha beta gamma alpha\n"]
    for reps in (1023, 1024, 1025):
        docs.append(few + b"alpha " * reps + b"beta beta gamma\n")
    docs.append(b"gamma delta\n")
    return docs


def test_count_limit_documents_leave_as_partial_records(monkeypatch):
    """VCAP = 4M slots: sbits 22, counts below 1024 fit.  The documents with 1024 and 1025
    repeats hold 8 distinct terms each and must leave as 16 partial records; the one with 1023
    stays packed (no partial record without packing, 16 with it)."""
    data, off = docs_to_arrays(count_limit_docs())
    res, info, info0 = packed_and_plain(monkeypatch, {"TFIDF_VCAP": "4194304"}, data, off)
    assert info["vocab_capacity"] == 4194304
    assert info["flags"] & tfidf_abi.RUN_K1_SL
    assert info["flags"] & tfidf_abi.RUN_REC_PACK and info["flags"] & tfidf_abi.RUN_REC_PACK_KEPT
    assert info0["partial_records"] == 0
    assert info["partial_records"] == 16
    alpha = res["terms"].index(b"alpha")
    counts = sorted(int(c) for c, t in zip(res["count"], res["term"]) if t == alpha)
    assert counts == [2, 1023, 1024, 1025]


def test_packed_flag_follows_the_k1_kernel(monkeypatch):
    data, off = docs_to_arrays(count_limit_docs())
    _, _, info = run_with(monkeypatch, {}, data, off)
    assert info["flags"] & tfidf_abi.RUN_K1_SL
    assert info["flags"] & tfidf_abi.RUN_REC_PACK and info["flags"] & tfidf_abi.RUN_REC_PACK_KEPT
    assert info["partial_records"] == 0      # 1M slots: counts below 4096 fit
    _, _, info = run_with(monkeypatch, {"TFIDF_K1": "vs"}, data, off)
    assert info["flags"] & tfidf_abi.RUN_K1_VS and not info["flags"] & tfidf_abi.RUN_K1_SL
    assert info["flags"] & (tfidf_abi.RUN_REC_PACK | tfidf_abi.RUN_REC_PACK_KEPT) == 0
    _, _, info = run_with(monkeypatch, {"TFIDF_REC_PACK": "0"}, data, off)
    assert info["flags"] & tfidf_abi.RUN_K1_SL
    assert info["flags"] & (tfidf_abi.RUN_REC_PACK | tfidf_abi.RUN_REC_PACK_KEPT) == 0


def test_vocabulary_past_the_lds_histogram_unpacks(monkeypatch):
    """70 000 distinct 4-letter terms stay in the default 1M-slot table (K1 packs) and V is past
    65 536: the records are unpacked after K1 and the run goes on with two words."""
    rng = np.random.default_rng(70000)
    words = [bytes(w) for w in fixed_words(rng.permutation(26 ** 4)[:70000], 4)]
    data, off = docs_to_arrays(docs_covering(words, 700, rng, extra=40))
    res, info, _ = packed_and_plain(monkeypatch, {}, data, off)
    assert res["nterms"] == 70000 and info["vocab_capacity"] == 1 << 20
    assert info["flags"] & tfidf_abi.RUN_K1_SL and info["flags"] & tfidf_abi.RUN_REC_PACK
    assert not info["flags"] & tfidf_abi.RUN_REC_PACK_KEPT


@pytest.mark.parametrize("cfg,scale", [("c2", 0.003), ("c5", 0.0005)])
def test_packed_beside_merged_documents(monkeypatch, cfg, scale):
    p = tfidf_configs.plan(cfg, scale=scale)
    data, off = tfidf_abi.synth_host(p["seed"], p["V"], p["mode"], p["cdf"], p["doc_ids"], p["ntok"])
    res, info, _ = packed_and_plain(monkeypatch, {}, data, off, p["doc_ids"], p["ndocs_total"])
    assert res["npairs"] > 0
    assert info["flags"] & tfidf_abi.RUN_REC_PACK and info["flags"] & tfidf_abi.RUN_REC_PACK_KEPT
