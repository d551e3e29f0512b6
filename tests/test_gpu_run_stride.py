"""tfidf_run itself with TFIDF_GRID_CUS = 1, 2 and unset on the run-stride corpus
(tests/run_stride_corpus.py), every K1 kernel instance, against the oracle.

The run's persistent kernels size their grids by the context's CU count: k_tokcount_sl and
k_tokcount_vs launch min(chunks, CUs x 4) workgroups that claim chunks from a global counter, the
score stage CUs x 6 and CUs x 4 workgroups, emit.hip CUs x 8 of four waves.  On a 256-CU device a
K1 workgroup is certain to take a second chunk only above 1 024 chunks (25 MB), a wave of emit a
second document only above 8 192 documents, and no oracle-compared run of the suite was that large:
what k_tokcount_sl leaves in its LDS table for the workgroup's next chunk (it clears the table once
per workgroup; sl_flush_few is always a chunk's last flush), a chunk that ends in overflow mode, the
claimed-ahead next chunk, an empty chunk between two others, and a wave of k_doc_text_write that
goes from a multi-round document or a direct-written long term to its next document ran only by
luck.  With one CU there are four K1 workgroups for 92 (24 KiB) or 183 (12 KiB) chunks;
test_run_stride_corpus_cpu.py shows without a GPU that every class of chunk then has at least
eight members that run behind a predecessor and eight that a successor follows, whichever workgroup
claims which.  tfidf_run_info.k1_workgroups shows that the variable reached the launch.

The oracle knows nothing of grids: equality at every setting is grid independence.  Everything
is compared exactly: integers, score bits, text bytes."""
import numpy as np
import pytest

import oracle_py
import run_stride_corpus as RC
import tfidf_abi
from helpers import assert_k1_instance, assert_same_result, docs_to_arrays, k1_engine
from test_gpu_grid_stride import device_cus

pytestmark = pytest.mark.gpu

PERSISTENT = ("sl_fast", "sl_full", "vs")
MAX_TERMS = 60000       # TFIDF_VCAP=4096 grows x4 per attempt: 60 000 terms fit well inside the engine's 8 attempts


@pytest.fixture(scope="module")
def want():
    """the corpus and the oracle's answer, computed once"""
    data, off = docs_to_arrays(RC.build()["docs"])
    ora = oracle_py.run(data, off)
    return dict(data=data, off=off, ora=ora, ntokens=int(ora["count"].astype(np.int64).sum()))


def set_cus(monkeypatch, cus):
    if cus is None:
        monkeypatch.delenv("TFIDF_GRID_CUS", raising=False)
    else:
        monkeypatch.setenv("TFIDF_GRID_CUS", cus)


def check_run(e, w):
    """the resident result, the host-formatted text and emit.hip's text are the oracle's"""
    res, ora = e.fetch(), w["ora"]
    assert_same_result(res, ora)
    assert res["output_txt"] == ora["output_txt"]
    assert e.text() == ora["output_txt"]
    info = e.info()
    assert info["ntokens"] == w["ntokens"]
    return info


@pytest.mark.parametrize("cus", ["1", "2", None])
@pytest.mark.parametrize("instance", ["sl_fast", "sl_full", "vs", "general"])
def test_run_at_this_cu_count(want, instance, cus, monkeypatch):
    set_cus(monkeypatch, cus)
    with k1_engine(instance) as e:                      # the environment is read at tfidf_open
        ncu = int(cus) if cus else device_cus()
        assert e.grid_cus() == ncu
        e.run_host(want["data"], want["off"])
        info = check_run(e, want)
    assert_k1_instance(info, instance)
    assert info["partial_records"] > 0
    print(instance, cus, "chunks", info["nchunks"], "K1 workgroups", info["k1_workgroups"])
    if instance in PERSISTENT:
        assert info["k1_workgroups"] == min(info["nchunks"], RC.K1_WG_PER_CU * ncu)
        if cus:
            assert info["k1_workgroups"] == 4 * int(cus)
            assert info["nchunks"] >= 10 * info["k1_workgroups"]
    else:                                               # the cross-check: a workgroup per chunk, nothing carried over
        assert info["k1_workgroups"] == info["nchunks"]


@pytest.mark.parametrize("instance", ["sl_fast", "vs"])
def test_vocabulary_retry_with_workgroups_several_chunks_in(want, instance, monkeypatch):
    """A table of 4 096 slots for 25 000 terms: the first attempts end in ST_VOCAB_FULL while the
    four workgroups are several chunks in, and the repeated attempts start from a cleared chunk
    counter and tables."""
    assert want["ora"]["nterms"] <= MAX_TERMS
    set_cus(monkeypatch, "1")
    for k in ("TFIDF_K1", "TFIDF_VLOAD_BIG", "TFIDF_SL_MAXCAP"):
        monkeypatch.delenv(k, raising=False)
    if instance == "vs":
        monkeypatch.setenv("TFIDF_K1", "vs")
    monkeypatch.setenv("TFIDF_VCAP", "4096")
    monkeypatch.setenv("TFIDF_VLOAD", "12")
    with tfidf_abi.Engine(0) as e:
        e.run_host(want["data"], want["off"])
        info = check_run(e, want)
    assert info["vocab_capacity"] > 4096
    assert info["vocab_capacity"] * 12 >= 100 * want["ora"]["nterms"]          # grown to the load limit
    assert_k1_instance(info, instance)
    assert info["k1_workgroups"] == 4 and info["nchunks"] >= 40


def test_output_file_in_groups(want, monkeypatch, tmp_path):
    """tfidf_write_output_gpu on an unformatted result formats in document groups:
    launch_emit_write with d0 > 0, each group's waves striding from the group's first document"""
    set_cus(monkeypatch, "1")
    path = tmp_path / "output.txt"
    with k1_engine("sl_fast") as e:
        e.run_host(want["data"], want["off"])
        e.write_output(str(path))                       # before any text(): the grouped path
        oi = e.output_info()
        assert e.text() == want["ora"]["output_txt"]    # the text the groups left in HBM
    assert oi["formatted"] == 1 and oi["text_bytes"] == len(want["ora"]["output_txt"])
    assert path.read_bytes() == want["ora"]["output_txt"]
