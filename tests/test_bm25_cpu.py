"""The BM25 entry points of include/tfidf.h without a GPU: argument and parameter errors, the
binding's export list and the structures' layout."""
import ctypes as C
import math
import subprocess

import tfidf_abi


def params(k1=1.2, b=0.75, avgdl=0.0, size=None):
    p = tfidf_abi.Bm25Params()
    p.size = C.sizeof(tfidf_abi.Bm25Params) if size is None else size
    p.k1, p.b, p.avgdl = k1, b, avgdl
    return p


def test_bm25_null_arguments_are_invalid():
    L = tfidf_abi.lib()
    qs, h, p = tfidf_abi.Queries(), tfidf_abi.Hits(), params()
    for fn in (L.tfidf_query_bm25, L.tfidf_group_query_bm25):
        assert fn(None, None, 3, None, None) == tfidf_abi.E_INVAL
        assert fn(None, C.byref(qs), 3, None, C.byref(h)) == tfidf_abi.E_INVAL
        assert fn(None, C.byref(qs), 3, C.byref(p), C.byref(h)) == tfidf_abi.E_INVAL
    bi = tfidf_abi.Bm25Info()
    bi.size = C.sizeof(tfidf_abi.Bm25Info)
    assert L.tfidf_last_bm25_info(None, C.byref(bi)) == tfidf_abi.E_INVAL
    assert not h.doc and not h.score and h.nqueries == 0


def test_bm25_bad_parameters_are_invalid():
    """Without a device no context can be opened, so these calls only show that a bad
    parameter struct next to a NULL handle is still an argument error (no crash, no other
    code).  That each of these structs, `size` too small included, is rejected for its own
    sake, and that a valid struct succeeds, is asserted on a live context in
    tests/test_gpu_bm25.py (test_bm25_errors, test_bm25_parameter_struct_on_a_live_context)."""
    L = tfidf_abi.lib()
    qs, h = tfidf_abi.Queries(), tfidf_abi.Hits()
    bad = [params(k1=-0.5), params(b=1.5), params(b=-0.1), params(k1=math.nan), params(b=math.nan),
           params(avgdl=math.nan), params(avgdl=-1.0), params(k1=math.inf), params(avgdl=math.inf),
           params(size=8), params(size=C.sizeof(tfidf_abi.Bm25Params) - 1)]
    for p in bad:
        assert L.tfidf_query_bm25(None, C.byref(qs), 3, C.byref(p), C.byref(h)) == tfidf_abi.E_INVAL
        assert L.tfidf_group_query_bm25(None, C.byref(qs), 3, C.byref(p), C.byref(h)) == tfidf_abi.E_INVAL


def test_cli_bm25_switches_need_a_query_file(tmp_path):
    """--bm25 or one of its parameters without --query is a usage error before anything is
    opened, not a silently ignored switch"""
    for flags in (["--bm25"], ["--bm25-k1", "2.0"], ["--bm25-b", "0.5"]):
        p = subprocess.run([tfidf_abi.CLI_PATH] + flags, cwd=tmp_path, capture_output=True, timeout=60)
        assert p.returncode == 2 and b"--query" in p.stderr, (flags, p.stderr)
        assert not (tmp_path / "output.txt").exists() and not (tmp_path / "hits.txt").exists()
    for flags in (["--query", "q.txt", "--bm25-b", "1.5"], ["--query", "q.txt", "--bm25-k1", "-1"],
                  ["--query", "q.txt", "--bm25-k1", "nan"], ["--query", "q.txt", "--bm25-b", "x"]):
        p = subprocess.run([tfidf_abi.CLI_PATH] + flags, cwd=tmp_path, capture_output=True, timeout=60)
        assert p.returncode == 2 and b"--bm25-k1" in p.stderr, (flags, p.stderr)


def test_bm25_names_are_exported():
    L = tfidf_abi.lib()
    for name in ("tfidf_query_bm25", "tfidf_group_query_bm25", "tfidf_last_bm25_info"):
        assert name in tfidf_abi.EXPORTS
        assert hasattr(L, name)
    assert L.tfidf_abi_version() == tfidf_abi.ABI_VERSION == 2      # the change is additive


def test_bm25_structures_mirror_the_header():
    # include/tfidf.h, LP64: u64 and three doubles; tfidf_query_info's 72 bytes and one double
    assert C.sizeof(tfidf_abi.Bm25Params) == 32
    assert tfidf_abi.Bm25Params.k1.offset == 8 and tfidf_abi.Bm25Params.avgdl.offset == 24
    assert C.sizeof(tfidf_abi.Bm25Info) == C.sizeof(tfidf_abi.QueryInfo) + 8 == 80
    assert tfidf_abi.Bm25Info.acc_bytes.offset == 32 and tfidf_abi.Bm25Info.ms_lookup.offset == 40
    assert tfidf_abi.Bm25Info.ms_total.offset == 64 and tfidf_abi.Bm25Info.avgdl.offset == 72
