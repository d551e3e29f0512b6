"""The size-prefixed tfidf_last_*_info structs (include/tfidf.h): every call copies
min(caller's size, sizeof) bytes, writes that number into `size`, touches no byte behind it and
rejects a null pointer or a size that cannot hold the prefix.  Raw buffers prefilled with 0xA5
on a context that has run nothing: the payload of every call is zero."""
import ctypes as C

import pytest

import tfidf_abi

pytestmark = pytest.mark.gpu

INFOS = [
    ("tfidf_last_output_info", tfidf_abi.OutputInfo),
    ("tfidf_last_query_info", tfidf_abi.QueryInfo),
    ("tfidf_last_bm25_info", tfidf_abi.Bm25Info),
    ("tfidf_last_terms_info", tfidf_abi.TermsInfo),
    ("tfidf_last_similar_info", tfidf_abi.SimilarInfo),
    ("tfidf_last_kmeans_info", tfidf_abi.KmeansInfo),
    ("tfidf_last_transform_info", tfidf_abi.TransformInfo),
    ("tfidf_last_model_info", tfidf_abi.ModelInfo),
    ("tfidf_last_analyze_info", tfidf_abi.AnalyzeInfoUtf8),
    ("tfidf_last_ngram_info", tfidf_abi.NgramInfo),
    ("tfidf_last_prune_info", tfidf_abi.PruneInfo),
    ("tfidf_last_reweight_info", tfidf_abi.ReweightInfo),
]
FILL = 0xA5
TAIL = 64


@pytest.fixture(scope="module")
def fresh():
    """a context of this module's own: nothing has been called on it"""
    with tfidf_abi.Engine(0) as e:
        yield e


def filled(nbytes: int, size: int):
    """a buffer of 0xA5 whose first eight bytes hold `size`"""
    buf = (C.c_uint8 * nbytes)(*([FILL] * nbytes))
    C.cast(buf, C.POINTER(C.c_uint64))[0] = size
    return buf


def call(name, handle, buf, struct):
    return getattr(tfidf_abi.lib(), name)(handle, None if buf is None else C.cast(buf, C.POINTER(struct)))


def size_of(buf) -> int:
    return int(C.cast(buf, C.POINTER(C.c_uint64))[0])


def assert_rejected(name, handle, struct, size: int):
    n = C.sizeof(struct) + TAIL
    buf = filled(n, size)
    assert call(name, handle, buf, struct) == tfidf_abi.E_INVAL, (name, size)
    assert bytes(buf) == bytes(filled(n, size)), (name, size)


@pytest.mark.parametrize("name,struct", INFOS, ids=[n for n, _ in INFOS])
def test_last_info(fresh, name, struct):
    S = C.sizeof(struct)
    assert call(name, None, filled(S, S), struct) == tfidf_abi.E_INVAL
    assert call(name, fresh.h, None, struct) == tfidf_abi.E_INVAL
    for size in (0, 4):
        assert_rejected(name, fresh.h, struct, size)
    buf = filled(S + TAIL, 8)                       # the prefix alone
    assert call(name, fresh.h, buf, struct) == 0
    assert size_of(buf) == 8 and bytes(buf)[8:] == bytes([FILL]) * (S + TAIL - 8)
    buf = filled(S + TAIL, S + TAIL)                # a caller built against a larger struct
    assert call(name, fresh.h, buf, struct) == 0
    assert size_of(buf) == S
    assert bytes(buf)[8:S] == bytes(S - 8), name    # nothing has been called: the payload is zero
    assert bytes(buf)[S:] == bytes([FILL]) * TAIL


def test_last_run_info(fresh):
    name, struct = "tfidf_last_run_info", tfidf_abi.RunInfo
    S = C.sizeof(struct)
    assert call(name, None, filled(S, S), struct) == tfidf_abi.E_INVAL
    assert call(name, fresh.h, None, struct) == tfidf_abi.E_INVAL
    for size in (0, 4, 8):                          # its minimum is 16
        assert_rejected(name, fresh.h, struct, size)
    for size in (16, S, S + TAIL):                  # before any run
        buf = filled(S + TAIL, size)
        assert call(name, fresh.h, buf, struct) == tfidf_abi.E_STATE
        assert bytes(buf) == bytes(filled(S + TAIL, size))
