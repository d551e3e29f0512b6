"""The retrieval entry points of include/tfidf.h without a GPU: argument errors, the
no-op free, and the binding's export list."""
import ctypes as C

import tfidf_abi


def test_query_null_arguments_are_invalid():
    L = tfidf_abi.lib()
    assert L.tfidf_query(None, None, 3, None) == tfidf_abi.E_INVAL
    assert L.tfidf_group_query(None, None, 3, None) == tfidf_abi.E_INVAL
    qs, h = tfidf_abi.Queries(), tfidf_abi.Hits()
    assert L.tfidf_query(None, C.byref(qs), 3, C.byref(h)) == tfidf_abi.E_INVAL
    assert L.tfidf_group_query(None, C.byref(qs), 3, C.byref(h)) == tfidf_abi.E_INVAL
    qi = tfidf_abi.QueryInfo()
    qi.size = C.sizeof(tfidf_abi.QueryInfo)
    assert L.tfidf_last_query_info(None, C.byref(qi)) == tfidf_abi.E_INVAL


def test_hits_free_of_a_zeroed_struct_is_a_no_op():
    L = tfidf_abi.lib()
    h = tfidf_abi.Hits()
    L.tfidf_hits_free(C.byref(h))
    L.tfidf_hits_free(C.byref(h))
    L.tfidf_hits_free(None)
    assert not h.doc and not h.score and h.nqueries == 0


def test_query_names_are_exported():
    L = tfidf_abi.lib()
    for name in ("tfidf_query", "tfidf_hits_free", "tfidf_group_query", "tfidf_last_query_info"):
        assert name in tfidf_abi.EXPORTS
        assert hasattr(L, name)
    assert tfidf_abi.QUERY_MAX_K == 1024
    assert L.tfidf_abi_version() == tfidf_abi.ABI_VERSION == 2      # the change is additive
    # the structs mirror include/tfidf.h (LP64 layout)
    assert C.sizeof(tfidf_abi.Queries) == 32 and C.sizeof(tfidf_abi.Hits) == 48
    assert C.sizeof(tfidf_abi.QueryInfo) == 72
