"""The similar-document entry points of include/tfidf.h without a GPU: argument errors, the
no-op free, the binding's export list and the structures' layout."""
import ctypes as C

import tfidf_abi


def test_similar_null_arguments_are_invalid():
    L = tfidf_abi.lib()
    n = tfidf_abi.Neighbors()
    assert L.tfidf_similar(None, None, 0, 3, None) == tfidf_abi.E_INVAL
    assert L.tfidf_similar(None, None, 0, 3, C.byref(n)) == tfidf_abi.E_INVAL
    assert L.tfidf_group_similar(None, None, 0, 3, None) == tfidf_abi.E_INVAL
    assert L.tfidf_group_similar(None, None, 0, 3, C.byref(n)) == tfidf_abi.E_INVAL
    si = tfidf_abi.SimilarInfo()
    si.size = C.sizeof(tfidf_abi.SimilarInfo)
    assert L.tfidf_last_similar_info(None, C.byref(si)) == tfidf_abi.E_INVAL
    assert not n.doc and not n.nb_score and n.ndocs == 0


def test_similar_k_out_of_range_is_invalid():
    """k is checked before the context is used: a group without ranks cannot exist, so the
    group entry point is given a NULL group and must still name the argument error"""
    L = tfidf_abi.lib()
    n = tfidf_abi.Neighbors()
    for k in (0, 1025):
        assert L.tfidf_similar(None, None, 0, k, C.byref(n)) == tfidf_abi.E_INVAL
        assert L.tfidf_group_similar(None, None, 0, k, C.byref(n)) == tfidf_abi.E_INVAL
    assert tfidf_abi.SIMILAR_MAX_K == 1024


def test_neighbors_free_of_a_zeroed_struct_is_a_no_op():
    L = tfidf_abi.lib()
    n = tfidf_abi.Neighbors()
    L.tfidf_neighbors_free(C.byref(n))
    L.tfidf_neighbors_free(C.byref(n))
    L.tfidf_neighbors_free(None)
    assert not n.doc and not n.norm and not n.nb_doc and n.ndocs == 0 and n.k == 0


def test_similar_names_are_exported():
    L = tfidf_abi.lib()
    for name in ("tfidf_similar", "tfidf_neighbors_free", "tfidf_group_similar", "tfidf_last_similar_info"):
        assert name in tfidf_abi.EXPORTS
        assert hasattr(L, name)
    assert L.tfidf_abi_version() == tfidf_abi.ABI_VERSION == 2      # the change is additive


def test_similar_structures_mirror_the_header():
    # include/tfidf.h, LP64: two u32 and nine pointers; u64, four u32, u64, two u32, five doubles
    assert C.sizeof(tfidf_abi.Neighbors) == 80
    assert C.sizeof(tfidf_abi.SimilarInfo) == 80
    assert tfidf_abi.Neighbors.doc.offset == 8 and tfidf_abi.Neighbors.norm.offset == 32
    assert tfidf_abi.Neighbors.nb_doc.offset == 56 and tfidf_abi.Neighbors.nb_score.offset == 72
    assert tfidf_abi.SimilarInfo.acc_bytes.offset == 24 and tfidf_abi.SimilarInfo.big_docs.offset == 32
    assert tfidf_abi.SimilarInfo.ms_norms.offset == 40 and tfidf_abi.SimilarInfo.ms_total.offset == 72
