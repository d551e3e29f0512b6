"""The keyword entry points of include/tfidf.h without a GPU: argument errors, the no-op
free, the binding's export list and the structures' layout."""
import ctypes as C

import tfidf_abi


def test_top_terms_null_arguments_are_invalid():
    L = tfidf_abi.lib()
    t = tfidf_abi.DocTerms()
    assert L.tfidf_top_terms(None, None, 0, 3, None) == tfidf_abi.E_INVAL
    assert L.tfidf_top_terms(None, None, 0, 3, C.byref(t)) == tfidf_abi.E_INVAL
    assert L.tfidf_group_top_terms(None, None, 0, 3, None) == tfidf_abi.E_INVAL
    assert L.tfidf_group_top_terms(None, None, 0, 3, C.byref(t)) == tfidf_abi.E_INVAL
    ti = tfidf_abi.TermsInfo()
    ti.size = C.sizeof(tfidf_abi.TermsInfo)
    assert L.tfidf_last_terms_info(None, C.byref(ti)) == tfidf_abi.E_INVAL
    assert not t.doc and not t.word_bytes and t.ndocs == 0


def test_doc_terms_free_of_a_zeroed_struct_is_a_no_op():
    L = tfidf_abi.lib()
    t = tfidf_abi.DocTerms()
    L.tfidf_doc_terms_free(C.byref(t))
    L.tfidf_doc_terms_free(C.byref(t))
    L.tfidf_doc_terms_free(None)
    assert not t.doc and not t.score and not t.word_off and t.ndocs == 0 and t.k == 0


def test_terms_names_are_exported():
    L = tfidf_abi.lib()
    for name in ("tfidf_top_terms", "tfidf_doc_terms_free", "tfidf_group_top_terms", "tfidf_last_terms_info"):
        assert name in tfidf_abi.EXPORTS
        assert hasattr(L, name)
    assert tfidf_abi.TERMS_MAX_K == 1024
    assert L.tfidf_abi_version() == tfidf_abi.ABI_VERSION == 2      # the change is additive


def test_terms_structures_mirror_the_header():
    # include/tfidf.h, LP64: two u32 and ten pointers; u64, four u32, u64, four doubles
    assert C.sizeof(tfidf_abi.DocTerms) == 88
    assert C.sizeof(tfidf_abi.TermsInfo) == 64
    assert tfidf_abi.DocTerms.word_bytes.offset == 80 and tfidf_abi.DocTerms.doc.offset == 8
    assert tfidf_abi.TermsInfo.out_bytes.offset == 24 and tfidf_abi.TermsInfo.ms_total.offset == 56
