"""The adversarial corpora of test_gpu_parity.py and test_gpu_k1_count_paths.py on the three
tokenize+count (K1) kernel instances those modules never reach: they run on the session
engine, which is k_tokcount_sl<true>.  Here every corpus also runs on

  sl_full   k_tokcount_sl<false> (a vocabulary table of 2^23 slots: the full count in every
            round, no stack; 12 KiB chunks),
  vs        k_tokcount_vs (what production runs past 2^25 slots; its own LDS table and
            FILL_LIMIT),
  general   k_tokcount (what an unaligned corpus base gets; a 2 048-slot LDS table, epochs of
            256 documents),

against the oracle, exactly as check_vs_oracle compares.  The 2 900 / 3 400-term documents
and the 255 / 256 / 257-document cases overflow each kernel's own table and document group,
not only k_tokcount_sl's.  Each test asserts from info() that the instance it is named for
ran."""
import functools

import pytest

import oracle_py
import test_gpu_k1_count_paths as cp
import test_gpu_parity as par
from helpers import assert_k1_instance, assert_same_result, k1_fixture

pytestmark = pytest.mark.gpu

k1 = k1_fixture(["sl_full", "vs", "general"])

CORPORA = {
    "document_boundaries": par.document_boundaries_corpus,
    "blank_docs": par.blank_docs_corpus,
    "nul_and_control_bytes": par.nul_and_control_bytes_corpus,
    "long_tokens": par.long_tokens_corpus,
    "windows_and_chunks": par.windows_and_chunks_corpus,
    "tiny_docs_without_separators": par.tiny_docs_without_separators_corpus,
    "more_pairs_than_lds_table": par.more_pairs_than_lds_table_corpus,
    "complete_doc_over_k5_limit": par.complete_doc_over_k5_limit_corpus,
    "big_docs_split": par.big_docs_split_corpus,
    "repeated_2900": lambda: cp.repeated_terms_corpus(2900, False),
    "repeated_3400_twice": lambda: cp.repeated_terms_corpus(3400, True),
    "hot_key": lambda: cp.hot_key_corpus()[:2],
    "docs_255": lambda: cp.many_documents_corpus(255),
    "docs_256": lambda: cp.many_documents_corpus(256),
    "docs_257": lambda: cp.many_documents_corpus(257),
    "docs_600": lambda: cp.many_documents_corpus(600),
}


@functools.lru_cache(maxsize=None)
def corpus_and_oracle(name):
    """built once and shared by the three instances"""
    data, off = CORPORA[name]()
    return data, off, oracle_py.run(data, off)


@pytest.mark.parametrize("name", list(CORPORA))
def test_edge_corpus_on_instance(k1, name):
    instance, e = k1
    data, off, ora = corpus_and_oracle(name)
    e.run_host(data, off)
    res = e.fetch()
    assert_same_result(res, ora)
    assert res["output_txt"] == ora["output_txt"]
    assert e.text() == ora["output_txt"]
    info = e.info()
    assert_k1_instance(info, instance)
    assert info["ntokens"] == int(ora["count"].sum())
