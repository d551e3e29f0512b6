"""ctypes binding of include/tfidf.h (libtfidf_hip.so).

Plumbing for tests and bench.py: every compute call goes through the C-ABI into the
gfx950 HIP kernels.  Loading fails loudly when the library has not been built; there is
no Python or CPU fallback for any stage.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# TFIDF_LIB=<variant> selects a diagnostic build lib/libtfidf_hip_<variant>.so (K1 phase
# stamps, K1 ablations); never used for benches or tests
_VARIANT = os.environ.get("TFIDF_LIB", "")
LIB_PATH = os.path.join(PKG_DIR, "lib", "libtfidf_hip_%s.so" % _VARIANT if _VARIANT else "libtfidf_hip.so")
CLI_PATH = os.path.join(PKG_DIR, "bin", "tfidf")

TFIDF_CORPUS_DEVICE = 1
UNIQUE_ID_BYTES = 128
RUN_K1_VS = 2   # tfidf_run_info.flags (include/tfidf.h): slot-keyed K1 ...
RUN_K1_ST = 4   # retired (round 3's k_tokcount_st, removed in round 5): never set
RUN_REC_PACK = 32        # K1 emitted one-word (count, slot) records (TFIDF_REC_PACK not 0, k_tokcount_sl, <= 4M slots)
RUN_REC_PACK_KEPT = 64   # ... kept one word through DF and the score kernels (else unpacked after K1)
RUN_K1_SL = 8   # ... run as k_tokcount_sl (the default up to 32M vocabulary slots; else k_tokcount_vs)
RUN_XCHG_DENSE = 16  # multi-rank: the DF exchange used the dense all-reduce form
ABI_VERSION = 2  # TFIDF_ABI_VERSION of include/tfidf.h this binding is written for

# exported symbols declared by include/tfidf.h
EXPORTS = [
    "tfidf_open", "tfidf_close", "tfidf_strerror", "tfidf_abi_version", "tfidf_comm_unique_id",
    "tfidf_comm_init", "tfidf_run", "tfidf_fetch", "tfidf_result_free", "tfidf_last_run_info", "tfidf_alloc_stats",
    "tfidf_alloc_live", "tfidf_grid_cus",
    "tfidf_stage_name", "tfidf_set_timing", "tfidf_write_output", "tfidf_print_jobs",
    "tfidf_ingest_dir", "tfidf_free", "tfidf_synth_host", "tfidf_synth_device",
    "tfidf_format", "tfidf_copy_text", "tfidf_write_output_gpu", "tfidf_format_f64",
    "tfidf_ingest_dir_device", "tfidf_hbm_probe", "tfidf_group_open", "tfidf_group_size", "tfidf_group_ctx",
    "tfidf_group_run", "tfidf_group_write_output", "tfidf_group_close", "tfidf_plan_dir", "tfidf_plan_free",
    "tfidf_ingest_shard_device", "tfidf_doc_name_order", "tfidf_shard_split", "tfidf_device_count",
    "tfidf_last_output_info", "tfidf_run_totals_get",
    "tfidf_query", "tfidf_hits_free", "tfidf_group_query", "tfidf_last_query_info",
    "tfidf_top_terms", "tfidf_doc_terms_free", "tfidf_group_top_terms", "tfidf_last_terms_info",
    "tfidf_similar", "tfidf_neighbors_free", "tfidf_group_similar", "tfidf_last_similar_info",
    "tfidf_kmeans", "tfidf_clusters_free", "tfidf_last_kmeans_info",
    "tfidf_query_bm25", "tfidf_group_query_bm25", "tfidf_last_bm25_info",
    "tfidf_clauses_check", "tfidf_query_clauses", "tfidf_group_query_clauses", "tfidf_last_clause_info",
    "tfidf_transform", "tfidf_rows_free", "tfidf_group_transform", "tfidf_last_transform_info",
    "tfidf_model_check", "tfidf_model_export", "tfidf_group_model_export", "tfidf_model_import",
    "tfidf_model_save", "tfidf_model_load", "tfidf_model_free", "tfidf_last_model_info",
    "tfidf_analyzer_check", "tfidf_analyze_host", "tfidf_analyze", "tfidf_last_analyze_info",
    "tfidf_stem_porter",
    "tfidf_ngram_check", "tfidf_ngrams_host", "tfidf_ngrams", "tfidf_last_ngram_info",
    "tfidf_prune_check", "tfidf_prune", "tfidf_group_prune", "tfidf_last_prune_info", "tfidf_model_prune",
    "tfidf_weighting_check", "tfidf_reweight", "tfidf_weighting_get", "tfidf_group_reweight",
    "tfidf_last_reweight_info", "tfidf_result_reweight",
    "tfidf_dedup_check", "tfidf_minhash", "tfidf_signatures_free", "tfidf_near_dups", "tfidf_dups_free",
    "tfidf_last_dedup_info", "tfidf_result_minhash", "tfidf_result_near_dups", "tfidf_dedup_groups",
    "tfidf_nb_check", "tfidf_nb_model_free", "tfidf_nb_labels_free", "tfidf_nb_fit", "tfidf_nb_predict",
    "tfidf_nb_predict_rows", "tfidf_nb_export", "tfidf_last_nb_info", "tfidf_result_nb_fit", "tfidf_nb_model_predict",
    "tfidf_match_check", "tfidf_match_terms", "tfidf_term_matches_free", "tfidf_group_match_terms",
    "tfidf_model_match_terms", "tfidf_last_match_info",
    "tfidf_snippets_check", "tfidf_snippets_free", "tfidf_snippet", "tfidf_group_snippet", "tfidf_result_snippet",
    "tfidf_last_snippet_info",
]
QUERY_MAX_K = 1024  # TFIDF_QUERY_MAX_K
RANK_TFIDF = 0  # TFIDF_RANK_TFIDF
RANK_BM25 = 1  # TFIDF_RANK_BM25
CLAUSE_MAX_TERMS = 4095  # TFIDF_CLAUSE_MAX_TERMS
CLAUSE_MAX_NOT = 255  # TFIDF_CLAUSE_MAX_NOT
TERMS_MAX_K = 1024  # TFIDF_TERMS_MAX_K
SIMILAR_MAX_K = 1024  # TFIDF_SIMILAR_MAX_K
KMEANS_MAX_K = 256  # TFIDF_KMEANS_MAX_K
KMEANS_MAX_TERMS = 64  # TFIDF_KMEANS_MAX_TERMS
NO_CLUSTER = 0xFFFFFFFF  # TFIDF_NO_CLUSTER: tfidf_clusters.label of a document with norm 0
NO_POS = 0xFFFFFFFF  # tfidf_doc_terms.pos of a document the shard does not hold
E_INVAL = -1
E_STATE = -10
TFIDF_GROUP_LOCAL = 1
E_PEER = -11
E_CAPACITY = -9
E_OUTPUT = -8
E_MODEL = -12
AN_LOWER = 1  # TFIDF_AN_LOWER
AN_PUNCT = 2  # TFIDF_AN_PUNCT
AN_UTF8 = 16  # TFIDF_AN_UTF8
STEM_NONE = 0  # TFIDF_STEM_NONE
STEM_PORTER = 1  # TFIDF_STEM_PORTER
AN_MAX_WORD = 64  # TFIDF_AN_MAX_WORD
AN_MAX_STOP = 4096  # TFIDF_AN_MAX_STOP
AN_MAX_STOP_BYTES = 32768  # TFIDF_AN_MAX_STOP_BYTES
AN_SLOT_CORPUS = 0  # TFIDF_AN_SLOT_CORPUS
AN_SLOT_BATCH = 1  # TFIDF_AN_SLOT_BATCH
NGRAM_MAX_N = 8  # TFIDF_NGRAM_MAX_N
NG_SLOT_CORPUS = 0  # TFIDF_NG_SLOT_CORPUS
NG_SLOT_BATCH = 1  # TFIDF_NG_SLOT_BATCH
TF_MODES = {"ratio": 0, "raw": 1, "log": 2, "binary": 3}  # TFIDF_TF_*
IDF_MODES = {"ref": 0, "smooth": 1, "plus1": 2, "none": 3}  # TFIDF_IDF_*
NORM_MODES = {"none": 0, "l2": 1, "l1": 2}  # TFIDF_NORM_*
MINHASH_MAX_H = 256  # TFIDF_MINHASH_MAX_H
NB_MAX_CLASSES = 256  # TFIDF_NB_MAX_CLASSES
NB_MAX_ALPHA = float.fromhex("0x1p+900")  # TFIDF_NB_MAX_ALPHA
NB_VARIANTS = {"multinomial": 0, "complement": 1}  # TFIDF_NB_MULTINOMIAL / TFIDF_NB_COMPLEMENT
NB_FEATURES = {"count": 0, "binary": 1}  # TFIDF_NB_COUNT / TFIDF_NB_BINARY
NB_ALL_SCORES = 1  # TFIDF_NB_ALL_SCORES
NO_CLASS = 0xFFFFFFFF  # TFIDF_NO_CLASS: tfidf_nb_labels.label of a document the context does not hold
MATCH_MAX_PATTERN = 64  # TFIDF_MATCH_MAX_PATTERN
MATCH_MAX_EDITS = 2  # TFIDF_MATCH_MAX_EDITS
MATCH_MAX_EXPANSIONS = 1024  # TFIDF_MATCH_MAX_EXPANSIONS
MATCH_MAX_PATTERNS = 65536  # TFIDF_MATCH_MAX_PATTERNS
MATCH_FUZZY = 0  # TFIDF_MATCH_FUZZY
MATCH_PREFIX = 1  # TFIDF_MATCH_PREFIX
MATCH_TRANSPOSE = 1  # TFIDF_MATCH_TRANSPOSE
MATCH_DEFAULT_RECORDS = 262144  # the device match list's default capacity (tfidf_match_params.list_records == 0)
SNIP_MAX_TERMS = 256  # TFIDF_SNIP_MAX_TERMS
SNIP_MAX_JOBS = 1 << 20  # TFIDF_SNIP_MAX_JOBS
SNIP_MAX_WINDOW = 1024  # TFIDF_SNIP_MAX_WINDOW
SNIP_MAX_MARKS = 1024  # TFIDF_SNIP_MAX_MARKS
SNIP_TEXT = 1  # TFIDF_SNIP_TEXT
SNIP_NO_DOC = 1  # TFIDF_SNIP_NO_DOC
SNIP_TRUNCATED = 2  # TFIDF_SNIP_TRUNCATED
SNIP_MIN_SCRATCH = 65536  # TFIDF_SNIP_MIN_SCRATCH


class Corpus(C.Structure):
    _fields_ = [
        ("bytes", C.c_void_p), ("nbytes", C.c_uint64), ("doc_off", C.c_void_p), ("doc_ids", C.c_void_p),
        ("ndocs", C.c_uint32), ("flags", C.c_uint32), ("ndocs_total", C.c_uint64),
    ]


class Result(C.Structure):
    _fields_ = [
        ("npairs", C.c_uint64), ("ndocs", C.c_uint32), ("nterms", C.c_uint32), ("ndocs_total", C.c_uint64),
        ("pair_doc", C.POINTER(C.c_uint32)), ("pair_term", C.POINTER(C.c_uint32)),
        ("pair_count", C.POINTER(C.c_uint32)), ("pair_docsize", C.POINTER(C.c_uint32)),
        ("pair_df", C.POINTER(C.c_uint32)), ("pair_score", C.POINTER(C.c_double)),
        ("doc_id", C.POINTER(C.c_uint32)), ("doc_size", C.POINTER(C.c_uint32)),
        ("term_off", C.POINTER(C.c_uint64)), ("term_bytes", C.POINTER(C.c_uint8)),
        ("term_df", C.POINTER(C.c_uint32)),
    ]


class RunInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("nbytes", C.c_uint64), ("ntokens", C.c_uint64), ("npairs", C.c_uint64), ("nterms", C.c_uint32),
        ("nterms_global", C.c_uint32), ("nchunks", C.c_uint64), ("partial_records", C.c_uint64),
        ("ndocs", C.c_uint32), ("vocab_capacity", C.c_uint32), ("ms_total", C.c_double),
        ("ms_tokcount", C.c_double), ("ms_stage", C.c_double * 16), ("nstages", C.c_uint32), ("flags", C.c_uint32),
        ("device_allocs", C.c_uint64), ("device_alloc_bytes", C.c_uint64),
        ("idf_logs", C.c_uint64), ("ms_idf_host", C.c_double), ("ms_idf_wait", C.c_double),
        ("k1_workgroups", C.c_uint32), ("reserved2", C.c_uint32),
    ]


class RunTotals(C.Structure):
    _fields_ = [("runs", C.c_uint64), ("ms_tokcount", C.c_double), ("ms_total", C.c_double),
                ("idf_logs", C.c_uint64), ("ms_idf_host", C.c_double), ("ms_idf_wait", C.c_double)]


class OutputInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("text_bytes", C.c_uint64), ("writers", C.c_uint32), ("formatted", C.c_uint32),
        ("ms_prepare", C.c_double), ("ms_d2h_busy", C.c_double), ("ms_write", C.c_double), ("ms_total", C.c_double),
    ]


class Queries(C.Structure):
    _fields_ = [("bytes", C.c_void_p), ("nbytes", C.c_uint64), ("q_off", C.c_void_p), ("nqueries", C.c_uint32)]


class Hits(C.Structure):
    _fields_ = [
        ("nqueries", C.c_uint32), ("k", C.c_uint32), ("nhits", C.POINTER(C.c_uint32)),
        ("nmatch", C.POINTER(C.c_uint64)), ("nterms_found", C.POINTER(C.c_uint32)),
        ("doc", C.POINTER(C.c_uint32)), ("score", C.POINTER(C.c_double)),
    ]


class QueryInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("nqueries", C.c_uint32), ("k", C.c_uint32), ("nterms", C.c_uint32),
        ("nterms_found", C.c_uint32), ("ngroups", C.c_uint32), ("group_queries", C.c_uint32),
        ("acc_bytes", C.c_uint64), ("ms_lookup", C.c_double), ("ms_score", C.c_double), ("ms_topk", C.c_double),
        ("ms_total", C.c_double),
    ]


class Bm25Params(C.Structure):
    _fields_ = [("size", C.c_uint64), ("k1", C.c_double), ("b", C.c_double), ("avgdl", C.c_double)]


class Bm25Info(C.Structure):
    _fields_ = QueryInfo._fields_ + [("avgdl", C.c_double)]


class Clauses(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("nqueries", C.c_uint32), ("ranking", C.c_uint32),
        ("must", C.POINTER(Queries)), ("should", C.POINTER(Queries)), ("must_not", C.POINTER(Queries)),
        ("min_should", C.c_void_p), ("bm25", C.POINTER(Bm25Params)),
    ]


class ClauseInfo(C.Structure):
    _fields_ = Bm25Info._fields_ + [("nq_unsatisfiable", C.c_uint32), ("ngroups_tab_lds", C.c_uint32)]


class DocTerms(C.Structure):
    _fields_ = [
        ("ndocs", C.c_uint32), ("k", C.c_uint32), ("doc", C.POINTER(C.c_uint32)), ("pos", C.POINTER(C.c_uint32)),
        ("npairs", C.POINTER(C.c_uint64)), ("nterms", C.POINTER(C.c_uint32)), ("term", C.POINTER(C.c_uint32)),
        ("count", C.POINTER(C.c_uint32)), ("score", C.POINTER(C.c_double)), ("pair", C.POINTER(C.c_uint64)),
        ("word_off", C.POINTER(C.c_uint64)), ("word_bytes", C.POINTER(C.c_uint8)),
    ]


class TermsInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("ndocs", C.c_uint32), ("k", C.c_uint32), ("nbatches", C.c_uint32),
        ("big_docs", C.c_uint32), ("out_bytes", C.c_uint64), ("ms_lookup", C.c_double), ("ms_select", C.c_double),
        ("ms_words", C.c_double), ("ms_total", C.c_double),
    ]


class Neighbors(C.Structure):
    _fields_ = [
        ("ndocs", C.c_uint32), ("k", C.c_uint32), ("doc", C.POINTER(C.c_uint32)), ("pos", C.POINTER(C.c_uint32)),
        ("npairs", C.POINTER(C.c_uint64)), ("norm", C.POINTER(C.c_double)), ("nmatch", C.POINTER(C.c_uint64)),
        ("nnb", C.POINTER(C.c_uint32)), ("nb_doc", C.POINTER(C.c_uint32)), ("nb_shared", C.POINTER(C.c_uint32)),
        ("nb_score", C.POINTER(C.c_double)),
    ]


class SimilarInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("rows", C.c_uint32), ("k", C.c_uint32), ("ngroups", C.c_uint32),
        ("group_rows", C.c_uint32), ("acc_bytes", C.c_uint64), ("big_docs", C.c_uint32), ("reserved", C.c_uint32),
        ("ms_norms", C.c_double), ("ms_table", C.c_double), ("ms_score", C.c_double), ("ms_topk", C.c_double),
        ("ms_total", C.c_double),
    ]


class KmeansParams(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("k", C.c_uint32), ("max_iter", C.c_uint32), ("nterms", C.c_uint32),
        ("nseeds", C.c_uint32), ("seeds", C.POINTER(C.c_uint32)),
    ]


class Clusters(C.Structure):
    _fields_ = [
        ("ndocs", C.c_uint32), ("k", C.c_uint32), ("iterations", C.c_uint32), ("converged", C.c_uint32),
        ("t", C.c_uint32), ("reserved", C.c_uint32), ("doc", C.POINTER(C.c_uint32)), ("label", C.POINTER(C.c_uint32)),
        ("sim", C.POINTER(C.c_double)), ("size", C.POINTER(C.c_uint32)), ("seed", C.POINTER(C.c_uint32)),
        ("nterms", C.POINTER(C.c_uint32)), ("term", C.POINTER(C.c_uint32)), ("weight", C.POINTER(C.c_double)),
        ("word_off", C.POINTER(C.c_uint64)), ("word_bytes", C.POINTER(C.c_uint8)),
    ]


class KmeansInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("ndocs", C.c_uint32), ("k", C.c_uint32), ("passes", C.c_uint32), ("updates", C.c_uint32),
        ("clusterable", C.c_uint32), ("split", C.c_uint32), ("matrix_bytes", C.c_uint64), ("work_bytes", C.c_uint64),
        ("ms_norms", C.c_double), ("ms_assign", C.c_double), ("ms_update", C.c_double), ("ms_terms", C.c_double),
        ("ms_total", C.c_double),
    ]


class Rows(C.Structure):
    _fields_ = [
        ("ndocs", C.c_uint32), ("reserved", C.c_uint32), ("npairs", C.c_uint64), ("ntokens", C.c_uint64),
        ("row_off", C.POINTER(C.c_uint64)), ("doc_size", C.POINTER(C.c_uint32)), ("doc_oov", C.POINTER(C.c_uint32)),
        ("term", C.POINTER(C.c_uint32)), ("count", C.POINTER(C.c_uint32)), ("df", C.POINTER(C.c_uint32)),
        ("score", C.POINTER(C.c_double)), ("word_off", C.POINTER(C.c_uint64)), ("word_len", C.POINTER(C.c_uint32)),
    ]


class TransformInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("ndocs", C.c_uint32), ("nslices", C.c_uint32), ("ntokens", C.c_uint64),
        ("npairs", C.c_uint64), ("noov", C.c_uint64), ("scratch_bytes", C.c_uint64), ("ms_tokens", C.c_double),
        ("ms_resolve", C.c_double), ("ms_sort", C.c_double), ("ms_pairs", C.c_double), ("ms_total", C.c_double),
    ]


class Model(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("ndocs_total", C.c_uint64), ("nterms", C.c_uint32), ("reserved", C.c_uint32),
        ("term_off", C.POINTER(C.c_uint64)), ("term_bytes", C.POINTER(C.c_uint8)), ("term_df", C.POINTER(C.c_uint32)),
    ]


class ModelInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("nterms", C.c_uint32), ("reserved", C.c_uint32), ("table_slots", C.c_uint64),
        ("blob_bytes", C.c_uint64), ("long_terms", C.c_uint64), ("ms_build", C.c_double), ("ms_total", C.c_double),
    ]


class Analyzer(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("flags", C.c_uint32), ("min_len", C.c_uint32), ("stop_bytes", C.c_void_p),
        ("stop_off", C.c_void_p), ("nstop", C.c_uint32), ("stemmer", C.c_uint32),
    ]


class AnalyzeInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("nbytes", C.c_uint64), ("ndocs", C.c_uint32), ("nstop", C.c_uint32),
        ("table_slots", C.c_uint32), ("lds_bytes", C.c_uint32), ("tile_bytes", C.c_uint32), ("grid", C.c_uint32),
        ("blanked_tokens", C.c_uint64), ("ms_kernel", C.c_double), ("ms_total", C.c_double),
        ("stemmed_tokens", C.c_uint64),
    ]


class AnalyzeInfoUtf8(AnalyzeInfo):
    """tfidf_analyze_info as it is now.  The struct is size-prefixed: AnalyzeInfo is the layout up
    to stemmed_tokens, which callers built before TFIDF_AN_UTF8 still pass."""
    _fields_ = [("utf8_changed", C.c_uint64)]


class NgramParams(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("min_n", C.c_uint32), ("max_n", C.c_uint32), ("joiner", C.c_uint8),
        ("reserved", C.c_uint8 * 7),
    ]


class NgramInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("nbytes_in", C.c_uint64), ("nbytes_out", C.c_uint64), ("ntokens", C.c_uint64),
        ("ngrams", C.c_uint64), ("ndocs", C.c_uint32), ("tile_bytes", C.c_uint32), ("grid", C.c_uint32),
        ("reserved", C.c_uint32), ("scratch_bytes", C.c_uint64), ("ms_bounds", C.c_double), ("ms_sizes", C.c_double),
        ("ms_write", C.c_double), ("ms_total", C.c_double),
    ]


class PruneParams(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("min_df", C.c_uint32), ("max_df", C.c_uint32), ("max_features", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class PruneInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("nterms_before", C.c_uint32), ("nterms_after", C.c_uint32),
        ("npairs_before", C.c_uint64), ("npairs_after", C.c_uint64), ("docs_emptied", C.c_uint32),
        ("cut_df", C.c_uint32), ("ms_select", C.c_double), ("ms_terms", C.c_double), ("ms_pairs", C.c_double),
        ("ms_total", C.c_double),
    ]


class Weighting(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("tf", C.c_uint32), ("idf", C.c_uint32), ("norm", C.c_uint32), ("reserved", C.c_uint32),
    ]


class ReweightInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("tf", C.c_uint32), ("idf", C.c_uint32), ("norm", C.c_uint32), ("changed", C.c_uint32),
        ("npairs", C.c_uint64), ("ndocs", C.c_uint32), ("zero_norm_docs", C.c_uint32), ("nlogs", C.c_uint64),
        ("max_count", C.c_uint32), ("listed_counts", C.c_uint32), ("big_docs", C.c_uint32), ("reserved", C.c_uint32),
        ("ms_tables", C.c_double), ("ms_pairs", C.c_double), ("ms_total", C.c_double),
    ]


class DedupParams(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("nhashes", C.c_uint32), ("rows", C.c_uint32), ("seed", C.c_uint64),
        ("threshold", C.c_double),
    ]


class Signatures(C.Structure):
    _fields_ = [
        ("ndocs", C.c_uint32), ("nhashes", C.c_uint32), ("doc", C.POINTER(C.c_uint32)),
        ("npairs", C.POINTER(C.c_uint32)), ("sig", C.POINTER(C.c_uint32)),
    ]


class Dups(C.Structure):
    _fields_ = [
        ("ndocs", C.c_uint32), ("ngroups", C.c_uint32), ("ncand", C.c_uint64), ("nedges", C.c_uint64),
        ("doc", C.POINTER(C.c_uint32)), ("group", C.POINTER(C.c_uint32)),
        ("a_pos", C.POINTER(C.c_uint32)), ("b_pos", C.POINTER(C.c_uint32)), ("a_doc", C.POINTER(C.c_uint32)),
        ("b_doc", C.POINTER(C.c_uint32)), ("shared", C.POINTER(C.c_uint32)), ("uni", C.POINTER(C.c_uint32)),
        ("same", C.POINTER(C.c_uint32)), ("jaccard", C.POINTER(C.c_double)),
    ]


class DedupInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("ndocs", C.c_uint32), ("nhashes", C.c_uint32), ("rows", C.c_uint32),
        ("clusterable", C.c_uint32), ("ncand", C.c_uint64), ("nedges", C.c_uint64), ("ngroups", C.c_uint32),
        ("big_docs", C.c_uint32), ("sig_bytes", C.c_uint64), ("work_bytes", C.c_uint64), ("ms_hash", C.c_double),
        ("ms_sig", C.c_double), ("ms_bands", C.c_double), ("ms_verify", C.c_double), ("ms_total", C.c_double),
    ]


class NbParams(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("nclasses", C.c_uint32), ("variant", C.c_uint32), ("feature", C.c_uint32),
        ("uniform_prior", C.c_uint32), ("alpha", C.c_double), ("nlabelled", C.c_uint64),
        ("doc", C.POINTER(C.c_uint32)), ("label", C.POINTER(C.c_uint32)),
    ]


class NbModel(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("nclasses", C.c_uint32), ("nterms", C.c_uint32), ("variant", C.c_uint32),
        ("feature", C.c_uint32), ("uniform_prior", C.c_uint32), ("reserved", C.c_uint32), ("alpha", C.c_double),
        ("nlabelled", C.c_uint64), ("class_docs", C.POINTER(C.c_uint64)), ("class_total", C.POINTER(C.c_uint64)),
        ("feature_count", C.POINTER(C.c_uint64)), ("prior", C.POINTER(C.c_double)), ("weight", C.POINTER(C.c_double)),
    ]


class NbLabels(C.Structure):
    _fields_ = [
        ("ndocs", C.c_uint32), ("nclasses", C.c_uint32), ("doc", C.POINTER(C.c_uint32)), ("pos", C.POINTER(C.c_uint32)),
        ("label", C.POINTER(C.c_uint32)), ("score", C.POINTER(C.c_double)), ("scores", C.POINTER(C.c_double)),
    ]


class NbInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("nclasses", C.c_uint32), ("nterms", C.c_uint32), ("nlabelled", C.c_uint64),
        ("matrix_bytes", C.c_uint64), ("nlogs", C.c_uint64), ("nlisted", C.c_uint64), ("predict_rows", C.c_uint32),
        ("reserved", C.c_uint32), ("ms_logs_host", C.c_double), ("ms_count", C.c_double), ("ms_weights", C.c_double),
        ("ms_predict", C.c_double), ("ms_total", C.c_double),
    ]


class Patterns(C.Structure):
    _fields_ = [
        ("bytes", C.c_void_p), ("nbytes", C.c_uint64), ("p_off", C.c_void_p), ("npatterns", C.c_uint32),
        ("kind", C.c_void_p), ("max_edits", C.c_void_p),
    ]


class MatchParams(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("max_expansions", C.c_uint32), ("flags", C.c_uint32), ("fixed_prefix", C.c_uint32),
        ("reserved", C.c_uint32), ("list_records", C.c_uint64),
    ]


class TermMatches(C.Structure):
    _fields_ = [
        ("npatterns", C.c_uint32), ("k", C.c_uint32), ("nmatch", C.POINTER(C.c_uint64)), ("nterms", C.POINTER(C.c_uint32)),
        ("term", C.POINTER(C.c_uint32)), ("dist", C.POINTER(C.c_uint8)), ("df", C.POINTER(C.c_uint32)),
        ("word_off", C.POINTER(C.c_uint64)), ("word_bytes", C.POINTER(C.c_uint8)),
    ]


class MatchInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("npatterns", C.c_uint32), ("k", C.c_uint32), ("ngroups", C.c_uint32),
        ("nbatches", C.c_uint32), ("nrecords", C.c_uint64), ("list_records", C.c_uint64), ("ms_scan", C.c_double),
        ("ms_select", C.c_double), ("ms_words", C.c_double), ("ms_total", C.c_double),
    ]


class SnippetParams(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("window", C.c_uint32), ("max_marks", C.c_uint32), ("flags", C.c_uint32),
        ("reserved", C.c_uint32), ("scratch_bytes", C.c_uint64),
    ]


class Snippets(C.Structure):
    _fields_ = [
        ("njobs", C.c_uint32), ("nqueries", C.c_uint32), ("flags", C.POINTER(C.c_uint32)),
        ("ntokens", C.POINTER(C.c_uint32)), ("nmatch", C.POINTER(C.c_uint32)),
        ("nterms_matched", C.POINTER(C.c_uint32)), ("win_tok", C.POINTER(C.c_uint32)),
        ("win_byte", C.POINTER(C.c_uint64)), ("cover", C.POINTER(C.c_uint32)), ("hits", C.POINTER(C.c_uint32)),
        ("mark_off", C.POINTER(C.c_uint64)), ("mark_byte", C.POINTER(C.c_uint64)), ("mark_len", C.POINTER(C.c_uint32)),
        ("mark_slot", C.POINTER(C.c_uint32)), ("text_off", C.POINTER(C.c_uint64)), ("text", C.POINTER(C.c_uint8)),
        ("qterm_off", C.POINTER(C.c_uint64)), ("qterm_pos", C.POINTER(C.c_uint64)), ("qterm_len", C.POINTER(C.c_uint32)),
        ("qterm_found", C.POINTER(C.c_uint8)),
    ]


class SnippetInfo(C.Structure):
    _fields_ = [
        ("size", C.c_uint64), ("njobs", C.c_uint32), ("nbatches", C.c_uint32), ("nsubbatches", C.c_uint32),
        ("nbig", C.c_uint32), ("ntiles", C.c_uint64), ("nbytes", C.c_uint64), ("ntokens", C.c_uint64),
        ("nmatches", C.c_uint64), ("scratch_bytes", C.c_uint64), ("ms_lookup", C.c_double), ("ms_count", C.c_double),
        ("ms_write", C.c_double), ("ms_select", C.c_double), ("ms_emit", C.c_double), ("ms_total", C.c_double),
    ]


class DirPlan(C.Structure):
    _fields_ = [
        ("ndocs", C.c_uint32), ("nshards", C.c_uint32), ("doc_ids", C.POINTER(C.c_uint32)),
        ("doc_bytes", C.POINTER(C.c_uint64)), ("shard_first", C.POINTER(C.c_uint32)),
        ("shard_bytes", C.POINTER(C.c_uint64)),
    ]


class IngestInfo(C.Structure):
    _fields_ = [
        ("nbytes", C.c_uint64), ("segments", C.c_uint64), ("ndocs", C.c_uint32), ("threads", C.c_uint32),
        ("ms_scan", C.c_double), ("ms_read", C.c_double), ("ms_total", C.c_double),
    ]


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"libtfidf_hip.so not built ({LIB_PATH}); run __graft_entry__.build()")
        L = C.CDLL(LIB_PATH)
        L.tfidf_open.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.tfidf_close.argtypes = [C.c_void_p]
        L.tfidf_close.restype = None
        L.tfidf_strerror.restype = C.c_char_p
        L.tfidf_run.argtypes = [C.c_void_p, C.POINTER(Corpus)]
        L.tfidf_fetch.argtypes = [C.c_void_p, C.POINTER(Result)]
        L.tfidf_result_free.argtypes = [C.POINTER(Result)]
        L.tfidf_result_free.restype = None
        L.tfidf_last_run_info.argtypes = [C.c_void_p, C.POINTER(RunInfo)]
        L.tfidf_run_totals_get.argtypes = [C.c_void_p, C.POINTER(RunTotals), C.c_int]
        L.tfidf_alloc_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.tfidf_alloc_live.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.tfidf_grid_cus.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.tfidf_stage_name.restype = C.c_char_p
        L.tfidf_set_timing.argtypes = [C.c_void_p, C.c_int]
        L.tfidf_comm_unique_id.argtypes = [C.c_void_p]
        L.tfidf_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.tfidf_write_output.argtypes = [C.POINTER(Result), C.c_char_p]
        L.tfidf_format.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.tfidf_copy_text.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
        L.tfidf_write_output_gpu.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.tfidf_last_output_info.argtypes = [C.c_void_p, C.POINTER(OutputInfo)]
        L.tfidf_format_f64.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.tfidf_synth_host.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
        L.tfidf_synth_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_uint32, C.c_uint64, C.POINTER(Corpus)]
        L.tfidf_ingest_dir_device.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(Corpus),
                                              C.POINTER(C.c_uint32), C.POINTER(IngestInfo)]
        L.tfidf_hbm_probe.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.tfidf_group_open.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.tfidf_group_size.argtypes = [C.c_void_p]
        L.tfidf_group_ctx.argtypes = [C.c_void_p, C.c_int]
        L.tfidf_group_ctx.restype = C.c_void_p
        L.tfidf_group_run.argtypes = [C.c_void_p, C.c_void_p]
        L.tfidf_group_write_output.argtypes = [C.c_void_p, C.c_char_p]
        L.tfidf_group_close.argtypes = [C.c_void_p]
        L.tfidf_group_close.restype = None
        L.tfidf_plan_dir.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.POINTER(DirPlan), C.POINTER(C.c_uint32)]
        L.tfidf_plan_free.argtypes = [C.POINTER(DirPlan)]
        L.tfidf_plan_free.restype = None
        L.tfidf_ingest_shard_device.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(DirPlan), C.c_uint32, C.c_int,
                                                C.POINTER(Corpus), C.POINTER(C.c_uint32), C.POINTER(IngestInfo)]
        L.tfidf_doc_name_order.argtypes = [C.c_uint32, C.c_void_p]
        L.tfidf_shard_split.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.tfidf_query.argtypes = [C.c_void_p, C.POINTER(Queries), C.c_uint32, C.POINTER(Hits)]
        L.tfidf_group_query.argtypes = [C.c_void_p, C.POINTER(Queries), C.c_uint32, C.POINTER(Hits)]
        L.tfidf_hits_free.argtypes = [C.POINTER(Hits)]
        L.tfidf_hits_free.restype = None
        L.tfidf_last_query_info.argtypes = [C.c_void_p, C.POINTER(QueryInfo)]
        L.tfidf_query_bm25.argtypes = [C.c_void_p, C.POINTER(Queries), C.c_uint32, C.POINTER(Bm25Params), C.POINTER(Hits)]
        L.tfidf_group_query_bm25.argtypes = [C.c_void_p, C.POINTER(Queries), C.c_uint32, C.POINTER(Bm25Params),
                                             C.POINTER(Hits)]
        L.tfidf_last_bm25_info.argtypes = [C.c_void_p, C.POINTER(Bm25Info)]
        L.tfidf_clauses_check.argtypes = [C.POINTER(Clauses)]
        L.tfidf_query_clauses.argtypes = [C.c_void_p, C.POINTER(Clauses), C.c_uint32, C.POINTER(Hits)]
        L.tfidf_group_query_clauses.argtypes = [C.c_void_p, C.POINTER(Clauses), C.c_uint32, C.POINTER(Hits)]
        L.tfidf_last_clause_info.argtypes = [C.c_void_p, C.POINTER(ClauseInfo)]
        L.tfidf_top_terms.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DocTerms)]
        L.tfidf_group_top_terms.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DocTerms)]
        L.tfidf_doc_terms_free.argtypes = [C.POINTER(DocTerms)]
        L.tfidf_doc_terms_free.restype = None
        L.tfidf_last_terms_info.argtypes = [C.c_void_p, C.POINTER(TermsInfo)]
        L.tfidf_similar.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Neighbors)]
        L.tfidf_group_similar.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Neighbors)]
        L.tfidf_neighbors_free.argtypes = [C.POINTER(Neighbors)]
        L.tfidf_neighbors_free.restype = None
        L.tfidf_last_similar_info.argtypes = [C.c_void_p, C.POINTER(SimilarInfo)]
        L.tfidf_kmeans.argtypes = [C.c_void_p, C.POINTER(KmeansParams), C.POINTER(Clusters)]
        L.tfidf_clusters_free.argtypes = [C.POINTER(Clusters)]
        L.tfidf_clusters_free.restype = None
        L.tfidf_last_kmeans_info.argtypes = [C.c_void_p, C.POINTER(KmeansInfo)]
        L.tfidf_transform.argtypes = [C.c_void_p, C.POINTER(Corpus), C.POINTER(Rows)]
        L.tfidf_group_transform.argtypes = [C.c_void_p, C.POINTER(Corpus), C.POINTER(Rows)]
        L.tfidf_rows_free.argtypes = [C.POINTER(Rows)]
        L.tfidf_rows_free.restype = None
        L.tfidf_last_transform_info.argtypes = [C.c_void_p, C.POINTER(TransformInfo)]
        L.tfidf_model_check.argtypes = [C.POINTER(Model)]
        L.tfidf_model_export.argtypes = [C.c_void_p, C.POINTER(Model)]
        L.tfidf_group_model_export.argtypes = [C.c_void_p, C.POINTER(Model)]
        L.tfidf_model_import.argtypes = [C.c_void_p, C.POINTER(Model)]
        L.tfidf_model_save.argtypes = [C.POINTER(Model), C.c_char_p]
        L.tfidf_model_load.argtypes = [C.c_char_p, C.POINTER(Model)]
        L.tfidf_model_free.argtypes = [C.POINTER(Model)]
        L.tfidf_model_free.restype = None
        L.tfidf_last_model_info.argtypes = [C.c_void_p, C.POINTER(ModelInfo)]
        L.tfidf_analyzer_check.argtypes = [C.POINTER(Analyzer)]
        L.tfidf_analyze_host.argtypes = [C.POINTER(Analyzer), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
        L.tfidf_stem_porter.argtypes = [C.c_void_p, C.c_uint32]
        L.tfidf_analyze.argtypes = [C.c_void_p, C.POINTER(Analyzer), C.POINTER(Corpus), C.c_uint32, C.POINTER(Corpus)]
        L.tfidf_last_analyze_info.argtypes = [C.c_void_p, C.POINTER(AnalyzeInfo)]
        L.tfidf_ngram_check.argtypes = [C.POINTER(NgramParams)]
        L.tfidf_ngrams_host.argtypes = [C.POINTER(NgramParams), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p)]
        L.tfidf_ngrams.argtypes = [C.c_void_p, C.POINTER(NgramParams), C.POINTER(Corpus), C.c_uint32, C.POINTER(Corpus)]
        L.tfidf_last_ngram_info.argtypes = [C.c_void_p, C.POINTER(NgramInfo)]
        L.tfidf_prune_check.argtypes = [C.POINTER(PruneParams)]
        L.tfidf_prune.argtypes = [C.c_void_p, C.POINTER(PruneParams)]
        L.tfidf_group_prune.argtypes = [C.c_void_p, C.POINTER(PruneParams)]
        L.tfidf_last_prune_info.argtypes = [C.c_void_p, C.POINTER(PruneInfo)]
        L.tfidf_model_prune.argtypes = [C.POINTER(Model), C.POINTER(PruneParams), C.POINTER(Model)]
        L.tfidf_weighting_check.argtypes = [C.POINTER(Weighting)]
        L.tfidf_reweight.argtypes = [C.c_void_p, C.POINTER(Weighting)]
        L.tfidf_weighting_get.argtypes = [C.c_void_p, C.POINTER(Weighting)]
        L.tfidf_group_reweight.argtypes = [C.c_void_p, C.POINTER(Weighting)]
        L.tfidf_last_reweight_info.argtypes = [C.c_void_p, C.POINTER(ReweightInfo)]
        L.tfidf_result_reweight.argtypes = [C.POINTER(Result), C.POINTER(Weighting)]
        L.tfidf_dedup_check.argtypes = [C.POINTER(DedupParams)]
        L.tfidf_minhash.argtypes = [C.c_void_p, C.POINTER(DedupParams), C.POINTER(Signatures)]
        L.tfidf_signatures_free.argtypes = [C.POINTER(Signatures)]
        L.tfidf_signatures_free.restype = None
        L.tfidf_near_dups.argtypes = [C.c_void_p, C.POINTER(DedupParams), C.POINTER(Dups)]
        L.tfidf_dups_free.argtypes = [C.POINTER(Dups)]
        L.tfidf_dups_free.restype = None
        L.tfidf_last_dedup_info.argtypes = [C.c_void_p, C.POINTER(DedupInfo)]
        L.tfidf_result_minhash.argtypes = [C.POINTER(Result), C.POINTER(DedupParams), C.POINTER(Signatures)]
        L.tfidf_result_near_dups.argtypes = [C.POINTER(Result), C.POINTER(DedupParams), C.POINTER(Dups)]
        L.tfidf_dedup_groups.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                         C.POINTER(C.c_uint32)]
        L.tfidf_nb_check.argtypes = [C.POINTER(NbParams)]
        L.tfidf_nb_model_free.argtypes = [C.POINTER(NbModel)]
        L.tfidf_nb_model_free.restype = None
        L.tfidf_nb_labels_free.argtypes = [C.POINTER(NbLabels)]
        L.tfidf_nb_labels_free.restype = None
        L.tfidf_nb_fit.argtypes = [C.c_void_p, C.POINTER(NbParams)]
        L.tfidf_nb_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(NbLabels)]
        L.tfidf_nb_predict_rows.argtypes = [C.c_void_p, C.POINTER(Rows), C.c_uint32, C.POINTER(NbLabels)]
        L.tfidf_nb_export.argtypes = [C.c_void_p, C.POINTER(NbModel)]
        L.tfidf_last_nb_info.argtypes = [C.c_void_p, C.POINTER(NbInfo)]
        L.tfidf_result_nb_fit.argtypes = [C.POINTER(Result), C.POINTER(NbParams), C.POINTER(NbModel)]
        L.tfidf_nb_model_predict.argtypes = [C.POINTER(NbModel), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_uint32, C.POINTER(NbLabels)]
        L.tfidf_match_check.argtypes = [C.POINTER(Patterns), C.POINTER(MatchParams)]
        L.tfidf_match_terms.argtypes = [C.c_void_p, C.POINTER(Patterns), C.POINTER(MatchParams), C.POINTER(TermMatches)]
        L.tfidf_group_match_terms.argtypes = [C.c_void_p, C.POINTER(Patterns), C.POINTER(MatchParams),
                                              C.POINTER(TermMatches)]
        L.tfidf_model_match_terms.argtypes = [C.POINTER(Model), C.POINTER(Patterns), C.POINTER(MatchParams),
                                              C.POINTER(TermMatches)]
        L.tfidf_term_matches_free.argtypes = [C.POINTER(TermMatches)]
        L.tfidf_term_matches_free.restype = None
        L.tfidf_last_match_info.argtypes = [C.c_void_p, C.POINTER(MatchInfo)]
        L.tfidf_snippets_check.argtypes = [C.POINTER(SnippetParams)]
        L.tfidf_snippets_free.argtypes = [C.POINTER(Snippets)]
        L.tfidf_snippets_free.restype = None
        snip = [C.POINTER(Queries), C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(SnippetParams), C.POINTER(Snippets)]
        L.tfidf_snippet.argtypes = [C.c_void_p] + snip
        L.tfidf_group_snippet.argtypes = [C.c_void_p] + snip
        L.tfidf_result_snippet.argtypes = [C.POINTER(Result), C.POINTER(Corpus)] + snip
        L.tfidf_last_snippet_info.argtypes = [C.c_void_p, C.POINTER(SnippetInfo)]
        if L.tfidf_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH}: ABI version {L.tfidf_abi_version()}, binding expects {ABI_VERSION} "
                               f"(stale build: rebuild with __graft_entry__.build())")
        _lib = L
    return _lib


class TfidfError(RuntimeError):
    def __init__(self, rc: int, what: str):
        super().__init__(f"{what}: {lib().tfidf_strerror(rc).decode()} ({rc})")
        self.rc = rc


def _chk(rc: int, what: str) -> None:
    if rc != 0:
        raise TfidfError(rc, what)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _queries(queries):
    """a tfidf_queries over bytes objects, and the arrays it points into"""
    data = np.frombuffer(b"".join(queries), dtype=np.uint8)
    off = np.zeros(len(queries) + 1, dtype=np.uint64)
    if len(queries):
        off[1:] = np.cumsum([len(q) for q in queries], dtype=np.uint64)
    qs = Queries()
    qs.bytes = data.ctypes.data if len(data) else None
    qs.nbytes = len(data)
    qs.q_off = off.ctypes.data
    qs.nqueries = len(queries)
    return qs, (data, off)


def _query(fn, handle, queries, k: int, what: str, params=None) -> dict:
    """One batch through tfidf_query / tfidf_group_query (or, with params, their BM25 forms):
    queries are bytes objects.  A Clauses struct as `queries` goes through as it is."""
    if isinstance(queries, Clauses):
        qs = queries
    else:
        qs, _keep = _queries(queries)
    h = Hits()
    if params is None:
        _chk(fn(handle, C.byref(qs), k, C.byref(h)), what)
    else:
        _chk(fn(handle, C.byref(qs), k, C.byref(params), C.byref(h)), what)
    try:
        nq = int(h.nqueries)

        def arr(p, n, dt):
            return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)

        return {
            "k": int(h.k), "nhits": arr(h.nhits, nq, np.uint32), "nmatch": arr(h.nmatch, nq, np.uint64),
            "nterms_found": arr(h.nterms_found, nq, np.uint32),
            "doc": arr(h.doc, nq * k, np.uint32).reshape(nq, k),
            "score": arr(h.score, nq * k, np.float64).reshape(nq, k),
        }
    finally:
        lib().tfidf_hits_free(C.byref(h))


def _bm25_params(k1: float, b: float, avgdl: float) -> Bm25Params:
    p = Bm25Params()
    p.size = C.sizeof(Bm25Params)
    p.k1, p.b, p.avgdl = k1, b, avgdl
    return p


def make_clauses(must=None, should=None, must_not=None, min_should=None, bm25=None, nqueries=None):
    """A tfidf_clauses and the objects it points into (keep both alive for the call).  must /
    should / must_not: lists of bytes objects of one length, or None (empty in every query);
    min_should: one integer per query, or None; bm25: None ranks by the summed TF-IDF scores,
    True by BM25 with the defaults, a dict(k1=, b=, avgdl=) by BM25 with these; nqueries: the
    count, when it is not the texts' own."""
    texts = [t for t in (must, should, must_not) if t is not None]
    c = Clauses()
    c.size = C.sizeof(Clauses)
    c.nqueries = nqueries if nqueries is not None else (len(texts[0]) if texts else
                                                        (len(min_should) if min_should is not None else 0))
    keep = []
    for name, text in (("must", must), ("should", should), ("must_not", must_not)):
        if text is not None:
            qs, arrays = _queries(text)
            keep += [qs, arrays]
            setattr(c, name, C.pointer(qs))
    if min_should is not None:
        ms = np.ascontiguousarray(min_should, dtype=np.uint32)
        if len(ms) == 0:
            ms = np.zeros(1, dtype=np.uint32)
        keep.append(ms)
        c.min_should = ms.ctypes.data
    c.ranking = RANK_TFIDF if bm25 is None else RANK_BM25
    if isinstance(bm25, dict):
        p = _bm25_params(bm25.get("k1", 1.2), bm25.get("b", 0.75), bm25.get("avgdl", 0.0))
        keep.append(p)
        c.bm25 = C.pointer(p)
    return c, keep


def clauses_check(must=None, should=None, must_not=None, min_should=None, bm25=None) -> int:
    """tfidf_clauses_check's return code for these clauses (host only)"""
    c, _keep = make_clauses(must, should, must_not, min_should, bm25)
    return lib().tfidf_clauses_check(C.byref(c))


def _top_terms(fn, handle, k: int, docs, what: str, words: bool = True) -> dict:
    """tfidf_top_terms / tfidf_group_top_terms: docs is None (every document in output order)
    or a sequence of global document ids."""
    ids = None if docs is None else np.ascontiguousarray(docs, dtype=np.uint32)
    n = 0 if ids is None else len(ids)
    if ids is not None and n == 0:
        ids = np.zeros(1, dtype=np.uint32)   # an empty list is a list: the pointer must not be NULL
    t = DocTerms()
    _chk(fn(handle, None if ids is None else ids.ctypes.data_as(C.c_void_p), n, k, C.byref(t)), what)
    try:
        R = int(t.ndocs)

        def arr(p, n, dt):
            return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)

        out = {
            "k": int(t.k), "doc": arr(t.doc, R, np.uint32), "pos": arr(t.pos, R, np.uint32),
            "npairs": arr(t.npairs, R, np.uint64), "nterms": arr(t.nterms, R, np.uint32),
            "term": arr(t.term, R * k, np.uint32).reshape(R, k), "count": arr(t.count, R * k, np.uint32).reshape(R, k),
            "score": arr(t.score, R * k, np.float64).reshape(R, k), "pair": arr(t.pair, R * k, np.uint64).reshape(R, k),
        }
        if words:
            woff = arr(t.word_off, R * k + 1, np.uint64).tolist()
            wb = bytes(arr(t.word_bytes, woff[-1], np.uint8))
            nt = out["nterms"].tolist()
            out["words"] = [[wb[woff[r * k + j]:woff[r * k + j + 1]] for j in range(nt[r])] for r in range(R)]
        return out
    finally:
        lib().tfidf_doc_terms_free(C.byref(t))


def _similar(fn, handle, k: int, docs, what: str) -> dict:
    """tfidf_similar / tfidf_group_similar: docs is None (every document in output order) or a
    sequence of global document ids."""
    ids = None if docs is None else np.ascontiguousarray(docs, dtype=np.uint32)
    n = 0 if ids is None else len(ids)
    if ids is not None and n == 0:
        ids = np.zeros(1, dtype=np.uint32)   # an empty list is a list: the pointer must not be NULL
    t = Neighbors()
    _chk(fn(handle, None if ids is None else ids.ctypes.data_as(C.c_void_p), n, k, C.byref(t)), what)
    try:
        R = int(t.ndocs)

        def arr(p, n, dt):
            return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)

        return {
            "k": int(t.k), "doc": arr(t.doc, R, np.uint32), "pos": arr(t.pos, R, np.uint32),
            "npairs": arr(t.npairs, R, np.uint64), "norm": arr(t.norm, R, np.float64),
            "nmatch": arr(t.nmatch, R, np.uint64), "nnb": arr(t.nnb, R, np.uint32),
            "nb_doc": arr(t.nb_doc, R * k, np.uint32).reshape(R, k),
            "nb_shared": arr(t.nb_shared, R * k, np.uint32).reshape(R, k),
            "nb_score": arr(t.nb_score, R * k, np.float64).reshape(R, k),
        }
    finally:
        lib().tfidf_neighbors_free(C.byref(t))


def _host_corpus(data, doc_off):
    """A host tfidf_corpus over numpy arrays; returns (Corpus, the arrays it points into)."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
    c = Corpus()
    c.bytes = data.ctypes.data if len(data) else None
    c.nbytes = len(data)
    c.doc_off = doc_off.ctypes.data
    c.doc_ids = None
    c.ndocs = len(doc_off) - 1
    c.flags = 0
    c.ndocs_total = 0
    return c, (data, doc_off)


def _transform(fn, handle, c: Corpus, batch_bytes, what: str) -> dict:
    """tfidf_transform / tfidf_group_transform of the batch c; batch_bytes: the batch's bytes on
    the host (the words are cut from them), or a callable that fetches them."""
    t = Rows()
    _chk(fn(handle, C.byref(c), C.byref(t)), what)
    try:
        N, P = int(t.ndocs), int(t.npairs)

        def arr(p, n, dt):
            return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)

        out = {
            "ndocs": N, "npairs": P, "ntokens": int(t.ntokens), "row_off": arr(t.row_off, N + 1, np.uint64),
            "doc_size": arr(t.doc_size, N, np.uint32), "doc_oov": arr(t.doc_oov, N, np.uint32),
            "term": arr(t.term, P, np.uint32), "count": arr(t.count, P, np.uint32), "df": arr(t.df, P, np.uint32),
            "score": arr(t.score, P, np.float64), "word_off": arr(t.word_off, P, np.uint64),
            "word_len": arr(t.word_len, P, np.uint32),
        }
    finally:
        lib().tfidf_rows_free(C.byref(t))
    bb = batch_bytes() if callable(batch_bytes) else batch_bytes
    bb = bb.tobytes() if isinstance(bb, np.ndarray) else bytes(bb)
    out["words"] = [bb[o:o + n] for o, n in zip(out["word_off"].tolist(), out["word_len"].tolist())]
    return out


def _model_dict(m: Model) -> dict:
    """A library-filled tfidf_model as a dict of copies: N, terms (list of bytes), df, term_off,
    term_bytes (numpy arrays)."""
    V = int(m.nterms)

    def arr(p, n, dt):
        return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)

    toff = arr(m.term_off, V + 1, np.uint64) if V else np.zeros(1, dtype=np.uint64)
    tb = arr(m.term_bytes, int(toff[-1]), np.uint8)
    raw = tb.tobytes()
    lo = toff.tolist()
    return {"N": int(m.ndocs_total), "terms": [raw[lo[i]:lo[i + 1]] for i in range(V)],
            "df": arr(m.term_df, V, np.uint32), "term_off": toff, "term_bytes": tb}


def _model_struct(model: dict, size=None):
    """A tfidf_model over the arrays of a model dict; with term_off / term_bytes present they are
    passed as they are (tests hand tfidf_model_check broken ones), else built from terms.
    Returns (struct, arrays to keep alive)."""
    df = np.ascontiguousarray(model["df"], dtype=np.uint32)
    if "term_off" in model:
        toff = np.ascontiguousarray(model["term_off"], dtype=np.uint64)
        tb = np.ascontiguousarray(model["term_bytes"], dtype=np.uint8)
    else:
        terms = list(model["terms"])
        toff = np.zeros(len(terms) + 1, dtype=np.uint64)
        if terms:
            toff[1:] = np.cumsum([len(t) for t in terms], dtype=np.uint64)
        tb = np.frombuffer(b"".join(terms), dtype=np.uint8)
    m = Model()
    m.size = C.sizeof(Model) if size is None else size
    m.ndocs_total = int(model["N"])
    m.nterms = len(toff) - 1
    m.term_off = toff.ctypes.data_as(C.POINTER(C.c_uint64))
    m.term_bytes = tb.ctypes.data_as(C.POINTER(C.c_uint8)) if len(tb) else None
    m.term_df = df.ctypes.data_as(C.POINTER(C.c_uint32)) if len(df) else None
    return m, (toff, tb, df)


def model_check(model: dict, size=None) -> int:
    """tfidf_model_check (host only): 0, or E_INVAL.  size overrides the struct's size field."""
    m, keep = _model_struct(model, size)
    return int(lib().tfidf_model_check(C.byref(m)))


def model_save(model: dict, path: str) -> None:
    """tfidf_model_save (host only): the model dict as a file."""
    m, keep = _model_struct(model)
    _chk(lib().tfidf_model_save(C.byref(m), os.fsencode(path)), "tfidf_model_save")


def model_load(path: str) -> dict:
    """tfidf_model_load (host only): the file as a model dict; TfidfError E_MODEL when it is none."""
    m = Model()
    _chk(lib().tfidf_model_load(os.fsencode(path), C.byref(m)), "tfidf_model_load")
    try:
        return _model_dict(m)
    finally:
        lib().tfidf_model_free(C.byref(m))


def analyzer(lower: bool = False, punct: bool = False, min_len: int = 0, stop=(), stem: bool = False, utf8: bool = False):
    """A tfidf_analyzer over a list of stop words (bytes objects, already folded; they are
    compared with the unstemmed tokens), with the Porter stemmer when `stem` and the UTF-8
    sequence map (TFIDF_AN_UTF8) when `utf8`; returns (struct, arrays to keep alive)."""
    stop = [bytes(w) for w in stop]
    sb = np.frombuffer(b"".join(stop), dtype=np.uint8)
    so = np.zeros(len(stop) + 1, dtype=np.uint64)
    if stop:
        so[1:] = np.cumsum([len(w) for w in stop], dtype=np.uint64)
    a = Analyzer()
    a.size = C.sizeof(Analyzer)
    a.flags = (AN_LOWER if lower else 0) | (AN_PUNCT if punct else 0) | (AN_UTF8 if utf8 else 0)
    a.min_len = min_len
    a.stop_bytes = sb.ctypes.data if len(sb) else None
    a.stop_off = so.ctypes.data if stop else None
    a.nstop = len(stop)
    a.stemmer = STEM_PORTER if stem else STEM_NONE
    return a, (sb, so)


def analyzer_check(a: Analyzer) -> int:
    """tfidf_analyzer_check (host only): 0, or E_INVAL."""
    return int(lib().tfidf_analyzer_check(C.byref(a)))


def stem_porter(word: bytes) -> bytes:
    """tfidf_stem_porter (host only): the Porter stem of one word; an ineligible word (shorter
    than 3 or longer than 64 bytes, a byte outside a..z) is returned as it is."""
    buf = np.frombuffer(bytes(word), dtype=np.uint8).copy()
    n = int(lib().tfidf_stem_porter(buf.ctypes.data if len(buf) else None, len(buf)))
    if n < 0:
        _chk(n, "tfidf_stem_porter")
    return bytes(buf[:n])


def analyze_host(data, off, lower: bool = False, punct: bool = False, min_len: int = 0, stop=(), in_place: bool = False,
                 stem: bool = False, utf8: bool = False):
    """tfidf_analyze_host (host only): the analyzed bytes of the documents data[off[i]:off[i + 1]]
    as a new array (in_place: computed in a copy that is both input and output)."""
    a, keep = analyzer(lower, punct, min_len, stop, stem, utf8)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    out = data.copy() if in_place else np.empty(len(data), dtype=np.uint8)
    src = out if in_place else data
    _chk(lib().tfidf_analyze_host(C.byref(a), src.ctypes.data if len(src) else None, len(data),
                                  off.ctypes.data if len(off) > 1 else None, max(len(off) - 1, 0),
                                  out.ctypes.data if len(out) else None), "tfidf_analyze_host")
    return out


def ngram_params(min_n: int = 1, max_n: int = 2, joiner: int = 0) -> NgramParams:
    """A tfidf_ngram_params; joiner 0 is the default '_'."""
    p = NgramParams()
    p.size = C.sizeof(NgramParams)
    p.min_n, p.max_n, p.joiner = min_n, max_n, joiner
    return p


def ngram_check(p: NgramParams) -> int:
    """tfidf_ngram_check (host only): 0, or E_INVAL."""
    return int(lib().tfidf_ngram_check(C.byref(p)))


def ngrams_host(data, off, min_n: int = 1, max_n: int = 2, joiner: int = 0):
    """tfidf_ngrams_host (host only): the word n-grams of the documents data[off[i]:off[i + 1]]
    as (bytes uint8, doc_off uint64), the shingled corpus."""
    p = ngram_params(min_n, max_n, joiner)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    ob, on, oo = C.c_void_p(), C.c_uint64(0), C.c_void_p()
    _chk(lib().tfidf_ngrams_host(C.byref(p), data.ctypes.data if len(data) else None, len(data),
                                 off.ctypes.data if len(off) > 1 else None, max(len(off) - 1, 0),
                                 C.byref(ob), C.byref(on), C.byref(oo)), "tfidf_ngrams_host")
    try:
        n = int(on.value)
        out = np.frombuffer(C.string_at(ob.value, n), dtype=np.uint8).copy() if n else np.zeros(0, dtype=np.uint8)
        out_off = np.frombuffer(C.string_at(oo.value, 8 * max(len(off), 1)), dtype=np.uint64).copy()
    finally:
        lib().tfidf_free(ob)
        lib().tfidf_free(oo)
    return out, out_off


def prune_params(min_df: int = 0, max_df: int = 0, max_features: int = 0) -> PruneParams:
    """A tfidf_prune_params: min_df 0 or 1 = no lower bound, max_df 0 = no upper bound,
    max_features 0 = no cut."""
    p = PruneParams()
    p.size = C.sizeof(PruneParams)
    p.min_df, p.max_df, p.max_features = min_df, max_df, max_features
    return p


def prune_check(p: PruneParams) -> int:
    """tfidf_prune_check (host only): 0, or E_INVAL; None stands for a NULL pointer."""
    return int(lib().tfidf_prune_check(None if p is None else C.byref(p)))


def model_prune(model: dict, min_df: int = 0, max_df: int = 0, max_features: int = 0) -> dict:
    """tfidf_model_prune (host only): the model dict without the pruned terms."""
    m, keep = _model_struct(model)
    p = prune_params(min_df, max_df, max_features)
    out = Model()
    _chk(lib().tfidf_model_prune(C.byref(m), C.byref(p), C.byref(out)), "tfidf_model_prune")
    try:
        return _model_dict(out)
    finally:
        lib().tfidf_model_free(C.byref(out))


def _mode(table: dict, v) -> int:
    return table[v] if isinstance(v, str) else int(v)


def weighting(tf="ratio", idf="ref", norm="none") -> Weighting:
    """A tfidf_weighting: names ("log", "smooth", "l2", ..) or the enum values."""
    w = Weighting()
    w.size = C.sizeof(Weighting)
    w.tf, w.idf, w.norm = _mode(TF_MODES, tf), _mode(IDF_MODES, idf), _mode(NORM_MODES, norm)
    return w


def _weighting_names(w: Weighting) -> dict:
    def name(table, v):
        return next((k for k, x in table.items() if x == v), v)
    return {"tf": name(TF_MODES, w.tf), "idf": name(IDF_MODES, w.idf), "norm": name(NORM_MODES, w.norm)}


def weighting_check(w: Weighting) -> int:
    """tfidf_weighting_check (host only): 0, or E_INVAL; None stands for a NULL pointer."""
    return int(lib().tfidf_weighting_check(None if w is None else C.byref(w)))


def result_reweight(res: dict, tf="ratio", idf="ref", norm="none", N: int = 0, params: Weighting = None) -> dict:
    """tfidf_result_reweight (host only, plain C) on a result dict (Engine.fetch's or the oracle's):
    the dict with score and output_txt replaced.  N: ndocs_total when the dict does not carry it."""
    w = params if params is not None else weighting(tf, idf, norm)
    P = int(res["npairs"])
    keep = [np.ascontiguousarray(res[k], dtype=np.uint32).copy() for k in ("doc", "count", "docsize", "df")]
    score = np.ascontiguousarray(res["score"], dtype=np.float64).copy()
    r = Result()
    r.npairs = P
    r.ndocs_total = int(N) if N else int(res["ndocs_total"])
    if P:
        u32 = C.POINTER(C.c_uint32)
        r.pair_doc, r.pair_count, r.pair_docsize, r.pair_df = (a.ctypes.data_as(u32) for a in keep)
        r.pair_score = score.ctypes.data_as(C.POINTER(C.c_double))
    _chk(lib().tfidf_result_reweight(C.byref(r), C.byref(w)), "tfidf_result_reweight")
    out = {k: v for k, v in res.items() if k not in ("tf_jobs", "idf_jobs")}
    out["score"] = score
    out["output_txt"] = format_lines(out)
    return out


def dedup_params(nhashes: int = 0, rows: int = 0, seed: int = 0, threshold: float = 0.8) -> DedupParams:
    """tfidf_dedup_params; nhashes = 0 selects the defaults H = 128, r = 4, seed = 1"""
    p = DedupParams()
    p.size = C.sizeof(DedupParams)
    p.nhashes, p.rows, p.seed, p.threshold = nhashes, rows, seed, threshold
    return p


def dedup_check(p: DedupParams) -> int:
    """tfidf_dedup_check (host only): 0, or E_INVAL; None stands for a NULL pointer."""
    return int(lib().tfidf_dedup_check(None if p is None else C.byref(p)))


def _u32s(p, n: int) -> np.ndarray:
    return np.ctypeslib.as_array(p, shape=(n,)).astype(np.uint32, copy=True) if n else np.zeros(0, dtype=np.uint32)


def _signatures_dict(s: Signatures) -> dict:
    N, H = int(s.ndocs), int(s.nhashes)
    return {"ndocs": N, "nhashes": H, "doc": _u32s(s.doc, N), "npairs": _u32s(s.npairs, N),
            "sig": _u32s(s.sig, N * H).reshape(N, H)}


def _dups_dict(d: Dups) -> dict:
    N, E = int(d.ndocs), int(d.nedges)
    out = {"ndocs": N, "ngroups": int(d.ngroups), "ncand": int(d.ncand), "nedges": E, "doc": _u32s(d.doc, N),
           "group": _u32s(d.group, N)}
    for k in ("a_pos", "b_pos", "a_doc", "b_doc", "shared", "uni", "same"):
        out[k] = _u32s(getattr(d, k), E)
    out["jaccard"] = (np.ctypeslib.as_array(d.jaccard, shape=(E,)).astype(np.float64, copy=True) if E
                      else np.zeros(0, dtype=np.float64))
    return out


def _dedup_result(res: dict, doc_ids):
    """a tfidf_result for the host dedup calls from a result dict whose terms may be numbered in
    any order (the oracle numbers them by first appearance): the term table in strcmp("word\t")
    order, pair_term renumbered.  doc_ids: every document of the shard (res["doc_id"] when absent).
    Returns (Result, the arrays that must outlive it)."""
    words = res["terms"]
    by_rank = sorted(range(len(words)), key=lambda i: words[i] + b"\t")
    rank = np.zeros(len(words) + 1, dtype=np.uint32)
    rank[np.array(by_rank, dtype=np.int64)] = np.arange(len(words), dtype=np.uint32)
    P = int(res["npairs"])
    doc = np.ascontiguousarray(res["doc"], dtype=np.uint32).copy()
    term = np.ascontiguousarray(rank[np.asarray(res["term"], dtype=np.int64)], dtype=np.uint32)
    ids = np.ascontiguousarray(res["doc_id"] if doc_ids is None else doc_ids, dtype=np.uint32).copy()
    toff = np.zeros(len(words) + 1, dtype=np.uint64)
    toff[1:] = np.cumsum([len(words[i]) for i in by_rank], dtype=np.uint64)
    tb = np.frombuffer(b"".join(words[i] for i in by_rank) + b"\0", dtype=np.uint8).copy()
    r = Result()
    r.npairs, r.ndocs, r.nterms = P, len(ids), len(words)
    u32 = C.POINTER(C.c_uint32)
    if P:
        r.pair_doc, r.pair_term = doc.ctypes.data_as(u32), term.ctypes.data_as(u32)
    if len(ids):
        r.doc_id = ids.ctypes.data_as(u32)
    r.term_off = toff.ctypes.data_as(C.POINTER(C.c_uint64))
    r.term_bytes = tb.ctypes.data_as(C.POINTER(C.c_uint8))
    return r, (doc, term, ids, toff, tb)


def result_minhash(res: dict, doc_ids=None, nhashes: int = 0, seed: int = 0, params: DedupParams = None) -> dict:
    """tfidf_result_minhash (host only, plain C) on a result dict."""
    p = params if params is not None else dedup_params(nhashes, 1 if nhashes else 0, seed, 0.0)
    r, keep = _dedup_result(res, doc_ids)
    s = Signatures()
    _chk(lib().tfidf_result_minhash(C.byref(r), C.byref(p), C.byref(s)), "tfidf_result_minhash")
    try:
        return _signatures_dict(s)
    finally:
        lib().tfidf_signatures_free(C.byref(s))


def result_near_dups(res: dict, doc_ids=None, nhashes: int = 0, rows: int = 0, seed: int = 0, threshold: float = 0.8,
                     params: DedupParams = None) -> dict:
    """tfidf_result_near_dups (host only, plain C) on a result dict."""
    p = params if params is not None else dedup_params(nhashes, rows, seed, threshold)
    r, keep = _dedup_result(res, doc_ids)
    d = Dups()
    _chk(lib().tfidf_result_near_dups(C.byref(r), C.byref(p), C.byref(d)), "tfidf_result_near_dups")
    try:
        return _dups_dict(d)
    finally:
        lib().tfidf_dups_free(C.byref(d))


def nb_params(docs, labels, nclasses: int, variant="multinomial", feature="count", alpha: float = 0.0,
              uniform_prior: bool = False, size=None):
    """tfidf_nb_params over the labelled (global doc id, class) entries; alpha = 0 selects 1.0.
    Returns (NbParams, the arrays it points into)."""
    d = np.ascontiguousarray(docs, dtype=np.uint32)
    lb = np.ascontiguousarray(labels, dtype=np.uint32)
    assert len(d) == len(lb)
    p = NbParams()
    p.size = C.sizeof(NbParams) if size is None else size
    p.nclasses, p.variant, p.feature = nclasses, _mode(NB_VARIANTS, variant), _mode(NB_FEATURES, feature)
    p.uniform_prior, p.alpha, p.nlabelled = int(bool(uniform_prior)), alpha, len(d)
    if len(d):
        p.doc, p.label = d.ctypes.data_as(C.POINTER(C.c_uint32)), lb.ctypes.data_as(C.POINTER(C.c_uint32))
    return p, (d, lb)


def nb_check(p) -> int:
    """tfidf_nb_check (host only): 0, or E_INVAL; None stands for a NULL pointer; a (NbParams, keep)
    pair as nb_params returns it is accepted."""
    if isinstance(p, tuple):
        p = p[0]
    return int(lib().tfidf_nb_check(None if p is None else C.byref(p)))


def _nb_model_dict(m: NbModel) -> dict:
    """A library-filled tfidf_nb_model as a dict of copies; the matrices as [V, K] arrays."""
    K, V = int(m.nclasses), int(m.nterms)

    def arr(p, n, dt):
        return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)

    return {"nclasses": K, "nterms": V, "variant": int(m.variant), "feature": int(m.feature),
            "uniform_prior": int(m.uniform_prior), "alpha": float(m.alpha), "nlabelled": int(m.nlabelled),
            "class_docs": arr(m.class_docs, K, np.uint64), "class_total": arr(m.class_total, K, np.uint64),
            "feature_count": arr(m.feature_count, V * K, np.uint64).reshape(V, K), "prior": arr(m.prior, K, np.float64),
            "weight": arr(m.weight, V * K, np.float64).reshape(V, K)}


def _nb_model_struct(model: dict):
    """tfidf_nb_model over a dict as _nb_model_dict returns it.  Returns (NbModel, keep)."""
    K, V = int(model["nclasses"]), int(model["nterms"])
    keep = [np.ascontiguousarray(model[k], dtype=dt).reshape(-1).copy()
            for k, dt in (("class_docs", np.uint64), ("class_total", np.uint64), ("feature_count", np.uint64),
                          ("prior", np.float64), ("weight", np.float64))]
    keep = [a if len(a) else np.zeros(1, dtype=a.dtype) for a in keep]
    m = NbModel()
    m.size = C.sizeof(NbModel)
    m.nclasses, m.nterms, m.variant, m.feature = K, V, int(model["variant"]), int(model["feature"])
    m.uniform_prior, m.alpha, m.nlabelled = int(model["uniform_prior"]), float(model["alpha"]), int(model["nlabelled"])
    u64, f64 = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    m.class_docs, m.class_total, m.feature_count = (a.ctypes.data_as(u64) for a in keep[:3])
    m.prior, m.weight = (a.ctypes.data_as(f64) for a in keep[3:])
    return m, keep


def _nb_labels_dict(t: NbLabels) -> dict:
    R, K = int(t.ndocs), int(t.nclasses)
    out = {"ndocs": R, "nclasses": K, "doc": _u32s(t.doc, R), "pos": _u32s(t.pos, R), "label": _u32s(t.label, R),
           "score": np.ctypeslib.as_array(t.score, shape=(R,)).astype(np.float64, copy=True) if R else np.zeros(0)}
    if t.scores:
        out["scores"] = (np.ctypeslib.as_array(t.scores, shape=(R * K,)).astype(np.float64, copy=True).reshape(R, K)
                         if R * K else np.zeros((R, K)))
    return out


def _nb_result(res: dict, doc_ids):
    """_dedup_result with the pairs' counts: what tfidf_result_nb_fit reads"""
    r, keep = _dedup_result(res, doc_ids)
    cnt = np.ascontiguousarray(res["count"], dtype=np.uint32).copy()
    if len(cnt):
        r.pair_count = cnt.ctypes.data_as(C.POINTER(C.c_uint32))
    return r, keep + (cnt,)


def result_nb_fit(res: dict, docs, labels, nclasses: int, doc_ids=None, params=None, **kw) -> dict:
    """tfidf_result_nb_fit (host only, plain C) on a result dict; term ranks are the strcmp("word\t")
    order of the result's words.  kw: nb_params' options."""
    p, keep_p = params if params is not None else nb_params(docs, labels, nclasses, **kw)
    r, keep = _nb_result(res, doc_ids)
    m = NbModel()
    _chk(lib().tfidf_result_nb_fit(C.byref(r), C.byref(p), C.byref(m)), "tfidf_result_nb_fit")
    try:
        return _nb_model_dict(m)
    finally:
        lib().tfidf_nb_model_free(C.byref(m))


def nb_model_predict(model: dict, row_off, term, count, all_scores: bool = True) -> dict:
    """tfidf_nb_model_predict (host only, plain C): rows of (term rank, count) pairs against a
    model dict."""
    m, keep = _nb_model_struct(model)
    ro = np.ascontiguousarray(row_off, dtype=np.uint64)
    tm = np.ascontiguousarray(term, dtype=np.uint32)
    ct = np.ascontiguousarray(count, dtype=np.uint32)
    t = NbLabels()
    _chk(lib().tfidf_nb_model_predict(C.byref(m), len(ro) - 1, _ptr(ro), _ptr(tm) if len(tm) else None,
                                      _ptr(ct) if len(ct) else None, NB_ALL_SCORES if all_scores else 0, C.byref(t)),
         "tfidf_nb_model_predict")
    try:
        return _nb_labels_dict(t)
    finally:
        lib().tfidf_nb_labels_free(C.byref(t))


def make_patterns(patterns, kinds=None, max_edits=None):
    """A tfidf_patterns over bytes objects and the arrays it points into (keep both alive for the
    call).  kinds / max_edits: one value for every pattern or one per pattern; the defaults are
    MATCH_FUZZY and 2."""
    n = len(patterns)

    def per(v, default):
        if v is None:
            v = default
        a = np.full(n, v, dtype=np.uint8) if np.isscalar(v) else np.ascontiguousarray(v, dtype=np.uint8)
        return a if len(a) else np.zeros(1, dtype=np.uint8)

    data = np.frombuffer(b"".join(patterns), dtype=np.uint8)
    if len(data) == 0:
        data = np.zeros(1, dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    if n:
        off[1:] = np.cumsum([len(p) for p in patterns], dtype=np.uint64)
    kind, edits = per(kinds, MATCH_FUZZY), per(max_edits, MATCH_MAX_EDITS)
    ps = Patterns()
    ps.bytes = data.ctypes.data
    ps.nbytes = int(off[-1])
    ps.p_off = off.ctypes.data
    ps.npatterns = n
    ps.kind = kind.ctypes.data
    ps.max_edits = edits.ctypes.data
    return ps, (data, off, kind, edits)


def match_params(max_expansions: int = 50, transpose: bool = True, fixed_prefix: int = 0, list_records: int = 0,
                 flags=None, size=None) -> MatchParams:
    """A tfidf_match_params; flags and size override what transpose and sizeof give."""
    p = MatchParams()
    p.size = C.sizeof(MatchParams) if size is None else size
    p.max_expansions = max_expansions
    p.flags = (MATCH_TRANSPOSE if transpose else 0) if flags is None else flags
    p.fixed_prefix = fixed_prefix
    p.list_records = list_records
    return p


def match_check(patterns, kinds=None, max_edits=None, params: MatchParams = None, **kw) -> int:
    """tfidf_match_check's return code (host only).  patterns: bytes objects, or a Patterns struct."""
    ps, _keep = (patterns, None) if isinstance(patterns, Patterns) else make_patterns(patterns, kinds, max_edits)
    p = params if params is not None else match_params(**kw)
    return int(lib().tfidf_match_check(C.byref(ps), C.byref(p)))


def _match_terms(fn, handle, patterns, kinds, max_edits, params, what: str, **kw) -> dict:
    """tfidf_match_terms / tfidf_group_match_terms / tfidf_model_match_terms: per pattern nmatch,
    nterms and the rows term, dist, df [npatterns][k], and words: a list of bytes per pattern."""
    ps, _keep = (patterns, None) if isinstance(patterns, Patterns) else make_patterns(patterns, kinds, max_edits)
    p = params if params is not None else match_params(**kw)
    t = TermMatches()
    _chk(fn(handle, C.byref(ps), C.byref(p), C.byref(t)), what)
    try:
        P, k = int(t.npatterns), int(t.k)

        def arr(q, n, dt):
            return np.ctypeslib.as_array(q, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)

        woff = arr(t.word_off, P * k + 1, np.uint64).tolist()
        wb = bytes(arr(t.word_bytes, woff[-1], np.uint8))
        nt = arr(t.nterms, P, np.uint32)
        return {
            "k": k, "nmatch": arr(t.nmatch, P, np.uint64), "nterms": nt,
            "term": arr(t.term, P * k, np.uint32).reshape(P, k), "dist": arr(t.dist, P * k, np.uint8).reshape(P, k),
            "df": arr(t.df, P * k, np.uint32).reshape(P, k),
            "words": [[wb[woff[r * k + j]:woff[r * k + j + 1]] for j in range(int(nt[r]))] for r in range(P)],
        }
    finally:
        lib().tfidf_term_matches_free(C.byref(t))


def model_match_terms(model: dict, patterns, kinds=None, max_edits=None, params: MatchParams = None, **kw) -> dict:
    """tfidf_model_match_terms (host only, plain C): the patterns against a model dict's term table;
    term is the index into it.  Keywords as match_params."""
    m, _keep = _model_struct(model)
    return _match_terms(lib().tfidf_model_match_terms, C.byref(m), patterns, kinds, max_edits, params,
                        "tfidf_model_match_terms", **kw)


def snippet_params(window: int = 32, max_marks: int = 32, text: bool = True, scratch_bytes: int = 0, flags=None,
                   size=None) -> SnippetParams:
    """A tfidf_snippet_params; flags and size override what text and sizeof give."""
    p = SnippetParams()
    p.size = C.sizeof(SnippetParams) if size is None else size
    p.window, p.max_marks = window, max_marks
    p.flags = (SNIP_TEXT if text else 0) if flags is None else flags
    p.scratch_bytes = scratch_bytes
    return p


def snippet_check(params: SnippetParams = None, **kw) -> int:
    """tfidf_snippets_check's return code (host only).  Keywords as snippet_params."""
    p = params if params is not None else snippet_params(**kw)
    return int(lib().tfidf_snippets_check(C.byref(p)))


def hits_to_jobs(hits: dict):
    """The (query, document) pairs of a query() result, row by row."""
    return [(q, int(hits["doc"][q, j])) for q in range(len(hits["nhits"])) for j in range(int(hits["nhits"][q]))]


def _snippets(fn, handles, queries, jobs, hits, params, what: str, **kw) -> dict:
    """tfidf_snippet / tfidf_group_snippet / tfidf_result_snippet.  jobs: (query index, global document
    id) pairs, or hits: a dict from query().  Returns the per-job arrays, marks: per job a list of
    (byte offset in the document, length, slot), text: per job the window's bytes (None without
    text), and qterms: per query a list of (offset in the query, length, found)."""
    if jobs is None:
        jobs = hits_to_jobs(hits) if hits is not None else []
    qs, _keep = _queries(queries)
    jq = np.ascontiguousarray([j[0] for j in jobs], dtype=np.uint32)
    jd = np.ascontiguousarray([j[1] for j in jobs], dtype=np.uint32)
    p = params if params is not None else snippet_params(**kw)
    t = Snippets()
    _chk(fn(*handles, C.byref(qs), _ptr(jq) if len(jobs) else None, _ptr(jd) if len(jobs) else None, len(jobs),
            C.byref(p), C.byref(t)), what)
    try:
        J, Q = int(t.njobs), int(t.nqueries)

        def arr(q, n, dt):
            return np.ctypeslib.as_array(q, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)

        moff = arr(t.mark_off, J + 1, np.uint64).tolist()
        toff = arr(t.text_off, J + 1, np.uint64).tolist()
        qoff = arr(t.qterm_off, Q + 1, np.uint64).tolist()
        mb, ml, ms = (arr(a, moff[-1], dt).tolist() for a, dt in
                      ((t.mark_byte, np.uint64), (t.mark_len, np.uint32), (t.mark_slot, np.uint32)))
        tb = bytes(arr(t.text, toff[-1], np.uint8))
        qp, ql, qf = (arr(a, qoff[-1], dt).tolist() for a, dt in
                      ((t.qterm_pos, np.uint64), (t.qterm_len, np.uint32), (t.qterm_found, np.uint8)))
        want_text = bool(p.flags & SNIP_TEXT)
        return {
            "flags": arr(t.flags, J, np.uint32), "ntokens": arr(t.ntokens, J, np.uint32),
            "nmatch": arr(t.nmatch, J, np.uint32), "nterms_matched": arr(t.nterms_matched, J, np.uint32),
            "win_tok": arr(t.win_tok, 2 * J, np.uint32).reshape(J, 2),
            "win_byte": arr(t.win_byte, 2 * J, np.uint64).reshape(J, 2),
            "cover": arr(t.cover, J, np.uint32), "hits": arr(t.hits, J, np.uint32),
            "marks": [list(zip(mb[moff[j]:moff[j + 1]], ml[moff[j]:moff[j + 1]], ms[moff[j]:moff[j + 1]]))
                      for j in range(J)],
            "text": [tb[toff[j]:toff[j + 1]] if want_text else None for j in range(J)],
            "qterms": [list(zip(qp[qoff[q]:qoff[q + 1]], ql[qoff[q]:qoff[q + 1]], qf[qoff[q]:qoff[q + 1]]))
                       for q in range(Q)],
        }
    finally:
        lib().tfidf_snippets_free(C.byref(t))


def result_snippets(res: dict, data, off, queries, jobs=None, hits=None, doc_ids=None, params: SnippetParams = None,
                    **kw) -> dict:
    """tfidf_result_snippet (host only, plain C): the definition over a fetched result's term table
    (res["terms"]) and the host corpus the run had.  Keywords as snippet_params."""
    terms = res["terms"]
    toff = np.zeros(len(terms) + 1, dtype=np.uint64)
    if terms:
        toff[1:] = np.cumsum([len(t) for t in terms], dtype=np.uint64)
    tb = np.frombuffer(b"".join(terms) + b"\0", dtype=np.uint8)
    r = Result()
    r.nterms = len(terms)
    r.term_off = toff.ctypes.data_as(C.POINTER(C.c_uint64))
    r.term_bytes = tb.ctypes.data_as(C.POINTER(C.c_uint8))
    c, _keep = _host_corpus(data, off)
    ids = None if doc_ids is None else np.ascontiguousarray(doc_ids, dtype=np.uint32)
    c.doc_ids = None if ids is None else ids.ctypes.data
    return _snippets(lib().tfidf_result_snippet, (C.byref(r), C.byref(c)), queries, jobs, hits, params,
                     "tfidf_result_snippet", **kw)


def synth_host(seed: int, V: int, mode: int, cdf, doc_ids, ntok):
    """Host generation (csrc/synth.h).  Returns (bytes uint8, doc_off uint64)."""
    ntok = np.ascontiguousarray(ntok, dtype=np.uint64)
    ids = None if doc_ids is None else np.ascontiguousarray(doc_ids, dtype=np.uint32)
    cdf = None if cdf is None else np.ascontiguousarray(cdf, dtype=np.float64)
    n = C.c_uint64(0)
    _chk(lib().tfidf_synth_host(seed, V, mode, _ptr(cdf), _ptr(ids), _ptr(ntok), len(ntok), None, C.byref(n), None),
         "synth size")
    buf = np.empty(max(int(n.value), 1), dtype=np.uint8)
    off = np.empty(len(ntok) + 1, dtype=np.uint64)
    _chk(lib().tfidf_synth_host(seed, V, mode, _ptr(cdf), _ptr(ids), _ptr(ntok), len(ntok), _ptr(buf), C.byref(n),
                                _ptr(off)), "synth")
    return buf[: int(n.value)], off


class Engine:
    """One GPU context (one HIP stream; optional RCCL communicator)."""

    def __init__(self, device: int = 0, handle=None):
        self._owned = handle is None
        if handle is None:
            h = C.c_void_p()
            _chk(lib().tfidf_open(device, C.byref(h)), "tfidf_open")
            handle = h
        self.h = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle)
        self._keep = None

    def close(self):
        if self.h and self._owned:
            lib().tfidf_close(self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_timing(self, on):
        """True / 1: every stage; 2: K1 and the whole run only; False / 0: none"""
        lvl = 2 if (on == 2 and on is not True) else (1 if on else 0)
        _chk(lib().tfidf_set_timing(self.h, lvl), "set_timing")

    def comm_init(self, uid: bytes, rank: int, nranks: int):
        buf = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(uid)
        _chk(lib().tfidf_comm_init(self.h, buf, rank, nranks), "tfidf_comm_init")

    def run_host(self, data: np.ndarray, doc_off: np.ndarray, doc_ids=None, ndocs_total: int = 0):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        ids = None if doc_ids is None else np.ascontiguousarray(doc_ids, dtype=np.uint32)
        c = Corpus()
        c.bytes = data.ctypes.data if len(data) else None
        c.nbytes = len(data)
        c.doc_off = doc_off.ctypes.data
        c.doc_ids = None if ids is None else ids.ctypes.data
        c.ndocs = len(doc_off) - 1
        c.flags = 0
        c.ndocs_total = ndocs_total
        self._keep = (data, doc_off, ids)
        _chk(lib().tfidf_run(self.h, C.byref(c)), "tfidf_run")

    def run_corpus(self, c: Corpus):
        _chk(lib().tfidf_run(self.h, C.byref(c)), "tfidf_run")

    def synth_device(self, seed, V, mode, cdf, doc_ids, ntok, ndocs_total=0) -> Corpus:
        ntok = np.ascontiguousarray(ntok, dtype=np.uint64)
        ids = None if doc_ids is None else np.ascontiguousarray(doc_ids, dtype=np.uint32)
        cdf = None if cdf is None else np.ascontiguousarray(cdf, dtype=np.float64)
        c = Corpus()
        _chk(lib().tfidf_synth_device(self.h, seed, V, mode, _ptr(cdf), _ptr(ids), _ptr(ntok), len(ntok),
                                      ndocs_total, C.byref(c)), "tfidf_synth_device")
        return c

    def ingest_dir(self, path: str, threads: int = 0):
        """input/doc1..N streamed into HBM (tfidf_ingest_dir_device).  Returns (Corpus, info);
        raises TfidfError (rc -6 / -7, `bad_doc` attribute set for -7) like the reference."""
        c, bad, ii = Corpus(), C.c_uint32(0), IngestInfo()
        rc = lib().tfidf_ingest_dir_device(self.h, path.encode(), threads, C.byref(c), C.byref(bad), C.byref(ii))
        if rc:
            e = TfidfError(rc, "tfidf_ingest_dir_device")
            e.bad_doc, e.ndocs = bad.value, c.ndocs
            raise e
        return c, {k: getattr(ii, k) for k, _ in IngestInfo._fields_}

    def hbm_probe(self, nbytes: int = 2 << 30, iters: int = 10) -> dict:
        """Measured streaming read / copy GB/s of this device (tfidf_hbm_probe)."""
        r, c = C.c_double(0), C.c_double(0)
        _chk(lib().tfidf_hbm_probe(self.h, nbytes, iters, C.byref(r), C.byref(c)), "tfidf_hbm_probe")
        return {"read_GBps": r.value, "copy_GBps": c.value}

    def corpus_bytes(self, c: Corpus) -> np.ndarray:
        """Device corpus bytes copied back to the host (test plumbing)."""
        out = np.empty(c.nbytes, dtype=np.uint8)
        hip = C.CDLL("libamdhip64.so.7")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        if c.nbytes and hip.hipMemcpy(out.ctypes.data, c.bytes, c.nbytes, 2) != 0:
            raise RuntimeError("hipMemcpy D2H failed")
        off = np.empty(c.ndocs + 1, dtype=np.uint64)
        if hip.hipMemcpy(off.ctypes.data, c.doc_off, off.nbytes, 2) != 0:
            raise RuntimeError("hipMemcpy D2H failed")
        return out, off

    def alloc_counters(self):
        """(device allocations, bytes) the library has made in this process so far."""
        a, b = C.c_uint64(), C.c_uint64()
        _chk(lib().tfidf_alloc_stats(C.byref(a), C.byref(b)), "tfidf_alloc_stats")
        return int(a.value), int(b.value)

    def grid_cus(self) -> int:
        """the CU count this context sizes its launches over the result by: the device's, or env
        TFIDF_GRID_CUS as tfidf_open read it."""
        n = C.c_uint32()
        _chk(lib().tfidf_grid_cus(self.h, C.byref(n)), "tfidf_grid_cus")
        return int(n.value)

    def totals(self, reset: bool = False) -> dict:
        """sums over the successful runs since the last reset (tfidf_run_totals_get)"""
        t = RunTotals()
        _chk(lib().tfidf_run_totals_get(self.h, C.byref(t), 1 if reset else 0), "tfidf_run_totals_get")
        return {k: getattr(t, k) for k, _ in RunTotals._fields_}

    def info(self) -> dict:
        """Counters of the last run (tfidf_last_run_info); k1_workgroups is the grid of its last
        tokenize+count launch."""
        r = RunInfo()
        r.size = C.sizeof(RunInfo)
        _chk(lib().tfidf_last_run_info(self.h, C.byref(r)), "tfidf_last_run_info")
        d = {k: getattr(r, k) for k, _ in RunInfo._fields_ if k not in ("ms_stage", "size", "reserved2")}
        d["stages"] = {lib().tfidf_stage_name(i).decode(): r.ms_stage[i] for i in range(r.nstages)}
        return d

    def format_bytes(self) -> int:
        """Formats the last run's lines on the GPU; returns the text size."""
        n = C.c_uint64(0)
        _chk(lib().tfidf_format(self.h, C.byref(n)), "tfidf_format")
        return int(n.value)

    def text(self) -> bytes:
        """output.txt bytes formatted on the GPU (tfidf_format + tfidf_copy_text)."""
        n = C.c_uint64(0)
        _chk(lib().tfidf_format(self.h, C.byref(n)), "tfidf_format")
        buf = np.empty(int(n.value), dtype=np.uint8)
        if n.value:
            _chk(lib().tfidf_copy_text(self.h, 0, buf.ctypes.data, n.value), "tfidf_copy_text")
        return buf.tobytes()

    def write_output(self, path: str, append: bool = False):
        _chk(lib().tfidf_write_output_gpu(self.h, path.encode(), 1 if append else 0), "tfidf_write_output_gpu")

    def output_info(self) -> dict:
        """Timings of the last write_output (tfidf_last_output_info)."""
        o = OutputInfo()
        o.size = C.sizeof(OutputInfo)
        _chk(lib().tfidf_last_output_info(self.h, C.byref(o)), "tfidf_last_output_info")
        return {k: getattr(o, k) for k, _ in OutputInfo._fields_ if k != "size"}

    def format_f64(self, vals) -> list:
        """The device %.16f formatter on host doubles (tests)."""
        v = np.ascontiguousarray(vals, dtype=np.float64)
        out = np.zeros(v.size * 32, dtype=np.uint8)
        _chk(lib().tfidf_format_f64(self.h, v.ctypes.data, v.size, out.ctypes.data), "tfidf_format_f64")
        return [bytes(out[i * 32:(i + 1) * 32]).rstrip(b"\0") for i in range(v.size)]

    def query(self, queries, k: int = 10) -> dict:
        """Top-k documents of this shard for every query (tfidf_query).  queries: bytes
        objects, tokenised like documents.  Returns numpy arrays nhits[nq], nmatch[nq],
        nterms_found[nq], doc[nq, k] (global ids) and score[nq, k]; rows are valid up to
        nhits."""
        return _query(lib().tfidf_query, self.h, queries, k, "tfidf_query")

    def query_info(self) -> dict:
        """Counters and device times of the last query (tfidf_last_query_info)."""
        q = QueryInfo()
        q.size = C.sizeof(QueryInfo)
        _chk(lib().tfidf_last_query_info(self.h, C.byref(q)), "tfidf_last_query_info")
        return {k: getattr(q, k) for k, _ in QueryInfo._fields_ if k != "size"}

    def query_bm25(self, queries, k: int = 10, k1: float = 1.2, b: float = 0.75, avgdl: float = 0.0) -> dict:
        """Engine.query ranked by Okapi BM25 (tfidf_query_bm25); avgdl 0: this shard's own
        average document length.  The same dict, plus the avgdl used."""
        res = _query(lib().tfidf_query_bm25, self.h, queries, k, "tfidf_query_bm25", _bm25_params(k1, b, avgdl))
        res["avgdl"] = self.bm25_info()["avgdl"]
        return res

    def query_clauses(self, must=None, should=None, must_not=None, k: int = 10, min_should=None, bm25=None) -> dict:
        """Engine.query with must / should / must-not clauses (tfidf_query_clauses): three lists
        of bytes objects of one length (None: empty in every query), min_should one integer per
        query; bm25: None, True or dict(k1=, b=, avgdl=) (make_clauses).  Returns what
        Engine.query returns."""
        c, _keep = make_clauses(must, should, must_not, min_should, bm25)
        return _query(lib().tfidf_query_clauses, self.h, c, k, "tfidf_query_clauses")

    def clause_info(self) -> dict:
        """Counters and device times of the last query_clauses (tfidf_last_clause_info)."""
        q = ClauseInfo()
        q.size = C.sizeof(ClauseInfo)
        _chk(lib().tfidf_last_clause_info(self.h, C.byref(q)), "tfidf_last_clause_info")
        return {k: getattr(q, k) for k, _ in ClauseInfo._fields_ if k != "size"}

    def bm25_info(self) -> dict:
        """Counters and device times of the last query_bm25 (tfidf_last_bm25_info)."""
        q = Bm25Info()
        q.size = C.sizeof(Bm25Info)
        _chk(lib().tfidf_last_bm25_info(self.h, C.byref(q)), "tfidf_last_bm25_info")
        return {k: getattr(q, k) for k, _ in Bm25Info._fields_ if k != "size"}

    def top_terms(self, k: int = 10, docs=None, words: bool = True) -> dict:
        """The k best-scoring words of each document of this shard (tfidf_top_terms).  docs:
        None for every document in output order, or global document ids (rows in that order;
        an id the shard does not hold has pos == NO_POS).  Returns numpy arrays doc[rows],
        pos[rows], npairs[rows], nterms[rows], term / count / score / pair [rows, k] (rows are
        valid up to nterms) and words: per row the list of the words' bytes (words=False
        leaves it out)."""
        return _top_terms(lib().tfidf_top_terms, self.h, k, docs, "tfidf_top_terms", words)

    def match_terms(self, patterns, kinds=None, max_edits=None, params: MatchParams = None, **kw) -> dict:
        """Fuzzy and prefix patterns against this context's term table (tfidf_match_terms).
        patterns: bytes objects; kinds / max_edits: one value or one per pattern (MATCH_FUZZY, 2);
        keywords as match_params (max_expansions, transpose, fixed_prefix, list_records)."""
        return _match_terms(lib().tfidf_match_terms, self.h, patterns, kinds, max_edits, params, "tfidf_match_terms", **kw)

    def match_info(self) -> dict:
        """Counters and device times of the last match_terms (tfidf_last_match_info)."""
        t = MatchInfo()
        t.size = C.sizeof(MatchInfo)
        _chk(lib().tfidf_last_match_info(self.h, C.byref(t)), "tfidf_last_match_info")
        return {k: getattr(t, k) for k, _ in MatchInfo._fields_ if k != "size"}

    def snippets(self, queries, jobs=None, hits=None, params: SnippetParams = None, **kw) -> dict:
        """Best passage and match marks of (query, document) jobs over the resident corpus
        (tfidf_snippet).  jobs: (query index, global document id) pairs, or hits: a dict from
        query(); keywords as snippet_params (window, max_marks, text, scratch_bytes)."""
        return _snippets(lib().tfidf_snippet, (self.h,), queries, jobs, hits, params, "tfidf_snippet", **kw)

    def snippet_info(self) -> dict:
        """Counters and device times of the last snippets (tfidf_last_snippet_info)."""
        t = SnippetInfo()
        t.size = C.sizeof(SnippetInfo)
        _chk(lib().tfidf_last_snippet_info(self.h, C.byref(t)), "tfidf_last_snippet_info")
        return {n: getattr(t, n) for n, _ in SnippetInfo._fields_ if n != "size"}

    def terms_info(self) -> dict:
        """Counters and device times of the last top_terms (tfidf_last_terms_info)."""
        t = TermsInfo()
        t.size = C.sizeof(TermsInfo)
        _chk(lib().tfidf_last_terms_info(self.h, C.byref(t)), "tfidf_last_terms_info")
        return {k: getattr(t, k) for k, _ in TermsInfo._fields_ if k != "size"}

    def similar(self, k: int = 10, docs=None) -> dict:
        """The k nearest neighbours of each document of this shard under the cosine similarity
        of the TF-IDF vectors (tfidf_similar).  docs: None for every document in output order
        (ceil(N / group) scans of the pairs), or global document ids (rows in that order; an id
        the shard does not hold has pos == NO_POS).  Returns numpy arrays doc[rows], pos[rows],
        npairs[rows], norm[rows], nmatch[rows], nnb[rows] and nb_doc / nb_shared / nb_score
        [rows, k] (rows are valid up to nnb)."""
        return _similar(lib().tfidf_similar, self.h, k, docs, "tfidf_similar")

    def similar_info(self) -> dict:
        """Counters and device times of the last similar (tfidf_last_similar_info)."""
        t = SimilarInfo()
        t.size = C.sizeof(SimilarInfo)
        _chk(lib().tfidf_last_similar_info(self.h, C.byref(t)), "tfidf_last_similar_info")
        return {k: getattr(t, k) for k, _ in SimilarInfo._fields_ if k not in ("size", "reserved")}

    def kmeans(self, k: int, max_iter: int = 0, nterms: int = 10, seeds=None) -> dict:
        """Spherical k-means over this shard's documents (tfidf_kmeans).  seeds: None for the
        default seeds or k global document ids; max_iter 0 is the default (20).  Returns
        iterations, converged and numpy arrays doc[n], label[n] (NO_CLUSTER: norm 0), sim[n] in
        output order, size[k], seed[k], nterms[k], term[k, nterms], weight[k, nterms] and
        words (per cluster the list of its best terms' bytes)."""
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint32)
        p = KmeansParams()
        p.size = C.sizeof(KmeansParams)
        p.k, p.max_iter, p.nterms = k, max_iter, nterms
        p.nseeds = 0 if sd is None else len(sd)
        if sd is not None and len(sd):
            p.seeds = sd.ctypes.data_as(C.POINTER(C.c_uint32))
        elif sd is not None:
            p.seeds = np.zeros(1, dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))   # an empty list is a list
        t = Clusters()
        _chk(lib().tfidf_kmeans(self.h, C.byref(p), C.byref(t)), "tfidf_kmeans")
        try:
            n, K, T = int(t.ndocs), int(t.k), int(t.t)

            def arr(ptr, m, dt):
                return np.ctypeslib.as_array(ptr, shape=(m,)).astype(dt, copy=True) if m else np.zeros(0, dtype=dt)

            out = {
                "k": K, "iterations": int(t.iterations), "converged": int(t.converged),
                "doc": arr(t.doc, n, np.uint32), "label": arr(t.label, n, np.uint32), "sim": arr(t.sim, n, np.float64),
                "size": arr(t.size, K, np.uint32), "seed": arr(t.seed, K, np.uint32), "nterms": arr(t.nterms, K, np.uint32),
                "term": arr(t.term, K * T, np.uint32).reshape(K, T), "weight": arr(t.weight, K * T, np.float64).reshape(K, T),
            }
            woff = arr(t.word_off, K * T + 1, np.uint64).tolist()
            wb = bytes(arr(t.word_bytes, woff[-1], np.uint8))
            nt = out["nterms"].tolist()
            out["words"] = [[wb[woff[c * T + i]:woff[c * T + i + 1]] for i in range(nt[c])] for c in range(K)]
            return out
        finally:
            lib().tfidf_clusters_free(C.byref(t))

    def kmeans_info(self) -> dict:
        """Counters and device times of the last kmeans (tfidf_last_kmeans_info)."""
        t = KmeansInfo()
        t.size = C.sizeof(KmeansInfo)
        _chk(lib().tfidf_last_kmeans_info(self.h, C.byref(t)), "tfidf_last_kmeans_info")
        return {k: getattr(t, k) for k, _ in KmeansInfo._fields_ if k != "size"}

    def transform(self, data, doc_off) -> dict:
        """Scores a host batch of unseen documents against the resident model of the last run
        (tfidf_transform): document r is data[doc_off[r]:doc_off[r + 1]].  Returns numpy arrays
        row_off[ndocs + 1], doc_size / doc_oov [ndocs] and, per pair in row order, term, count,
        df, score, word_off, word_len, plus words: the pairs' words as bytes."""
        c, keep = _host_corpus(data, doc_off)
        return _transform(lib().tfidf_transform, self.h, c, keep[0], "tfidf_transform")

    def transform_corpus(self, c: Corpus) -> dict:
        """Engine.transform of a tfidf_corpus, host or device (ingest_dir, synth_device, tests'
        device copies); a device batch's bytes are copied back once to cut the words."""
        if c.flags & TFIDF_CORPUS_DEVICE:
            words_from = lambda: self.corpus_bytes(c)[0] if c.nbytes else b""   # noqa: E731
        else:
            words_from = C.string_at(c.bytes, c.nbytes) if c.nbytes and c.bytes else b""
        return _transform(lib().tfidf_transform, self.h, c, words_from, "tfidf_transform")

    def transform_info(self) -> dict:
        """Counters and device times of the last transform (tfidf_last_transform_info)."""
        t = TransformInfo()
        t.size = C.sizeof(TransformInfo)
        _chk(lib().tfidf_last_transform_info(self.h, C.byref(t)), "tfidf_last_transform_info")
        return {k: getattr(t, k) for k, _ in TransformInfo._fields_ if k != "size"}

    def analyze(self, corpus, off=None, lower: bool = False, punct: bool = False, min_len: int = 0, stop=(),
                slot: int = AN_SLOT_CORPUS, doc_ids=None, ndocs_total: int = 0, stem: bool = False,
                utf8: bool = False) -> Corpus:
        """tfidf_analyze: corpus is a Corpus (host or device), or host bytes with their offsets
        `off`.  Returns the analyzed device Corpus in the context's slot buffers, valid until
        the next analyze with the same slot."""
        a, keep = analyzer(lower, punct, min_len, stop, stem, utf8)
        if isinstance(corpus, Corpus):
            c = corpus
        else:
            c, keep2 = _host_corpus(corpus, off)
            ids = None if doc_ids is None else np.ascontiguousarray(doc_ids, dtype=np.uint32)
            c.doc_ids = None if ids is None else ids.ctypes.data
            c.ndocs_total = ndocs_total
            keep = (keep, keep2, ids)
        out = Corpus()
        _chk(lib().tfidf_analyze(self.h, C.byref(a), C.byref(c), slot, C.byref(out)), "tfidf_analyze")
        return out

    def analyze_info(self) -> dict:
        """Counters and device time of the last analyze (tfidf_last_analyze_info)."""
        t = AnalyzeInfoUtf8()
        t.size = C.sizeof(AnalyzeInfoUtf8)
        _chk(lib().tfidf_last_analyze_info(self.h, C.byref(t)), "tfidf_last_analyze_info")
        names = [k for k, _ in AnalyzeInfo._fields_ + AnalyzeInfoUtf8._fields_]
        return {k: getattr(t, k) for k in names if k not in ("size", "reserved")}

    def ngrams(self, corpus, off=None, min_n: int = 1, max_n: int = 2, joiner: int = 0, slot: int = NG_SLOT_CORPUS,
               doc_ids=None, ndocs_total: int = 0) -> Corpus:
        """tfidf_ngrams: corpus is a Corpus (host or device), or host bytes with their offsets
        `off`.  Returns the shingled device Corpus in the context's slot buffers, valid until
        the next ngrams with the same slot."""
        p = ngram_params(min_n, max_n, joiner)
        if isinstance(corpus, Corpus):
            c = corpus
        else:
            c, keep = _host_corpus(corpus, off)
            ids = None if doc_ids is None else np.ascontiguousarray(doc_ids, dtype=np.uint32)
            c.doc_ids = None if ids is None else ids.ctypes.data
            c.ndocs_total = ndocs_total
        out = Corpus()
        _chk(lib().tfidf_ngrams(self.h, C.byref(p), C.byref(c), slot, C.byref(out)), "tfidf_ngrams")
        return out

    def ngram_info(self) -> dict:
        """Counters and device times of the last ngrams (tfidf_last_ngram_info)."""
        t = NgramInfo()
        t.size = C.sizeof(NgramInfo)
        _chk(lib().tfidf_last_ngram_info(self.h, C.byref(t)), "tfidf_last_ngram_info")
        return {k: getattr(t, k) for k, _ in NgramInfo._fields_ if k not in ("size", "reserved")}

    def model_export(self) -> dict:
        """The context's model (tfidf_model_export): N, terms (list of bytes in term-table order),
        df, term_off, term_bytes: tfidf_fetch's term table without the pairs."""
        m = Model()
        _chk(lib().tfidf_model_export(self.h, C.byref(m)), "tfidf_model_export")
        try:
            return _model_dict(m)
        finally:
            lib().tfidf_model_free(C.byref(m))

    def model_import(self, model: dict) -> None:
        """Puts the context into the model-only state of tfidf_model_import: transform and
        model_export work, everything that needs pairs raises E_STATE."""
        m, keep = _model_struct(model)
        _chk(lib().tfidf_model_import(self.h, C.byref(m)), "tfidf_model_import")

    def model_info(self) -> dict:
        """Counters of the last model_import / model_export (tfidf_last_model_info)."""
        t = ModelInfo()
        t.size = C.sizeof(ModelInfo)
        _chk(lib().tfidf_last_model_info(self.h, C.byref(t)), "tfidf_last_model_info")
        return {k: getattr(t, k) for k, _ in ModelInfo._fields_ if k not in ("size", "reserved")}

    def prune(self, min_df: int = 0, max_df: int = 0, max_features: int = 0, params: PruneParams = None) -> dict:
        """Removes the terms outside [min_df, max_df] or behind the max_features cut, and their
        pairs, from the resident result (tfidf_prune); returns prune_info()."""
        p = params if params is not None else prune_params(min_df, max_df, max_features)
        _chk(lib().tfidf_prune(self.h, C.byref(p)), "tfidf_prune")
        return self.prune_info()

    def prune_info(self) -> dict:
        """Counters and device times of the last prune (tfidf_last_prune_info)."""
        t = PruneInfo()
        t.size = C.sizeof(PruneInfo)
        _chk(lib().tfidf_last_prune_info(self.h, C.byref(t)), "tfidf_last_prune_info")
        return {k: getattr(t, k) for k, _ in PruneInfo._fields_ if k != "size"}

    def reweight(self, tf="ratio", idf="ref", norm="none", params: Weighting = None) -> dict:
        """Replaces the resident scores by the scheme's (tfidf_reweight); returns reweight_info()."""
        w = params if params is not None else weighting(tf, idf, norm)
        _chk(lib().tfidf_reweight(self.h, C.byref(w)), "tfidf_reweight")
        return self.reweight_info()

    def weighting(self) -> dict:
        """The active scheme as names (tfidf_weighting_get)."""
        w = Weighting()
        w.size = C.sizeof(Weighting)
        _chk(lib().tfidf_weighting_get(self.h, C.byref(w)), "tfidf_weighting_get")
        return _weighting_names(w)

    def reweight_info(self) -> dict:
        """Counters and device times of the last reweight (tfidf_last_reweight_info)."""
        t = ReweightInfo()
        t.size = C.sizeof(ReweightInfo)
        _chk(lib().tfidf_last_reweight_info(self.h, C.byref(t)), "tfidf_last_reweight_info")
        return {k: getattr(t, k) for k, _ in ReweightInfo._fields_ if k not in ("size", "reserved")}

    def minhash(self, nhashes: int = 0, seed: int = 0, params: DedupParams = None) -> dict:
        """MinHash signatures of the resident documents in output order (tfidf_minhash)."""
        p = params if params is not None else dedup_params(nhashes, 1 if nhashes else 0, seed, 0.0)
        s = Signatures()
        _chk(lib().tfidf_minhash(self.h, C.byref(p), C.byref(s)), "tfidf_minhash")
        try:
            return _signatures_dict(s)
        finally:
            lib().tfidf_signatures_free(C.byref(s))

    def near_dups(self, threshold: float = 0.8, nhashes: int = 0, rows: int = 0, seed: int = 0,
                  params: DedupParams = None) -> dict:
        """Near-duplicate pairs and groups of the resident documents (tfidf_near_dups): LSH
        candidates, every one verified by its exact Jaccard."""
        p = params if params is not None else dedup_params(nhashes, rows, seed, threshold)
        d = Dups()
        _chk(lib().tfidf_near_dups(self.h, C.byref(p), C.byref(d)), "tfidf_near_dups")
        try:
            return _dups_dict(d)
        finally:
            lib().tfidf_dups_free(C.byref(d))

    def dedup_info(self) -> dict:
        """Counters and device times of the last minhash or near_dups (tfidf_last_dedup_info)."""
        t = DedupInfo()
        t.size = C.sizeof(DedupInfo)
        _chk(lib().tfidf_last_dedup_info(self.h, C.byref(t)), "tfidf_last_dedup_info")
        return {k: getattr(t, k) for k, _ in DedupInfo._fields_ if k != "size"}

    def nb_fit(self, docs, labels, nclasses: int, params=None, **kw) -> None:
        """Fits the Naive Bayes model on the labelled resident documents (tfidf_nb_fit): docs are
        global ids, labels their classes 0..nclasses-1.  kw: variant ("multinomial" /
        "complement"), feature ("count" / "binary"), alpha (0: 1.0), uniform_prior."""
        p, keep = params if params is not None else nb_params(docs, labels, nclasses, **kw)
        _chk(lib().tfidf_nb_fit(self.h, C.byref(p)), "tfidf_nb_fit")

    def nb_predict(self, docs=None, all_scores: bool = False) -> dict:
        """Labels of resident documents (tfidf_nb_predict): every document in output order, or the
        listed global ids.  Returns numpy arrays doc, pos (NO_POS: not held), label (NO_CLASS
        then), score and with all_scores scores[ndocs, nclasses]."""
        ids = None if docs is None else np.ascontiguousarray(docs, dtype=np.uint32)
        n = 0 if ids is None else len(ids)
        if ids is not None and not n:
            ids = np.zeros(1, dtype=np.uint32)                                   # an empty list is a list
        t = NbLabels()
        _chk(lib().tfidf_nb_predict(self.h, _ptr(ids), n, NB_ALL_SCORES if all_scores else 0, C.byref(t)),
             "tfidf_nb_predict")
        try:
            return _nb_labels_dict(t)
        finally:
            lib().tfidf_nb_labels_free(C.byref(t))

    def nb_predict_rows(self, rows: dict, all_scores: bool = False) -> dict:
        """Labels of the rows of a transform of this context (tfidf_nb_predict_rows): rows is the
        dict Engine.transform returns; row_off, term and count are read."""
        ro = np.ascontiguousarray(rows["row_off"], dtype=np.uint64)
        tm = np.ascontiguousarray(rows["term"], dtype=np.uint32)
        ct = np.ascontiguousarray(rows["count"], dtype=np.uint32)
        r = Rows()
        r.ndocs, r.npairs = len(ro) - 1, len(tm)
        r.row_off = ro.ctypes.data_as(C.POINTER(C.c_uint64))
        if len(tm):
            r.term, r.count = tm.ctypes.data_as(C.POINTER(C.c_uint32)), ct.ctypes.data_as(C.POINTER(C.c_uint32))
        t = NbLabels()
        _chk(lib().tfidf_nb_predict_rows(self.h, C.byref(r), NB_ALL_SCORES if all_scores else 0, C.byref(t)),
             "tfidf_nb_predict_rows")
        try:
            return _nb_labels_dict(t)
        finally:
            lib().tfidf_nb_labels_free(C.byref(t))

    def nb_export(self) -> dict:
        """The fitted model on the host (tfidf_nb_export): class_docs, class_total, prior [K],
        feature_count and weight [V, K], and the parameters."""
        m = NbModel()
        _chk(lib().tfidf_nb_export(self.h, C.byref(m)), "tfidf_nb_export")
        try:
            return _nb_model_dict(m)
        finally:
            lib().tfidf_nb_model_free(C.byref(m))

    def nb_info(self) -> dict:
        """Counters and times of the last nb_fit and predict call (tfidf_last_nb_info)."""
        t = NbInfo()
        t.size = C.sizeof(NbInfo)
        _chk(lib().tfidf_last_nb_info(self.h, C.byref(t)), "tfidf_last_nb_info")
        return {k: getattr(t, k) for k, _ in NbInfo._fields_ if k not in ("size", "reserved")}

    @contextlib.contextmanager
    def fetched(self):
        """The last run's result as numpy views of the library's host arrays (tfidf_fetch
        without copies and without the text; valid inside the with block): for full-size
        runs whose pairs do not fit twice in host memory."""
        r = Result()
        _chk(lib().tfidf_fetch(self.h, C.byref(r)), "tfidf_fetch")
        try:
            P, N, V = int(r.npairs), int(r.ndocs), int(r.nterms)

            def view(p, n):
                return np.ctypeslib.as_array(p, shape=(n,)) if n else np.zeros(0, dtype=np.uint8)

            yield {
                "npairs": P, "ndocs": N, "nterms": V, "ndocs_total": int(r.ndocs_total),
                "doc": view(r.pair_doc, P), "term": view(r.pair_term, P), "count": view(r.pair_count, P),
                "docsize": view(r.pair_docsize, P), "df": view(r.pair_df, P), "score": view(r.pair_score, P),
                "doc_id": view(r.doc_id, N), "doc_size": view(r.doc_size, N), "term_df": view(r.term_df, V),
                "term_off": view(r.term_off, V + 1),
                "term_bytes": view(r.term_bytes, int(r.term_off[V]) if V else 0),
            }
        finally:
            lib().tfidf_result_free(C.byref(r))

    def fetch(self) -> dict:
        r = Result()
        _chk(lib().tfidf_fetch(self.h, C.byref(r)), "tfidf_fetch")
        try:
            P, N, V = int(r.npairs), int(r.ndocs), int(r.nterms)

            def arr(p, n, dt):
                if n == 0:
                    return np.zeros(0, dtype=dt)
                return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True)

            out = {
                "npairs": P, "ndocs": N, "nterms": V, "ndocs_total": int(r.ndocs_total),
                "doc": arr(r.pair_doc, P, np.uint32), "term": arr(r.pair_term, P, np.uint32),
                "count": arr(r.pair_count, P, np.uint32), "docsize": arr(r.pair_docsize, P, np.uint32),
                "df": arr(r.pair_df, P, np.uint32), "score": arr(r.pair_score, P, np.float64),
                "doc_id": arr(r.doc_id, N, np.uint32), "doc_size": arr(r.doc_size, N, np.uint32),
                "term_df": arr(r.term_df, V, np.uint32),
            }
            toff = arr(r.term_off, V + 1, np.uint64)
            tb = bytes(arr(r.term_bytes, int(toff[-1]) if V else 0, np.uint8))
            out["terms"] = [tb[int(toff[i]):int(toff[i + 1])] for i in range(V)]
            out["output_txt"] = format_lines(out)
            return out
        finally:
            lib().tfidf_result_free(C.byref(r))


class Group:
    """Several shards in this process (tfidf_group_*): rank r on devices[r]; RCCL when
    every rank has its own GPU, the in-process transport when a device is shared (or
    local=True).  Every run is collective over all ranks."""

    def __init__(self, nranks: int, devices=None, local: bool = False):
        dev = None if devices is None else (C.c_int * nranks)(*devices)
        h = C.c_void_p()
        _chk(lib().tfidf_group_open(nranks, dev, TFIDF_GROUP_LOCAL if local else 0, C.byref(h)), "tfidf_group_open")
        self.h = h
        self.n = nranks
        self.ranks = [Engine(handle=lib().tfidf_group_ctx(h, r)) for r in range(nranks)]
        self._keep = None

    def close(self):
        if self.h:
            lib().tfidf_group_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def run(self, shards):
        """shards: list of Corpus (one per rank)."""
        arr = (Corpus * self.n)(*shards)
        _chk(lib().tfidf_group_run(self.h, arr), "tfidf_group_run")

    def run_host(self, shards):
        """shards: list of (data, doc_off, doc_ids, ndocs_total) host arrays, one per rank."""
        cs, keep = [], []
        for data, off, ids, nt in shards:
            data = np.ascontiguousarray(data, dtype=np.uint8)
            off = np.ascontiguousarray(off, dtype=np.uint64)
            ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32)
            c = Corpus()
            c.bytes = data.ctypes.data if len(data) else None
            c.nbytes = len(data)
            c.doc_off = off.ctypes.data
            c.doc_ids = None if ids is None else ids.ctypes.data
            c.ndocs = len(off) - 1
            c.flags = 0
            c.ndocs_total = nt
            cs.append(c)
            keep.append((data, off, ids))
        self._keep = keep
        self.run(cs)

    def write_output(self, path: str):
        _chk(lib().tfidf_group_write_output(self.h, path.encode()), "tfidf_group_write_output")

    def query(self, queries, k: int = 10) -> dict:
        """Top-k documents over all shards (tfidf_group_query); see Engine.query."""
        return _query(lib().tfidf_group_query, self.h, queries, k, "tfidf_group_query")

    def query_bm25(self, queries, k: int = 10, k1: float = 1.2, b: float = 0.75, avgdl: float = 0.0) -> dict:
        """BM25 ranking over all shards (tfidf_group_query_bm25); avgdl 0: the average over
        every shard's documents.  See Engine.query_bm25."""
        res = _query(lib().tfidf_group_query_bm25, self.h, queries, k, "tfidf_group_query_bm25",
                     _bm25_params(k1, b, avgdl))
        res["avgdl"] = self.ranks[0].bm25_info()["avgdl"]   # every rank scored with the same value
        return res

    def query_clauses(self, must=None, should=None, must_not=None, k: int = 10, min_should=None, bm25=None) -> dict:
        """Clauses over all shards (tfidf_group_query_clauses); see Engine.query_clauses."""
        c, _keep = make_clauses(must, should, must_not, min_should, bm25)
        return _query(lib().tfidf_group_query_clauses, self.h, c, k, "tfidf_group_query_clauses")

    def top_terms(self, k: int = 10, docs=None, words: bool = True) -> dict:
        """The k best-scoring words of each document over all shards (tfidf_group_top_terms);
        see Engine.top_terms.  term is the rank in the holding shard's term table."""
        return _top_terms(lib().tfidf_group_top_terms, self.h, k, docs, "tfidf_group_top_terms", words)

    def match_terms(self, patterns, kinds=None, max_edits=None, params: MatchParams = None, **kw) -> dict:
        """Fuzzy and prefix patterns against every shard's term table, merged
        (tfidf_group_match_terms); see Engine.match_terms.  term is UINT32_MAX, nmatch the largest
        rank's count."""
        return _match_terms(lib().tfidf_group_match_terms, self.h, patterns, kinds, max_edits, params,
                            "tfidf_group_match_terms", **kw)

    def snippets(self, queries, jobs=None, hits=None, params: SnippetParams = None, **kw) -> dict:
        """Snippets over all shards (tfidf_group_snippet); see Engine.snippets."""
        return _snippets(lib().tfidf_group_snippet, (self.h,), queries, jobs, hits, params, "tfidf_group_snippet", **kw)

    def similar(self, k: int = 10, docs=None) -> dict:
        """The k nearest neighbours of each document over all shards (tfidf_group_similar): the
        single-shard result bit for bit; see Engine.similar."""
        return _similar(lib().tfidf_group_similar, self.h, k, docs, "tfidf_group_similar")

    def transform(self, data, doc_off) -> dict:
        """Scores a host batch against every shard's vocabulary, rows merged by word
        (tfidf_group_transform): the single-shard result bit for bit, term = 0xFFFFFFFF; see
        Engine.transform."""
        c, keep = _host_corpus(data, doc_off)
        return _transform(lib().tfidf_group_transform, self.h, c, keep[0], "tfidf_group_transform")

    def model_export(self) -> dict:
        """The model of the whole group (tfidf_group_model_export): the ranks' term tables merged,
        byte-identical to a single-shard export of the same corpus; see Engine.model_export."""
        m = Model()
        _chk(lib().tfidf_group_model_export(self.h, C.byref(m)), "tfidf_group_model_export")
        try:
            return _model_dict(m)
        finally:
            lib().tfidf_model_free(C.byref(m))

    def prune(self, min_df: int = 0, max_df: int = 0, max_features: int = 0) -> None:
        """tfidf_group_prune: every rank prunes its shard by the global df; max_features != 0 is
        E_INVAL."""
        p = prune_params(min_df, max_df, max_features)
        _chk(lib().tfidf_group_prune(self.h, C.byref(p)), "tfidf_group_prune")

    def reweight(self, tf="ratio", idf="ref", norm="none") -> None:
        """tfidf_group_reweight: every rank reweights its shard (N and df are global)."""
        w = weighting(tf, idf, norm)
        _chk(lib().tfidf_group_reweight(self.h, C.byref(w)), "tfidf_group_reweight")

    def transform_corpus(self, c: Corpus) -> dict:
        """Group.transform of a tfidf_corpus (a device batch is E_INVAL)."""
        host = not (c.flags & TFIDF_CORPUS_DEVICE)
        bb = C.string_at(c.bytes, c.nbytes) if host and c.nbytes and c.bytes else b""
        return _transform(lib().tfidf_group_transform, self.h, c, bb, "tfidf_group_transform")


def plan_dir(path: str, nshards: int, threads: int = 0) -> dict:
    """tfidf_plan_dir: byte-balanced "docN@"-ordered shards of an input directory."""
    p, bad = DirPlan(), C.c_uint32(0)
    rc = lib().tfidf_plan_dir(path.encode(), nshards, threads, C.byref(p), C.byref(bad))
    if rc:
        e = TfidfError(rc, "tfidf_plan_dir")
        e.bad_doc, e.ndocs = bad.value, p.ndocs
        raise e
    try:
        N = int(p.ndocs)
        ids = np.ctypeslib.as_array(p.doc_ids, shape=(N,)).copy() if N else np.zeros(0, np.uint32)
        nb = np.ctypeslib.as_array(p.doc_bytes, shape=(N,)).copy() if N else np.zeros(0, np.uint64)
        first = np.ctypeslib.as_array(p.shard_first, shape=(nshards + 1,)).copy()
        sb = np.ctypeslib.as_array(p.shard_bytes, shape=(nshards,)).copy()
        return {"ndocs": N, "doc_ids": ids, "doc_bytes": nb, "shard_first": first, "shard_bytes": sb}
    finally:
        lib().tfidf_plan_free(C.byref(p))


def doc_name_order(n: int) -> np.ndarray:
    out = np.zeros(max(n, 1), dtype=np.uint32)
    _chk(lib().tfidf_doc_name_order(n, out.ctypes.data), "tfidf_doc_name_order")
    return out[:n]


def shard_split(sizes, nshards: int) -> np.ndarray:
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    first = np.zeros(nshards + 1, dtype=np.uint32)
    _chk(lib().tfidf_shard_split(sizes.ctypes.data if len(sizes) else None, len(sizes), nshards, first.ctypes.data),
         "tfidf_shard_split")
    return first


def format_lines(res: dict) -> bytes:
    """output.txt bytes ("docN@word\\t%.16f\\n", TFIDF.c:245,281) from a fetched result."""
    terms = res["terms"]
    parts = []
    for d, t, s in zip(res["doc"].tolist(), res["term"].tolist(), res["score"].tolist()):
        parts.append(b"doc%d@" % d + terms[t] + b"\t%.16f\n" % s)
    return b"".join(parts)


def device_count() -> int:
    """Visible HIP devices (tfidf_device_count; 0 without a GPU)."""
    return int(lib().tfidf_device_count())


def alloc_live():
    """(device allocations, bytes) the library holds in this process right now: allocations minus
    frees (tfidf_alloc_live).  The same before an Engine or Group is opened and after it is closed."""
    a, b = C.c_uint64(), C.c_uint64()
    _chk(lib().tfidf_alloc_live(C.byref(a), C.byref(b)), "tfidf_alloc_live")
    return int(a.value), int(b.value)


def comm_unique_id() -> bytes:
    buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
    _chk(lib().tfidf_comm_unique_id(buf), "tfidf_comm_unique_id")
    return bytes(buf)
