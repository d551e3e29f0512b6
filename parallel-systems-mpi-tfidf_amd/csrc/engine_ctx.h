/*
 * engine_ctx.h — private to csrc/engine*.cpp (not installed, not part of include/tfidf.h): the
 * context behind the C-ABI's opaque tfidf_ctx, the error macros, and the helpers that more
 * than one engine file uses.
 *
 * File map (each add-on file drives the .hip file of the same name):
 *   engine.cpp            context open/close, comm, the DF exchange, run_*, the idf pool, fetch,
 *                         synth, format and output writing: the measured pipeline of tfidf_run
 *   engine_query.cpp      tfidf_query, tfidf_query_bm25, tfidf_query_clauses (query.hip, bm25.hip); the topk_* driver
 *   engine_transform.cpp  tfidf_transform
 *   engine_text.cpp       tfidf_analyze, tfidf_ngrams (analyze.hip, ngram.hip); corpus intake and
 *                         token bounds, shared with tfidf_transform
 *   engine_model.cpp      tfidf_model_export, tfidf_model_import
 *   engine_prune.cpp      tfidf_prune; ensure_spare
 *   engine_weight.cpp     tfidf_reweight (reweight.hip); the rw_* helpers tfidf_transform shares
 *   engine_terms.cpp      tfidf_top_terms; ensure_term_meta, lookup_ids
 *   engine_similar.cpp    tfidf_similar, the halves of tfidf_group_similar; sim_norms
 *   engine_kmeans.cpp     tfidf_kmeans
 *   engine_dedup.cpp      tfidf_minhash, tfidf_near_dups (dedup.hip; the groups: dedup_host.c)
 *   engine_nb.cpp         tfidf_nb_fit, tfidf_nb_predict, tfidf_nb_predict_rows, tfidf_nb_export
 *                         (nb.hip; the check and the host twin: nb_host.c)
 *   engine_match.cpp      tfidf_match_terms (match.hip; the check and the host twin: match_host.c)
 *   engine_snippets.cpp   tfidf_snippet (snippets.hip; the check and the host twin: snippet_host.c)
 * The add-on calls run between runs on the context's stream and use the run's arena as scratch
 * only; none of them is on the path tfidf_run times.  The add-on launches and the run's own
 * persistent kernels alike take their CU count from ctx_ncu below.
 *   devbuf.h              tfidf_dev_malloc / tfidf_dev_free and DevBuf (group.cpp's transports too)
 *   knobs.h               the table of tfidf_open's numeric environment knobs and its parser
 *
 * Ownership: every member of tfidf_ctx that holds a device buffer, a stream, an event or pinned
 * memory is of a type that releases it (DevBuf, Stream, Event, Pinned), so a member added to the
 * context needs no line elsewhere: tfidf_close is `delete ctx`, and tfidf_open's failure returns
 * leak nothing.  ~tfidf_ctx does only what needs an order.  tfidf_alloc_live (allocations minus
 * frees of the process) is the test's check that nothing outlives a context.
 * Invalidation: a call that changes the result says so once, through result_changed below, whose
 * table lists every cache kept per result.
 */
#ifndef TFIDF_ENGINE_CTX_H
#define TFIDF_ENGINE_CTX_H

#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/tfidf.h"
#include "kernels.h"
#include "xport.h"
#include "devbuf.h"

/* ---- owning handles.  Each destroys what it holds when it holds something, so a member added to
 * the context needs no line elsewhere: tfidf_close is `delete ctx`.  They convert to the raw
 * handle, so the use sites read as they did with raw members. ---- */
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
};
/* one event; the calls' event sets are arrays of them (call_begin creates what is missing) */
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
    hipError_t create() { return hipEventCreate(&e); }
    hipError_t create_untimed() { return hipEventCreateWithFlags(&e, hipEventDisableTiming); }
};
/* pinned host memory */
template <typename T> struct Pinned {
    T* p = nullptr;
    Pinned() = default;
    Pinned(const Pinned&) = delete;
    Pinned& operator=(const Pinned&) = delete;
    ~Pinned() { release(); }
    operator T*() const { return p; }
    T* operator->() const { return p; }
    /* `bytes` anew: what it held is freed first */
    hipError_t alloc(size_t bytes, unsigned flags = hipHostMallocDefault) {
        release();
        const hipError_t e = hipHostMalloc((void**)&p, bytes, flags);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
    }
};
enum Stage { S_PREP, S_TOKCOUNT, S_VOCAB, S_MERGE, S_DF, S_EXCHANGE, S_IDF, S_ORDER, S_SCORE, S_NSTAGES };

struct tfidf_ctx {
    /* engine.cpp: only what needs an order (the device, the three streams drained, xp, the idf
     * workers, the live count); every member below releases what it owns by its own destructor */
    ~tfidf_ctx();
    bool live = false;      /* counted among the process's open contexts (tfidf_open's last step) */
    int device = 0;
    Stream stream;
    Xport* xp = nullptr;    /* peers of the DF exchange (RCCL or in-process); owned */
    int rank = 0, nranks = 1;
    int timing = 1;         /* tfidf_set_timing: 0 none, 1 every stage, 2 K1 and the whole run only */
    int k1_mode = 0;        /* 0 auto (k_tokcount_sl up to K1_SL_MAX_CAP slots, k_tokcount_vs beyond),
                               1 round-1 kernel (TFIDF_K1=vs), 2 general K1 (TFIDF_K1=general),
                               3 k_tokcount_sl (TFIDF_K1=sl) — cross-checks and A/B timing;
                               round 3's k_tokcount_st was retired in round 5, round 6's two-pass form of
                               k_tokcount_sl (measured slower: DESIGN §8) in round 6 (git history) */
    bool stamps_on = false; /* env TFIDF_STAMPS=1 with the diagnostic library build */
    int xfail_rank = -1;    /* env TFIDF_TEST_XFAIL_RANK (tests): this rank fails inside the exchange of
                               its first run, right after the key all-gather (the abort path of
                               exchange_df) */
    int xnomem_rank = -1;   /* env TFIDF_TEST_XNOMEM_RANK (tests): this rank's receive-side allocation
                               of its first exchange fails (the agreed path: no abort) */
    DevBuf stamps;
    bool k1_vs = false;     /* last run used the slot-keyed kernel (default) */
    bool k1_sl = false;     /* ... or tokcount_sl (else tokcount_vs) */
    uint64_t sl_maxcap = K1_SL_MAX_CAP;   /* env TFIDF_SL_MAXCAP: tokcount_sl up to this many vocabulary slots */
    Pinned<K1Out> k1out_host;      /* pinned: tokcount_sl's output block, copied to k1out_dev per run */
    DevBuf k1out_dev;
    bool k1out_valid = false;      /* k1out_dev holds *k1out_host (the copy is skipped when a run's block is the same) */
    Event ev[S_NSTAGES + 1];
    Arena arena;
    DevBuf arena_buf;
    /* side stream: the document-order sort (needs only the document ids) runs beside the
     * vocabulary / merge / DF stages, after K1 (K1's persistent grid wants every CU) */
    Stream stream2;
    Event ev_fork, ev_order;
    Event ev_spin;                  /* the run's host waits (spin_sync) */
    uint64_t wait_token = 0;        /* the last completion token of a status-words kernel (words_wait) */
    Stream stream3;                 /* the idf table's upload, beside the merge / DF stages */
    Event ev_idf_up;
    bool idf_early = false;         /* this run's table is on its way up stream3 (run_post waits on ev_idf_up) */
    /* split DF (runs with partial records): the main records' histogram runs on stream2
     * beside the merge stage, the merged records' is added on the main stream after it */
    bool df_split = true;           /* env TFIDF_DF_SPLIT=0: one DF pass after the merge */
    Event ev_vrank, ev_dfmain;
    /* packed records: k_tokcount_sl over a table of at most K1_ST_MAX_CAP slots emits a
     * complete document's record as one word; the run keeps it one word through DF and the score
     * kernels where df_keeps_packed allows, and unpacks it after K1 otherwise */
    bool rec_pack = true;           /* env TFIDF_REC_PACK=0: two-word records throughout */
    bool run_pack = false;          /* this run's K1 emitted packed records */
    bool run_pack_kept = false;     /* ... and they stayed packed through DF and the score kernels */
    DevBuf df_scratch;
    size_t df_scratch_min = 0;      /* grown when the split DF pass reported a shortfall (retried) */
    Arena arena2;
    DevBuf arena2_buf;
    /* host-input staging */
    DevBuf in_bytes, in_off, in_ids;
    /* synthetic corpus */
    DevBuf syn_bytes, syn_off, syn_ids, syn_ntok, syn_blkfirst, syn_blkbytes, syn_cdf;
    /* stage buffers */
    DevBuf chunk_start, chunk_doc;
    DevBuf vkeys, vrep;
    /* vocabulary table: K1 is measurably faster at low load (fewer displaced keys behind
     * the two slots it loads per token): 1M slots (16 MB) to start, x4 past 12 % load */
    uint64_t vcap = 1ull << 20;
#define VOCAB_LOW_LOAD_CAP (1ull << 24)
#define IDF_FULL_MAX (1ull << 18)   /* documents up to which the idf table covers every df (beyond:
                                       the distinct df values of the run, one host round trip) */
    uint32_t vload_pct = 12;
    uint32_t vload_big_pct = 45;   /* load limit of tables of VOCAB_LOW_LOAD_CAP slots and more */
    DevBuf rec_slot, rec_cnt;
    uint64_t rec_cap = 0;
    DevBuf part_doc, part_slot, part_cnt;
    uint64_t part_cap = 0;
    DevBuf doc_recoff, doc_npairs, doc_size, doc_flags;
    DevBuf counters;
    /* pinned host words for the per-run device-to-host reads (corpus bounds, K1 counters,
     * final status): asynchronous copies on the stream and one synchronisation each, instead
     * of pageable or synchronous copies (two round trips per run saved) */
    Pinned<uint64_t> hpin;
    uint64_t* hpin_dev = nullptr;   /* hpin as the device addresses it (status words written by kernels) */
    DevBuf dense, vslot, skey0, skey1, seq0, seq1, rank_of_slot, slot_of_rank, rank16;
    DevBuf pkey0, pkey1, pseq0, pseq1, phead;
    DevBuf big_list, big_idx, dense_cnt, kcnt, tile_cnt;   /* dense merge of long documents */
    DevBuf df_local, df_global, present, idf_vals;
    uint64_t idf_full_n = 0;   /* idf_vals holds log(N/df) for df = 0..N of this N (0: not) */
    /* the per-run idf table (N <= IDF_FULL_MAX): host threads fill the pinned idf_pin with
     * log(N/df) for df = 0..N while the device runs the stages before the score; run_post
     * joins them and uploads it (every run: round 4's per-N cache was retired in round 6) */
    Pinned<double> idf_pin;
    size_t idf_pin_n = 0;
    bool idf_pin_busy = false;            /* an upload from idf_pin is enqueued and not known complete (the
                                             run's final wait clears it; no event record: each costs
                                             the stream ~5 us, scripts/micro/host_api_cost.hip) */
    struct IdfPool {                      /* persistent workers: no thread start per run */
        std::mutex mu;
        std::condition_variable go, done;
        std::vector<std::thread> th;
        uint64_t gen = 0;
        bool stop = false, busy = false;
        unsigned active = 0, left = 0;
        double* lut = nullptr;
        uint64_t Nt = 0;
        const uint32_t* vals = nullptr;   /* null: lut[d] for every df d = 1..Nt; else lut[k] for df vals[k], k < n */
        uint64_t n = 0;
        uint32_t mode = 0;                /* TFIDF_IDF_REF: the run's log(N/df); else a weighting scheme's idf (tfidf_reweight) */
        std::chrono::steady_clock::time_point t0;
        int64_t end_ns = 0;
    } idf_pool;
    uint64_t idf_logs = 0;                /* log() calls of the last run */
    tfidf_run_totals totals{};            /* sums over the runs since the last tfidf_run_totals_get reset */
    double ms_idf_host = 0, ms_idf_wait = 0;
    DevBuf dkey0, dkey1, dseq0, dseq1, npairs_ord, out_off, doc_meta;
    DevBuf out_term, out_cnt, out_score, idf_rank, large_list, split_tasks, cls_off;
    /* DF exchange (hash owners): this rank's keys by term rank, the send side grouped by
     * owner (key, local df, term rank), the owner side (received keys and df, their table
     * slots, the replies, the aggregation table), the returned global df, the count matrix */
    DevBuf x_mine, x_srec, x_sidx, x_back, x_cnt;
    DevBuf x_rrec, x_rslot, x_reply, x_tkey, x_tdf;
    /* dense exchange (small vocabularies): gathered keys, shared positions, the DF vector */
    DevBuf x_gkeys, x_pos, x_dense;
    /* cross-rank check of long terms (exchange_long_check): this rank's list, its send block
     * (entries + bytes), the gathered blocks, the check's key table */
    DevBuf x_lloc, x_lsend, x_lgath, x_ltab;
    int xchg_mode = 0;      /* env TFIDF_XCHG: 0 auto (dense up to DENSE_XCHG_MAXV terms per rank), 1 owner, 2 dense,
                               3 dense with table numbering */
    bool last_dense = false;   /* the last exchange used the dense form */
    bool local_long = false;   /* this rank's vocabulary holds terms of >= 16 bytes (K1 status) */
    bool xagg_table = false;   /* env TFIDF_XAGG=table: the owner aggregates in an HBM table (A/B) */
    uint32_t xb_stage_max = ~0u;   /* env TFIDF_XB_STAGE_MAX (tests): the owner's largest bucket staged in LDS */
    /* sizes the local part of a run hands to the exchange and the stages after it */
    uint32_t run_N = 0, run_V = 0;
    uint64_t run_cap = 0, run_R_total = 0;
    const uint32_t* run_merged = nullptr;
    /* output text (emit.hip) */
    DevBuf t_key, t_len, doc_tbytes, doc_toff, text;
    /* top-k retrieval (tfidf_query, query.hip): the batch's terms and their ranks, a group's
     * term table, the (query, output position) accumulators and matched counts, the list of
     * long documents, the top-k rounds' two candidate buffers, per-query counters */
    DevBuf q_terms, q_rank, q_tab, q_acc, q_cnt, q_big, q_cand0, q_cand1, q_misc;
    uint64_t query_acc_bytes = 1024ull << 20;   /* env TFIDF_QUERY_ACC_MB: accumulator budget of a query group */
    Event ev_q[3];                              /* lookup / score / top-k bounds (created by the first query) */
    uint32_t ncu = 0;
    tfidf_query_info qinfo{};
    /* BM25 ranking (tfidf_query_bm25, bm25.hip): tfidf_query's buffers; L = the sum of doc_size
     * over this context's documents, kept until the next run */
    uint64_t bm25_L = 0;
    bool bm25_L_valid = false;
    tfidf_bm25_info binfo{};
    tfidf_clause_info cinfo{};                  /* tfidf_query_clauses: tfidf_query's buffers too */
    /* per-document top-k terms (tfidf_top_terms, terms.hip): the requested ids and their output
     * positions, a batch's per-row words (npairs, nterms, id), its k entries per row (score
     * bits, pair, term, count, word length -> offset), the gathered words, the list of long
     * documents */
    DevBuf tm_ids, tm_rows, tm_score, tm_pair, tm_term, tm_cnt, tm_woff, tm_words, tm_big;
    uint64_t terms_bytes = 256ull << 20;        /* env TFIDF_TERMS_MB: device result buffers of a batch of rows */
    Event ev_t[5];                              /* lookup or select / scan / gather bounds (created by the first call) */
    bool tmeta_valid = false;                   /* t_key / t_len hold this run's term metadata */
    tfidf_terms_info tinfo{};
    /* top-k similar documents (tfidf_similar, similar.hip): sq and norm by output position
     * (kept until the next run), the call's row ids and rows (vector range, norm, sq, position,
     * id), a group's term masks, counts, postings offsets and weights, the neighbours' positions and
     * shared-term counts, and for vectors another shard exported their scores; the exported
     * vectors (terms, scores, word lengths -> offsets, word bytes) of tfidf_group_similar.  The
     * accumulators, candidates and counters are tfidf_query's (q_acc .. q_misc). */
    DevBuf sm_norm, sm_ids, sm_rows, sm_mask, sm_cnt, sm_off, sm_pw, sm_res, sm_escore;
    DevBuf sm_xterm, sm_xscore, sm_xwoff, sm_xwords, sm_xoff;
    Event ev_s[6];                              /* norms / table / score / top-k bounds (created by the first call) */
    bool norm_valid = false;                    /* sm_norm holds this run's norms */
    tfidf_similar_info sinfo{};
    /* spherical k-means (tfidf_kmeans, kmeans.hip): the dense centroid matrix [V][K] (the update's
     * sums are built in it), the per-document and per-cluster words (ids, two label arrays, sim,
     * members, sizes, offsets, seed positions, centroid norms, the changed counter), the top-term
     * selection's lists and the selected words.  The norms are tfidf_similar's (sm_norm). */
    DevBuf km_C, km_work, km_top, km_words;
    uint64_t kmeans_bytes = 1024ull << 20;      /* env TFIDF_KMEANS_MB: budget of km_C + km_work */
    uint32_t kmeans_split = 0;                  /* env TFIDF_KMEANS_SPLIT: update workgroups per cluster (0: fill the GPU) */
    uint32_t an_grid = 0;                       /* env TFIDF_AN_GRID: at most that many workgroups of the analyzer's tile kernel (0: the resident ones) */
    uint32_t grid_cus = 0;                      /* env TFIDF_GRID_CUS: the CU count `ncu` takes in place of the device's (0: the device's), for the run's kernels too */
    Event ev_k[4];                              /* assign / update / top-term bounds (created by the first call) */
    tfidf_kmeans_info kinfo{};
    /* unseen documents against the resident model (tfidf_transform, transform.hip): a host
     * batch's bytes and offsets, a slice's boundary scratch (document-start bitmap, per-tile
     * counts, per-document words) and its token and pair arrays */
    DevBuf tr_bytes, tr_off, tr_a, tr_b;
    uint64_t transform_bytes = 512ull << 20;    /* env TFIDF_TRANSFORM_MB: device scratch of a slice */
    Event ev_tr[5];                             /* tokens / resolve / sort / pairs bounds (created by the first call) */
    tfidf_transform_info trinfo{};
    /* the portable model (tfidf_model_import / tfidf_model_export, model.hip).  have_model: the
     * context holds what tfidf_transform reads (table, ranks, df, idf, V, N), from a run or from
     * an import.  model_only: from an import; the uploaded term bytes (m_blob, m_blob_bytes)
     * stand where the run's corpus does (dev_bytes / corpus.nbytes) and m_off holds the term
     * offsets, so the term table is those two buffers.  m_stat: the build's status word. */
    bool have_model = false, model_only = false;
    DevBuf m_off, m_blob, m_stat;
    uint64_t m_blob_bytes = 0;
    Event ev_m[2];                              /* clear + build bounds (created by the first import) */
    tfidf_model_info minfo{};
    /* the analyzer (tfidf_analyze, analyze.hip): a host input's staged bytes; per slot the
     * analyzed bytes and the context's copies of the offsets and ids; the document-start bitmap,
     * the stop-word table and the blanked-token counter of the call in flight */
    DevBuf an_in, an_bytes[2], an_off[2], an_ids[2], an_dstart, an_tab, an_cnt;
    Event ev_an[2];                             /* the kernels' bounds (created by the first call) */
    tfidf_analyze_info aninfo{};
    /* word n-grams (tfidf_ngrams, ngram.hip): a host input's staged bytes and offsets; per slot
     * the output bytes, the new offsets and the context's copy of the ids; the boundary scratch
     * (status, gram counter, bitmap, per-tile counts), the 24 bytes per token (start, end,
     * segment offset) and the write kernel's tile index of the call in flight */
    DevBuf ng_in, ng_inoff, ng_bytes[2], ng_off[2], ng_ids[2], ng_a, ng_b, ng_tseg;
    Event ev_ng[4];                             /* bounds / sizes / write bounds (created by the first call) */
    tfidf_ngram_info nginfo{};
    /* vocabulary pruning (tfidf_prune, prune.hip): the keep flags (then the new ranks), the keep
     * bitmap, the max_features sort's ping-pong buffers, the per-tile counts and first documents,
     * the emptied-documents counter; and the spare copies of the resident arrays the call writes
     * into and swaps with the context's own when every step has succeeded (slot_of_rank, df by
     * rank, out_term, out_cnt, out_score, out_off), each as large as the buffer it stands in for */
    DevBuf pr_flag, pr_bits, pr_k0, pr_k1, pr_v0, pr_v1, pr_tcnt, pr_tdoc, pr_misc;
    DevBuf pr_sor, pr_df, pr_term, pr_cnt, pr_score, pr_off;
    Event ev_pr[4];                             /* select / terms / pairs bounds (created by the first call) */
    tfidf_prune_info pinfo{};
    uint64_t info_npairs = 0;                   /* the run's P and V as tfidf_last_run_info reports them (a prune */
    uint32_t info_V = 0;                        /* changes npairs and V, not what the run was) */
    /* weighting schemes (tfidf_reweight, reweight.hip): the active scheme; the scheme's idf table in
     * the layout of idf_vals (by df, or through `present`), which is never overwritten; the
     * sublinear tf table fl(1 + log c), c = 0..rw_lut_n (the values do not depend on the run, so
     * the table only ever grows), the listed counts above it and their values; the list of big
     * documents; the count maximum and the counters.  The new scores go into prune's spare
     * pr_score; the idf by rank into the run's idf_rank, which has no reader after a run. */
    uint32_t wt_tf = 0, wt_idf = 0, wt_norm = 0;
    uint32_t rw_idf_mode = 0;                   /* the idf mode rw_idf holds for this run or model (0: none) */
    DevBuf rw_idf, rw_lut, rw_list, rw_listv, rw_big, rw_misc;
    uint32_t rw_lut_n = 0;
    std::vector<double> rw_lut_host;
    std::vector<uint32_t> rw_list_host;
    std::vector<double> rw_listv_host;
    Event ev_rw[3];                             /* tables / pairs bounds (created by the first call) */
    tfidf_reweight_info rwinfo{};
    /* near duplicates (tfidf_minhash / tfidf_near_dups, dedup.hip): h0 by term rank (kept until the
     * next run, prune or import), the signatures by output position, the hash family, the counter
     * words with the list of big documents behind them, and the band and verify stages' work
     * buffer (keys, values, flags, candidates, the positions with pairs) */
    DevBuf dd_h0, dd_sig, dd_fam, dd_misc, dd_work;
    uint64_t dedup_bytes = 1024ull << 20;       /* env TFIDF_DEDUP_MB: signatures + the bound on candidate scratch */
    Event ev_dd[3];                             /* hash / signature, bands / verify bounds (created by the first call) */
    bool h0_valid = false;                      /* dd_h0 holds this result's term hashes */
    tfidf_dedup_info ddinfo{};
    /* Naive Bayes (tfidf_nb_fit / tfidf_nb_predict, nb.hip): the two dense matrices [V][K] (feature
     * counts, weights); the per-term and per-class words (F, T, the classes' logarithms, the priors,
     * the counters, the labels by output position); the logarithm table and the sorted list behind
     * it; the fit's or a predict call's ids and positions; uploaded rows; a predict batch's labels
     * and scores.  The model stays until the next run, prune, import or fit (nb_valid). */
    DevBuf nb_FC, nb_W, nb_work, nb_lut, nb_list, nb_ids, nb_rows, nb_out;
    uint64_t nb_bytes = 1024ull << 20;          /* env TFIDF_NB_MB: budget of nb_FC + nb_W + nb_work */
    Event ev_nb[4];                             /* count / weights or predict bounds (created by the first call) */
    bool nb_valid = false;
    uint32_t nb_K = 0, nb_V = 0, nb_variant = 0, nb_feature = 0, nb_uniform = 0;
    double nb_alpha = 0;
    uint64_t nb_n = 0;
    const double* nb_prior_dev = nullptr;       /* points into nb_work */
    const uint64_t* nb_T_dev = nullptr;
    std::vector<uint64_t> nb_class_docs;        /* n_c, kept for tfidf_nb_export */
    tfidf_nb_info nbinfo{};
    /* term matching (tfidf_match_terms, match.hip): the call's pattern block (MT_PAT bytes per
     * pattern, then lengths, kinds, budgets); the per-pattern match counts with the list's cursor
     * behind them; the match list and its sort's second half (keys, values); a batch's segment
     * offsets, its k entries per pattern (term, dist, df, word length -> offset) and the gathered
     * words.  Nothing is kept per result. */
    DevBuf mt_pat, mt_cnt, mt_k0, mt_k1, mt_v0, mt_v1, mt_seg, mt_term, mt_dist, mt_df, mt_woff, mt_words;
    Event ev_mt[6];                             /* scan / select / words bounds (created by the first call) */
    tfidf_match_info mtinfo{};
    /* snippets (tfidf_snippet, snippets.hip): the call's term offsets, bytes, keys and found flags; the
     * queries' table words and term tables; the jobs' ids, positions, queries and documents; a batch's
     * tile words (the jobs' first tiles, the per-tile token and match counts and their scans, the
     * per-job totals, slices, best keys and slot masks); a sub-batch's match records, its per-job
     * results with the marks' and texts' offsets, and the marks and window bytes.  Nothing is kept
     * per result: positions are found anew by every call, so the invalidation table below has no row. */
    DevBuf sn_terms, sn_tab, sn_jobs, sn_tile, sn_rec, sn_out, sn_marks;
    Event ev_sn[10];                            /* lookup / count / write, select, emit / fill bounds (created by the first call) */
    tfidf_snippet_info sninfo{};
#define WR_NBUF 8
#define WR_BUF (16ull << 20)
#define WR_GROUPS 8
    Pinned<uint8_t> wr_buf[WR_NBUF];   /* pinned output staging ring */
    Event wr_ev[WR_NBUF];
    Event wr_fmt[WR_GROUPS];
#define WR_WRITERS 8   /* page-cache writes run ~3 GB/s per thread (profiles/r04_cli_c2.json) */
    tfidf_output_info out_info{};
    uint64_t text_bytes = 0;
    bool text_valid = false;
    uint32_t* sorted_dense = nullptr; /* points into seq0/seq1 */
    uint4* sorted_skey = nullptr;
    const uint32_t* order = nullptr;
    /* last run */
    bool have_result = false;
    bool have_info = false;   /* run counters/timings valid */
    uint64_t run_nbytes = 0;  /* corpus bytes of the last run (its bounds, read once by the run) */
    tfidf_corpus corpus{};
    const uint8_t* dev_bytes = nullptr;
    const uint32_t* dev_ids = nullptr;
    uint64_t npairs = 0, ntokens = 0, nchunks = 0, nrec_part = 0, ndocs_total = 0;
    uint32_t ndocs = 0, V = 0, Vg = 0;
    uint32_t k1_workgroups = 0;   /* the grid of the last K1 launch (0: none was launched) */
    double ms_stage[S_NSTAGES] = {0};
    double ms_total = 0;
    hipError_t last_err = hipSuccess;
};
#define HIPCHK(x)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            ctx->last_err = e_;                                                            \
            fprintf(stderr, "tfidf: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            return TFIDF_E_HIP;                                                            \
        }                                                                                  \
    } while (0)
/* TFIDF_DEBUG_ALLOC=1: every (re)allocation of a stage buffer is named on stderr (which
 * buffer still grows after the warm-up runs) */
static inline int debug_alloc() {
    static const int on = [] { const char* e = getenv("TFIDF_DEBUG_ALLOC"); return e && e[0] == '1'; }();
    return on;
}
static inline int ensure_named(DevBuf& b, size_t bytes, const char* name) {
    const void* p0 = b.p;
    const int rc = b.ensure(bytes);
    if (debug_alloc() && (b.p != p0 || rc))
        fprintf(stderr, "tfidf: alloc %s %zu bytes (asked %zu)%s\n", name, b.cap, bytes, rc ? " FAILED" : "");
    return rc;
}
#define ENSURE(buf, bytes)                                   \
    do {                                                     \
        if (ensure_named((buf), (size_t)(bytes), #buf) != 0) return TFIDF_E_NOMEM; \
    } while (0)
#define LCHK(x)                                              \
    do {                                                     \
        int l_ = (x);                                        \
        if (l_ == -2) return 1; /* arena too small: retry */ \
        LAUNCH(l_ < 0);                                      \
    } while (0)

static inline int arena_reset(tfidf_ctx* ctx, size_t want) {
    if (want > ctx->arena_buf.cap) {
        if (ctx->arena_buf.ensure(want) != 0) return TFIDF_E_NOMEM;
    }
    ctx->arena.base = (uint8_t*)ctx->arena_buf.p;
    ctx->arena.cap = ctx->arena_buf.cap;
    ctx->arena.used = 0;
    return 0;
}

/* the run's global df by term rank: the exchange's result, or with one rank the local df */
static inline uint32_t* df_of_run(tfidf_ctx* ctx) {
    return ctx->xp ? ctx->df_global.as<uint32_t>() : ctx->df_local.as<uint32_t>();
}
/* a launcher of kernels.h that returned non-zero: HIP's error when there is one, else TFIDF_E_HIP */
#define LAUNCH(x)                                  \
    do {                                           \
        if (x) {                                   \
            HIPCHK(hipGetLastError());             \
            return TFIDF_E_HIP;                    \
        }                                          \
    } while (0)

/* a scan of prims.h in the arena: -2 = the arena is too small */
#define SCAN(x)                                    \
    do {                                           \
        const int s_ = (x);                        \
        if (s_ == -2) return TFIDF_E_NOMEM;        \
        LAUNCH(s_);                                \
    } while (0)

static inline size_t scan_scratch(uint64_t n) { return (size_t)(n / 16) + 8192; }
/* the run's arena as a call's scratch of at least `want` bytes, emptied: between runs nothing of
 * a result lives in it (as format_prepare) */
static inline int arena_scratch(tfidf_ctx* ctx, size_t want) {
    if (want > ctx->arena_buf.cap && arena_reset(ctx, want) != 0) return -1;
    ctx->arena.used = 0;
    return 0;
}
static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

/* ---- what every add-on call starts and ends with ---- */

/* the CU count the launches over the result (kernels.h, *_WG_PER_CU) and the run's own persistent
 * kernels (K1, the score stage, emit.hip) are sized by: env TFIDF_GRID_CUS when it was set at
 * tfidf_open, else the device's; settled once per context */
static inline uint32_t ctx_ncu(tfidf_ctx* ctx) {
    if (!ctx->ncu) {
        int n = 0;
        if (ctx->grid_cus) n = (int)ctx->grid_cus;
        else if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || n <= 0) n = 256;
        ctx->ncu = (uint32_t)n;
    }
    return ctx->ncu;
}

/* the context's device, the call's events (created by the first call) and the CU count */
template <size_t NEV> static inline int call_begin(tfidf_ctx* ctx, Event (&ev)[NEV]) {
    HIPCHK(hipSetDevice(ctx->device));
    for (Event& e : ev)
        if (!e) HIPCHK(e.create());
    ctx_ncu(ctx);
    return TFIDF_OK;
}

/* ---- what a change of the result makes stale.  Every cache kept per result is a row here, and
 * every call that changes the result says which kind of change it made; a new cache adds its row
 * and its flag below and touches no other file.
 *
 *   cache (flag)                      SCORES   TERMS    NEW      RUN     filled by
 *   text, text_bytes (text_valid)       x                                 tfidf_format, write_output
 *   sm_norm (norm_valid)                x                                 sim_norms
 *   t_key, t_len (tmeta_valid)                   x                        ensure_term_meta
 *   dd_h0 (h0_valid)                             x                        dd_signatures
 *   nb_* model (nb_valid)                        x                        tfidf_nb_fit (which also resets it)
 *   bm25_L (bm25_L_valid)                                 x               tfidf_ctx_bm25_lengths
 *   have_result, have_model, model_only                   x               tfidf_run, tfidf_model_import
 *   have_info                                                      x      tfidf_run
 *
 *   tfidf_reweight      RC_SCORES                        (docSize, the ranks and the classifier's counts stay)
 *   tfidf_prune         RC_SCORES | RC_TERMS             (docSize stays: bm25_L does)
 *   tfidf_model_import  RC_SCORES | RC_TERMS | RC_NEW    (the last run's counters stay readable)
 *   tfidf_run           RC_SCORES | RC_TERMS | RC_NEW | RC_RUN
 * rw_idf (rw_idf_mode) and the active scheme (wt_*) are not caches of that kind: a run and an
 * import reset them where they succeed, tfidf_reweight sets them. ---- */
enum : unsigned {
    RC_SCORES = 1u,   /* the pairs' scores were rewritten */
    RC_TERMS = 2u,    /* terms were renumbered or removed, and pairs with them */
    RC_NEW = 4u,      /* another corpus or model takes the context: the old result is gone, also when the call fails */
    RC_RUN = 8u,      /* ... through tfidf_run, whose counters and timings go with it */
};
static inline void result_changed(tfidf_ctx* ctx, unsigned what) {
    if (what & RC_SCORES) ctx->text_valid = ctx->norm_valid = false;
    if (what & RC_TERMS) ctx->tmeta_valid = ctx->h0_valid = ctx->nb_valid = false;
    if (what & RC_NEW) ctx->have_result = ctx->have_model = ctx->model_only = ctx->bm25_L_valid = false;
    if (what & RC_RUN) ctx->have_info = false;
}
static inline double wall_ms(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
static inline double ev_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, a, b);
    return ms;
}
/* tfidf_last_*_info: the size-prefixed copy of the call's record, up to the caller's size */
template <typename T> static inline int copy_info(T* info, const T& last) {
    if (!info || info->size < sizeof(uint64_t)) return TFIDF_E_INVAL;
    const uint64_t n = info->size < sizeof(T) ? info->size : sizeof(T);
    T o = last;
    o.size = n;
    memcpy(info, &o, (size_t)n);
    return TFIDF_OK;
}

/* ---- engine.cpp: the idf table's workers (model import and the weighting tables post jobs) ---- */
void idf_post(tfidf_ctx* ctx, double* lut, uint64_t Nt, const uint32_t* vals, uint64_t n, uint32_t mode = TFIDF_IDF_REF);
int idf_pin_quiesce(tfidf_ctx* ctx);
void idf_join(tfidf_ctx* ctx);
/* idf_pin of at least n doubles (contents not kept); the caller has quiesced its uploads */
static inline int idf_pin_reserve(tfidf_ctx* ctx, size_t n) {
    if (ctx->idf_pin_n >= n) return TFIDF_OK;
    ctx->idf_pin_n = 0;
    if (ctx->idf_pin.alloc(n * 8) != hipSuccess) return TFIDF_E_NOMEM;
    ctx->idf_pin_n = n;
    return TFIDF_OK;
}
struct IdfJoin {
    tfidf_ctx* c;
    ~IdfJoin() { idf_join(c); }
};

/* ---- engine_query.cpp: what tfidf_query, tfidf_query_bm25 and tfidf_similar share on the host:
 * the group budget, the top-k rounds over a group's dense accumulators, the read-back ---- */
struct TopkPlan {
    uint64_t nsl0;      /* slices of the first round */
    uint64_t per_q;     /* bytes of accumulators and candidates per query (row) */
    uint64_t G;         /* queries (rows) per group */
    uint64_t cand_el;   /* entries of one candidate buffer */
};
/* a candidate buffer: cand_el score bits, cand_el ids, then the lists' lengths */
struct TopkCand {
    uint64_t* s;
    uint32_t* id;
    uint32_t* n;
};
TopkPlan topk_plan(uint32_t N, uint32_t k, uint32_t rows, uint64_t acc_bytes);
int topk_ensure(tfidf_ctx* ctx, const TopkPlan& p, uint32_t N);
int topk_rounds(tfidf_ctx* ctx, const TopkPlan& p, const double* acc, const uint32_t* cnt, uint32_t N, uint32_t k,
                uint32_t gn, unsigned long long* d_nm, TopkCand* res, const uint32_t* need = nullptr);
int topk_read_back(tfidf_ctx* ctx, const TopkCand& res, const unsigned long long* d_nm, uint32_t gn, uint32_t k,
                   uint64_t* h_s, uint32_t* h_id, uint32_t* h_n, uint64_t* h_nm);

/* ---- engine_text.cpp: corpus intake and token bounds (transform, analyze, n-grams) ---- */

/* The offsets of `in` on the host: its own array, or for a device corpus a copy in `copy` (one
 * round trip on the stream).  Checks what every caller checks: offsets where there are
 * documents, monotone, doc_off[ndocs] <= nbytes.  The rule about null bytes and the slot check
 * differ per call and stay with the callers. */
int corpus_offsets(tfidf_ctx* ctx, const tfidf_corpus& in, std::vector<uint64_t>& copy, const uint64_t** off);
/* Where the kernels read `in`: a device corpus where it is; of a host corpus the window
 * [off[0], off[N]) alone is staged, at its own offsets in `bytes`, and the offsets in `offs`. */
int stage_window(tfidf_ctx* ctx, const tfidf_corpus& in, const uint64_t* off, DevBuf& bytes, DevBuf& offs,
                 const uint8_t** d_bytes, const uint64_t** d_off);
/* the device tfidf_corpus a call hands back */
void corpus_out(tfidf_corpus* out, const tfidf_corpus& in, const uint8_t* bytes, uint64_t nbytes, const uint64_t* doc_off,
                const DevBuf& ids);

/* the upper bound of a slice's device scratch before its tokens are known: its bytes hold at
 * most one token per two bytes and one more per document (a document boundary ends a token);
 * per token 84 bytes of records, sort buffers and pairs */
constexpr uint64_t TR_TOKEN_BYTES = 84;
static inline uint64_t tr_max_tokens(uint64_t nbytes, uint64_t nd) {
    const uint64_t t = (nbytes + 1) / 2 + nd;
    return t < nbytes ? t : nbytes;
}
static inline uint64_t tr_a_bytes(uint64_t nbytes, uint64_t nd) {
    const uint64_t ntiles = nbytes / TR_TILE + 2;
    return (ntiles * (TR_TILE / 32u) + 1u) * 4u + 2 * (ntiles + 1) * 8 + nd * 8 + (nd + 1) * 8 + 4096;
}
static inline uint64_t tr_bound(uint64_t nbytes, uint64_t nd) {
    return tr_a_bytes(nbytes, nd) + tr_max_tokens(nbytes, nd) * TR_TOKEN_BYTES + 4096;
}
/* The token bounds of a slice: documents [d0, d1) = bytes [b0, b1) of a device corpus, filled in
 * by the caller.  token_scratch lays the document-start bitmap and the per-tile counts into
 * `scratch` behind `head` bytes that are the caller's (sl.status is their first word; the caller
 * zeroes what it keeps there before token_bounds) and returns the scratch's end.  token_bounds
 * marks, counts, scans and reads the totals back (one round trip): *T tokens; `who` names the
 * caller on the diagnostic line.  token_write writes the T starts and ends into the caller's
 * arrays; the arena is reset (grown to arena_want when smaller) for what the caller runs next. */
int token_scratch(tfidf_ctx* ctx, TrSlice& sl, DevBuf& scratch, size_t head, size_t* a_end);
int token_bounds(tfidf_ctx* ctx, const TrSlice& sl, const char* who, uint64_t* T);
int token_write(tfidf_ctx* ctx, TrSlice& sl, uint64_t* tok_start, uint64_t* tok_end, uint64_t T, size_t arena_want);

/* ---- engine_terms.cpp: the two preambles the calls over the result share ---- */
/* t_key / t_len of this result (launch_term_meta), once per result: tmeta_valid */
int ensure_term_meta(tfidf_ctx* ctx);
/* n document ids from the host into `ids` and their output positions (k_terms_lookup; UINT32_MAX:
 * not held) to d_pos, or when d_pos is null behind the ids in the same buffer.  Enqueued only:
 * event records and read-backs are the caller's. */
int lookup_ids(tfidf_ctx* ctx, DevBuf& ids, const uint32_t* host_ids, uint32_t n, uint32_t* d_pos);

/* ---- engine_prune.cpp ---- */
int ensure_spare(DevBuf& spare, const DevBuf& orig, size_t need);

/* ---- engine_weight.cpp: a transform slice's rows are scored by reweight.hip when a scheme other
 * than the reference's is active ---- */
enum { RWM_BIG = 0, RWM_ZERO = 1, RWM_CMAX = 2, RWM_NLIST = 3 };   /* rw_misc's words */
int rw_cmax_launch(tfidf_ctx* ctx, const uint32_t* count, uint64_t n, const uint32_t* n_dev);
int rw_tf_finish(tfidf_ctx* ctx, uint32_t cmax, uint32_t nlist, uint32_t* nlisted, uint64_t* nlogs);
void rw_scheme_args(tfidf_ctx* ctx, RwArgs& a, uint32_t tf, uint32_t norm, uint32_t nlisted);

/* ---- engine_similar.cpp: sq and norm by output position, once per run (tfidf_kmeans reads them) ---- */
int sim_norms(tfidf_ctx* ctx, tfidf_similar_info& si);

#endif
