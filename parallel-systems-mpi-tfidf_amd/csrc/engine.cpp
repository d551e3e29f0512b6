/*
 * engine.cpp — C-ABI implementation (include/tfidf.h): context, HBM buffers, stage
 * orchestration on one HIP stream, RCCL exchange, result fetch.
 *
 * Pipeline of tfidf_run (reference lines replaced in brackets):
 *   K0 plan chunks                                       [TFIDF.c:125-130 doc->rank split]
 *   K1 tokenize + LDS-hash count + global vocabulary     [TFIDF.c:130-196]
 *   vocabulary ranking (radix sort of strcmp keys)        [TFIDF.c:227-234 linear joins]
 *   partial-document merge (radix sort + reduce-by-key)
 *   DF histogram                                          [TFIDF.c:169-188,291-326]
 *   RCCL: identity-key all-gather + DF all-reduce         [TFIDF.c:209-222 MPI_Reduce/Bcast]
 *   idf LUT over the distinct df values, host libm log    [TFIDF.c:243]
 *   document order + per-document term sort + score       [TFIDF.c:202,244-245,253-273]
 * No stage has a CPU fallback: a missing device or HIP error is returned as an error.
 */
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/tfidf.h"
#include "kernels.h"
#include "analyze_tab.h"
#include "synth.h"
#include "xport.h"

extern "C" void tfidf_synth_spec(syn_spec* s, uint64_t seed, uint32_t V, uint32_t mode, const double* cdf);

namespace {

/* every device allocation of the engine goes through dev_malloc: the counters behind
 * tfidf_run_info.device_allocs / device_alloc_bytes (a steady-state run makes none) */
std::atomic<uint64_t> g_dev_allocs{0}, g_dev_alloc_bytes{0};

}  // namespace

hipError_t tfidf_dev_malloc(void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) {
        g_dev_allocs.fetch_add(1, std::memory_order_relaxed);
        g_dev_alloc_bytes.fetch_add(bytes, std::memory_order_relaxed);
    }
    return e;
}

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap && p) return 0;
        const bool regrow = p != nullptr;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        /* 1/8 headroom (at least 4 KiB) on the first allocation, 1/2 on a regrowth: sizes
         * that vary from run to run (the record totals after K1's overflow records, the
         * partial-record sort buffers: K1's overflow mode depends on the order in which
         * workgroups claim LDS entries) must not reallocate in steady state — hipFree
         * synchronises the device and a 1 GB hipMalloc inside a stage left the GPU idle for
         * ~0.7 ms (the bench counts allocations in its timed steps).  Near the HBM capacity
         * the headroom is dropped rather than failing a size that fits exactly. */
        const size_t head = regrow ? bytes / 2 : bytes / 8;
        const size_t want = bytes < 256 ? 256 : bytes + (head > 4096 ? head : 4096);
        if (tfidf_dev_malloc(&p, want) == hipSuccess) { cap = want; return 0; }
        (void)hipGetLastError();
        p = nullptr;
        if (want != bytes && tfidf_dev_malloc(&p, bytes) == hipSuccess) { cap = bytes; return 0; }
        (void)hipGetLastError();
        p = nullptr;
        return -1;
    }
    /* grow preserving the first `keep` bytes */
    int grow_keep(size_t bytes, size_t keep, hipStream_t s) {
        if (bytes <= cap && p) return 0;
        void* q = nullptr;
        if (tfidf_dev_malloc(&q, bytes) != hipSuccess) return -1;
        if (p && keep) {
            if (hipMemcpyAsync(q, p, keep, hipMemcpyDeviceToDevice, s) != hipSuccess) return -1;
            if (hipStreamSynchronize(s) != hipSuccess) return -1;
        }
        if (p) (void)hipFree(p);
        p = q;
        cap = bytes;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <typename T> T* as() const { return (T*)p; }
};

enum Stage { S_PREP, S_TOKCOUNT, S_VOCAB, S_MERGE, S_DF, S_EXCHANGE, S_IDF, S_ORDER, S_SCORE, S_NSTAGES };
const char* kStageNames[S_NSTAGES] = {"prep", "tokcount", "vocab", "merge", "df", "exchange", "idf", "order", "score"};

}  // namespace

struct tfidf_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
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
    K1Out* k1out_host = nullptr;   /* pinned: tokcount_sl's output block, copied to k1out_dev per run */
    DevBuf k1out_dev;
    bool k1out_valid = false;      /* k1out_dev holds *k1out_host (the copy is skipped when a run's block is the same) */
    hipEvent_t ev[S_NSTAGES + 1];
    Arena arena;
    DevBuf arena_buf;
    /* side stream: the document-order sort (needs only the document ids) runs beside the
     * vocabulary / merge / DF stages, after K1 (K1's persistent grid wants every CU) */
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_order = nullptr;
    hipEvent_t ev_spin = nullptr;   /* the run's host waits (spin_sync) */
    uint64_t wait_token = 0;        /* the last completion token of a status-words kernel (words_wait) */
    hipStream_t stream3 = nullptr;  /* the idf table's upload, beside the merge / DF stages */
    hipEvent_t ev_idf_up = nullptr;
    bool idf_early = false;         /* this run's table is on its way up stream3 (run_post waits on ev_idf_up) */
    /* split DF (runs with partial records): the main records' histogram runs on stream2
     * beside the merge stage, the merged records' is added on the main stream after it */
    bool df_split = true;           /* env TFIDF_DF_SPLIT=0: one DF pass after the merge */
    hipEvent_t ev_vrank = nullptr, ev_dfmain = nullptr;
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
    uint64_t* hpin = nullptr;
    uint64_t* hpin_dev = nullptr;   /* hpin as the device addresses it (status words written by kernels) */
    DevBuf dense, vslot, skey0, skey1, seq0, seq1, rank_of_slot, slot_of_rank, rank16;
    DevBuf pkey0, pkey1, pseq0, pseq1, phead;
    DevBuf big_list, big_idx, dense_cnt, kcnt, tile_cnt;   /* dense merge of long documents */
    DevBuf df_local, df_global, present, idf_vals;
    uint64_t idf_full_n = 0;   /* idf_vals holds log(N/df) for df = 0..N of this N (0: not) */
    /* the per-run idf table (N <= IDF_FULL_MAX): host threads fill the pinned idf_pin with
     * log(N/df) for df = 0..N while the device runs the stages before the score; run_post
     * joins them and uploads it (every run: round 4's per-N cache was retired in round 6) */
    double* idf_pin = nullptr;
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
    hipEvent_t ev_q[3] = {};                    /* lookup / score / top-k bounds (created by the first query) */
    uint32_t ncu = 0;
    tfidf_query_info qinfo{};
    /* BM25 ranking (tfidf_query_bm25, bm25.hip): tfidf_query's buffers; L = the sum of doc_size
     * over this context's documents, kept until the next run */
    uint64_t bm25_L = 0;
    bool bm25_L_valid = false;
    tfidf_bm25_info binfo{};
    /* per-document top-k terms (tfidf_top_terms, terms.hip): the requested ids and their output
     * positions, a batch's per-row words (npairs, nterms, id), its k entries per row (score
     * bits, pair, term, count, word length -> offset), the gathered words, the list of long
     * documents */
    DevBuf tm_ids, tm_rows, tm_score, tm_pair, tm_term, tm_cnt, tm_woff, tm_words, tm_big;
    uint64_t terms_bytes = 256ull << 20;        /* env TFIDF_TERMS_MB: device result buffers of a batch of rows */
    hipEvent_t ev_t[5] = {};                    /* lookup or select / scan / gather bounds (created by the first call) */
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
    hipEvent_t ev_s[6] = {};                    /* norms / table / score / top-k bounds (created by the first call) */
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
    hipEvent_t ev_k[4] = {};                    /* assign / update / top-term bounds (created by the first call) */
    tfidf_kmeans_info kinfo{};
    /* unseen documents against the resident model (tfidf_transform, transform.hip): a host
     * batch's bytes and offsets, a slice's boundary scratch (document-start bitmap, per-tile
     * counts, per-document words) and its token and pair arrays */
    DevBuf tr_bytes, tr_off, tr_a, tr_b;
    uint64_t transform_bytes = 512ull << 20;    /* env TFIDF_TRANSFORM_MB: device scratch of a slice */
    hipEvent_t ev_tr[5] = {};                   /* tokens / resolve / sort / pairs bounds (created by the first call) */
    tfidf_transform_info trinfo{};
    /* the portable model (tfidf_model_import / tfidf_model_export, model.hip).  have_model: the
     * context holds what tfidf_transform reads (table, ranks, df, idf, V, N), from a run or from
     * an import.  model_only: from an import; the uploaded term bytes (m_blob, m_blob_bytes)
     * stand where the run's corpus does (dev_bytes / corpus.nbytes) and m_off holds the term
     * offsets, so the term table is those two buffers.  m_stat: the build's status word. */
    bool have_model = false, model_only = false;
    DevBuf m_off, m_blob, m_stat;
    uint64_t m_blob_bytes = 0;
    hipEvent_t ev_m[2] = {};                    /* clear + build bounds (created by the first import) */
    tfidf_model_info minfo{};
    /* the analyzer (tfidf_analyze, analyze.hip): a host input's staged bytes; per slot the
     * analyzed bytes and the context's copies of the offsets and ids; the document-start bitmap,
     * the stop-word table and the blanked-token counter of the call in flight */
    DevBuf an_in, an_bytes[2], an_off[2], an_ids[2], an_dstart, an_tab, an_cnt;
    hipEvent_t ev_an[2] = {};                   /* the kernels' bounds (created by the first call) */
    tfidf_analyze_info aninfo{};
    /* word n-grams (tfidf_ngrams, ngram.hip): a host input's staged bytes and offsets; per slot
     * the output bytes, the new offsets and the context's copy of the ids; the boundary scratch
     * (status, gram counter, bitmap, per-tile counts), the 24 bytes per token (start, end,
     * segment offset) and the write kernel's tile index of the call in flight */
    DevBuf ng_in, ng_inoff, ng_bytes[2], ng_off[2], ng_ids[2], ng_a, ng_b, ng_tseg;
    hipEvent_t ev_ng[4] = {};                   /* bounds / sizes / write bounds (created by the first call) */
    tfidf_ngram_info nginfo{};
    /* vocabulary pruning (tfidf_prune, prune.hip): the keep flags (then the new ranks), the keep
     * bitmap, the max_features sort's ping-pong buffers, the per-tile counts and first documents,
     * the emptied-documents counter; and the spare copies of the resident arrays the call writes
     * into and swaps with the context's own when every step has succeeded (slot_of_rank, df by
     * rank, out_term, out_cnt, out_score, out_off), each as large as the buffer it stands in for */
    DevBuf pr_flag, pr_bits, pr_k0, pr_k1, pr_v0, pr_v1, pr_tcnt, pr_tdoc, pr_misc;
    DevBuf pr_sor, pr_df, pr_term, pr_cnt, pr_score, pr_off;
    hipEvent_t ev_pr[4] = {};                   /* select / terms / pairs bounds (created by the first call) */
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
    hipEvent_t ev_rw[3] = {};                   /* tables / pairs bounds (created by the first call) */
    tfidf_reweight_info rwinfo{};
#define WR_NBUF 8
#define WR_BUF (16ull << 20)
#define WR_GROUPS 8
    uint8_t* wr_buf[WR_NBUF] = {};   /* pinned output staging ring */
    hipEvent_t wr_ev[WR_NBUF] = {};
    hipEvent_t wr_fmt[WR_GROUPS] = {};
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
    double ms_stage[S_NSTAGES] = {0};
    double ms_total = 0;
    hipError_t last_err = hipSuccess;
};
static void idf_pool_stop(tfidf_ctx* ctx);   /* the per-run idf table's workers (idf_start) */
static bool idf_done(tfidf_ctx* ctx);
static void idf_join(tfidf_ctx* ctx);
/* open contexts in this process: the idf workers of all of them share IDF_POOL threads' worth
 * of work (a group of K shards in one process would otherwise start 8 K of them) */
static std::atomic<int> g_live_ctx{0};

#define HIPCHK(x)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            ctx->last_err = e_;                                                            \
            fprintf(stderr, "tfidf: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
            return TFIDF_E_HIP;                                                            \
        }                                                                                  \
    } while (0)
/* a wait for the run's stream once collectives may be in it: through the transport, so
 * that a failed peer cannot leave this rank waiting (xport.h, comm_rank.h) */
#define XSYNC(s_)                                                                          \
    do {                                                                                   \
        if (ctx->xp) {                                                                     \
            const int w_ = ctx->xp->wait(s_);                                              \
            if (w_) return w_;                                                             \
        } else {                                                                           \
            HIPCHK(spin_sync(ctx, s_));                                                    \
        }                                                                                  \
    } while (0)
/* TFIDF_DEBUG_ALLOC=1: every (re)allocation of a stage buffer is named on stderr (which
 * buffer still grows after the warm-up runs) */
static int debug_alloc() {
    static const int on = [] { const char* e = getenv("TFIDF_DEBUG_ALLOC"); return e && e[0] == '1'; }();
    return on;
}
static int ensure_named(DevBuf& b, size_t bytes, const char* name) {
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
        if (l_ < 0) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; } \
    } while (0)

static int arena_reset(tfidf_ctx* ctx, size_t want) {
    if (want > ctx->arena_buf.cap) {
        if (ctx->arena_buf.ensure(want) != 0) return TFIDF_E_NOMEM;
    }
    ctx->arena.base = (uint8_t*)ctx->arena_buf.p;
    ctx->arena.cap = ctx->arena_buf.cap;
    ctx->arena.used = 0;
    return 0;
}

/* each event record costs the stream ~5 us (scripts/micro/host_api_cost.hip): level 2 records
 * only the four K1 and whole-run bounds */
static void mark(tfidf_ctx* ctx, int stage) {
    if (ctx->timing == 1 ||
        (ctx->timing == 2 && (stage == S_PREP || stage == S_TOKCOUNT || stage == S_VOCAB || stage == S_NSTAGES)))
        (void)hipEventRecord(ctx->ev[stage], ctx->stream);
}

/* Status words into hpin (launch_words_to_host at hpin_dev + at) and the wait for them: in
 * a single-context process the kernel also writes a completion token after the words and
 * the host polls that word in pinned memory — no event record on the stream (~5 us each) and
 * no blocking wake-up; bounded (2 s, then the stream is synchronised, which also reports a
 * failed kernel).  Several contexts in the process: the stream is synchronised. */
static hipError_t words_wait(tfidf_ctx* ctx, WordList& wl, uint32_t at, hipStream_t s) {
    const bool poll = g_live_ctx.load() <= 1;
    wl.token = poll ? (0x7A5E000000000000ull | ++ctx->wait_token) : 0ull;
    if (launch_words_to_host(wl, ctx->hpin_dev + at, s)) return hipErrorLaunchFailure;
    if (!poll) return hipStreamSynchronize(s);
    volatile uint64_t* tok = ctx->hpin + at + wl.n;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t it = 0; *tok != wl.token; ++it) {
        if ((it & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            const hipError_t e = hipStreamSynchronize(s);
            if (e != hipSuccess) return e;
            return *tok == wl.token ? hipSuccess : hipErrorUnknown;
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return hipSuccess;
}

/* the run's global df by term rank: the exchange's result, or with one rank the local df */
static uint32_t* df_of_run(tfidf_ctx* ctx) {
    return ctx->xp ? ctx->df_global.as<uint32_t>() : ctx->df_local.as<uint32_t>();
}

/* The run's waits for its own stream (K1's counters, the final status): the host polls an
 * event instead of blocking in hipStreamSynchronize, whose wake-up after a millisecond-long
 * kernel left the device idle for tens of microseconds before the next launches. */
static hipError_t spin_sync(tfidf_ctx* ctx, hipStream_t s) {
    if (g_live_ctx.load() > 1) return hipStreamSynchronize(s);   /* several ranks' threads in this process */
    hipError_t e = hipEventRecord(ctx->ev_spin, s);
    if (e != hipSuccess) return e;
    while ((e = hipEventQuery(ctx->ev_spin)) == hipErrorNotReady) {
    }
    return e;
}

extern "C" {

int tfidf_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0 ? n : 0;
}

int tfidf_open(int device, tfidf_ctx** out) {
    if (!out) return TFIDF_E_INVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return TFIDF_E_NODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return TFIDF_E_NODEV;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fprintf(stderr, "tfidf: device %d is %s, need gfx950\n", device, prop.gcnArchName);
        return TFIDF_E_NODEV;
    }
    if (hipSetDevice(device) != hipSuccess) return TFIDF_E_NODEV;
    tfidf_ctx* ctx = new tfidf_ctx();
    ctx->device = device;
    const char* km = getenv("TFIDF_K1");
    if (km && !strcmp(km, "general")) ctx->k1_mode = 2;
    if (km && !strcmp(km, "vs")) ctx->k1_mode = 1;
    if (km && !strcmp(km, "sl")) ctx->k1_mode = 3;
    {
        const char* sm = getenv("TFIDF_SL_MAXCAP");
        const unsigned long long v = sm ? strtoull(sm, nullptr, 0) : 0ull;
        if (v >= 1024 && v <= K1_SL_MAX_CAP) ctx->sl_maxcap = v;
    }
    const char* ks = getenv("TFIDF_STAMPS");
    ctx->stamps_on = ks && ks[0] == '1';
    const char* kx = getenv("TFIDF_TEST_XFAIL_RANK");
    ctx->xfail_rank = kx ? atoi(kx) : -1;
    const char* kxm = getenv("TFIDF_XCHG");
    if (kxm && !strcmp(kxm, "owner")) ctx->xchg_mode = 1;
    if (kxm && !strcmp(kxm, "dense")) ctx->xchg_mode = 2;
    if (kxm && !strcmp(kxm, "dense_table")) ctx->xchg_mode = 3;
    const char* kxa = getenv("TFIDF_XAGG");
    ctx->xagg_table = kxa && !strcmp(kxa, "table");
    const char* kxb = getenv("TFIDF_XB_STAGE_MAX");
    ctx->xb_stage_max = kxb ? (uint32_t)atoi(kxb) : ~0u;
    const char* kds = getenv("TFIDF_DF_SPLIT");
    ctx->df_split = !(kds && !strcmp(kds, "0"));
    const char* kq = getenv("TFIDF_QUERY_ACC_MB");
    if (kq) {
        const unsigned long long mb = strtoull(kq, nullptr, 0);
        if (mb >= 1 && mb <= (1ull << 20)) ctx->query_acc_bytes = mb << 20;
    }
    const char* kt = getenv("TFIDF_TERMS_MB");
    if (kt) {
        const unsigned long long mb = strtoull(kt, nullptr, 0);
        if (mb >= 1 && mb <= (1ull << 20)) ctx->terms_bytes = mb << 20;
    }
    const char* ktr = getenv("TFIDF_TRANSFORM_MB");
    if (ktr) {
        const unsigned long long mb = strtoull(ktr, nullptr, 0);
        if (mb >= 1 && mb <= (1ull << 20)) ctx->transform_bytes = mb << 20;
    }
    const char* kkm = getenv("TFIDF_KMEANS_MB");
    if (kkm) {
        const unsigned long long mb = strtoull(kkm, nullptr, 0);
        if (mb >= 1 && mb <= (1ull << 20)) ctx->kmeans_bytes = mb << 20;
    }
    const char* kks = getenv("TFIDF_KMEANS_SPLIT");
    if (kks) {
        const unsigned long sp = strtoul(kks, nullptr, 0);
        if (sp >= 1 && sp <= 1024) ctx->kmeans_split = (uint32_t)sp;
    }
    const char* kag = getenv("TFIDF_AN_GRID");
    if (kag) {
        const unsigned long ag = strtoul(kag, nullptr, 0);
        if (ag >= 1 && ag <= 65536) ctx->an_grid = (uint32_t)ag;
    }
    const char* kn = getenv("TFIDF_TEST_XNOMEM_RANK");
    ctx->xnomem_rank = kn ? atoi(kn) : -1;
    /* diagnostics: initial vocabulary capacity (power of two) and the loads it may reach
     * before the run is repeated with a larger table (TFIDF_VLOAD percent below 16M slots,
     * default 12; TFIDF_VLOAD_BIG from 16M slots on, default 45) */
    const char* kv = getenv("TFIDF_VCAP");
    if (kv) {
        uint64_t c = strtoull(kv, nullptr, 0);
        if (c >= 1024 && (c & (c - 1)) == 0) ctx->vcap = c;
    }
    const char* kb = getenv("TFIDF_VLOAD_BIG");
    if (kb) {
        uint32_t l = (uint32_t)strtoul(kb, nullptr, 0);
        if (l >= 10 && l <= 90) ctx->vload_big_pct = l;
    }
    const char* kl = getenv("TFIDF_VLOAD");
    if (kl) {
        uint32_t l = (uint32_t)strtoul(kl, nullptr, 0);
        if (l >= 10 && l <= 90) ctx->vload_pct = l;
    }
    HIPCHK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&ctx->stream3, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ctx->ev_order, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ctx->ev_spin, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ctx->ev_idf_up, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ctx->ev_vrank, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ctx->ev_dfmain, hipEventDisableTiming));
    for (int i = 0; i <= S_NSTAGES; ++i) HIPCHK(hipEventCreate(&ctx->ev[i]));
    if (arena_reset(ctx, 64ull << 20) != 0) { delete ctx; return TFIDF_E_NOMEM; }
    if (ctx->counters.ensure(256) != 0) { delete ctx; return TFIDF_E_NOMEM; }
    /* coherent: the status words a kernel writes (and its completion token) reach the host
     * without a cache flush at the kernel's end */
    if (hipHostMalloc((void**)&ctx->hpin, 256, hipHostMallocCoherent) != hipSuccess) { delete ctx; return TFIDF_E_NOMEM; }
    if (hipHostGetDevicePointer((void**)&ctx->hpin_dev, ctx->hpin, 0) != hipSuccess || !ctx->hpin_dev) {
        delete ctx;
        return TFIDF_E_NOMEM;
    }
    if (hipHostMalloc((void**)&ctx->k1out_host, sizeof(K1Out), hipHostMallocDefault) != hipSuccess ||
        ctx->k1out_dev.ensure(sizeof(K1Out)) != 0) { delete ctx; return TFIDF_E_NOMEM; }
    g_live_ctx.fetch_add(1);
    *out = ctx;
    return TFIDF_OK;
}

void tfidf_close(tfidf_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    delete ctx->xp;
    if (ctx->stream2) { (void)hipStreamSynchronize(ctx->stream2); (void)hipStreamDestroy(ctx->stream2); }
    if (ctx->stream3) { (void)hipStreamSynchronize(ctx->stream3); (void)hipStreamDestroy(ctx->stream3); }
    if (ctx->ev_idf_up) (void)hipEventDestroy(ctx->ev_idf_up);
    if (ctx->ev_vrank) (void)hipEventDestroy(ctx->ev_vrank);
    if (ctx->ev_dfmain) (void)hipEventDestroy(ctx->ev_dfmain);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_spin) (void)hipEventDestroy(ctx->ev_spin);
    if (ctx->ev_order) (void)hipEventDestroy(ctx->ev_order);
    idf_pool_stop(ctx);
    g_live_ctx.fetch_sub(1);
    if (ctx->idf_pin) (void)hipHostFree(ctx->idf_pin);
    for (int i = 0; i < WR_NBUF; ++i) {
        if (ctx->wr_buf[i]) (void)hipHostFree(ctx->wr_buf[i]);
        if (ctx->wr_ev[i]) (void)hipEventDestroy(ctx->wr_ev[i]);
    }
    for (int i = 0; i < WR_GROUPS; ++i)
        if (ctx->wr_fmt[i]) (void)hipEventDestroy(ctx->wr_fmt[i]);
    ctx->arena2_buf.release();
    ctx->df_scratch.release();
    for (hipEvent_t e : ctx->ev_q)
        if (e) (void)hipEventDestroy(e);
    for (DevBuf* b : {&ctx->q_terms, &ctx->q_rank, &ctx->q_tab, &ctx->q_acc, &ctx->q_cnt, &ctx->q_big, &ctx->q_cand0,
                      &ctx->q_cand1, &ctx->q_misc})
        b->release();
    for (hipEvent_t e : ctx->ev_t)
        if (e) (void)hipEventDestroy(e);
    for (DevBuf* b : {&ctx->tm_ids, &ctx->tm_rows, &ctx->tm_score, &ctx->tm_pair, &ctx->tm_term, &ctx->tm_cnt, &ctx->tm_woff,
                      &ctx->tm_words, &ctx->tm_big})
        b->release();
    for (hipEvent_t e : ctx->ev_s)
        if (e) (void)hipEventDestroy(e);
    for (DevBuf* b : {&ctx->sm_norm, &ctx->sm_ids, &ctx->sm_rows, &ctx->sm_mask, &ctx->sm_cnt, &ctx->sm_off, &ctx->sm_pw,
                      &ctx->sm_res, &ctx->sm_escore, &ctx->sm_xterm, &ctx->sm_xscore, &ctx->sm_xwoff, &ctx->sm_xwords,
                      &ctx->sm_xoff})
        b->release();
    for (hipEvent_t e : ctx->ev_k)
        if (e) (void)hipEventDestroy(e);
    for (DevBuf* b : {&ctx->km_C, &ctx->km_work, &ctx->km_top, &ctx->km_words}) b->release();
    for (hipEvent_t e : ctx->ev_tr)
        if (e) (void)hipEventDestroy(e);
    for (DevBuf* b : {&ctx->tr_bytes, &ctx->tr_off, &ctx->tr_a, &ctx->tr_b}) b->release();
    for (hipEvent_t e : ctx->ev_m)
        if (e) (void)hipEventDestroy(e);
    for (DevBuf* b : {&ctx->m_off, &ctx->m_blob, &ctx->m_stat}) b->release();
    for (hipEvent_t e : ctx->ev_an)
        if (e) (void)hipEventDestroy(e);
    for (DevBuf* b : {&ctx->an_in, &ctx->an_bytes[0], &ctx->an_bytes[1], &ctx->an_off[0], &ctx->an_off[1], &ctx->an_ids[0],
                      &ctx->an_ids[1], &ctx->an_dstart, &ctx->an_tab, &ctx->an_cnt})
        b->release();
    for (hipEvent_t e : ctx->ev_ng)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->ev_pr)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->ev_rw)
        if (e) (void)hipEventDestroy(e);
    for (DevBuf* b : {&ctx->rw_idf, &ctx->rw_lut, &ctx->rw_list, &ctx->rw_listv, &ctx->rw_big, &ctx->rw_misc}) b->release();
    for (DevBuf* b : {&ctx->pr_flag, &ctx->pr_bits, &ctx->pr_k0, &ctx->pr_k1, &ctx->pr_v0, &ctx->pr_v1, &ctx->pr_tcnt,
                      &ctx->pr_tdoc, &ctx->pr_misc, &ctx->pr_sor, &ctx->pr_df, &ctx->pr_term, &ctx->pr_cnt, &ctx->pr_score,
                      &ctx->pr_off})
        b->release();
    for (DevBuf* b : {&ctx->ng_in, &ctx->ng_inoff, &ctx->ng_bytes[0], &ctx->ng_bytes[1], &ctx->ng_off[0], &ctx->ng_off[1],
                      &ctx->ng_ids[0], &ctx->ng_ids[1], &ctx->ng_a, &ctx->ng_b, &ctx->ng_tseg})
        b->release();
    DevBuf* bufs[] = {&ctx->arena_buf, &ctx->in_bytes, &ctx->in_off, &ctx->in_ids, &ctx->syn_bytes, &ctx->syn_off,
                      &ctx->syn_ids, &ctx->syn_ntok, &ctx->syn_blkfirst, &ctx->syn_blkbytes, &ctx->syn_cdf,
                      &ctx->chunk_start, &ctx->chunk_doc, &ctx->vkeys, &ctx->vrep, &ctx->rec_slot, &ctx->rec_cnt,
                      &ctx->part_doc, &ctx->part_slot, &ctx->part_cnt, &ctx->doc_recoff, &ctx->doc_npairs,
                      &ctx->doc_size, &ctx->doc_flags, &ctx->counters, &ctx->dense, &ctx->vslot, &ctx->skey0,
                      &ctx->skey1, &ctx->seq0, &ctx->seq1, &ctx->rank_of_slot, &ctx->slot_of_rank, &ctx->rank16, &ctx->pkey0,
                      &ctx->pkey1, &ctx->pseq0, &ctx->pseq1, &ctx->phead, &ctx->df_local, &ctx->df_global,
                      &ctx->present, &ctx->idf_vals, &ctx->dkey0, &ctx->dkey1, &ctx->dseq0, &ctx->dseq1,
                      &ctx->npairs_ord, &ctx->out_off, &ctx->doc_meta, &ctx->t_key, &ctx->t_len, &ctx->doc_tbytes,
                      &ctx->doc_toff, &ctx->text, &ctx->out_term, &ctx->out_cnt,
                      &ctx->out_score, &ctx->idf_rank, &ctx->large_list, &ctx->split_tasks, &ctx->cls_off, &ctx->x_mine, &ctx->x_srec,
                      &ctx->x_sidx, &ctx->x_back, &ctx->x_cnt, &ctx->x_rrec, &ctx->x_rslot, &ctx->x_reply, &ctx->x_gkeys,
                      &ctx->x_pos, &ctx->x_dense, &ctx->x_lloc, &ctx->x_lsend, &ctx->x_lgath, &ctx->x_ltab,
                      &ctx->x_tkey, &ctx->x_tdf, &ctx->stamps, &ctx->big_list, &ctx->big_idx, &ctx->dense_cnt, &ctx->kcnt,
                      &ctx->tile_cnt};
    for (DevBuf* b : bufs) b->release();
    for (int i = 0; i <= S_NSTAGES; ++i) (void)hipEventDestroy(ctx->ev[i]);
    if (ctx->hpin) (void)hipHostFree(ctx->hpin);
    if (ctx->k1out_host) (void)hipHostFree(ctx->k1out_host);
    ctx->k1out_dev.release();
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int tfidf_set_timing(tfidf_ctx* ctx, int enable) {
    if (!ctx) return TFIDF_E_INVAL;
    ctx->timing = enable == 2 ? 2 : (enable != 0 ? 1 : 0);
    return TFIDF_OK;
}

const char* tfidf_stage_name(int stage) { return (stage >= 0 && stage < S_NSTAGES) ? kStageNames[stage] : "?"; }

int tfidf_comm_unique_id(uint8_t id[TFIDF_UNIQUE_ID_BYTES]) {
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return TFIDF_E_RCCL;
    memcpy(id, &u, TFIDF_UNIQUE_ID_BYTES);
    return TFIDF_OK;
}

int tfidf_comm_init(tfidf_ctx* ctx, const uint8_t id[TFIDF_UNIQUE_ID_BYTES], int rank, int nranks) {
    /* ranks <= 1024: the DF exchange's per-owner counts live in LDS (k_owner_count) */
    if (!ctx || !id || nranks < 1 || nranks > 1024 || rank < 0 || rank >= nranks) return TFIDF_E_INVAL;
    HIPCHK(hipSetDevice(ctx->device));
    tfidf_ctx_attach_xport(ctx, nullptr);
    static_assert(sizeof(ncclUniqueId) == TFIDF_UNIQUE_ID_BYTES, "unique id size");
    Xport* x = nullptr;
    const int rc = rccl_init_rank(id, rank, nranks, ctx->device, &x);
    if (rc) return rc;
    return tfidf_ctx_attach_xport(ctx, x);
}

}  // extern "C"

int tfidf_ctx_attach_xport(tfidf_ctx* ctx, Xport* xp) {
    if (!ctx) { delete xp; return TFIDF_E_INVAL; }
    delete ctx->xp;
    ctx->xp = xp;
    ctx->rank = xp ? xp->rank : 0;
    ctx->nranks = xp ? xp->nranks : 1;
    return TFIDF_OK;
}
int tfidf_ctx_device(const tfidf_ctx* ctx) { return ctx->device; }
hipStream_t tfidf_ctx_stream(const tfidf_ctx* ctx) { return ctx->stream; }

/* ------------------------------------------------------------------------------ */

/* ---- the DF exchange (replaces MPI_Reduce(CustomReduce) + MPI_Bcast, TFIDF.c:209-222,
 * 291-326).  Every rank enters it once per attempt, also when its local stages failed or
 * asked for a retry, so the ranks always agree:
 *   1. words(status, V): any error -> every rank returns an error (its own, or
 *      TFIDF_E_PEER); any retry -> every rank returns 1 and repeats the run in step.  Every
 *      rank learns every rank's V, which sizes everything after it.
 *   2. one of two forms (the same results; TFIDF_XCHG=owner|dense forces one):
 *      dense  (every rank's V <= DENSE_XCHG_MAXV: c2, c3, c5) — north_star's form: the
 *             ranks' term keys are all-gathered (padded to the largest V), every rank numbers
 *             the distinct keys identically, scatters its local df into a dense vector over
 *             those numbers, and ONE all-reduce (sum) gives every rank the global df; global
 *             V = the distinct keys.  The numbering: when no rank holds terms of >= 16 bytes
 *             (a flag in step 1's word) each gathered list is in term order and a key's
 *             number is its position in the merged lists (binary searches, no table:
 *             launch_dense_merge_ids); otherwise its smallest gathered position, from a hash
 *             table of all gathered keys (TFIDF_XCHG=dense_table forces this).  Buffers are sized
 *             before step 1 from the rank's own V (padded by a quarter), so their allocation
 *             status travels in step 1's word; only when the largest V exceeds some rank's
 *             padding do all ranks grow them and agree once more.  Then one all-gather and
 *             one all-reduce: one host synchronisation in all (step 1's).
 *      owner  (larger V: c4) — SURVEY §8e's hash-owner partitioning: every term goes to an
 *             owner rank (a hash of its key); the per-owner counts are all-gathered together
 *             with each rank's allocation status (an allocation failure is agreed there, no
 *             extra exchange), one all-to-all sends 20-byte (key, local df) records, each owner
 *             sums equal keys (LDS tables over hash buckets of the received records; an HBM
 *             hash table with TFIDF_XAGG=table) and one all-to-all returns the global df of
 *             each record plus, per sender, the owner's distinct-key count (global V = their sum).
 *             Per rank ~V entries move; the owner aggregates ~ΣV/R.
 *   Global V stays on the device and is read with the run's final status (no host round
 *   trip of its own).  From step 2 on no stage of the run returns "retry" (run_local checked
 *   the post-exchange stages' scratch before step 1); an error inside a collective sequence
 *   aborts the transport (releasing the peers), an agreed failure does not. */
static uint64_t status_word(int rc) { return rc < 0 ? 0x100ull | (uint64_t)(-rc) : (uint64_t)rc; }

static size_t scan_scratch(uint64_t n) { return (size_t)(n / 16) + 8192; }

#define DENSE_XCHG_MAXV (1u << 17)

/* words(status, v) over the ranks: 0 all fine, 1 retry (some rank asked), <0 an error (this
 * rank's own, else TFIDF_E_PEER); vs (optional) = every rank's v */
static int exchange_agree(tfidf_ctx* ctx, int local_rc, uint64_t v, std::vector<uint64_t>* vs) {
    Xport* xp = ctx->xp;
    std::vector<uint64_t> all(2 * (size_t)xp->nranks);
    const uint64_t mine[2] = {status_word(local_rc), v};
    const int rc = xp->words(mine, all.data(), ctx->stream);
    if (rc) return rc;
    uint64_t worst = 0;
    if (vs) vs->assign((size_t)xp->nranks, 0);
    for (int r = 0; r < xp->nranks; ++r) {
        worst = all[2 * r] > worst ? all[2 * r] : worst;
        if (vs) (*vs)[r] = all[2 * r + 1];
    }
    if (worst >= 0x100) return local_rc < 0 ? local_rc : TFIDF_E_PEER;
    return worst ? 1 : 0;
}

/* errors inside the collective sequence: no retry is possible any more */
#define XCHK(x)                                                             \
    do {                                                                    \
        int l_ = (x);                                                       \
        if (l_ == -2) return TFIDF_E_CAPACITY;                              \
        if (l_ < 0) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }      \
    } while (0)

static uint64_t table_cap(uint64_t n) {   /* load <= 2/3: short probe runs */
    uint64_t t = 1024;
    while (t < n + n / 2) t *= 2;
    return t;
}

/* the hash-owner form (step 2 above); *agreed = true when the returned failure was decided
 * by all ranks together (nothing half-done in a collective: the transport stays usable) */
static int exchange_owner(tfidf_ctx* ctx, uint32_t V, const std::vector<uint64_t>& vs, bool* agreed) {
    hipStream_t s = ctx->stream;
    Xport* xp = ctx->xp;
    const int R = xp->nranks, me = xp->rank;
    unsigned long long* cnt = ctx->counters.as<unsigned long long>();
    uint64_t sumv = 0;
    for (uint64_t x : vs) sumv += x;
    /* everything sized here from the agreed V's: the receive side holds at most every
     * rank's terms; a failure travels as the status word of the count row (below) */
    int arc = 0;
    auto ens = [&](DevBuf& b, size_t bytes) { if (!arc && b.ensure(bytes) != 0) arc = TFIDF_E_NOMEM; };
    if (!ctx->sorted_skey) ens(ctx->x_mine, (size_t)V * 16 + 16);
    ens(ctx->x_srec, (size_t)V * 20 + 20);
    ens(ctx->x_sidx, (size_t)V * 4 + 4);
    ens(ctx->x_back, ((size_t)V + R) * 4 + 4);
    ens(ctx->x_rrec, sumv * 20 + 20);
    ens(ctx->x_reply, (sumv + R) * 4 + 4);
    if (ctx->xagg_table) {   /* TFIDF_XAGG=table: the HBM table and its df column */
        ens(ctx->x_tkey, table_cap(sumv) * 16);
        ens(ctx->x_tdf, table_cap(sumv) * 4);
        ens(ctx->x_rslot, sumv * 4 + 4);
    } else {                 /* the bucketed form's sort scratch */
        ens(ctx->x_tkey, owner_bucket_scratch(sumv));
    }
    if (ctx->xnomem_rank == me) {   /* tests: an agreed allocation failure (once) */
        ctx->xnomem_rank = -1;
        arc = TFIDF_E_NOMEM;
    }
    /* x_cnt (sized in run_local): [R + 1] this rank's row (counts per owner + status),
     * [R (R + 1)] all rows, [R + 1] soff, [R + 1] roff */
    uint32_t* row = ctx->x_cnt.as<uint32_t>();
    uint32_t* mat = row + (R + 1);
    uint32_t* soff = mat + (size_t)R * (R + 1);
    uint32_t* roff = soff + (R + 1);
    uint32_t* cur = roff + (R + 1);
    if (!arc) {
        /* the keys straight from the vocabulary sort (run_local): sorted by rank after the
         * tile sort (and gathered so for the long-term fix-up after the radix sort), else
         * gathered here from the radix sort's compact keys in dense order */
        OwnerKeySrc ks;
        ks.skey = ctx->sorted_skey;
        if (!ks.skey) {
            XCHK(launch_gather_u128(ctx->skey0.as<uint4>(), ctx->sorted_dense, V, ctx->x_mine.as<uint4>(), s));
            ks.skey = ctx->x_mine.as<uint4>();
        }
        ks.slot_of_rank = ctx->slot_of_rank.as<uint32_t>();
        ks.vkeys = ctx->vkeys.as<uint4>();
        XCHK(launch_owner_partition(ks, ctx->df_local.as<uint32_t>(), V, (uint32_t)R, row, cur,
                                    ctx->x_srec.as<uint32_t>(), ctx->x_sidx.as<uint32_t>(), s));
    } else {
        HIPCHK(hipMemsetAsync(row, 0, (size_t)R * 4, s));
    }
    ctx->hpin[15] = (uint64_t)(uint32_t)arc;
    HIPCHK(hipMemcpyAsync(row + R, ctx->hpin + 15, 4, hipMemcpyHostToDevice, s));
    int rc = xp->allgather(row, mat, (size_t)(R + 1) * 4, s);
    if (rc) return rc;
    std::vector<uint32_t> m((size_t)R * (R + 1));
    HIPCHK(hipMemcpyAsync(m.data(), mat, m.size() * 4, hipMemcpyDeviceToHost, s));
    XSYNC(s);
    int peer_fail = 0;
    for (int p = 0; p < R; ++p)
        if (m[(size_t)p * (R + 1) + R]) peer_fail = 1;
    if (peer_fail) { *agreed = true; return arc ? arc : TFIDF_E_PEER; }
    std::vector<uint64_t> scnt(R), rcnt(R), scnt1(R), rcnt1(R);
    uint64_t nrecv = 0, nsend = 0;
    for (int p = 0; p < R; ++p) {
        scnt[p] = m[(size_t)me * (R + 1) + p];
        rcnt[p] = m[(size_t)p * (R + 1) + me];
        scnt1[p] = scnt[p] + 1;   /* the replies carry one trailer word per owner */
        rcnt1[p] = rcnt[p] + 1;
        nrecv += rcnt[p];
        nsend += scnt[p];
    }
    if (nsend != V || nrecv > sumv) return TFIDF_E_STATE;
    if (ctx->xfail_rank == me) {   /* tests: a rank-local failure after a collective (once) */
        ctx->xfail_rank = -1;
        fprintf(stderr, "tfidf: rank %d: injected exchange failure (TFIDF_TEST_XFAIL_RANK)\n", me);
        return TFIDF_E_HIP;
    }
    XCHK(launch_owner_offsets(mat, (uint32_t)R, (uint32_t)me, soff, roff, s));
    /* (key, local df) records to the owners */
    rc = xp->alltoallv(ctx->x_srec.p, scnt.data(), ctx->x_rrec.p, rcnt.data(), 20, s);
    if (rc) return rc;
    /* the owner: df summed per distinct key, every received record answered in order */
    unsigned long long* used = cnt + 10;
    if (ctx->xagg_table) {   /* TFIDF_XAGG=table: round 3's table of 1.5x the records (A/B) */
        XCHK(launch_owner_aggregate(ctx->x_rrec.as<uint32_t>(), nrecv, roff, (uint32_t)R, ctx->x_tkey.as<uint4>(),
                                    table_cap(nrecv), ctx->x_tdf.as<uint32_t>(), ctx->x_rslot.as<uint32_t>(),
                                    ctx->x_reply.as<uint32_t>(), used, (uint32_t*)(cnt + 3), s));
    } else {   /* bucketed: x_tkey is its scratch */
        XCHK(launch_owner_aggregate_buckets(ctx->x_rrec.as<uint32_t>(), nrecv, roff, (uint32_t)R, ctx->x_tkey.p,
                                            ctx->x_tkey.cap, ctx->x_reply.as<uint32_t>(), used, (uint32_t*)(cnt + 3),
                                            ctx->xb_stage_max, s));
    }
    rc = xp->alltoallv(ctx->x_reply.p, rcnt1.data(), ctx->x_back.p, scnt1.data(), 4, s);
    if (rc) return rc;
    XCHK(launch_owner_back(ctx->x_back.as<uint32_t>(), soff, (uint32_t)R, ctx->x_sidx.as<uint32_t>(), V,
                           ctx->df_global.as<uint32_t>(), (uint32_t*)(cnt + 12), s));
    return 0;
}

/* The dense form's buffers for gathers of R blocks of `maxv` keys.  Sized before the
 * agreement from this rank's own V (padded: dense_pad) so that, when every rank's padded V
 * covers the largest V, no second agreement is needed (allocation failures travel in the
 * agreement's status word). */
static uint64_t dense_pad(uint64_t v) { return v + v / 4 + 64; }
static int dense_alloc(tfidf_ctx* ctx, uint32_t V, uint64_t maxv, uint64_t R) {
    const uint64_t n = R * maxv, sumv = R * maxv;
    if (ctx->x_mine.ensure(maxv * 16 + 16) || ctx->x_gkeys.ensure(n * 16 + 16) ||
        ctx->x_tkey.ensure(table_cap(sumv) * 16) || ctx->x_tdf.ensure(table_cap(sumv) * 4) ||
        ctx->x_pos.ensure((size_t)V * 4 + 4) || ctx->x_dense.ensure(n * 4 + 4))
        return TFIDF_E_NOMEM;
    return 0;
}

/* the dense form (step 2 above) */
static int exchange_dense(tfidf_ctx* ctx, uint32_t V, const std::vector<uint64_t>& vs, bool merge, bool* agreed) {
    hipStream_t s = ctx->stream;
    Xport* xp = ctx->xp;
    const int R = xp->nranks, me = xp->rank;
    unsigned long long* cnt = ctx->counters.as<unsigned long long>();
    uint64_t maxv = 1, sumv = 0, minpad = ~0ull;
    for (uint64_t x : vs) {
        maxv = x > maxv ? x : maxv;
        sumv += x;
        minpad = dense_pad(x) < minpad ? dense_pad(x) : minpad;
    }
    const uint64_t n = (uint64_t)R * maxv;   /* gathered positions */
    /* every rank sized its buffers for R blocks of dense_pad(its V) before the agreement
     * (exchange_df); only when some rank's padding is short of the largest V do all ranks
     * grow them and agree once more (the same decision on every rank: it depends on vs) */
    if (maxv > minpad) {
        int arc = dense_alloc(ctx, V, maxv, (uint64_t)R);
        if (ctx->xnomem_rank == me) {   /* tests: an agreed allocation failure (once) */
            ctx->xnomem_rank = -1;
            arc = TFIDF_E_NOMEM;
        }
        int rc = exchange_agree(ctx, arc, 0, nullptr);
        if (rc == 1) rc = TFIDF_E_STATE;
        if (rc) { *agreed = true; return rc; }
    }
    int rc = 0;
    if (ctx->xfail_rank == me) {   /* tests: a rank-local failure after a collective (once) */
        ctx->xfail_rank = -1;
        fprintf(stderr, "tfidf: rank %d: injected exchange failure (TFIDF_TEST_XFAIL_RANK)\n", me);
        return TFIDF_E_HIP;
    }
    uint4* mine = ctx->x_mine.as<uint4>();
    /* padding: all-ones keys (above every short key) for the merge numbering, else EMPTY */
    HIPCHK(hipMemsetAsync(mine, merge ? 0xFF : 0xEE, maxv * 16, s));
    XCHK(launch_keys_by_rank(ctx->vkeys.as<uint4>(), ctx->slot_of_rank.as<uint32_t>(), V, mine, s));
    rc = xp->allgather(mine, ctx->x_gkeys.p, maxv * 16, s);
    if (rc) return rc;
    if (merge) {   /* positions in the merged term order: no table (x_tdf holds the R x V lb's) */
        HIPCHK(hipMemsetAsync(ctx->x_dense.p, 0, (sumv + 1) * 4, s));
        XCHK(launch_dense_merge_ids(ctx->x_gkeys.as<uint4>(), maxv, (uint32_t)R, (uint32_t)me, V,
                                    ctx->x_tdf.as<uint32_t>(), ctx->df_local.as<uint32_t>(), sumv,
                                    ctx->x_pos.as<uint32_t>(), ctx->x_dense.as<uint32_t>(), s));
        rc = xp->allreduce_u32(ctx->x_dense.as<uint32_t>(), sumv + 1, s);
        if (rc) return rc;
        XCHK(launch_dense_gather(ctx->x_dense.as<uint32_t>(), ctx->x_pos.as<uint32_t>(), V,
                                 ctx->df_global.as<uint32_t>(), s));
        HIPCHK(hipMemcpyAsync(cnt + 12, ctx->x_dense.as<uint32_t>() + sumv, 4, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    const uint64_t tcap = table_cap(sumv);
    uint32_t* status = (uint32_t*)(cnt + 3);
    XCHK(launch_dense_ids(ctx->x_gkeys.as<uint4>(), n, ctx->x_tkey.as<uint4>(), ctx->x_tdf.as<uint32_t>(), tcap, cnt + 10,
                          status, s));
    HIPCHK(hipMemsetAsync(ctx->x_dense.p, 0, n * 4, s));
    XCHK(launch_dense_scatter(mine, ctx->df_local.as<uint32_t>(), V, ctx->x_tkey.as<uint4>(), tcap,
                              ctx->x_tdf.as<uint32_t>(), ctx->x_pos.as<uint32_t>(), ctx->x_dense.as<uint32_t>(), status,
                              s));
    rc = xp->allreduce_u32(ctx->x_dense.as<uint32_t>(), n, s);
    if (rc) return rc;
    XCHK(launch_dense_gather(ctx->x_dense.as<uint32_t>(), ctx->x_pos.as<uint32_t>(), V, ctx->df_global.as<uint32_t>(), s));
    /* global V = the distinct keys (the same on every rank) */
    HIPCHK(hipMemcpyAsync(cnt + 12, cnt + 10, 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

/* Cross-rank identity of terms of >= 16 bytes (TFIDF.c:229 joins words across ranks with
 * strcmp).  A long term's identity key is a 120-bit hash of its bytes: inside a rank every
 * key match is checked against the bytes (dev_vocab.h), and here, after the DF exchange, so is
 * every key that two ranks share.  The ranks agree on the largest byte total of their long
 * terms, all-gather their lists (key, length, blob offset; padded with EMPTY keys) and blobs,
 * and every rank compares each entry with the first entry of its key (finalize.hip
 * k_long_verify).  Every rank checks the same gathered data, so all reach the same verdict: a
 * mismatch fails the run everywhere with TFIDF_E_CAPACITY (the terms are never merged), with
 * the transport still usable (*agreed).  Only when some rank holds a long term (bit 32 of the
 * agreement word), so runs without long terms pay nothing. */
static int exchange_long_check(tfidf_ctx* ctx, uint32_t V, const uint8_t* bytes, bool* agreed) {
    hipStream_t s = ctx->stream;
    Xport* xp = ctx->xp;
    const uint64_t R = (uint64_t)xp->nranks;
    int arc = ctx->x_lloc.ensure((size_t)V * (sizeof(LongEnt) + 8) + 64) ? TFIDF_E_NOMEM : 0;
    LongEnt* ents = ctx->x_lloc.as<LongEnt>();
    uint64_t* src = reinterpret_cast<uint64_t*>(ents + V);
    unsigned long long* lc = reinterpret_cast<unsigned long long*>(src + V);
    uint64_t L = 0, B = 0;
    if (!arc) {
        XCHK(launch_long_list(ctx->vkeys.as<uint4>(), ctx->vrep.as<uint64_t>(), ctx->slot_of_rank.as<uint32_t>(), V, ents,
                              src, lc, s));
        HIPCHK(hipMemcpyAsync(ctx->hpin + 28, lc, 16, hipMemcpyDeviceToHost, s));
        XSYNC(s);
        L = ctx->hpin[28];
        B = ctx->hpin[29];
    }
    std::vector<uint64_t> bs;
    int rc = exchange_agree(ctx, arc, B, &bs);
    if (rc) { *agreed = true; return rc == 1 ? TFIDF_E_STATE : rc; }
    uint64_t maxb = 0;
    for (uint64_t x : bs) maxb = x > maxb ? x : maxb;
    const uint64_t lcap = maxb / 16 + 1;            /* a long term has >= 16 bytes */
    const uint64_t bcap = (maxb + 16) & ~15ull;
    const uint64_t n = R * lcap, tcap = table_cap(n);
    arc = (ctx->x_lsend.ensure(lcap * sizeof(LongEnt) + bcap) || ctx->x_lgath.ensure(n * sizeof(LongEnt) + R * bcap) ||
           ctx->x_ltab.ensure(tcap * 20))
              ? TFIDF_E_NOMEM
              : 0;
    rc = exchange_agree(ctx, arc, 0, nullptr);
    if (rc) { *agreed = true; return rc == 1 ? TFIDF_E_STATE : rc; }
    LongEnt* se = ctx->x_lsend.as<LongEnt>();
    uint8_t* sblob = reinterpret_cast<uint8_t*>(se + lcap);
    HIPCHK(hipMemsetAsync(se, 0xEE, lcap * sizeof(LongEnt), s));
    if (L) HIPCHK(hipMemcpyAsync(se, ents, L * sizeof(LongEnt), hipMemcpyDeviceToDevice, s));
    XCHK(launch_long_bytes(ents, src, (uint32_t)L, bytes, sblob, s));
    LongEnt* ge = ctx->x_lgath.as<LongEnt>();
    uint8_t* gblob = reinterpret_cast<uint8_t*>(ge + n);
    rc = xp->allgather(se, ge, lcap * sizeof(LongEnt), s);
    if (rc) return rc;
    rc = xp->allgather(sblob, gblob, bcap, s);
    if (rc) return rc;
    uint4* tkey = ctx->x_ltab.as<uint4>();
    uint32_t* status = reinterpret_cast<uint32_t*>(lc);   /* the list's counters are read: reused */
    HIPCHK(hipMemsetAsync(status, 0, 4, s));
    XCHK(launch_long_verify(ge, n, lcap, gblob, bcap, tkey, reinterpret_cast<uint32_t*>(tkey + tcap), tcap, status, s));
    ctx->hpin[30] = 0;
    HIPCHK(hipMemcpyAsync(ctx->hpin + 30, status, 4, hipMemcpyDeviceToHost, s));
    XSYNC(s);
    const uint32_t st = (uint32_t)ctx->hpin[30];
    *agreed = true;   /* the same verdict on every rank */
    if (st & ST_LONG_COLLIDE) {
        fprintf(stderr, "tfidf: two distinct terms of 16 bytes or more on different ranks share their 120-bit identity key\n");
        return TFIDF_E_CAPACITY;
    }
    if (st & (ST_BOUNDS | ST_VOCAB_SPIN)) {
        fprintf(stderr, "tfidf: internal bounds check tripped in the long-term check (status 0x%x)\n", st);
        return TFIDF_E_STATE;
    }
    return 0;
}

static int exchange_df(tfidf_ctx* ctx, int local_rc, uint32_t V, const uint8_t* bytes) {
    std::vector<uint64_t> vs;
    /* the dense form's buffers, sized from this rank's V before the agreement; a failure
     * travels as bit 33 of step 1's word (no extra exchange): the ranks then take the owner
     * form, which sizes its own buffers, unless the dense form is forced */
    bool dense_nomem = false;
    if (local_rc == 0 && (ctx->xchg_mode >= 2 || (ctx->xchg_mode == 0 && V <= DENSE_XCHG_MAXV))) {
        int arc = dense_alloc(ctx, V, dense_pad(V), (uint64_t)ctx->xp->nranks);
        if (ctx->xnomem_rank == ctx->xp->rank && ctx->xchg_mode != 1) {   /* tests: an allocation failure (once) */
            ctx->xnomem_rank = -1;
            arc = TFIDF_E_NOMEM;
        }
        dense_nomem = arc != 0;
    }
    /* step 1; bit 32 of the word: this rank holds terms of >= 16 bytes; bit 33: its dense
     * buffers could not be allocated */
    int rc = exchange_agree(ctx, local_rc,
                            (uint64_t)V | (ctx->local_long ? 1ull << 32 : 0ull) | (dense_nomem ? 1ull << 33 : 0ull), &vs);
    if (rc) return rc;
    uint64_t maxv = 0;
    bool any_long = false, any_dense_nomem = false;
    for (uint64_t& x : vs) {
        any_long |= ((x >> 32) & 1u) != 0;
        any_dense_nomem |= ((x >> 33) & 1u) != 0;
        x &= 0xFFFFFFFFull;
        maxv = x > maxv ? x : maxv;
    }
    if (any_dense_nomem && ctx->xchg_mode >= 2)   /* the dense form forced: an agreed failure */
        return dense_nomem ? TFIDF_E_NOMEM : TFIDF_E_PEER;
    const bool dense = ctx->xchg_mode >= 2 || (ctx->xchg_mode == 0 && maxv <= DENSE_XCHG_MAXV && !any_dense_nomem);
    ctx->last_dense = dense;
    bool agreed = false;
    rc = dense ? exchange_dense(ctx, V, vs, !any_long && ctx->xchg_mode != 3, &agreed)
               : exchange_owner(ctx, V, vs, &agreed);
    if (!rc && any_long) {
        agreed = false;
        rc = exchange_long_check(ctx, V, bytes, &agreed);
    }
    if (rc && rc != TFIDF_E_PEER && !agreed) ctx->xp->abort();
    return rc;
}

/* The document order (`docN@` strcmp order of the run's documents) on the side stream,
 * joined before the per-position metadata (run_post).  Enqueued right after K1 for a large
 * N (its radix sort is long: started early, it is done long before it is needed), after the
 * vocabulary stage's launches for up to SORT_TILE_MAXN documents (two short launches: the
 * device runs the vocabulary stage while the host enqueues them; c2 +0.9 %, while c5's
 * 1e6-document sort beside its merge stage slowed that by 0.07 ms). */
static int enqueue_doc_order(tfidf_ctx* ctx, const uint32_t* dev_ids, uint32_t N, hipStream_t s2) {
    ENSURE(ctx->dkey0, (size_t)N * 8 + 8);
    ENSURE(ctx->dkey1, (size_t)N * 8 + 8);
    ENSURE(ctx->dseq0, (size_t)N * 4 + 4);
    ENSURE(ctx->dseq1, (size_t)N * 4 + 4);
    {
        /* the radix histograms, or the tile sort's staging (20 B per document) */
        const size_t need2 = (size_t)256 * 4 * ((N + 2047) / 2048 + 1) + (size_t)N * 20 + (1u << 20);
        if (need2 > ctx->arena2_buf.cap && ctx->arena2_buf.ensure(need2) != 0) return TFIDF_E_NOMEM;
        ctx->arena2.base = (uint8_t*)ctx->arena2_buf.p;
        ctx->arena2.cap = ctx->arena2_buf.cap;
        ctx->arena2.used = 0;
        HIPCHK(hipStreamWaitEvent(s2, ctx->ev_fork, 0));   /* recorded when the attempt started */
        LCHK(launch_doc_keys(dev_ids, N, ctx->dkey0.as<uint64_t>(), ctx->dseq0.as<uint32_t>(), s2));
        /* base-11 keys of 10 digits are < 11^10 < 2^35: five bytes, no probe */
        /* up to SORT_TILE_MAXN documents: two launches (tile bitonic sort + rank) instead of
         * two per digit byte */
        int dc = N <= SORT_TILE_MAXN
            ? tile_sort_u64(ctx->dkey0.as<uint64_t>(), ctx->dseq0.as<uint32_t>(), ctx->dkey1.as<uint64_t>(),
                            ctx->dseq1.as<uint32_t>(), N, ctx->arena2, s2)
            : radix_sort_u64(ctx->dkey0.as<uint64_t>(), ctx->dseq0.as<uint32_t>(), ctx->dkey1.as<uint64_t>(),
                             ctx->dseq1.as<uint32_t>(), N, 0x1Fu, ctx->arena2, s2);
        LCHK(dc);
        ctx->order = dc ? ctx->dseq1.as<uint32_t>() : ctx->dseq0.as<uint32_t>();
        HIPCHK(hipEventRecord(ctx->ev_order, s2));
    }
    return 0;
}

/* The local stages of one attempt (this shard only, no collective): K0, K1, vocabulary,
 * merge, local DF.  Returns 0, 1 to retry with grown capacities, <0 on error.  Also
 * checks that the main arena holds what the stages after the exchange need, so that they
 * never ask for a retry. */
static int run_local(tfidf_ctx* ctx, const CorpusDev& c, const uint32_t* dev_ids, uint64_t Nt) {
    hipStream_t s = ctx->stream;
    Arena& ar = ctx->arena;
    const uint32_t N = c.ndocs;
    ar.used = 0;
    ctx->run_N = N;
    ctx->run_V = 0;
    mark(ctx, S_PREP);
    /* the side stream's fork point (the document order needs only the run's inputs): recorded
     * first, while the device still waits for the host's first launches, since a record costs
     * the stream ~5 us wherever it sits */
    HIPCHK(hipEventRecord(ctx->ev_fork, s));
    /* ---- buffers ---- */
    if (ctx->xp) {   /* the exchange's count rows (sized before its agreement: see exchange_owner) */
        const size_t R = (size_t)ctx->nranks;
        ENSURE(ctx->x_cnt, ((R + 1) * (R + 4)) * 4);
    }
    const uint64_t span = c.hi - c.lo;
    /* K1 variant: the slot-keyed kernels (tokcount_st / tokcount_vs) need a 16-byte aligned
     * corpus base; TFIDF_K1=general selects the general kernel (cross-checks).  The LDS-staged
     * kernel runs up to the largest table it addresses (2^25 slots): round 6's leaner rounds
     * made it faster than the round-1 kernel on config 4 too (a 32M-slot table for ~1e7 terms,
     * nearly every token a new (doc, term) pair: K1 4.67 vs 5.02 ms, c4 76.8 vs 75.0 GB/s,
     * profiles/r06_k1_ab_c2.txt call r06l); beyond, k_tokcount_vs */
    const bool aligned = (((uintptr_t)c.bytes & 15u) == 0);
    ctx->k1_vs = aligned && ctx->k1_mode != 2;
    if (ctx->k1_vs && ctx->vcap > K1_VS_MAX_CAP) return TFIDF_E_CAPACITY;
    ctx->k1_sl = ctx->k1_vs && (ctx->k1_mode == 0 || ctx->k1_mode == 3) &&
                 ctx->vcap <= ctx->sl_maxcap;
    /* tokcount_sl over a high-cardinality table (past K1_ST_MAX_CAP slots): half-size chunks,
     * as tokcount_vs, since nearly every token is a new pair for its LDS table */
    const uint32_t cb = ctx->k1_sl ? (ctx->vcap > K1_ST_MAX_CAP ? CHUNK_BYTES : CHUNK_BYTES_ST) : CHUNK_BYTES;
    const uint64_t nchunks = span ? (span + cb - 1) / cb : 0;
    if (ctx->rec_cap == 0) ctx->rec_cap = span / 6 + 4096;
    if (ctx->part_cap == 0) ctx->part_cap = span / 64 + 4096;
    ENSURE(ctx->chunk_start, (nchunks + 1) * 8);
    ENSURE(ctx->chunk_doc, (nchunks + 1) * 4);
    ENSURE(ctx->vkeys, ctx->vcap * 16);
    ENSURE(ctx->vrep, ctx->vcap * 8);
    ENSURE(ctx->rec_slot, ctx->rec_cap * 4);
    ENSURE(ctx->rec_cnt, ctx->rec_cap * 4);
    ENSURE(ctx->part_doc, ctx->part_cap * 4);
    ENSURE(ctx->part_slot, ctx->part_cap * 4);
    ENSURE(ctx->part_cnt, ctx->part_cap * 4);
    ENSURE(ctx->doc_recoff, (size_t)N * 8 + 8);
    ENSURE(ctx->doc_npairs, (size_t)N * 4 + 4);
    ENSURE(ctx->doc_size, (size_t)N * 4 + 4);
    ENSURE(ctx->doc_flags, (size_t)N + 1);
    unsigned long long* cnt = ctx->counters.as<unsigned long long>(); /* rec, part, ntok, status */
    {   /* the run's clears in one launch: the vocabulary table (EMPTY keys), K1's counters,
         * status and sharded chunk counters, the per-document pairs / sizes / flags */
        FillList fl{};
        auto add = [&](void* p, uint64_t bytes, uint32_t byte) {
            fl.p[fl.n] = p;
            fl.bytes[fl.n] = bytes;
            fl.val[fl.n] = byte * 0x01010101u;
            ++fl.n;
        };
        add(ctx->vkeys.p, ctx->vcap * 16, 0xEEu);
        add(cnt, 256, 0u);
        add(ctx->doc_npairs.p, (size_t)N * 4 + 4, 0u);
        add(ctx->doc_size.p, (size_t)N * 4 + 4, 0u);
        add(ctx->doc_flags.p, (size_t)N + 1, 0u);
        LCHK(launch_fill_multi(fl, s));
    }
    ENSURE(ctx->big_list, (size_t)BIG_LIST_CAP * 4);
    if (nchunks)
        LCHK(launch_plan_chunks(c, nchunks, cb, ctx->chunk_start.as<uint64_t>(), ctx->chunk_doc.as<uint32_t>(),
                                ctx->big_list.as<uint32_t>(), cnt + 6, s));
    /* ---- K1 ---- */
    mark(ctx, S_TOKCOUNT);
    VocabDev vd{ctx->vkeys.as<uint4>(), ctx->vrep.as<uint64_t>(), ctx->vcap - 1};
    K1Out o{};
    o.rec_slot = ctx->rec_slot.as<uint32_t>();
    o.rec_cnt = ctx->rec_cnt.as<uint32_t>();
    o.rec_alloc = cnt + 0;
    o.rec_cap = ctx->rec_cap;
    o.part_doc = ctx->part_doc.as<uint32_t>();
    o.part_slot = ctx->part_slot.as<uint32_t>();
    o.part_cnt = ctx->part_cnt.as<uint32_t>();
    o.part_alloc = cnt + 1;
    o.part_cap = ctx->part_cap;
    o.doc_recoff = ctx->doc_recoff.as<uint64_t>();
    o.doc_npairs = ctx->doc_npairs.as<uint32_t>();
    o.doc_size = ctx->doc_size.as<uint32_t>();
    o.doc_flags = ctx->doc_flags.as<uint8_t>();
    o.ntokens = cnt + 2;
    o.chunk_ctr = cnt + 5;
    o.chunk_shard = cnt + 16;
    o.status = (uint32_t*)(cnt + 3);
    o.stamps = nullptr;
    if (ctx->stamps_on) {
        ENSURE(ctx->stamps, 8 * K1_DEBUG_WORDS);
        HIPCHK(hipMemsetAsync(ctx->stamps.p, 0, 8 * K1_DEBUG_WORDS, s));
        o.stamps = ctx->stamps.as<unsigned long long>();
    }
    if (nchunks && ctx->k1_sl) {
        /* pinned source: the copy is stream-ordered before the launch, and the block is not
         * rewritten before the next run (every run synchronises with the host after K1) */
        if (!ctx->k1out_valid || memcmp(ctx->k1out_host, &o, sizeof(K1Out)) != 0) {   /* steady state: unchanged */
            ctx->k1out_valid = false;   /* until the copy of the new block is enqueued */
            *ctx->k1out_host = o;
            HIPCHK(hipMemcpyAsync(ctx->k1out_dev.p, ctx->k1out_host, sizeof(K1Out), hipMemcpyHostToDevice, s));
            ctx->k1out_valid = true;
        }
        LCHK(launch_tokcount_sl(c, ctx->chunk_start.as<uint64_t>(), ctx->chunk_doc.as<uint32_t>(), 0, nchunks, vd,
                                ctx->k1out_dev.as<K1Out>(), s));
    } else if (nchunks && ctx->k1_vs)
        LCHK(launch_tokcount_vs(c, ctx->chunk_start.as<uint64_t>(), ctx->chunk_doc.as<uint32_t>(), 0, nchunks, vd, o, s));
    else if (nchunks)
        LCHK(launch_tokcount(c, ctx->chunk_start.as<uint64_t>(), ctx->chunk_doc.as<uint32_t>(), 0, nchunks, vd, o, s));
    mark(ctx, S_VOCAB);
    /* the vocabulary's used-slot flags and count are enqueued before the host reads K1's
     * counters: one host round trip for both */
    const uint64_t cap = ctx->vcap;
    ENSURE(ctx->dense, (cap + 1) * 4);
    LCHK(launch_vocab_flags(vd, cap, ctx->dense.as<uint32_t>(), s));
    LCHK(scan_excl_u32(ctx->dense.as<uint32_t>(), ctx->dense.as<uint32_t>(), cap, ar, s));
    uint64_t* hp = ctx->hpin;
    {   /* K1's counters (hp[0..7]) and the vocabulary size (hp[8]): one launch */
        WordList wl{};
        for (int i = 0; i < 8; ++i) { wl.src[i] = cnt + i; wl.bytes[i] = 8; }
        wl.src[8] = ctx->dense.as<uint32_t>() + cap;
        wl.bytes[8] = 4;
        wl.n = 9;
        HIPCHK(words_wait(ctx, wl, 0, s));
    }
    const uint32_t V = (uint32_t)hp[8];
    unsigned long long hc[8];
    for (int i = 0; i < 8; ++i) hc[i] = hp[i];
    const uint64_t R_main = hc[0], Q = hc[1], nbig = hc[6];
    const uint32_t st = (uint32_t)hc[3];
    ctx->local_long = (st & ST_HAS_LONG) != 0;
    ctx->ntokens = hc[2];
    ctx->nchunks = nchunks;
    ctx->nrec_part = Q;
    if (st & (ST_VOCAB_SPIN | ST_TERM_LONG)) return TFIDF_E_CAPACITY;
    if (st & ST_LONG_COLLIDE) {   /* dev_vocab.h: reported, never merged */
        fprintf(stderr, "tfidf: two distinct terms of 16 bytes or more share their 120-bit identity key\n");
        return TFIDF_E_CAPACITY;
    }
    bool retry = false;
    if (st & ST_BOUNDS) {
        fprintf(stderr, "tfidf: internal bounds check tripped in K1 (status 0x%x)\n", st);
        return TFIDF_E_STATE;
    }
    if (st & ST_VOCAB_FULL) {   /* the run stopped inserting early: V unknown */
        if (ctx->vcap >= K1_VS_MAX_CAP) return TFIDF_E_CAPACITY;
        ctx->vcap = ctx->vcap * 4 < K1_VS_MAX_CAP ? ctx->vcap * 4 : K1_VS_MAX_CAP;
        retry = true;
    }
    if (st & ST_REC_FULL) { ctx->rec_cap = R_main + R_main / 4 + 4096; retry = true; }
    if (st & ST_PART_FULL) { ctx->part_cap = Q + Q / 4 + 4096; retry = true; }
    if (retry) return 1;
    if (N > SORT_TILE_MAXN) {   /* see enqueue_doc_order */
        const int rc = enqueue_doc_order(ctx, dev_ids, N, ctx->stream2);
        if (rc) return rc;
    }
    /* ---- vocabulary ---- */
    ctx->V = V;
    /* keep probes short: the low load pays while the table is L2/MALL-sized (<= 16M slots,
     * 256 MB of keys); past that every probe is an HBM access anyway, so up to 45 % */
    if ((uint64_t)V * 100 > cap * (cap < VOCAB_LOW_LOAD_CAP ? ctx->vload_pct : ctx->vload_big_pct)) {
        /* the smallest table within the load limit: a table twice too large costs its
         * clear and a sparser compaction pass (c4: 64M -> 32M slots, vocabulary stage
         * 3.1 -> 2.65 ms) */
        while ((uint64_t)V * 100 > ctx->vcap * (ctx->vcap < VOCAB_LOW_LOAD_CAP ? ctx->vload_pct : ctx->vload_big_pct))
            ctx->vcap *= 2;
        if (ctx->vcap > K1_VS_MAX_CAP && cap < K1_VS_MAX_CAP) ctx->vcap = K1_VS_MAX_CAP;
        if (ctx->vcap != cap) return 1;
    }
    ENSURE(ctx->vslot, (size_t)V * 4 + 4);
    ENSURE(ctx->skey0, (size_t)V * 16 + 16);
    ENSURE(ctx->skey1, (size_t)V * 16 + 16);
    ENSURE(ctx->seq0, (size_t)V * 4 + 4);
    ENSURE(ctx->seq1, (size_t)V * 4 + 4);
    /* rank maps: one entry per slot */
    ENSURE(ctx->rank_of_slot, cap * 4);
    ENSURE(ctx->slot_of_rank, (size_t)V * 4 + 4);
    LCHK(launch_vocab_compact(vd, cap, ctx->dense.as<uint32_t>(), c, ctx->vslot.as<uint32_t>(), ctx->skey0.as<uint4>(),
                              ctx->seq0.as<uint32_t>(), s));
    if (V <= SORT_TILE_MAXN) { /* two launches, no varying-byte probe (no host sync) */
        const int cur = tile_sort_u128(ctx->skey0.as<uint4>(), ctx->seq0.as<uint32_t>(), ctx->skey1.as<uint4>(),
                             ctx->seq1.as<uint32_t>(), V, ar, s);
        LCHK(cur);
        ctx->sorted_skey = cur ? ctx->skey1.as<uint4>() : ctx->skey0.as<uint4>();
        ctx->sorted_dense = cur ? ctx->seq1.as<uint32_t>() : ctx->seq0.as<uint32_t>();
    } else {
        /* a u64 LSD sort of the keys' high halves (their first 8 bytes) over the varying
         * bytes, then the runs of equal prefixes re-ordered by the low halves
         * (launch_vocab_prefix_ties: few at c4, so 8 digit passes instead of 13; vocabulary
         * 2.19 -> 2.00 ms, profiles/r04_c4_ab.txt); skey0 stays in dense order,
         * skey1 holds the two u64 ping-pong buffers */
        uint32_t vm = 0;
        LCHK(key_varying_bytes_u128(ctx->skey0.as<uint4>(), V, &vm, ar, s));
        uint64_t* const ka = (uint64_t*)ctx->skey1.p;
        uint64_t* const kb = ka + V;
        uint32_t* const sa = ctx->seq0.as<uint32_t>();
        uint32_t* const sbq = ctx->seq1.as<uint32_t>();
        LCHK(launch_sortkey_half(ctx->skey0.as<uint4>(), V, nullptr, 1, ka, s));
        const int c1 = radix_sort_u64(ka, sa, kb, sbq, V, (vm >> 8) & 0xFFu, ar, s);
        LCHK(c1);
        ctx->sorted_dense = c1 ? sbq : sa;
        LCHK(launch_vocab_prefix_ties(c1 ? kb : ka, ctx->sorted_dense, ctx->skey0.as<uint4>(), V, vm & 0xFFu, ar, s));
        ctx->sorted_skey = nullptr;
        if (st & ST_HAS_LONG) {   /* the fix-up reads the keys in sorted order */
            LCHK(launch_gather_u128(ctx->skey0.as<uint4>(), ctx->sorted_dense, V, ctx->skey1.as<uint4>(), s));
            ctx->sorted_skey = ctx->skey1.as<uint4>();
        }
    }
    if (st & ST_HAS_LONG)   /* terms of >= 16 bytes exist: order the ones tied on 16 bytes */
        LCHK(launch_vocab_long_fixup(ctx->sorted_skey, ctx->sorted_dense, ctx->vslot.as<uint32_t>(), vd, c, V, ar, s));
    uint16_t* r16 = nullptr;
    if (V <= 65536u) { ENSURE(ctx->rank16, cap * 2); r16 = ctx->rank16.as<uint16_t>(); }
    LCHK(launch_vocab_rank(ctx->sorted_dense, ctx->vslot.as<uint32_t>(), V, ctx->rank_of_slot.as<uint32_t>(),
                           ctx->slot_of_rank.as<uint32_t>(), r16, s));
    if (N <= SORT_TILE_MAXN) {   /* see enqueue_doc_order */
        const int rc = enqueue_doc_order(ctx, dev_ids, N, ctx->stream2);
        if (rc) return rc;
    }
    /* split DF: with partial records to merge, the main records' histogram (which needs only
     * the term ranks) starts on stream2 now and runs beside the merge stage's short
     * launches; the merged records are added after the merge (accumulate pass below) */
    const bool df_split = ctx->df_split && Q && R_main;
    ENSURE(ctx->df_local, (size_t)V * 4 + 4);
    ENSURE(ctx->df_global, (size_t)V * 4 + 4);
    if (df_split) {
        if (R_main + Q > ctx->rec_cap) {   /* the merge's growth, done before stream2 reads the records */
            uint64_t ncap = R_main + Q + (R_main + Q) / 8 + 4096;
            if (ctx->rec_slot.grow_keep(ncap * 4, R_main * 4, s) || ctx->rec_cnt.grow_keep(ncap * 4, R_main * 4, s))
                return TFIDF_E_NOMEM;
            ctx->rec_cap = ncap;
        }
        const size_t dneed = df_hist_scratch(R_main, V);
        ENSURE(ctx->df_scratch, dneed > ctx->df_scratch_min ? dneed : ctx->df_scratch_min);
        Arena da;
        da.base = (uint8_t*)ctx->df_scratch.p;
        da.cap = ctx->df_scratch.cap;
        HIPCHK(hipEventRecord(ctx->ev_vrank, s));
        HIPCHK(hipStreamWaitEvent(ctx->stream2, ctx->ev_vrank, 0));
        const int dl = launch_df_hist(ctx->rec_slot.as<uint32_t>(), R_main, nullptr, R_main, ctx->rank_of_slot.as<uint32_t>(),
                                      r16, V, cap, (uint32_t*)(cnt + 3), ctx->df_local.as<uint32_t>(), da, ctx->stream2);
        if (dl == -2) {   /* its own scratch was short: grow it (not the arena) and retry */
            ctx->df_scratch_min = da.peak + da.peak / 2 + 4096;
            return 1;
        }
        LCHK(dl);
        HIPCHK(hipEventRecord(ctx->ev_dfmain, ctx->stream2));
    }
    /* this run's full idf table (idf_start's workers finish during K1 in practice) goes up
     * on its own copy stream now, beside the merge and DF stages, instead of inside the idf
     * stage on the main stream (an SDMA copy of (N+1) doubles: ~35 us there for c2) */
    if (ctx->idf_pool.busy && !ctx->idf_early && idf_done(ctx)) {
        idf_join(ctx);
        ENSURE(ctx->idf_vals, (size_t)(Nt + 1) * 8);
        HIPCHK(hipMemcpyAsync(ctx->idf_vals.p, ctx->idf_pin, (size_t)(Nt + 1) * 8, hipMemcpyHostToDevice,
                              ctx->stream3));
        HIPCHK(hipEventRecord(ctx->ev_idf_up, ctx->stream3));
        ctx->idf_pin_busy = true;
        ctx->idf_early = true;
    }
    /* ---- partial documents ---- */
    mark(ctx, S_MERGE);
    uint64_t R_total = R_main;
    const uint32_t* merged_count = nullptr;   /* device: merged + dense records beyond R_main */
    {
        /* Q follows K1's overflow records, which vary from run to run (the order of the LDS
         * claims): at least 2^20 entries (28 MB in all), also when this run has none, so that
         * a shard with few or no partial records does not allocate in steady state (c5 at 8
         * shards: 0 -> 28 K -> 90 K, ten device allocations in its timed steps,
         * TFIDF_DEBUG_ALLOC=1) */
        const uint64_t Qc = Q < (1ull << 20) ? (1ull << 20) : Q;
        ENSURE(ctx->pkey0, Qc * 8);
        ENSURE(ctx->pkey1, Qc * 8);
        ENSURE(ctx->pseq0, Qc * 4);
        ENSURE(ctx->pseq1, Qc * 4);
        ENSURE(ctx->phead, (Qc + 1) * 4);
    }
    if (Q) {
        /* merged (and dense) records land in [R_main, R_main + Q): size for the worst case */
        if (R_main + Q > ctx->rec_cap) {
            uint64_t ncap = R_main + Q + (R_main + Q) / 8 + 4096;
            if (ctx->rec_slot.grow_keep(ncap * 4, R_main * 4, s) || ctx->rec_cnt.grow_keep(ncap * 4, R_main * 4, s))
                return TFIDF_E_NOMEM;
            ctx->rec_cap = ncap;
        }
        /* documents longer than DENSE_DOC (listed by K0): their partial records are summed
         * in dense per-document arrays over ranks (<= 256 MB of them) instead of sorted */
        uint32_t nb = 0;
        if (nbig && V) {
            const uint64_t lim = (256ull << 20) / (4ull * V * DENSE_REP);
            uint64_t m = nbig < (uint64_t)BIG_LIST_CAP ? nbig : (uint64_t)BIG_LIST_CAP;
            nb = (uint32_t)(m < lim ? m : lim);
        }
        uint64_t Qs = Q;                                  /* records to sort */
        const uint32_t* scnt = ctx->part_cnt.as<uint32_t>();
        if (nb) {
            ENSURE(ctx->big_idx, (size_t)N * 4 + 4);
            ENSURE(ctx->dense_cnt, (size_t)nb * V * 4 * DENSE_REP);
            ENSURE(ctx->kcnt, Q * 4);
            uint32_t* nkeep = (uint32_t*)(cnt + 7);   /* zeroed with the run's counters */
            HIPCHK(hipMemsetAsync(ctx->big_idx.p, 0xFF, (size_t)N * 4 + 4, s));
            HIPCHK(hipMemsetAsync(ctx->dense_cnt.p, 0, (size_t)nb * V * 4 * DENSE_REP, s));
            LCHK(launch_set_big_idx(ctx->big_list.as<uint32_t>(), nb, ctx->big_idx.as<uint32_t>(), s));
            LCHK(launch_part_dense(ctx->part_doc.as<uint32_t>(), ctx->part_slot.as<uint32_t>(), ctx->part_cnt.as<uint32_t>(),
                                   Q, ctx->big_idx.as<uint32_t>(), ctx->rank_of_slot.as<uint32_t>(), V,
                                   ctx->dense_cnt.as<uint32_t>(), ctx->pkey0.as<uint64_t>(), ctx->pseq0.as<uint32_t>(),
                                   ctx->kcnt.as<uint32_t>(), nkeep, s));
            /* the sort needs its size on the host: one round trip, dense runs only */
            ctx->hpin[9] = 0;
            HIPCHK(hipMemcpyAsync(ctx->hpin + 9, nkeep, 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            const uint32_t qk = (uint32_t)ctx->hpin[9];
            Qs = qk;
            scnt = ctx->kcnt.as<uint32_t>();
        } else {
            LCHK(launch_part_keys(ctx->part_doc.as<uint32_t>(), ctx->part_slot.as<uint32_t>(),
                                  ctx->rank_of_slot.as<uint32_t>(), Q, ctx->pkey0.as<uint64_t>(),
                                  ctx->pseq0.as<uint32_t>(), s));
        }
        uint32_t* ph = ctx->phead.as<uint32_t>();
        if (Qs) {
            uint32_t pm = 0;
            /* key = (local doc << 32) | rank: the varying bytes follow from N and V (no probe,
             * no host sync) */
            {
                const uint32_t rb = V > 1 ? 32u - (uint32_t)__builtin_clz(V - 1) : 1u;
                const uint32_t db = N > 1 ? 32u - (uint32_t)__builtin_clz(N - 1) : 1u;
                for (uint32_t b = 0; b < (rb + 7) / 8; ++b) pm |= 1u << b;
                for (uint32_t b = 0; b < (db + 7) / 8; ++b) pm |= 1u << (4 + b);
            }
            int pc = Qs <= SORT_TILE_MAXN   /* c2's ~1e5 partial records: two launches, not two per byte */
                ? tile_sort_u64(ctx->pkey0.as<uint64_t>(), ctx->pseq0.as<uint32_t>(), ctx->pkey1.as<uint64_t>(),
                                ctx->pseq1.as<uint32_t>(), Qs, ar, s)
                : radix_sort_u64(ctx->pkey0.as<uint64_t>(), ctx->pseq0.as<uint32_t>(), ctx->pkey1.as<uint64_t>(),
                                 ctx->pseq1.as<uint32_t>(), Qs, pm, ar, s);
            LCHK(pc);
            uint64_t* pk = pc ? ctx->pkey1.as<uint64_t>() : ctx->pkey0.as<uint64_t>();
            uint32_t* ps = pc ? ctx->pseq1.as<uint32_t>() : ctx->pseq0.as<uint32_t>();
            LCHK(launch_part_heads(pk, Qs, ph, s));
            LCHK(scan_excl_u32(ph, ph, Qs, ar, s));
            /* U = ph[Qs] merged records (<= Qs) stays on the device: no host round trip */
            LCHK(launch_part_merge(pk, ps, scnt, ph, Qs, ctx->slot_of_rank.as<uint32_t>(), R_main,
                                   ctx->rec_slot.as<uint32_t>(), ctx->rec_cnt.as<uint32_t>(),
                                   ctx->doc_recoff.as<uint64_t>(), ctx->doc_npairs.as<uint32_t>(),
                                   ctx->doc_flags.as<uint8_t>(), s));
        } else {
            HIPCHK(hipMemsetAsync(ph, 0, 4, s));
        }
        if (nb) {
            const uint64_t nt = ((uint64_t)V + 1023) / 1024;
            ENSURE(ctx->tile_cnt, (nt * nb + 1) * 4);
            LCHK(launch_dense_emit(ctx->dense_cnt.as<uint32_t>(), nb, V, ctx->big_list.as<uint32_t>(),
                                   ctx->slot_of_rank.as<uint32_t>(), R_main, ph + Qs, ctx->tile_cnt.as<uint32_t>(),
                                   ctx->rec_slot.as<uint32_t>(), ctx->rec_cnt.as<uint32_t>(),
                                   ctx->doc_recoff.as<uint64_t>(), ctx->doc_npairs.as<uint32_t>(),
                                   ctx->doc_flags.as<uint8_t>(), ar, s));
        }
        merged_count = ph + Qs;
        R_total = R_main + Q; /* an upper bound: the true count is R_main + *merged_count */
    }
    /* ---- DF ---- */
    mark(ctx, S_DF);
    if (df_split) {   /* the merged records (term ranks) added to the main records' df */
        HIPCHK(hipStreamWaitEvent(s, ctx->ev_dfmain, 0));
        LCHK(launch_df_hist(ctx->rec_slot.as<uint32_t>() + R_main, 0, merged_count, R_total - R_main,
                            ctx->rank_of_slot.as<uint32_t>(), r16, V, cap, (uint32_t*)(cnt + 3),
                            ctx->df_local.as<uint32_t>(), ar, s, true));
    } else {
        /* also rewrites every record's slot as its term rank (K5 then needs no rank gather) */
        LCHK(launch_df_hist(ctx->rec_slot.as<uint32_t>(), R_main, merged_count, R_total,
                            ctx->rank_of_slot.as<uint32_t>(), r16, V, cap, (uint32_t*)(cnt + 3),
                            ctx->df_local.as<uint32_t>(), ar, s));
    }
    ctx->run_V = V;
    ctx->run_cap = cap;
    ctx->run_R_total = R_total;
    ctx->run_merged = merged_count;
    /* the stages after the exchange take their scratch from what is left of the arena */
    const size_t post_need = scan_scratch(Nt + 1) + (size_t)(Nt + 2) * 4 + 512 + scan_scratch(N) +
                             scan_scratch(3ull * ((N + 255) / 256) + 1);   /* K5's document classes */
    if (ar.cap - ar.used < post_need) {
        ar.peak = ar.used + post_need > ar.peak ? ar.used + post_need : ar.peak;
        return 1;
    }
    return 0;
}

/* ---- the per-run idf table: log(N/df) for every df = 0..N on the host's libm
 * (TFIDF.c:243 evaluates log(1.0*N/df) per pair; the table holds the same doubles), on up to
 * eight host threads per process (shared out over its open contexts) posted when the run
 * starts, so the logs run beside K1 .. DF on the device.  run_post waits for them (ms_idf_wait: normally 0) and uploads the table. */
#define IDF_POOL 8
static void idf_worker(tfidf_ctx::IdfPool* P, unsigned i) {
    uint64_t seen = 0;
    for (;;) {
        std::unique_lock<std::mutex> lk(P->mu);
        P->go.wait(lk, [&] { return P->stop || P->gen != seen; });
        if (P->stop) return;
        seen = P->gen;
        if (i >= P->active) continue;
        double* lut = P->lut;
        const uint32_t* vals = P->vals;
        const uint64_t Nt = P->Nt, n = P->n, lo = (n * i) / P->active, hi = (n * (i + 1)) / P->active;
        const uint32_t mode = P->mode;
        const auto t0 = P->t0;
        lk.unlock();
        if (mode != TFIDF_IDF_REF) {   /* weight_host.c's formula, the one tfidf_result_reweight uses */
            if (vals)
                for (uint64_t k = lo; k < hi; ++k) lut[k] = tfidf_weight_idf(mode, Nt, vals[k]);
            else
                for (uint64_t d = lo + 1; d < hi + 1; ++d) lut[d] = tfidf_weight_idf(mode, Nt, (uint32_t)d);
        } else if (vals)
            for (uint64_t k = lo; k < hi; ++k) lut[k] = log(1.0 * (double)Nt / (double)vals[k]);
        else
            for (uint64_t d = lo + 1; d < hi + 1; ++d) lut[d] = log(1.0 * (double)Nt / (double)d);
        const int64_t e = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        lk.lock();
        P->end_ns = e > P->end_ns ? e : P->end_ns;
        if (--P->left == 0) P->done.notify_all();
    }
}
static void idf_pool_stop(tfidf_ctx* ctx) {
    tfidf_ctx::IdfPool& P = ctx->idf_pool;
    {
        std::unique_lock<std::mutex> lk(P.mu);
        P.done.wait(lk, [&] { return P.left == 0; });
        P.stop = true;
    }
    P.go.notify_all();
    for (auto& t : P.th) t.join();
    P.th.clear();
}
/* posts a table job to the context's workers (lut: n values; vals null = every df 1..n) */
static void idf_post(tfidf_ctx* ctx, double* lut, uint64_t Nt, const uint32_t* vals, uint64_t n,
                     uint32_t mode = TFIDF_IDF_REF) {
    tfidf_ctx::IdfPool& P = ctx->idf_pool;
    const int live = g_live_ctx.load();
    const unsigned share = live > 1 ? (unsigned)(IDF_POOL / live > 1 ? IDF_POOL / live : 1) : IDF_POOL;
    const unsigned want = (unsigned)(n / 16384 < 1 ? 1 : (n / 16384 > share ? share : n / 16384));
    while (P.th.size() < want) P.th.emplace_back(idf_worker, &P, (unsigned)P.th.size());   /* started once, as needed */
    {
        std::lock_guard<std::mutex> lk(P.mu);
        P.active = want;
        P.left = P.active;
        P.lut = lut;
        P.Nt = Nt;
        P.vals = vals;
        P.n = n;
        P.mode = mode;
        P.t0 = std::chrono::steady_clock::now();
        P.end_ns = 0;
        P.busy = true;
        ++P.gen;
    }
    P.go.notify_all();
}
/* Waits for every upload that may still read idf_pin or write idf_vals: a failed run can leave
 * the early upload (stream3, run_local) or the late one (the main stream, run_post) queued, and
 * the next run must neither rewrite / free idf_pin under it nor have it land after its own copy */
static int idf_pin_quiesce(tfidf_ctx* ctx) {
    if (!ctx->idf_pin_busy) return TFIDF_OK;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream3));
    ctx->idf_pin_busy = false;
    return TFIDF_OK;
}
static int idf_start(tfidf_ctx* ctx, uint64_t Nt) {
    ctx->idf_logs = 0;
    ctx->idf_early = false;
    ctx->ms_idf_host = ctx->ms_idf_wait = 0;
    if (Nt > IDF_FULL_MAX) return TFIDF_OK;                          /* distinct-df path in run_post */
    if (const int q = idf_pin_quiesce(ctx)) return q;   /* a failed run left an upload of idf_pin unwaited */
    const size_t n = (size_t)Nt + 1;
    if (ctx->idf_pin_n < n) {
        if (ctx->idf_pin) (void)hipHostFree(ctx->idf_pin);
        ctx->idf_pin = nullptr;
        ctx->idf_pin_n = 0;
        if (hipHostMalloc((void**)&ctx->idf_pin, n * 8, hipHostMallocDefault) != hipSuccess) return TFIDF_E_NOMEM;
        ctx->idf_pin_n = n;
    }
    ctx->idf_full_n = 0;   /* idf_vals is rewritten by this run */
    ctx->idf_pin[0] = 0.0;   /* df >= 1 for every term that occurs */
    idf_post(ctx, ctx->idf_pin, Nt, nullptr, Nt);
    ctx->idf_logs = Nt;
    return TFIDF_OK;
}
/* waits for the table's workers (also on every error path of tfidf_run) */
static void idf_join(tfidf_ctx* ctx) {
    tfidf_ctx::IdfPool& P = ctx->idf_pool;
    if (!P.busy) return;
    const auto w0 = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> lk(P.mu);
    P.done.wait(lk, [&] { return P.left == 0; });
    P.busy = false;
    ctx->ms_idf_wait = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    ctx->ms_idf_host = (double)P.end_ns * 1e-6;
}
struct IdfJoin {
    tfidf_ctx* c;
    ~IdfJoin() { idf_join(c); }
};
/* the table finished by now? (no wait) */
static bool idf_done(tfidf_ctx* ctx) {
    tfidf_ctx::IdfPool& P = ctx->idf_pool;
    std::lock_guard<std::mutex> lk(P.mu);
    return P.left == 0;
}

/* The stages after the DF exchange: idf LUT, document order, score.  They never return 1
 * (run_local checked their scratch before the exchange), so no rank can ever enter the
 * collectives of a repeated attempt alone: every `return` below is an error or success. */
static int run_post(tfidf_ctx* ctx, uint64_t Nt) {
    hipStream_t s = ctx->stream;
    Arena& ar = ctx->arena;
    const uint32_t N = ctx->run_N, V = ctx->run_V;
    const uint64_t cap = ctx->run_cap, R_total = ctx->run_R_total;
    unsigned long long* cnt = ctx->counters.as<unsigned long long>();
    /* ---- idf: log(N/df) on the host's libm (TFIDF.c:243) ----
     * Up to IDF_FULL_MAX documents the host tabulates every possible value, df = 1..N,
     * once per N (cached with the context and uploaded once): the device then reads
     * idf[df] directly and the run needs no host round trip between DF and the score.
     * Above it (c3-size N on one rank) the distinct df values are listed on the device and
     * come back in one round trip with the pair total. */
    mark(ctx, S_IDF);
    const bool full_lut = Nt <= IDF_FULL_MAX;
    uint32_t K = 0;
    uint32_t* vals_dev = nullptr;
    constexpr uint32_t IDF_SPEC = 16384;
    std::vector<uint32_t> vals;
    if (full_lut) {
        if (ctx->idf_early) {       /* on its way up stream3 (run_local) */
            HIPCHK(hipStreamWaitEvent(s, ctx->ev_idf_up, 0));
            ctx->idf_full_n = Nt;
        } else if (ctx->idf_pool.busy) {   /* this run's table (idf_start): join, upload */
            ENSURE(ctx->idf_vals, (size_t)(Nt + 1) * 8);
            idf_join(ctx);
            HIPCHK(hipMemcpyAsync(ctx->idf_vals.p, ctx->idf_pin, (size_t)(Nt + 1) * 8, hipMemcpyHostToDevice, s));
            ctx->idf_pin_busy = true;
            ctx->idf_full_n = Nt;
        } else if (ctx->idf_full_n != Nt) {
            return TFIDF_E_STATE;   /* idf_start made no table and none is cached: not reachable */
        }
    } else {
        ctx->idf_full_n = 0;   /* idf_vals is rewritten below */
        ENSURE(ctx->present, (Nt + 2) * 4);
        HIPCHK(hipMemsetAsync(ctx->present.p, 0, (Nt + 2) * 4, s));
        XCHK(launch_df_mark(df_of_run(ctx), V, ctx->present.as<uint32_t>(), s));
        XCHK(scan_excl_u32(ctx->present.as<uint32_t>(), ctx->present.as<uint32_t>(), Nt + 1, ar, s));
        vals_dev = (uint32_t*)ar.get((size_t)(Nt + 2) * 4);
        if (!vals_dev) return TFIDF_E_CAPACITY;   /* checked by run_local: not reachable */
        XCHK(launch_df_list(ctx->present.as<uint32_t>(), Nt + 1, vals_dev, s));
        const uint32_t spec = (uint32_t)((Nt + 1) < IDF_SPEC ? (Nt + 1) : IDF_SPEC);
        vals.resize(spec);
        HIPCHK(hipMemcpyAsync(&K, ctx->present.as<uint32_t>() + Nt + 1, 4, hipMemcpyDeviceToHost, s));
        if (spec) HIPCHK(hipMemcpyAsync(vals.data(), vals_dev, (size_t)spec * 4, hipMemcpyDeviceToHost, s));
    }
    /* ---- document order: per-position metadata and pair offsets ---- */
    mark(ctx, S_ORDER);
    ENSURE(ctx->npairs_ord, (size_t)N * 8 + 8);
    ENSURE(ctx->out_off, (size_t)N * 8 + 8);
    HIPCHK(hipStreamWaitEvent(s, ctx->ev_order, 0)); /* join the side stream's document order */
    ENSURE(ctx->doc_meta, (size_t)N * 16 + 16);
    XCHK(launch_gather_meta(ctx->order, ctx->doc_npairs.as<uint32_t>(), ctx->doc_recoff.as<uint64_t>(),
                            ctx->doc_size.as<uint32_t>(), ctx->doc_flags.as<uint8_t>(), N,
                            ctx->npairs_ord.as<uint64_t>(), ctx->doc_meta.as<uint4>(), s));
    XCHK(scan_excl_u64(ctx->npairs_ord.as<uint64_t>(), ctx->out_off.as<uint64_t>(), N, ar, s));
    if (!full_lut) {
        XSYNC(s);
        const uint32_t spec = (uint32_t)vals.size();
        if (K > spec) {
            vals.resize(K);
            HIPCHK(hipMemcpy(vals.data() + spec, vals_dev + spec, (size_t)(K - spec) * 4, hipMemcpyDeviceToHost));
        }
        ENSURE(ctx->idf_vals, (size_t)K * 8 + 8);
        /* the distinct df values' logs on the context's workers, into pinned memory */
        if (const int q = idf_pin_quiesce(ctx)) return q;   /* a failed run left an upload of idf_pin unwaited */
        if (ctx->idf_pin_n < (size_t)K + 1) {
            if (ctx->idf_pin) (void)hipHostFree(ctx->idf_pin);
            ctx->idf_pin = nullptr;
            ctx->idf_pin_n = 0;
            if (hipHostMalloc((void**)&ctx->idf_pin, ((size_t)K + 1) * 8, hipHostMallocDefault) != hipSuccess)
                return TFIDF_E_NOMEM;
            ctx->idf_pin_n = (size_t)K + 1;
        }
        if (K) {
            if (K < 2 * 16384) {   /* one worker's share: on this thread, no hand-off and wake-up */
                const auto t0 = std::chrono::steady_clock::now();
                for (uint32_t k = 0; k < K; ++k) ctx->idf_pin[k] = log(1.0 * (double)Nt / (double)vals[k]);
                ctx->ms_idf_host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            } else {
                idf_post(ctx, ctx->idf_pin, Nt, vals.data(), K);
                idf_join(ctx);
            }
            HIPCHK(hipMemcpyAsync(ctx->idf_vals.p, ctx->idf_pin, (size_t)K * 8, hipMemcpyHostToDevice, s));
            ctx->idf_pin_busy = true;
        }
        ctx->idf_logs = K;   /* this run's distinct df values */
    }
    /* the output arrays are sized by the record bound (pairs <= records): the pair total P
     * comes back with the final status word */
    const uint64_t Pmax = R_total;
    /* ---- score + per-document term order ---- */
    mark(ctx, S_SCORE);
    ENSURE(ctx->out_term, Pmax * 4 + 4);
    ENSURE(ctx->out_cnt, Pmax * 4 + 4);
    ENSURE(ctx->out_score, Pmax * 8 + 8);
    ENSURE(ctx->idf_rank, (size_t)V * 8 + 8);
    ENSURE(ctx->large_list, (size_t)N * 8 + 16);   /* wide ranks: handed-off documents; then the K5 class list */
    K5Args a{};
    a.order = ctx->order;
    a.meta = ctx->doc_meta.as<uint4>();
    a.out_off = ctx->out_off.as<uint64_t>();
    a.doc_recoff = ctx->doc_recoff.as<uint64_t>();
    a.doc_npairs = ctx->doc_npairs.as<uint32_t>();
    a.doc_size = ctx->doc_size.as<uint32_t>();
    a.doc_flags = ctx->doc_flags.as<uint8_t>();
    a.rec_slot = ctx->rec_slot.as<uint32_t>();
    a.rec_cnt = ctx->rec_cnt.as<uint32_t>();
    a.rank_of_slot = ctx->rank_of_slot.as<uint32_t>();
    a.df_of_rank = df_of_run(ctx);
    a.idf_idx = full_lut ? nullptr : ctx->present.as<uint32_t>();   /* null: idf indexed by df */
    a.idf = ctx->idf_vals.as<double>();
    a.idf_rank = ctx->idf_rank.as<double>();
    /* large V: 4-byte df gathers + the small idf-by-df table instead of 8-byte idf gathers;
     * only with ranks over 21 bits (the score kernels' wide instance: k5_radix and the
     * common instance read idf by rank) */
    a.idf_by_df = (full_lut && V > (1u << 21)) ? 1u : 0u;
    a.large_list = ctx->large_list.as<uint32_t>() + 1;
    a.large_count = ctx->large_list.as<uint32_t>();
    a.cls_nblk = (N + 255) / 256;
    a.cls_list = ctx->large_list.as<uint32_t>() + N + 2;
    ENSURE(ctx->cls_off, ((size_t)3 * a.cls_nblk + 8) * 4);
    a.cls_off = ctx->cls_off.as<uint32_t>();
    {   /* presorted documents over 4096 pairs are emitted in 4096-pair chunks: <= 2 R / 4096 tasks */
        const uint64_t cap_t = 2 * R_total / 4096 + 64;
        ENSURE(ctx->split_tasks, cap_t * 8 + 8);
        a.split_count = ctx->split_tasks.as<uint32_t>();
        a.split_tasks = ctx->split_tasks.as<uint2>() + 1;
        a.split_cap = (uint32_t)(cap_t < 0xFFFFFFFFull ? cap_t : 0xFFFFFFFFull);
    }
    a.ndocs = N;
    a.nterms = V;
    a.rank_bits = V > 1 ? 32u - (uint32_t)__builtin_clz(V - 1) : 1u;
    a.rec_total = R_total;
    a.slot_cap = cap;
    a.status = (uint32_t*)(cnt + 3);
    a.out_term = ctx->out_term.as<uint32_t>();
    a.out_cnt = ctx->out_cnt.as<uint32_t>();
    a.out_score = ctx->out_score.as<double>();
    XCHK(launch_score_order(a, ar, s, ctx->stream2, ctx->ev_fork, ctx->ev_order));
    mark(ctx, S_NSTAGES);
    {   /* the final status, the pair total and (with a transport) global V: one launch */
        WordList wl{};
        wl.src[0] = cnt + 3;
        wl.bytes[0] = 4;
        wl.src[1] = ctx->out_off.as<uint64_t>() + N;
        wl.bytes[1] = 8;
        wl.src[2] = cnt + 12;
        wl.bytes[2] = 4;
        wl.n = ctx->xp ? 3 : 2;
        if (ctx->xp) {
            XCHK(launch_words_to_host(wl, ctx->hpin_dev + 24, s));
            XSYNC(s);
        } else {
            HIPCHK(words_wait(ctx, wl, 24, s));
        }
    }
    ctx->idf_pin_busy = false;   /* the stream has drained */
    const uint32_t st_end = (uint32_t)ctx->hpin[24];
    const uint64_t P = ctx->hpin[25];
    ctx->npairs = P;
    if (ctx->xp) ctx->Vg = (uint32_t)ctx->hpin[26];
    if (st_end & ST_BOUNDS) {
        fprintf(stderr, "tfidf: internal bounds check tripped (status 0x%x)\n", st_end);
        return TFIDF_E_STATE;
    }
    return 0;
}

/* One attempt of the pipeline: local stages, the DF exchange (with an attached
 * transport every rank enters it, whatever its local status, see exchange_df), the
 * stages after it.  Returns 0 on success, 1 to retry with grown capacities (with a
 * transport: decided by all ranks together), <0 on error. */
static int run_once(tfidf_ctx* ctx, const CorpusDev& c, const uint32_t* dev_ids, uint64_t Nt) {
    int rc = run_local(ctx, c, dev_ids, Nt);
    mark(ctx, S_EXCHANGE);
    if (ctx->xp) {
        rc = exchange_df(ctx, rc, ctx->run_V, c.bytes);
        if (rc) return rc;
    } else {
        if (rc) return rc;
        ctx->Vg = ctx->run_V;   /* one rank: the global df is the local one (df_of_run) */
    }
    return run_post(ctx, Nt);
}

/* Host-side preparation of a run: argument checks, the host corpus copied to HBM. */
static int run_prepare(tfidf_ctx* ctx, const tfidf_corpus* in, CorpusDev& c, const uint32_t*& dev_ids, uint64_t& Nt) {
    if (in->ndocs && !in->doc_off) return TFIDF_E_INVAL;
    if (in->nbytes && !in->bytes) return TFIDF_E_INVAL;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint32_t N = in->ndocs;
    const bool dev = (in->flags & TFIDF_CORPUS_DEVICE) != 0;
    dev_ids = nullptr;
    uint64_t lo = 0, hi = 0;
    if (dev) {
        c.bytes = in->bytes;
        c.doc_off = in->doc_off;
        dev_ids = in->doc_ids;
        uint64_t e[2] = {0, 0};
        if (N) {   /* one round trip on the run's stream (after any work already queued on it) */
            HIPCHK(hipMemcpyAsync(ctx->hpin + 12, in->doc_off, 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(ctx->hpin + 13, in->doc_off + N, 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            e[0] = ctx->hpin[12];
            e[1] = ctx->hpin[13];
        }
        lo = e[0]; hi = e[1];
    } else {
        ENSURE(ctx->in_bytes, in->nbytes + 64);
        ENSURE(ctx->in_off, ((size_t)N + 1) * 8);
        if (in->nbytes) HIPCHK(hipMemcpyAsync(ctx->in_bytes.p, in->bytes, in->nbytes, hipMemcpyHostToDevice, s));
        if (N || in->doc_off) HIPCHK(hipMemcpyAsync(ctx->in_off.p, in->doc_off, ((size_t)N + 1) * 8, hipMemcpyHostToDevice, s));
        if (in->doc_ids) {
            ENSURE(ctx->in_ids, (size_t)N * 4 + 4);
            HIPCHK(hipMemcpyAsync(ctx->in_ids.p, in->doc_ids, (size_t)N * 4, hipMemcpyHostToDevice, s));
            dev_ids = ctx->in_ids.as<uint32_t>();
        }
        c.bytes = ctx->in_bytes.as<uint8_t>();
        c.doc_off = ctx->in_off.as<uint64_t>();
        if (N) { lo = in->doc_off[0]; hi = in->doc_off[N]; }
        HIPCHK(hipStreamSynchronize(s));
    }
    if (hi > in->nbytes || lo > hi) return TFIDF_E_INVAL;
    c.nbytes = in->nbytes;
    c.ndocs = N;
    c.lo = lo;
    c.hi = hi;
    Nt = in->ndocs_total ? in->ndocs_total : N;
    if (Nt < N || Nt > 0xFFFFFFFFull) return TFIDF_E_INVAL;
    return TFIDF_OK;
}

extern "C" int tfidf_run(tfidf_ctx* ctx, const tfidf_corpus* in) {
    if (!ctx) return TFIDF_E_INVAL;
    ctx->have_result = false;
    ctx->have_model = false;   /* an imported model goes as a previous run's does */
    ctx->model_only = false;
    ctx->have_info = false;
    ctx->text_valid = false;
    ctx->tmeta_valid = false;
    ctx->norm_valid = false;
    ctx->bm25_L_valid = false;
    CorpusDev c{};
    const uint32_t* dev_ids = nullptr;
    uint64_t Nt = 0;
    int rc = in ? run_prepare(ctx, in, c, dev_ids, Nt) : TFIDF_E_INVAL;
    if (rc) {
        /* a rank that fails before its first stage still takes part in the agreement, so
         * its peers return TFIDF_E_PEER instead of waiting for it */
        if (ctx->xp) (void)exchange_agree(ctx, rc, 0, nullptr);
        return rc;
    }
    hipStream_t s = ctx->stream;
    const uint32_t N = in->ndocs;
    IdfJoin idf_guard{ctx};
    rc = idf_start(ctx, Nt);
    if (rc) {
        if (ctx->xp) (void)exchange_agree(ctx, rc, 0, nullptr);
        return rc;
    }
    rc = 1;
    for (int attempt = 0; attempt < 8 && rc == 1; ++attempt) {
        const size_t need = ctx->arena.peak > ctx->arena_buf.cap ? ctx->arena.peak * 2 : ctx->arena_buf.cap;
        const int arc = arena_reset(ctx, need);
        /* with peers, an allocation failure is reported through the agreement as well */
        rc = arc ? arc : run_once(ctx, c, dev_ids, Nt);
        if (arc && ctx->xp) (void)exchange_agree(ctx, arc, 0, nullptr);
        if (rc == 1) {
            HIPCHK(hipStreamSynchronize(s));
            HIPCHK(hipStreamSynchronize(ctx->stream2));
            HIPCHK(hipStreamSynchronize(ctx->stream3));   /* the early idf upload (run_local) */
        }
    }
    if (rc == 1) return TFIDF_E_CAPACITY;
    if (rc) return rc;
    ctx->corpus = *in;
    ctx->run_nbytes = c.hi - c.lo;
    ctx->dev_bytes = c.bytes;
    ctx->dev_ids = dev_ids;
    ctx->ndocs = N;
    ctx->ndocs_total = Nt;
    ctx->have_result = true;
    ctx->have_model = true;
    ctx->have_info = true;
    ctx->info_npairs = ctx->npairs;
    ctx->info_V = ctx->V;
    ctx->wt_tf = ctx->wt_idf = ctx->wt_norm = 0;   /* a run's scores are the reference's */
    ctx->rw_idf_mode = 0;
    if (ctx->timing) (void)hipEventSynchronize(ctx->ev[S_NSTAGES]);   /* done on the device; the runtime may not know yet */
    if (ctx->timing == 2) {
        for (int i = 0; i < S_NSTAGES; ++i) ctx->ms_stage[i] = 0;
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ctx->ev[S_TOKCOUNT], ctx->ev[S_VOCAB]);
        ctx->ms_stage[S_TOKCOUNT] = ms;
        float tot = 0;
        (void)hipEventElapsedTime(&tot, ctx->ev[S_PREP], ctx->ev[S_NSTAGES]);
        ctx->ms_total = tot;
    } else if (ctx->timing) {
        for (int i = 0; i < S_NSTAGES; ++i) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, ctx->ev[i], ctx->ev[i + 1]);
            ctx->ms_stage[i] = ms;
        }
        float tot = 0;
        (void)hipEventElapsedTime(&tot, ctx->ev[S_PREP], ctx->ev[S_NSTAGES]);
        ctx->ms_total = tot;
    }
    ctx->totals.runs += 1;
    ctx->totals.ms_tokcount += ctx->timing ? ctx->ms_stage[S_TOKCOUNT] : 0.0;
    ctx->totals.ms_total += ctx->timing ? ctx->ms_total : 0.0;
    ctx->totals.idf_logs += ctx->idf_logs;
    ctx->totals.ms_idf_host += ctx->ms_idf_host;
    ctx->totals.ms_idf_wait += ctx->ms_idf_wait;
    return TFIDF_OK;
}

extern "C" int tfidf_run_totals_get(tfidf_ctx* ctx, tfidf_run_totals* out, int reset) {
    if (!ctx || !out) return TFIDF_E_INVAL;
    *out = ctx->totals;
    if (reset) ctx->totals = tfidf_run_totals{};
    return TFIDF_OK;
}

extern "C" int tfidf_debug_k1_stamps(tfidf_ctx* ctx, uint64_t* out, int n) {
    if (!ctx || !out || n <= 0) return TFIDF_E_INVAL;
    if (!ctx->stamps_on || !ctx->stamps.p) return TFIDF_E_STATE;
    int m = n < K1_DEBUG_WORDS ? n : K1_DEBUG_WORDS;
    HIPCHK(hipMemcpy(out, ctx->stamps.p, 8 * (size_t)m, hipMemcpyDeviceToHost));
    return m;
}

/* Measured HBM streaming peaks: `iters` timed passes of a read-only stream
 * over nbytes and of an nbytes copy (counted as 2 x nbytes), after one warm-up pass each;
 * the buffers are allocated for the call and released. */
extern "C" int tfidf_hbm_probe(tfidf_ctx* ctx, uint64_t nbytes, int iters, double* read_gbps, double* copy_gbps) {
    if (!ctx || !read_gbps || !copy_gbps || nbytes < 4096 || iters <= 0) return TFIDF_E_INVAL;
    HIPCHK(hipSetDevice(ctx->device));
    nbytes &= ~(uint64_t)4095;
    hipStream_t s = ctx->stream;
    void *a = nullptr, *b = nullptr;
    uint32_t* sink = nullptr;
    if (tfidf_dev_malloc(&a, nbytes) != hipSuccess) return TFIDF_E_NOMEM;
    if (tfidf_dev_malloc(&b, nbytes) != hipSuccess) { (void)hipFree(a); return TFIDF_E_NOMEM; }
    if (tfidf_dev_malloc((void**)&sink, 256) != hipSuccess) { (void)hipFree(a); (void)hipFree(b); return TFIDF_E_NOMEM; }
    int ncu = 256, dev = 0;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    const unsigned grid = (unsigned)(ncu > 0 ? ncu : 256) * 16u;
    hipEvent_t e0, e1;
    int rc = TFIDF_OK;
    float ms_r = 0.f, ms_c = 0.f;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = TFIDF_E_HIP;
    if (!rc && (hipMemsetAsync(a, 0, nbytes, s) != hipSuccess || hipMemsetAsync(b, 0, nbytes, s) != hipSuccess)) rc = TFIDF_E_HIP;
    if (!rc && (launch_stream_read(a, nbytes, sink, grid, s) || launch_stream_copy(a, b, nbytes, grid, s))) rc = TFIDF_E_HIP;
    if (!rc) {
        bool ok = hipEventRecord(e0, s) == hipSuccess;
        for (int i = 0; ok && i < iters; ++i) ok = launch_stream_read(a, nbytes, sink, grid, s) == 0;
        ok = ok && hipEventRecord(e1, s) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
             hipEventElapsedTime(&ms_r, e0, e1) == hipSuccess;
        ok = ok && hipEventRecord(e0, s) == hipSuccess;
        for (int i = 0; ok && i < iters; ++i) ok = launch_stream_copy(a, b, nbytes, grid, s) == 0;
        ok = ok && hipEventRecord(e1, s) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
             hipEventElapsedTime(&ms_c, e0, e1) == hipSuccess;
        if (!ok) rc = TFIDF_E_HIP;
    }
    if (!rc) {
        *read_gbps = ms_r > 0 ? (double)nbytes * iters / (ms_r * 1e-3) / 1e9 : 0.0;
        *copy_gbps = ms_c > 0 ? 2.0 * (double)nbytes * iters / (ms_c * 1e-3) / 1e9 : 0.0;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipStreamSynchronize(s);
    (void)hipFree(a);
    (void)hipFree(b);
    (void)hipFree(sink);
    return rc;
}

extern "C" int tfidf_alloc_stats(uint64_t* allocs, uint64_t* bytes) {
    if (!allocs || !bytes) return TFIDF_E_INVAL;
    *allocs = g_dev_allocs.load(std::memory_order_relaxed);
    *bytes = g_dev_alloc_bytes.load(std::memory_order_relaxed);
    return TFIDF_OK;
}

extern "C" int tfidf_last_run_info(tfidf_ctx* ctx, tfidf_run_info* out) {
    tfidf_run_info* info = out;
    if (!ctx || !info || info->size < 16) return TFIDF_E_INVAL;
    if (!ctx->have_info) return TFIDF_E_STATE;
    const size_t want = info->size < sizeof(tfidf_run_info) ? (size_t)info->size : sizeof(tfidf_run_info);
    tfidf_run_info full;
    memset(&full, 0, sizeof(full));
    info = &full;   /* filled whole here, copied out up to the caller's size below */
    info->nbytes = ctx->run_nbytes;   /* no device round trip: the run read the bounds */
    info->ntokens = ctx->ntokens;
    info->npairs = ctx->info_npairs;
    info->nterms = ctx->info_V;
    info->nterms_global = ctx->Vg;
    info->nchunks = ctx->nchunks;
    info->partial_records = ctx->nrec_part;
    info->ndocs = ctx->ndocs;
    info->vocab_capacity = (uint32_t)ctx->vcap;
    info->ms_total = ctx->ms_total;
    info->ms_tokcount = ctx->ms_stage[S_TOKCOUNT];
    for (int i = 0; i < S_NSTAGES; ++i) info->ms_stage[i] = ctx->ms_stage[i];
    info->nstages = S_NSTAGES;
    info->flags = (ctx->k1_vs ? TFIDF_RUN_K1_VS : 0u) | (ctx->k1_sl ? TFIDF_RUN_K1_SL : 0u) |
                  (ctx->xp && ctx->last_dense ? TFIDF_RUN_XCHG_DENSE : 0u);
    info->device_allocs = g_dev_allocs.load(std::memory_order_relaxed);
    info->device_alloc_bytes = g_dev_alloc_bytes.load(std::memory_order_relaxed);
    info->idf_logs = ctx->idf_logs;
    info->ms_idf_host = ctx->ms_idf_host;
    info->ms_idf_wait = ctx->ms_idf_wait;
    full.size = want;
    memcpy(out, &full, want);
    return TFIDF_OK;
}

/* ------------------------------------------------------------------- fetch -- */

extern "C" void tfidf_result_free(tfidf_result* r) {
    if (!r) return;
    free(r->pair_doc); free(r->pair_term); free(r->pair_count); free(r->pair_docsize); free(r->pair_df);
    free(r->pair_score); free(r->doc_id); free(r->doc_size); free(r->term_off); free(r->term_bytes);
    free(r->term_df);
    memset(r, 0, sizeof(*r));
}

extern "C" int tfidf_fetch(tfidf_ctx* ctx, tfidf_result* r) {
    if (!ctx || !r) return TFIDF_E_INVAL;
    if (!ctx->have_result) return TFIDF_E_STATE;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    memset(r, 0, sizeof(*r));
    const uint64_t P = ctx->npairs;
    const uint32_t N = ctx->ndocs, V = ctx->V;
    r->npairs = P;
    r->ndocs = N;
    r->nterms = V;
    r->ndocs_total = ctx->ndocs_total;
    size_t p4 = (size_t)P * 4 + 4;
    r->pair_doc = (uint32_t*)malloc(p4);
    r->pair_term = (uint32_t*)malloc(p4);
    r->pair_count = (uint32_t*)malloc(p4);
    r->pair_docsize = (uint32_t*)malloc(p4);
    r->pair_df = (uint32_t*)malloc(p4);
    r->pair_score = (double*)malloc((size_t)P * 8 + 8);
    r->doc_id = (uint32_t*)malloc((size_t)N * 4 + 4);
    r->doc_size = (uint32_t*)malloc((size_t)N * 4 + 4);
    r->term_df = (uint32_t*)malloc((size_t)V * 4 + 4);
    r->term_off = (uint64_t*)malloc(((size_t)V + 1) * 8);
    if (!r->pair_doc || !r->pair_term || !r->pair_count || !r->pair_docsize || !r->pair_df || !r->pair_score ||
        !r->doc_id || !r->doc_size || !r->term_df || !r->term_off) {
        tfidf_result_free(r);
        return TFIDF_E_NOMEM;
    }
    std::vector<uint32_t> order(N);
    std::vector<uint64_t> ooff((size_t)N + 1);
    if (P) {
        HIPCHK(hipMemcpyAsync(r->pair_term, ctx->out_term.p, P * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(r->pair_count, ctx->out_cnt.p, P * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(r->pair_score, ctx->out_score.p, P * 8, hipMemcpyDeviceToHost, s));
    }
    if (N) {
        HIPCHK(hipMemcpyAsync(r->doc_size, ctx->doc_size.p, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(order.data(), ctx->order, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(ooff.data(), ctx->out_off.p, ((size_t)N + 1) * 8, hipMemcpyDeviceToHost, s));
    }
    if (V) HIPCHK(hipMemcpyAsync(r->term_df, df_of_run(ctx), (size_t)V * 4, hipMemcpyDeviceToHost, s));
    /* term strings in rank order */
    std::vector<uint4> keys(V);
    std::vector<uint32_t> sor(V);
    if (V) {
        HIPCHK(hipMemcpyAsync(sor.data(), ctx->slot_of_rank.p, (size_t)V * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        ENSURE(ctx->x_mine, (size_t)V * 16 + 16);
        if (launch_keys_by_rank(ctx->vkeys.as<uint4>(), ctx->slot_of_rank.as<uint32_t>(), V, ctx->x_mine.as<uint4>(), s))
            return TFIDF_E_HIP;
        HIPCHK(hipMemcpyAsync(keys.data(), ctx->x_mine.p, (size_t)V * 16, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->corpus.doc_ids && !(ctx->corpus.flags & TFIDF_CORPUS_DEVICE)) {
        memcpy(r->doc_id, ctx->corpus.doc_ids, (size_t)N * 4);
    } else if (ctx->dev_ids) {
        HIPCHK(hipMemcpy(r->doc_id, ctx->dev_ids, (size_t)N * 4, hipMemcpyDeviceToHost));
    } else {
        for (uint32_t i = 0; i < N; ++i) r->doc_id[i] = i + 1;
    }
    /* per-pair document, docSize and df: expanded from the per-document output order
     * (K5 writes 16 bytes per pair) */
    for (uint32_t j = 0; j < N; ++j) {
        const uint32_t d = order[j];
        const uint32_t id = r->doc_id[d], dsz = r->doc_size[d];
        for (uint64_t q = ooff[j]; q < ooff[j + 1] && q < P; ++q) {
            r->pair_doc[q] = id;
            r->pair_docsize[q] = dsz;
        }
    }
    for (uint64_t q = 0; q < P; ++q) r->pair_df[q] = r->pair_term[q] < V ? r->term_df[r->pair_term[q]] : 0u;
    std::string pool;
    pool.reserve((size_t)V * 8);
    for (uint32_t t = 0; t < V; ++t) {
        r->term_off[t] = pool.size();
        uint64_t lo = ((uint64_t)keys[t].y << 32) | keys[t].x, hi = ((uint64_t)keys[t].w << 32) | keys[t].z;
        if ((hi >> 56) == 0xFFu) {
            uint64_t rep = 0;
            HIPCHK(hipMemcpy(&rep, ctx->vrep.as<uint64_t>() + sor[t], 8, hipMemcpyDeviceToHost));
            uint64_t off = rep & 0xFFFFFFFFFFull, len = rep >> 40;
            std::string w(len, '\0');
            HIPCHK(hipMemcpy(&w[0], ctx->dev_bytes + off, len, hipMemcpyDeviceToHost));
            pool += w;
        } else {
            uint8_t b[16];
            memcpy(b, &lo, 8);
            memcpy(b + 8, &hi, 8);
            int n = 0;
            while (n < 16 && b[n] != 0x09) ++n;
            pool.append((const char*)b, (size_t)n);
        }
    }
    r->term_off[V] = pool.size();
    r->term_bytes = (uint8_t*)malloc(pool.size() + 1);
    if (!r->term_bytes) { tfidf_result_free(r); return TFIDF_E_NOMEM; }
    memcpy(r->term_bytes, pool.data(), pool.size());
    return TFIDF_OK;
}

/* ----------------------------------------------------------------- synthetic -- */

/* ----------------------------------------------------------------- ingest ----
 * ingest.cpp streams input/doc1..N into the context's host-input buffers (§8f row 2). */
int tfidf_ctx_ingest_buffers(tfidf_ctx* ctx, uint64_t nbytes, uint32_t ndocs, uint8_t** dbytes, uint64_t** doff,
                             uint32_t** dids) {
    HIPCHK(hipSetDevice(ctx->device));
    ENSURE(ctx->in_bytes, nbytes + 64);
    ENSURE(ctx->in_off, ((size_t)ndocs + 1) * 8);
    *dbytes = ctx->in_bytes.as<uint8_t>();
    *doff = ctx->in_off.as<uint64_t>();
    if (dids) {
        ENSURE(ctx->in_ids, (size_t)ndocs * 4 + 4);
        *dids = ctx->in_ids.as<uint32_t>();
    }
    return TFIDF_OK;
}

extern "C" int tfidf_synth_device(tfidf_ctx* ctx, uint64_t seed, uint32_t V, uint32_t mode, const double* cdf,
                                  const uint32_t* doc_ids, const uint64_t* ntok, uint32_t ndocs,
                                  uint64_t ndocs_total, tfidf_corpus* out) {
    if (!ctx || !ntok || !out || V == 0 || (mode == SYN_MODE_ZIPF && !cdf)) return TFIDF_E_INVAL;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    std::vector<uint64_t> bf((size_t)ndocs + 1);
    uint64_t nb = 0;
    for (uint32_t i = 0; i < ndocs; ++i) { bf[i] = nb; nb += (ntok[i] + SYN_BLOCK_TOKENS - 1) / SYN_BLOCK_TOKENS; }
    bf[ndocs] = nb;
    ENSURE(ctx->syn_blkfirst, bf.size() * 8);
    ENSURE(ctx->syn_ntok, (size_t)ndocs * 8 + 8);
    ENSURE(ctx->syn_blkbytes, (nb + 1) * 8);
    ENSURE(ctx->syn_off, ((size_t)ndocs + 1) * 8);
    HIPCHK(hipMemcpyAsync(ctx->syn_blkfirst.p, bf.data(), bf.size() * 8, hipMemcpyHostToDevice, s));
    if (ndocs) HIPCHK(hipMemcpyAsync(ctx->syn_ntok.p, ntok, (size_t)ndocs * 8, hipMemcpyHostToDevice, s));
    const uint32_t* dids = nullptr;
    if (doc_ids) {
        ENSURE(ctx->syn_ids, (size_t)ndocs * 4 + 4);
        HIPCHK(hipMemcpyAsync(ctx->syn_ids.p, doc_ids, (size_t)ndocs * 4, hipMemcpyHostToDevice, s));
        dids = ctx->syn_ids.as<uint32_t>();
    }
    const double* dcdf = nullptr;
    if (mode == SYN_MODE_ZIPF) {
        ENSURE(ctx->syn_cdf, (size_t)V * 8);
        HIPCHK(hipMemcpyAsync(ctx->syn_cdf.p, cdf, (size_t)V * 8, hipMemcpyHostToDevice, s));
        dcdf = ctx->syn_cdf.as<double>();
    }
    syn_spec sp;
    tfidf_synth_spec(&sp, seed, V, mode, dcdf);
    if (arena_reset(ctx, ctx->arena_buf.cap) != 0) return TFIDF_E_NOMEM;
    if (launch_synth_bytes(&sp, dids, ctx->syn_ntok.as<uint64_t>(), ctx->syn_blkfirst.as<uint64_t>(), nb, ndocs,
                           ctx->syn_blkbytes.as<uint64_t>(), s))
        return TFIDF_E_HIP;
    if (scan_excl_u64(ctx->syn_blkbytes.as<uint64_t>(), ctx->syn_blkbytes.as<uint64_t>(), nb, ctx->arena, s))
        return TFIDF_E_HIP;
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, ctx->syn_blkbytes.as<uint64_t>() + nb, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ENSURE(ctx->syn_bytes, total + 64);
    if (launch_synth_fill(&sp, dids, ctx->syn_ntok.as<uint64_t>(), ctx->syn_blkfirst.as<uint64_t>(), nb, ndocs,
                          ctx->syn_blkbytes.as<uint64_t>(), ctx->syn_bytes.as<uint8_t>(), ctx->syn_off.as<uint64_t>(), s))
        return TFIDF_E_HIP;
    HIPCHK(hipStreamSynchronize(s));
    memset(out, 0, sizeof(*out));
    out->bytes = ctx->syn_bytes.as<uint8_t>();
    out->nbytes = total;
    out->doc_off = ctx->syn_off.as<uint64_t>();
    out->doc_ids = dids;
    out->ndocs = ndocs;
    out->flags = TFIDF_CORPUS_DEVICE;
    out->ndocs_total = ndocs_total ? ndocs_total : ndocs;
    return TFIDF_OK;
}

/* ------------------------------------------------------------ emission (GPU) ----
 * the "docN@word\t%.16f\n" lines (TFIDF.c:245,281) formatted in HBM
 * by emit.hip (exact round-half-even %.16f), then copied out / written to output.txt
 * (TFIDF.c:274-282). */
/* the length pass: term metadata, bytes per output position, their scan (doc_toff) and
 * the text buffer sized to the total (one synchronisation for the total) */
static int format_prepare(tfidf_ctx* ctx, EmitLaunch& e, uint64_t& total) {
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint32_t N = ctx->ndocs, V = ctx->V;
    unsigned long long* cnt = ctx->counters.as<unsigned long long>();
    uint32_t* status = (uint32_t*)(cnt + 3);
    HIPCHK(hipMemsetAsync(status, 0, 4, s));
    ENSURE(ctx->t_key, (size_t)V * 16 + 16);
    ENSURE(ctx->t_len, (size_t)V * 4 + 4);
    ENSURE(ctx->doc_tbytes, ((size_t)N + 1) * 8);
    ENSURE(ctx->doc_toff, ((size_t)N + 1) * 8);
    if (launch_term_meta(ctx->vkeys.as<uint4>(), ctx->vrep.as<uint64_t>(), ctx->slot_of_rank.as<uint32_t>(), V,
                         ctx->t_key.as<uint4>(), ctx->t_len.as<uint32_t>(), s))
        return TFIDF_E_HIP;
    ctx->tmeta_valid = true;
    e = EmitLaunch{ctx->order, ctx->dev_ids, ctx->out_off.as<uint64_t>(), ctx->out_term.as<uint32_t>(),
                   ctx->out_score.as<double>(), ctx->t_key.as<uint4>(), ctx->t_len.as<uint32_t>(), ctx->dev_bytes, N,
                   status};
    total = 0;
    if (N) {
        if (launch_emit_bytes(e, ctx->doc_tbytes.as<uint64_t>(), s)) return TFIDF_E_HIP;
        ctx->arena.used = 0;
        if (scan_excl_u64(ctx->doc_tbytes.as<uint64_t>(), ctx->doc_toff.as<uint64_t>(), N, ctx->arena, s))
            return TFIDF_E_HIP;
        HIPCHK(hipMemcpyAsync(&ctx->hpin[20], ctx->doc_toff.as<uint64_t>() + N, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        total = ctx->hpin[20];
    }
    ENSURE(ctx->text, total + 64);
    return TFIDF_OK;
}

/* the formatter's status after its launches (the stream is synchronised by the caller) */
static int format_finish(tfidf_ctx* ctx, uint64_t total) {
    uint32_t* status = (uint32_t*)(ctx->counters.as<unsigned long long>() + 3);
    ctx->hpin[21] = 0;
    HIPCHK(hipMemcpyAsync(&ctx->hpin[21], status, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if ((uint32_t)ctx->hpin[21] & ST_BOUNDS) {
        fprintf(stderr, "tfidf: score outside the %%.16f formatter's range\n");
        return TFIDF_E_STATE;
    }
    ctx->text_bytes = total;
    ctx->text_valid = true;
    return TFIDF_OK;
}

extern "C" int tfidf_format(tfidf_ctx* ctx, uint64_t* nbytes) {
    if (!ctx || !nbytes) return TFIDF_E_INVAL;
    if (!ctx->have_result) return TFIDF_E_STATE;
    if (ctx->text_valid) { *nbytes = ctx->text_bytes; return TFIDF_OK; }
    EmitLaunch e{};
    uint64_t total = 0;
    int rc = format_prepare(ctx, e, total);
    if (rc) return rc;
    if (total && launch_emit_write(e, ctx->doc_toff.as<uint64_t>(), ctx->text.as<uint8_t>(), ctx->stream))
        return TFIDF_E_HIP;
    rc = format_finish(ctx, total);
    if (!rc) *nbytes = total;
    return rc;
}

extern "C" int tfidf_copy_text(tfidf_ctx* ctx, uint64_t off, void* dst, uint64_t n) {
    if (!ctx || (n && !dst)) return TFIDF_E_INVAL;
    if (!ctx->text_valid) return TFIDF_E_STATE;
    if (off > ctx->text_bytes || n > ctx->text_bytes - off) return TFIDF_E_INVAL;
    if (!n) return TFIDF_OK;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpy(dst, ctx->text.as<uint8_t>() + off, n, hipMemcpyDeviceToHost));
    return TFIDF_OK;
}

/* output.txt (TFIDF.c:274-282): the text leaves HBM through a ring of WR_NBUF pinned
 * 16 MB staging buffers owned by the context (allocated on first use and kept: pinning
 * 128 MB costs ~20 ms per call).  The copies run on stream2 while the host writes the
 * buffers already copied; when the text is not yet formatted, the formatter runs in
 * WR_GROUPS document groups on the main stream and each copy waits only for the group
 * that holds its last byte, so formatting of group g+1 overlaps the copy of group g. */
static int wr_ring_init(tfidf_ctx* ctx) {
    if (ctx->wr_buf[0]) return TFIDF_OK;
    for (int i = 0; i < WR_NBUF; ++i) {
        if (hipHostMalloc((void**)&ctx->wr_buf[i], WR_BUF, hipHostMallocDefault) != hipSuccess) {
            ctx->wr_buf[i] = nullptr;
            for (int j = 0; j < i; ++j) { (void)hipHostFree(ctx->wr_buf[j]); ctx->wr_buf[j] = nullptr; }
            return TFIDF_E_NOMEM;
        }
    }
    for (int i = 0; i < WR_NBUF; ++i) HIPCHK(hipEventCreateWithFlags(&ctx->wr_ev[i], hipEventDisableTiming));
    for (int i = 0; i < WR_GROUPS; ++i) HIPCHK(hipEventCreateWithFlags(&ctx->wr_fmt[i], hipEventDisableTiming));
    return TFIDF_OK;
}

static double now_ms() {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

extern "C" int tfidf_write_output_gpu(tfidf_ctx* ctx, const char* path, int append) {
    if (!ctx || !path) return TFIDF_E_INVAL;
    if (!ctx->have_result) return TFIDF_E_STATE;
    const double t0 = now_ms();
    tfidf_output_info oi{};
    oi.size = sizeof(oi);
    HIPCHK(hipSetDevice(ctx->device));
    int rc = wr_ring_init(ctx);
    if (rc) return rc;
    hipStream_t s = ctx->stream, cs = ctx->stream2;
    const uint32_t N = ctx->ndocs;
    uint64_t total = ctx->text_bytes;
    /* group g covers output positions [N g / ng, N (g+1) / ng) and text bytes [gb[g], gb[g+1]) */
    uint64_t gb[WR_GROUPS + 1];
    int ng = 0;
    const bool fmt = !ctx->text_valid;
    if (fmt) {
        EmitLaunch e{};
        rc = format_prepare(ctx, e, total);
        if (rc) return rc;
        ng = N ? (N < WR_GROUPS ? (int)N : WR_GROUPS) : 0;
        std::vector<uint64_t> toff((size_t)N + 1);
        if (N) HIPCHK(hipMemcpy(toff.data(), ctx->doc_toff.p, ((size_t)N + 1) * 8, hipMemcpyDeviceToHost));
        for (int g = 0; g < ng; ++g) {
            const uint32_t d0 = (uint32_t)((uint64_t)N * g / ng), d1 = (uint32_t)((uint64_t)N * (g + 1) / ng);
            gb[g] = toff[d0];
            gb[g + 1] = toff[d1];
            if (launch_emit_write(e, ctx->doc_toff.as<uint64_t>(), ctx->text.as<uint8_t>(), s, d0, d1))
                return TFIDF_E_HIP;
            HIPCHK(hipEventRecord(ctx->wr_fmt[g], s));
        }
        oi.formatted = 1;
    }
    const double t_prep = now_ms();
    oi.ms_prepare = fmt ? t_prep - t0 : 0.0;
    const int fd = open(path, O_WRONLY | O_CREAT | (append ? 0 : O_TRUNC), 0644);
    if (fd < 0) { (void)hipStreamSynchronize(s); return TFIDF_E_OUTPUT; }
    struct stat fst;
    const bool regular = fstat(fd, &fst) == 0 && S_ISREG(fst.st_mode);
    /* a regular file: blocks written at their offsets by WR_WRITERS threads (page-cache
     * copies in parallel); anything else (a pipe, /dev/null): one thread, in order */
    const uint64_t base = append && regular ? (uint64_t)fst.st_size : 0;
    if (!regular && append) (void)lseek(fd, 0, SEEK_END);
    const uint8_t* src = ctx->text.as<uint8_t>();
    const uint64_t nblk = (total + WR_BUF - 1) / WR_BUF;
    const int nw = regular ? (nblk < (uint64_t)WR_WRITERS ? (int)(nblk ? nblk : 1) : WR_WRITERS) : 1;
    oi.writers = (uint32_t)nw;
    std::mutex mu;
    std::condition_variable cv;
    uint64_t issued = 0;             /* blocks whose copies were sent */
    uint64_t freed[WR_NBUF] = {0};   /* per ring buffer: blocks it has finished (written) */
    bool failed = false;
    int wrc = TFIDF_OK;
    double t_last_copy = t_prep, write_ms = 0.0;
    auto blk_n = [&](uint64_t k) { return (k + 1) * WR_BUF <= total ? WR_BUF : total - k * WR_BUF; };
    /* writer w takes blocks k = w, w + nw, ...: waits for the copy, writes, frees the buffer */
    auto writer = [&](int w) {
        double my_write = 0.0, my_last = 0.0;
        for (uint64_t k = (uint64_t)w; k < nblk; k += (uint64_t)nw) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return issued > k || failed; });
                if (failed) break;
            }
            const int b = (int)(k % WR_NBUF);
            bool ok = hipEventSynchronize(ctx->wr_ev[b]) == hipSuccess;
            const double tc = now_ms();
            my_last = tc > my_last ? tc : my_last;
            const uint64_t n = blk_n(k);
            uint64_t done = 0;
            while (ok && done < n) {
                const ssize_t r = regular ? pwrite(fd, ctx->wr_buf[b] + done, n - done, (off_t)(base + k * WR_BUF + done))
                                          : write(fd, ctx->wr_buf[b] + done, n - done);
                if (r <= 0) { ok = false; break; }
                done += (uint64_t)r;
            }
            my_write += now_ms() - tc;
            std::lock_guard<std::mutex> lk(mu);
            if (!ok) {
                failed = true;
                if (!wrc) wrc = done < n ? TFIDF_E_OUTPUT : TFIDF_E_HIP;
            }
            freed[b] = k + 1;
            cv.notify_all();
            if (failed) break;
        }
        std::lock_guard<std::mutex> lk(mu);
        write_ms += my_write;
        if (my_last > t_last_copy) t_last_copy = my_last;
    };
    std::vector<std::thread> th;
    for (int w = 1; w < nw; ++w) th.emplace_back(writer, w);
    /* issue: block k reuses ring buffer k % WR_NBUF once block k - WR_NBUF is written; its
     * copy waits (on the copy stream) for every format group holding one of its bytes */
    std::thread issuer([&] {
        (void)hipSetDevice(ctx->device);
        int gwait = 0;
        for (uint64_t k = 0; k < nblk; ++k) {
            const int b = (int)(k % WR_NBUF);
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return k < WR_NBUF || freed[b] >= k - WR_NBUF + 1 || failed; });
                if (failed) return;
            }
            const uint64_t b0 = k * WR_BUF, n = blk_n(k);
            bool ok = true;
            while (fmt && gwait < ng && gb[gwait] < b0 + n) {
                if (hipStreamWaitEvent(cs, ctx->wr_fmt[gwait], 0) != hipSuccess) ok = false;
                ++gwait;
            }
            if (ok && (hipMemcpyAsync(ctx->wr_buf[b], src + b0, n, hipMemcpyDeviceToHost, cs) != hipSuccess ||
                       hipEventRecord(ctx->wr_ev[b], cs) != hipSuccess))
                ok = false;
            std::lock_guard<std::mutex> lk(mu);
            if (!ok) { failed = true; if (!wrc) wrc = TFIDF_E_HIP; }
            else issued = k + 1;
            cv.notify_all();
            if (failed) return;
        }
    });
    (void)hipSetDevice(ctx->device);
    writer(0);
    issuer.join();
    for (auto& t : th) t.join();
    (void)hipStreamSynchronize(cs);
    rc = wrc;
    if (fmt) {
        const int r2 = format_finish(ctx, total);   /* synchronises the main stream */
        if (!rc) rc = r2;
        /* a formatting error (a score outside the %.16f range: ST_BOUNDS) found after the
         * blocks were written: no complete-looking file is left behind — the file (or the
         * appended shard) is cut back to where this call started */
        if (r2 && regular) (void)!ftruncate(fd, (off_t)base);
    }
    if (close(fd) != 0 && !rc) rc = TFIDF_E_OUTPUT;
    oi.text_bytes = total;
    oi.ms_d2h_busy = nblk ? t_last_copy - t_prep : 0.0;
    oi.ms_write = write_ms;
    oi.ms_total = now_ms() - t0;
    ctx->out_info = oi;
    return rc;
}

extern "C" int tfidf_last_output_info(const tfidf_ctx* ctx, tfidf_output_info* info) {
    if (!ctx || !info || info->size < sizeof(uint64_t)) return TFIDF_E_INVAL;
    const uint64_t n = info->size < sizeof(tfidf_output_info) ? info->size : sizeof(tfidf_output_info);
    tfidf_output_info o = ctx->out_info;
    o.size = n;
    memcpy(info, &o, (size_t)n);
    return TFIDF_OK;
}

extern "C" int tfidf_format_f64(tfidf_ctx* ctx, const double* vals, uint64_t n, char* out) {
    if (!ctx || (n && (!vals || !out))) return TFIDF_E_INVAL;
    if (!n) return TFIDF_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    DevBuf v, o;
    if (v.ensure(n * 8) || o.ensure(n * 32)) { v.release(); o.release(); return TFIDF_E_NOMEM; }
    unsigned long long* cnt = ctx->counters.as<unsigned long long>();
    uint32_t* status = (uint32_t*)(cnt + 3);
    uint32_t st = 0;
    int rc = TFIDF_OK;
    if (hipMemsetAsync(status, 0, 4, s) != hipSuccess ||
        hipMemcpyAsync(v.p, vals, n * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
        launch_format_f64(v.as<double>(), n, o.as<uint8_t>(), status, s) ||
        hipMemcpyAsync(out, o.p, n * 32, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(&st, status, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        rc = TFIDF_E_HIP;
    v.release();
    o.release();
    if (!rc && (st & ST_BOUNDS)) rc = TFIDF_E_INVAL;
    return rc;
}

/* ------------------------------------------------------------------- query ----
 * Top-k retrieval over the resident result (query.hip).  The host tokenises the batch
 * (fscanf("%s") tokens, terms cut at their first NUL: TFIDF.c:141-147,152), the device maps
 * the batch's distinct terms to term ranks, and every group of queries takes one pass over
 * the pairs and a few top-k rounds.  The vocabulary table is only read: no stage after K1
 * writes vkeys or vrep (the vocabulary stage reads them into its own sort keys and writes
 * rank_of_slot at the used slots; fetch and format read them again), and all three K1
 * kernels insert from the pair-aligned home (vocab_insert's default, VS_HOME). */

static inline bool query_is_ws(uint8_t c) { return c == 0x20u || (c >= 0x09u && c <= 0x0Du); }

extern "C" void tfidf_hits_free(tfidf_hits* h) {
    if (!h) return;
    free(h->nhits); free(h->nmatch); free(h->nterms_found); free(h->doc); free(h->score);
    memset(h, 0, sizeof(*h));
}

/* the exact sum of doc_size over the context's documents (BM25's default avgdl): a host sum
 * over one copy, kept until the next run */
int tfidf_ctx_bm25_lengths(tfidf_ctx* ctx, uint64_t* L, uint64_t* n) {
    if (!ctx || !L || !n) return TFIDF_E_INVAL;
    if (!ctx->have_result) return TFIDF_E_STATE;
    if (!ctx->bm25_L_valid) {
        HIPCHK(hipSetDevice(ctx->device));
        std::vector<uint32_t> dsz(ctx->ndocs);
        if (ctx->ndocs) {
            HIPCHK(hipMemcpyAsync(dsz.data(), ctx->doc_size.p, (size_t)ctx->ndocs * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
        }
        uint64_t sum = 0;
        for (uint32_t v : dsz) sum += v;
        ctx->bm25_L = sum;
        ctx->bm25_L_valid = true;
    }
    *L = ctx->bm25_L;
    *n = ctx->ndocs;
    return TFIDF_OK;
}

int tfidf_bm25_params_check(const tfidf_bm25_params* p, Bm25Call* out) {
    Bm25Call c{TFIDF_BM25_DEFAULT_K1, TFIDF_BM25_DEFAULT_B, 0.0};
    if (p) {
        if (p->size < sizeof(tfidf_bm25_params)) return TFIDF_E_INVAL;
        c = Bm25Call{p->k1, p->b, p->avgdl};
    }
    /* written so that a NaN fails every test */
    if (!(c.k1 >= 0.0 && c.k1 <= TFIDF_BM25_MAX_K1)) return TFIDF_E_INVAL;
    if (!(c.b >= 0.0 && c.b <= 1.0)) return TFIDF_E_INVAL;
    if (!(c.avgdl == 0.0 || (c.avgdl >= TFIDF_BM25_MIN_AVGDL && c.avgdl <= DBL_MAX))) return TFIDF_E_INVAL;
    *out = c;
    return TFIDF_OK;
}

/* ---- what tfidf_query, tfidf_query_bm25 and tfidf_similar share on the host: the group
 * budget, the top-k rounds over a group's dense accumulators, the read-back of the result ---- */
static_assert(SG_MAX == QG_MAX, "queries and rows share one group budget");
struct TopkPlan {
    uint64_t nsl0;      /* slices of the first round */
    uint64_t per_q;     /* bytes of accumulators and candidates per query (row) */
    uint64_t G;         /* queries (rows) per group */
    uint64_t cand_el;   /* entries of one candidate buffer */
};
static TopkPlan topk_plan(uint32_t N, uint32_t k, uint32_t rows, uint64_t acc_bytes) {
    TopkPlan p{};
    p.nsl0 = ((uint64_t)N + QT_SLICE - 1) / QT_SLICE;
    p.per_q = (uint64_t)N * 12 + 2 * (p.nsl0 * k * 12 + p.nsl0 * 4) + 8;
    p.G = acc_bytes / p.per_q;
    p.G = p.G < 1 ? 1 : (p.G > QG_MAX ? QG_MAX : p.G);
    if (p.G > rows) p.G = rows ? rows : 1;
    p.cand_el = p.G * p.nsl0 * k;
    return p;
}
/* the plan's buffers: apart from the budget, because a call with nothing to scan allocates nothing */
static int topk_ensure(tfidf_ctx* ctx, const TopkPlan& p, uint32_t N) {
    ENSURE(ctx->q_acc, p.G * N * 8);
    ENSURE(ctx->q_cnt, p.G * N * 4);
    ENSURE(ctx->q_big, (size_t)N * 4 + 4);
    ENSURE(ctx->q_cand0, p.cand_el * 12 + p.G * p.nsl0 * 4);
    ENSURE(ctx->q_cand1, p.cand_el * 12 + p.G * p.nsl0 * 4);
    ENSURE(ctx->q_misc, p.G * 8 + 16);
    return TFIDF_OK;
}
/* a candidate buffer: cand_el score bits, cand_el ids, then the lists' lengths */
struct TopkCand {
    uint64_t* s;
    uint32_t* id;
    uint32_t* n;
};
static TopkCand topk_cand(tfidf_ctx* ctx, const TopkPlan& p, int c) {
    uint64_t* s = (c ? ctx->q_cand1 : ctx->q_cand0).as<uint64_t>();
    uint32_t* id = (uint32_t*)(s + p.cand_el);
    return TopkCand{s, id, id + p.cand_el};
}
/* the top-k rounds of a group of gn queries (rows): the accumulators' slices, then the slices'
 * lists until one is left per query: row q = entries [q * k, q * k + n[q]) of *res */
static int topk_rounds(tfidf_ctx* ctx, const TopkPlan& p, const double* acc, const uint32_t* cnt, uint32_t N, uint32_t k,
                       uint32_t gn, unsigned long long* d_nm, TopkCand* res) {
    hipStream_t s = ctx->stream;
    int cur = 0;
    TopkCand o = topk_cand(ctx, p, cur);
    QTopkArgs ta{};
    ta.acc = acc;
    ta.cnt = cnt;
    ta.order = ctx->order;
    ta.doc_ids = ctx->dev_ids;
    ta.n_in = N;
    ta.kk = k;
    ta.out_s = o.s;
    ta.out_id = o.id;
    ta.out_n = o.n;
    ta.out_slices = (uint32_t)p.nsl0;
    ta.nmatch = d_nm;
    if (launch_query_topk(ta, gn, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
    uint64_t nsl = p.nsl0;
    while (nsl > 1) {
        const TopkCand in = o;
        QTopkArgs tb{};
        tb.in_s = in.s;
        tb.in_id = in.id;
        tb.in_n = in.n;
        tb.in_slices = (uint32_t)nsl;
        tb.n_in = nsl * k;
        tb.kk = k;
        nsl = (tb.n_in + QT_SLICE - 1) / QT_SLICE;
        cur ^= 1;
        o = topk_cand(ctx, p, cur);
        tb.out_s = o.s;
        tb.out_id = o.id;
        tb.out_n = o.n;
        tb.out_slices = (uint32_t)nsl;
        tb.nmatch = d_nm;
        if (launch_query_topk(tb, gn, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
    }
    *res = o;
    return TFIDF_OK;
}
/* the result of topk_rounds and the match counts on the host; waits for the stream */
static int topk_read_back(tfidf_ctx* ctx, const TopkCand& res, const unsigned long long* d_nm, uint32_t gn, uint32_t k,
                          uint64_t* h_s, uint32_t* h_id, uint32_t* h_n, uint64_t* h_nm) {
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(h_s, res.s, (size_t)gn * k * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_id, res.id, (size_t)gn * k * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_n, res.n, (size_t)gn * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_nm, d_nm, (size_t)gn * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return TFIDF_OK;
}

int tfidf_ctx_query(tfidf_ctx* ctx, const tfidf_queries* qs, uint32_t k, tfidf_hits* out, std::vector<uint8_t>* found_out,
                    std::vector<uint64_t>* found_off_out, const Bm25Call* bm) {
    if (!ctx || !qs || !out) return TFIDF_E_INVAL;
    if (k == 0 || k > TFIDF_QUERY_MAX_K || qs->nqueries > TFIDF_QUERY_MAX_QUERIES) return TFIDF_E_INVAL;
    const uint32_t nq = qs->nqueries;
    if (nq && !qs->q_off) return TFIDF_E_INVAL;
    for (uint32_t q = 0; q < nq; ++q)
        if (qs->q_off[q] > qs->q_off[q + 1]) return TFIDF_E_INVAL;
    if (nq && (qs->q_off[nq] > qs->nbytes || (qs->q_off[nq] > qs->q_off[0] && !qs->bytes))) return TFIDF_E_INVAL;
    if (!ctx->have_result) return TFIDF_E_STATE;
    const auto wall0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    double avgdl = 0.0;   /* BM25: 0 = no document has a token, every row is empty */
    if (bm) {
        avgdl = bm->avgdl;
        if (!(avgdl > 0.0)) {
            uint64_t L = 0, n = 0;
            const int rc = tfidf_ctx_bm25_lengths(ctx, &L, &n);
            if (rc) return rc;
            avgdl = L ? (double)L / (double)n : 0.0;
        }
    }
    for (hipEvent_t& e : ctx->ev_q)
        if (!e) HIPCHK(hipEventCreate(&e));
    if (!ctx->ncu) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || n <= 0) n = 256;
        ctx->ncu = (uint32_t)n;
    }
    memset(out, 0, sizeof(*out));
    out->nqueries = nq;
    out->k = k;
    out->nhits = (uint32_t*)calloc((size_t)nq + 1, 4);
    out->nmatch = (uint64_t*)calloc((size_t)nq + 1, 8);
    out->nterms_found = (uint32_t*)calloc((size_t)nq + 1, 4);
    out->doc = (uint32_t*)calloc((size_t)nq * k + 1, 4);
    out->score = (double*)calloc((size_t)nq * k + 1, 8);
    struct HitsGuard {   /* an error return leaves *out zeroed */
        tfidf_hits* h;
        ~HitsGuard() { if (h) tfidf_hits_free(h); }
    } guard{out};
    if (!out->nhits || !out->nmatch || !out->nterms_found || !out->doc || !out->score) return TFIDF_E_NOMEM;

    /* ---- tokens -> the batch's distinct terms, per query (term, weight) in first-occurrence order ---- */
    std::unordered_map<std::string, uint32_t> term_id;
    std::vector<const std::string*> terms;
    std::vector<uint64_t> qt_off((size_t)nq + 1, 0);
    std::vector<uint32_t> qt_term, qt_w;
    for (uint32_t q = 0; q < nq; ++q) {
        const uint8_t* b = qs->bytes;
        const uint64_t e = qs->q_off[q + 1];
        std::unordered_map<uint32_t, size_t> seen;
        for (uint64_t i = qs->q_off[q]; i < e;) {
            while (i < e && query_is_ws(b[i])) ++i;
            if (i >= e) break;
            const uint64_t t0 = i;
            while (i < e && !query_is_ws(b[i])) ++i;
            uint64_t tl = 0;
            while (t0 + tl < i && b[t0 + tl] != 0) ++tl;   /* strcmp semantics: up to the first NUL */
            auto ins = term_id.emplace(std::string((const char*)b + t0, (size_t)tl), (uint32_t)terms.size());
            if (ins.second) terms.push_back(&ins.first->first);
            auto at = seen.emplace(ins.first->second, qt_term.size());
            if (at.second) { qt_term.push_back(ins.first->second); qt_w.push_back(1u); }
            else if (qt_w[at.first->second] != 0xFFFFFFFFu) ++qt_w[at.first->second];
        }
        qt_off[q + 1] = qt_term.size();
    }
    const uint32_t nT = (uint32_t)terms.size();
    tfidf_query_info qi{};
    qi.nqueries = nq;
    qi.k = k;
    qi.nterms = nT;

    /* ---- lookup: one lane per distinct term ---- */
    std::vector<uint32_t> rank(nT, QUERY_NO_TERM), df_found(bm ? nT : 0, 0u);
    std::vector<uint64_t> toff((size_t)nT + 1, 0);
    std::string blob;
    if (nT && ctx->V) {
        for (uint32_t t = 0; t < nT; ++t) { toff[t] = blob.size(); blob += *terms[t]; }
        toff[nT] = blob.size();
        const size_t offb = ((size_t)nT + 1) * 8;
        ENSURE(ctx->q_terms, offb + blob.size() + 16);
        ENSURE(ctx->q_rank, (size_t)nT * (bm ? 8 : 4) + 4);   /* BM25: the found terms' df behind the ranks */
        HIPCHK(hipMemcpyAsync(ctx->q_terms.p, toff.data(), offb, hipMemcpyHostToDevice, s));
        if (!blob.empty())
            HIPCHK(hipMemcpyAsync(ctx->q_terms.as<uint8_t>() + offb, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
        QLookupArgs la{};
        la.tbytes = ctx->q_terms.as<uint8_t>() + offb;
        la.toff = ctx->q_terms.as<uint64_t>();
        la.nterms = nT;
        la.vkeys = ctx->vkeys.as<uint4>();
        la.vrep = ctx->vrep.as<uint64_t>();
        la.mask = ctx->vcap - 1;
        la.home = ~1ull;
        la.rank_of_slot = ctx->rank_of_slot.as<uint32_t>();
        la.corpus = ctx->dev_bytes;
        la.corpus_bytes = ctx->corpus.nbytes;
        la.V = ctx->V;
        la.rank_out = ctx->q_rank.as<uint32_t>();
        HIPCHK(hipEventRecord(ctx->ev_q[0], s));
        if (launch_query_lookup(la, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        if (bm && launch_bm25_df(la.rank_out, nT, df_of_run(ctx), ctx->V, la.rank_out + nT, s)) {
            HIPCHK(hipGetLastError());
            return TFIDF_E_HIP;
        }
        HIPCHK(hipEventRecord(ctx->ev_q[1], s));
        HIPCHK(hipMemcpyAsync(rank.data(), ctx->q_rank.p, (size_t)nT * 4, hipMemcpyDeviceToHost, s));
        if (bm) HIPCHK(hipMemcpyAsync(df_found.data(), la.rank_out + nT, (size_t)nT * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ctx->ev_q[0], ctx->ev_q[1]);
        qi.ms_lookup = ms;
    }
    for (uint32_t t = 0; t < nT; ++t) qi.nterms_found += rank[t] != QUERY_NO_TERM;
    if (found_out) found_out->assign(qt_term.size(), 0);
    if (found_off_out) *found_off_out = qt_off;
    for (uint32_t q = 0; q < nq; ++q)
        for (uint64_t x = qt_off[q]; x < qt_off[q + 1]; ++x)
            if (rank[qt_term[x]] != QUERY_NO_TERM) {
                ++out->nterms_found[q];
                if (found_out) (*found_out)[x] = 1;
            }

    /* ---- BM25: idf per distinct found term, the host's libm log (one operation per line) ---- */
    std::vector<double> idf(bm ? nT : 0, 0.0);
    for (uint32_t t = 0; bm && t < nT; ++t) {
        if (rank[t] == QUERY_NO_TERM) continue;
        const uint64_t Nt = ctx->ndocs_total, df = df_found[t] < Nt ? df_found[t] : Nt;
        const double num = (double)(Nt - df) + 0.5;
        const double den = (double)df + 0.5;
        const double ratio = num / den;
        const double arg = 1.0 + ratio;
        idf[t] = log(arg);
    }

    /* ---- query groups under the accumulator budget ---- */
    /* BM25 with avgdl 0 (L = 0: no document of the context has a token, so there are no pairs):
     * N = 0 turns every group below off and the rows stay empty, as the header defines */
    const uint32_t N = bm && !(avgdl > 0.0) ? 0u : ctx->ndocs;
    const TopkPlan plan = topk_plan(N, k, nq, ctx->query_acc_bytes);
    const uint64_t G = plan.G;
    qi.group_queries = (uint32_t)G;
    qi.acc_bytes = G * plan.per_q;
    if (N && nq) {
        const int rc = topk_ensure(ctx, plan, N);
        if (rc) return rc;
    }
    std::vector<uint64_t> h_s((size_t)G * k), h_nm(G);
    std::vector<uint32_t> h_id((size_t)G * k), h_n(G);
    struct Post { uint32_t rank, q, w, term; };
    std::vector<Post> posts;
    std::vector<uint32_t> tab;
    for (uint32_t g0 = 0; N && g0 < nq; g0 += (uint32_t)G) {
        const uint32_t gn = nq - g0 < G ? nq - g0 : (uint32_t)G;
        posts.clear();
        for (uint32_t q = 0; q < gn; ++q)
            for (uint64_t x = qt_off[g0 + q]; x < qt_off[g0 + q + 1]; ++x)
                if (rank[qt_term[x]] != QUERY_NO_TERM) posts.push_back(Post{rank[qt_term[x]], q, qt_w[x], qt_term[x]});
        if (posts.empty()) continue;   /* no term of the group is in the vocabulary: no hits */
        if (posts.size() > 0x7FFFFFFFull) return TFIDF_E_CAPACITY;
        ++qi.ngroups;
        std::sort(posts.begin(), posts.end(), [](const Post& a, const Post& b) { return a.rank != b.rank ? a.rank < b.rank : a.q < b.q; });
        /* the group's table: sorted distinct ranks, CSR offsets, postings' queries and weights */
        uint32_t nG = 0;
        for (size_t i = 0; i < posts.size(); ++i) nG += i == 0 || posts[i].rank != posts[i - 1].rank;
        const uint32_t nP = (uint32_t)posts.size();
        /* BM25: the weights are binary64 W(q,t) = fl(w * idf), at the next even word */
        const size_t w_at = (size_t)2 * nG + 1 + nP + (bm ? (nP + 1) & 1u : 0u);
        tab.assign(w_at + (bm ? 2 : 1) * (size_t)nP, 0);
        uint32_t* gterm = tab.data();
        uint32_t* poff = gterm + nG;
        uint32_t* pq = poff + nG + 1;
        uint32_t* pw = gterm + w_at;
        for (uint32_t i = 0, t = 0; i < nP; ++i) {
            if (i == 0 || posts[i].rank != posts[i - 1].rank) { gterm[t] = posts[i].rank; poff[t] = i; ++t; }
            pq[i] = posts[i].q;
            if (bm) {
                const double W = (double)posts[i].w * idf[posts[i].term];
                memcpy(pw + 2 * (size_t)i, &W, 8);
            } else {
                pw[i] = posts[i].w;
            }
        }
        poff[nG] = nP;
        ENSURE(ctx->q_tab, tab.size() * 4 + 16);
        HIPCHK(hipMemcpyAsync(ctx->q_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
        unsigned long long* d_nm = ctx->q_misc.as<unsigned long long>();
        HIPCHK(hipMemsetAsync(d_nm, 0, (size_t)G * 8, s));
        DocScanArgs sa{};
        sa.out_off = ctx->out_off.as<uint64_t>();
        sa.out_term = ctx->out_term.as<uint32_t>();
        sa.ndocs = N;
        sa.npairs = ctx->npairs;
        sa.gterm = ctx->q_tab.as<uint32_t>();
        sa.ngterm = nG;
        sa.post_off = sa.gterm + nG;
        sa.post_q = sa.post_off + nG + 1;
        sa.post_w = sa.gterm + w_at;
        sa.tab_words = tab.size() <= 0xFFFFFFFFull ? (uint32_t)tab.size() : 0u;
        sa.nq = gn;
        sa.acc = ctx->q_acc.as<double>();
        sa.cnt = ctx->q_cnt.as<uint32_t>();
        sa.big_list = ctx->q_big.as<uint32_t>();
        sa.big_count = (uint32_t*)(d_nm + G);
        HIPCHK(hipEventRecord(ctx->ev_q[0], s));
        int lrc;
        if (bm) {
            BScoreArgs ba{sa};
            ba.out_cnt = ctx->out_cnt.as<uint32_t>();
            ba.order = ctx->order;
            ba.doc_size = ctx->doc_size.as<uint32_t>();
            ba.k1 = bm->k1;
            ba.b = bm->b;
            ba.avgdl = avgdl;
            ba.k1_plus_1 = bm->k1 + 1.0;
            ba.one_minus_b = 1.0 - bm->b;
            lrc = launch_bm25_score(ba, ctx->ncu, s);
        } else {
            QScoreArgs ta{sa};
            ta.out_score = ctx->out_score.as<double>();
            lrc = launch_query_score(ta, ctx->ncu, s);
        }
        if (lrc) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_q[1], s));
        TopkCand res{};
        int rc = topk_rounds(ctx, plan, sa.acc, sa.cnt, N, k, gn, d_nm, &res);
        if (rc) return rc;
        HIPCHK(hipEventRecord(ctx->ev_q[2], s));
        rc = topk_read_back(ctx, res, d_nm, gn, k, h_s.data(), h_id.data(), h_n.data(), h_nm.data());
        if (rc) return rc;
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ctx->ev_q[0], ctx->ev_q[1]);
        qi.ms_score += ms;
        (void)hipEventElapsedTime(&ms, ctx->ev_q[1], ctx->ev_q[2]);
        qi.ms_topk += ms;
        for (uint32_t q = 0; q < gn; ++q) {
            const uint32_t n = h_n[q] < k ? h_n[q] : k;
            out->nhits[g0 + q] = n;
            out->nmatch[g0 + q] = h_nm[q];
            for (uint32_t i = 0; i < n; ++i) {
                out->doc[(size_t)(g0 + q) * k + i] = h_id[(size_t)q * k + i];
                memcpy(&out->score[(size_t)(g0 + q) * k + i], &h_s[(size_t)q * k + i], 8);
            }
        }
    }
    qi.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    if (bm) {
        tfidf_bm25_info bi{};
        bi.nqueries = qi.nqueries; bi.k = qi.k; bi.nterms = qi.nterms; bi.nterms_found = qi.nterms_found;
        bi.ngroups = qi.ngroups; bi.group_queries = qi.group_queries; bi.acc_bytes = qi.acc_bytes;
        bi.ms_lookup = qi.ms_lookup; bi.ms_score = qi.ms_score; bi.ms_topk = qi.ms_topk; bi.ms_total = qi.ms_total;
        bi.avgdl = avgdl;
        ctx->binfo = bi;
    } else {
        ctx->qinfo = qi;
    }
    guard.h = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_query(tfidf_ctx* ctx, const tfidf_queries* queries, uint32_t k, tfidf_hits* out) {
    return tfidf_ctx_query(ctx, queries, k, out, nullptr, nullptr);
}

extern "C" int tfidf_query_bm25(tfidf_ctx* ctx, const tfidf_queries* queries, uint32_t k, const tfidf_bm25_params* params,
                                tfidf_hits* out) {
    if (!ctx || !queries || !out) return TFIDF_E_INVAL;
    Bm25Call bm{};
    const int rc = tfidf_bm25_params_check(params, &bm);
    if (rc) return rc;
    return tfidf_ctx_query(ctx, queries, k, out, nullptr, nullptr, &bm);
}

extern "C" int tfidf_last_bm25_info(const tfidf_ctx* ctx, tfidf_bm25_info* info) {
    if (!ctx || !info || info->size < sizeof(uint64_t)) return TFIDF_E_INVAL;
    const uint64_t n = info->size < sizeof(tfidf_bm25_info) ? info->size : sizeof(tfidf_bm25_info);
    tfidf_bm25_info o = ctx->binfo;
    o.size = n;
    memcpy(info, &o, (size_t)n);
    return TFIDF_OK;
}

extern "C" int tfidf_last_query_info(const tfidf_ctx* ctx, tfidf_query_info* info) {
    if (!ctx || !info || info->size < sizeof(uint64_t)) return TFIDF_E_INVAL;
    const uint64_t n = info->size < sizeof(tfidf_query_info) ? info->size : sizeof(tfidf_query_info);
    tfidf_query_info o = ctx->qinfo;
    o.size = n;
    memcpy(info, &o, (size_t)n);
    return TFIDF_OK;
}

/* --------------------------------------------------------------- transform ----
 * Unseen documents against the resident model (transform.hip).  The run leaves vkeys / vrep /
 * rank_of_slot, df_of_run, idf_vals and (N over IDF_FULL_MAX) its `present` index in buffers of
 * the context that nothing after the run writes (tfidf_query's note above; the query, keyword
 * and similarity calls use their own buffers and the arena only as scratch), so the scores
 * read the very doubles the run multiplied with.  The batch is cut into slices at document
 * boundaries; a slice is: boundaries (counted, scanned, written) -> one round trip for the
 * token total -> resolve -> stable sort of (row << 32 | rank, token index) -> run heads, scan,
 * pairs -> copies into the caller's arrays. */

extern "C" void tfidf_rows_free(tfidf_rows* r) {
    if (!r) return;
    free(r->row_off); free(r->doc_size); free(r->doc_oov); free(r->term); free(r->count); free(r->df);
    free(r->score); free(r->word_off); free(r->word_len);
    memset(r, 0, sizeof(*r));
}

namespace {
struct RowsGuard {   /* an error return leaves *out zeroed */
    tfidf_rows* r;
    ~RowsGuard() { if (r) tfidf_rows_free(r); }
};
template <typename T> bool grow_host(T*& p, uint64_t n) {
    void* q = realloc(p, (size_t)(n + 1) * sizeof(T));
    if (!q) return false;
    p = (T*)q;
    return true;
}
/* the upper bound of a slice's device scratch before its tokens are known: its bytes hold at
 * most one token per two bytes and one more per document (a document boundary ends a token);
 * per token 84 bytes of records, sort buffers and pairs */
constexpr uint64_t TR_TOKEN_BYTES = 84;
inline uint64_t tr_max_tokens(uint64_t nbytes, uint64_t nd) {
    const uint64_t t = (nbytes + 1) / 2 + nd;
    return t < nbytes ? t : nbytes;
}
inline uint64_t tr_a_bytes(uint64_t nbytes, uint64_t nd) {
    const uint64_t ntiles = nbytes / TR_TILE + 2;
    return (ntiles * (TR_TILE / 32u) + 1u) * 4u + 2 * (ntiles + 1) * 8 + nd * 8 + (nd + 1) * 8 + 4096;
}
inline uint64_t tr_bound(uint64_t nbytes, uint64_t nd) {
    return tr_a_bytes(nbytes, nd) + tr_max_tokens(nbytes, nd) * TR_TOKEN_BYTES + 4096;
}
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
}  // namespace

/* the weighting section's helpers (below): a slice's rows are scored by reweight.hip when a
 * scheme other than the reference's is active */
enum { RWM_BIG = 0, RWM_ZERO = 1, RWM_CMAX = 2, RWM_NLIST = 3 };   /* rw_misc's words */
static int rw_cmax_launch(tfidf_ctx* ctx, const uint32_t* count, uint64_t n, const uint32_t* n_dev);
static int rw_tf_finish(tfidf_ctx* ctx, uint32_t cmax, uint32_t nlist, uint32_t* nlisted, uint64_t* nlogs);
static void rw_scheme_args(tfidf_ctx* ctx, RwArgs& a, uint32_t tf, uint32_t norm, uint32_t nlisted);

extern "C" int tfidf_transform(tfidf_ctx* ctx, const tfidf_corpus* batch, tfidf_rows* out) {
    return tfidf_ctx_transform(ctx, batch, out, true);
}

int tfidf_ctx_transform(tfidf_ctx* ctx, const tfidf_corpus* batch, tfidf_rows* out, bool norm) {
    if (!ctx || !batch || !out) return TFIDF_E_INVAL;
    const uint32_t N = batch->ndocs;
    if (N && !batch->doc_off) return TFIDF_E_INVAL;
    if (!ctx->have_model) return TFIDF_E_STATE;   /* a run's model or an imported one */
    const auto wall0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const bool dev = (batch->flags & TFIDF_CORPUS_DEVICE) != 0;
    /* the offsets on the host: the slices are cut here */
    std::vector<uint64_t> off_copy;
    const uint64_t* off = batch->doc_off;
    if (dev && N) {
        off_copy.resize((size_t)N + 1);
        HIPCHK(hipMemcpyAsync(off_copy.data(), batch->doc_off, ((size_t)N + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        off = off_copy.data();
    }
    for (uint32_t d = 0; d < N; ++d)
        if (off[d] > off[d + 1]) return TFIDF_E_INVAL;
    if (N && (off[N] > batch->nbytes || (off[N] > off[0] && !batch->bytes))) return TFIDF_E_INVAL;
    const uint8_t* d_bytes = batch->bytes;
    const uint64_t* d_off = batch->doc_off;
    if (!dev && N) {   /* the run's own host corpus lives in in_bytes: the batch gets its own buffers */
        ENSURE(ctx->tr_bytes, batch->nbytes + 64);
        ENSURE(ctx->tr_off, ((size_t)N + 1) * 8);
        if (off[N] > off[0])
            HIPCHK(hipMemcpyAsync(ctx->tr_bytes.as<uint8_t>() + off[0], batch->bytes + off[0], off[N] - off[0],
                                  hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(ctx->tr_off.p, off, ((size_t)N + 1) * 8, hipMemcpyHostToDevice, s));
        d_bytes = ctx->tr_bytes.as<uint8_t>();
        d_off = ctx->tr_off.as<uint64_t>();
    }
    for (hipEvent_t& e : ctx->ev_tr)
        if (!e) HIPCHK(hipEventCreate(&e));

    memset(out, 0, sizeof(*out));
    RowsGuard guard{out};
    out->ndocs = N;
    out->row_off = (uint64_t*)calloc((size_t)N + 1, 8);
    out->doc_size = (uint32_t*)calloc((size_t)N + 1, 4);
    out->doc_oov = (uint32_t*)calloc((size_t)N + 1, 4);
    if (!out->row_off || !out->doc_size || !out->doc_oov) return TFIDF_E_NOMEM;
    if (!grow_host(out->term, 0) || !grow_host(out->count, 0) || !grow_host(out->df, 0) || !grow_host(out->score, 0) ||
        !grow_host(out->word_off, 0) || !grow_host(out->word_len, 0))
        return TFIDF_E_NOMEM;

    tfidf_transform_info ti{};
    ti.ndocs = N;
    const uint32_t V = ctx->V;
    const bool full_lut = ctx->ndocs_total <= IDF_FULL_MAX;   /* run_post: idf_vals by df, else through `present` */
    /* the active weighting scheme (tfidf_reweight); the reference's takes the path it always took */
    const uint32_t wtf = ctx->wt_tf, widf = ctx->wt_idf, wnorm = norm ? ctx->wt_norm : (uint32_t)TFIDF_NORM_NONE;
    const bool ref_scheme = wtf == TFIDF_TF_RATIO && widf == TFIDF_IDF_REF && ctx->wt_norm == TFIDF_NORM_NONE;
    if (!ref_scheme) ENSURE(ctx->rw_misc, 256);
    uint64_t Ptot = 0;
    std::vector<uint64_t> h_rowoff;
    for (uint32_t d0 = 0; d0 < N;) {
        /* ---- the slice: documents [d0, d1) whose scratch bound stays under the budget ---- */
        uint32_t d1 = d0 + 1;
        while (d1 < N && tr_bound(off[d1 + 1] - off[d0], (uint64_t)d1 + 1 - d0) <= ctx->transform_bytes) ++d1;
        const uint32_t nd = d1 - d0;
        const uint64_t b0 = off[d0], b1 = off[d1];
        ++ti.nslices;
        for (uint32_t r = 0; r <= nd; ++r) out->row_off[d0 + r] = Ptot;   /* rows without a token stay empty */
        if (b1 == b0) { d0 = d1; continue; }
        TrSlice sl{};
        sl.bytes = d_bytes;
        sl.nbytes = batch->nbytes;
        sl.doc_off = d_off;
        sl.d0 = d0;
        sl.d1 = d1;
        sl.b0 = b0;
        sl.b1 = b1;
        sl.p0 = (long long)b0 - (long long)(((uintptr_t)d_bytes + b0) & 15u);
        sl.ntiles = (uint64_t)((long long)b1 - sl.p0 + (TR_TILE - 1)) / TR_TILE;
        /* tr_a: status, per-document words, the bitmap, the per-tile counts */
        const size_t a_status = 0, a_dsize = 256, a_doov = al256(a_dsize + (size_t)nd * 4);
        const size_t a_rowoff = al256(a_doov + (size_t)nd * 4), a_dstart = al256(a_rowoff + ((size_t)nd + 1) * 8);
        const size_t a_cs = al256(a_dstart + (size_t)(sl.ntiles * (TR_TILE / 32u) + 1u) * 4);
        const size_t a_ce = al256(a_cs + (size_t)(sl.ntiles + 1) * 8), a_end = al256(a_ce + (size_t)(sl.ntiles + 1) * 8);
        ENSURE(ctx->tr_a, a_end);
        uint8_t* A = ctx->tr_a.as<uint8_t>();
        sl.status = (uint32_t*)(A + a_status);
        sl.dstart = (uint32_t*)(A + a_dstart);
        sl.cnt_s = (uint64_t*)(A + a_cs);
        sl.cnt_e = (uint64_t*)(A + a_ce);
        HIPCHK(hipMemsetAsync(A, 0, a_rowoff, s));   /* status, doc_size, doc_oov */
        HIPCHK(hipEventRecord(ctx->ev_tr[0], s));
        ctx->arena.used = 0;   /* as format_prepare: nothing of the result lives in the arena */
        if (launch_tr_docstarts(sl, s) || launch_tr_count(sl, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        if (scan_excl_u64(sl.cnt_s, sl.cnt_s, sl.ntiles, ctx->arena, s) ||
            scan_excl_u64(sl.cnt_e, sl.cnt_e, sl.ntiles, ctx->arena, s)) {
            HIPCHK(hipGetLastError());
            return TFIDF_E_HIP;
        }
        uint64_t tot[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(&tot[0], sl.cnt_s + sl.ntiles, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&tot[1], sl.cnt_e + sl.ntiles, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const uint64_t T = tot[0];
        if (tot[1] != T || T > tr_max_tokens(b1 - b0, nd)) {
            fprintf(stderr, "tfidf: transform: %llu token starts, %llu ends in %llu bytes\n", (unsigned long long)tot[0],
                    (unsigned long long)tot[1], (unsigned long long)(b1 - b0));
            return TFIDF_E_STATE;
        }
        if (T > 0xFFFFFFFEull) return TFIDF_E_CAPACITY;
        if (T == 0) {   /* whitespace only */
            const uint64_t sb = a_end;
            if (sb > ti.scratch_bytes) ti.scratch_bytes = sb;
            d0 = d1;
            continue;
        }
        /* tr_b: token records, sort buffers, pairs (sized by the slice's tokens) */
        size_t bo = 0;
        auto take = [&bo](size_t bytes) { const size_t at = bo; bo = al256(bo + bytes); return at; };
        const size_t b_ts = take(T * 8), b_te = take(T * 8), b_tl = take(T * 4);
        const size_t b_k0 = take(T * 8), b_k1 = take(T * 8), b_v0 = take(T * 4), b_v1 = take(T * 4);
        const size_t b_pos = take((T + 1) * 4);
        const size_t b_prow = take(T * 4), b_pterm = take(T * 4), b_pcnt = take(T * 4), b_pdf = take(T * 4);
        const size_t b_psc = take(T * 8), b_pwo = take(T * 8), b_pwl = take(T * 4);
        ENSURE(ctx->tr_b, bo);
        if (a_end + bo > ti.scratch_bytes) ti.scratch_bytes = a_end + bo;
        {   /* the sort's histograms and the scans' block sums */
            const size_t want = (size_t)(T / 2 + T / 64) + (8u << 20);
            if (want > ctx->arena_buf.cap && arena_reset(ctx, want) != 0) return TFIDF_E_NOMEM;
            ctx->arena.used = 0;
        }
        uint8_t* B = ctx->tr_b.as<uint8_t>();
        sl.tok_start = (uint64_t*)(B + b_ts);
        sl.tok_end = (uint64_t*)(B + b_te);
        sl.tok_cap = T;
        if (launch_tr_write(sl, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_tr[1], s));
        TrResolve ra{};
        ra.sl = sl;
        ra.ntok = T;
        ra.voc = VocabRO{ctx->vkeys.as<uint4>(), ctx->vrep.as<uint64_t>(), ctx->vcap - 1, ~1ull,
                         ctx->rank_of_slot.as<uint32_t>(), ctx->dev_bytes, ctx->corpus.nbytes, V};
        ra.key = (uint64_t*)(B + b_k0);
        ra.val = (uint32_t*)(B + b_v0);
        ra.tlen = (uint32_t*)(B + b_tl);
        if (launch_tr_resolve(ra, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_tr[2], s));
        /* only the bytes that vary are sorted: the ranks 0..V below, the rows d0..d1-1 above */
        uint32_t byte_mask = 0;
        for (uint32_t b = 0; b < 4; ++b) {
            if ((V >> (8 * b)) != 0) byte_mask |= 1u << b;
            if (((d0 ^ (d1 - 1)) >> (8 * b)) != 0) byte_mask |= 1u << (4 + b);
        }
        const int where = radix_sort_u64(ra.key, ra.val, (uint64_t*)(B + b_k1), (uint32_t*)(B + b_v1), T, byte_mask,
                                         ctx->arena, s);
        if (where < 0) { HIPCHK(hipGetLastError()); return where == -2 ? TFIDF_E_NOMEM : TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_tr[3], s));
        TrPairs pa{};
        pa.key = where ? (uint64_t*)(B + b_k1) : ra.key;
        pa.val = where ? (uint32_t*)(B + b_v1) : ra.val;
        pa.ntok = T;
        pa.d0 = d0;
        pa.d1 = d1;
        pa.V = V;
        pa.doc_off = d_off;
        pa.tok_start = sl.tok_start;
        pa.tlen = ra.tlen;
        pa.flag = (uint32_t*)(B + b_pos);
        pa.pos = pa.flag;   /* scanned in place */
        pa.df = df_of_run(ctx);
        pa.idf_idx = full_lut ? nullptr : ctx->present.as<uint32_t>();
        pa.idf = ctx->idf_vals.as<double>();
        pa.Nt = ctx->ndocs_total;
        pa.doc_size = (uint32_t*)(A + a_dsize);
        pa.doc_oov = (uint32_t*)(A + a_doov);
        pa.row_off = (uint64_t*)(A + a_rowoff);
        pa.p_row = (uint32_t*)(B + b_prow);
        pa.p_term = (uint32_t*)(B + b_pterm);
        pa.p_count = (uint32_t*)(B + b_pcnt);
        pa.p_df = (uint32_t*)(B + b_pdf);
        pa.p_score = (double*)(B + b_psc);
        pa.p_woff = (uint64_t*)(B + b_pwo);
        pa.p_wlen = (uint32_t*)(B + b_pwl);
        pa.status = sl.status;
        if (launch_tr_flags(pa, s) || scan_excl_u32(pa.flag, pa.flag, T, ctx->arena, s) ||
            (ref_scheme ? launch_tr_pairs(pa, s) : launch_tr_pairs_w(pa, s))) {
            HIPCHK(hipGetLastError());
            return TFIDF_E_HIP;
        }
        uint32_t cw[2] = {0, 0};   /* sublinear tf: the slice's largest count and its counts above the table */
        if (!ref_scheme && wtf == TFIDF_TF_LOG) {
            if (const int rc = rw_cmax_launch(ctx, pa.p_count, T, pa.pos + T)) return rc;
            HIPCHK(hipMemcpyAsync(cw, ctx->rw_misc.as<uint32_t>() + RWM_CMAX, 8, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipEventRecord(ctx->ev_tr[4], s));
        /* ---- back to the host: the slice's words first (the pair total sizes the rest) ---- */
        uint32_t P32 = 0, st = 0;
        h_rowoff.resize((size_t)nd + 1);
        HIPCHK(hipMemcpyAsync(&P32, pa.pos + T, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&st, sl.status, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->doc_size + d0, pa.doc_size, (size_t)nd * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->doc_oov + d0, pa.doc_oov, (size_t)nd * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_rowoff.data(), pa.row_off, ((size_t)nd + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (st & ST_BOUNDS) {
            fprintf(stderr, "tfidf: transform: internal bounds check tripped (status 0x%x)\n", st);
            return TFIDF_E_STATE;
        }
        const uint64_t P = P32;
        if (!ref_scheme && P) {   /* the rows' scores by the scheme: w, then the norm over each row's pairs */
            uint32_t nlisted = 0;
            uint64_t nlogs = 0;
            if (wtf == TFIDF_TF_LOG)
                if (const int rc = rw_tf_finish(ctx, cw[0], cw[1], &nlisted, &nlogs)) return rc;
            ENSURE(ctx->rw_big, (size_t)nd * 4 + 4);
            RwArgs wa{};
            wa.off = pa.row_off;
            wa.npairs = P;
            wa.ndocs = nd;
            wa.doc_size = pa.doc_size;
            wa.count = pa.p_count;
            wa.key = pa.p_df;
            wa.key_n = ctx->ndocs_total + 1;
            if (widf != TFIDF_IDF_NONE) {
                wa.idf = widf == TFIDF_IDF_REF ? ctx->idf_vals.as<double>() : ctx->rw_idf.as<double>();
                wa.idf_idx = pa.idf_idx;
            }
            wa.score = pa.p_score;
            rw_scheme_args(ctx, wa, wtf, wnorm, nlisted);
            if (launch_rw_pairs(wa, ctx->ncu, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        }
        if (!grow_host(out->term, Ptot + P) || !grow_host(out->count, Ptot + P) || !grow_host(out->df, Ptot + P) ||
            !grow_host(out->score, Ptot + P) || !grow_host(out->word_off, Ptot + P) || !grow_host(out->word_len, Ptot + P))
            return TFIDF_E_NOMEM;
        if (P) {
            HIPCHK(hipMemcpyAsync(out->term + Ptot, pa.p_term, (size_t)P * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out->count + Ptot, pa.p_count, (size_t)P * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out->df + Ptot, pa.p_df, (size_t)P * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out->score + Ptot, pa.p_score, (size_t)P * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out->word_off + Ptot, pa.p_woff, (size_t)P * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out->word_len + Ptot, pa.p_wlen, (size_t)P * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        for (uint32_t r = 0; r <= nd; ++r) out->row_off[d0 + r] = Ptot + h_rowoff[r];
        Ptot += P;
        ti.ntokens += T;
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ctx->ev_tr[0], ctx->ev_tr[1]);
        ti.ms_tokens += ms;
        (void)hipEventElapsedTime(&ms, ctx->ev_tr[1], ctx->ev_tr[2]);
        ti.ms_resolve += ms;
        (void)hipEventElapsedTime(&ms, ctx->ev_tr[2], ctx->ev_tr[3]);
        ti.ms_sort += ms;
        (void)hipEventElapsedTime(&ms, ctx->ev_tr[3], ctx->ev_tr[4]);
        ti.ms_pairs += ms;
        d0 = d1;
    }
    if (N) out->row_off[N] = Ptot;
    out->npairs = Ptot;
    out->ntokens = ti.ntokens;
    for (uint32_t d = 0; d < N; ++d) ti.noov += out->doc_oov[d];
    ti.npairs = Ptot;
    ti.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    ctx->trinfo = ti;
    guard.r = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_last_transform_info(const tfidf_ctx* ctx, tfidf_transform_info* info) {
    if (!ctx || !info || info->size < sizeof(uint64_t)) return TFIDF_E_INVAL;
    const uint64_t n = info->size < sizeof(tfidf_transform_info) ? info->size : sizeof(tfidf_transform_info);
    tfidf_transform_info o = ctx->trinfo;
    o.size = n;
    memcpy(info, &o, (size_t)n);
    return TFIDF_OK;
}

/* ---------------------------------------------------------------- analyzer ----
 * include/tfidf.h, section "analyzer"; analyze.hip.  The check, the table build and the host
 * definition are analyze_host.c.  The call stands beside a run: it reads and writes buffers of
 * its own and none of the run's state. */
extern "C" int tfidf_analyze(tfidf_ctx* ctx, const tfidf_analyzer* an, const tfidf_corpus* in_, uint32_t slot,
                             tfidf_corpus* out) {
    if (!ctx || !an || !in_ || !out || slot > 1u) return TFIDF_E_INVAL;
    const int arc = tfidf_analyzer_check(an);
    if (arc) return arc;
    const tfidf_corpus in = *in_;   /* out may be the same struct */
    const uint32_t N = in.ndocs;
    if (N && !in.doc_off) return TFIDF_E_INVAL;
    if (in.nbytes && !in.bytes) return TFIDF_E_INVAL;
    const bool dev = (in.flags & TFIDF_CORPUS_DEVICE) != 0;
    DevBuf& ob = ctx->an_bytes[slot];
    if (dev && ob.p && in.bytes >= ob.as<uint8_t>() && in.bytes < ob.as<uint8_t>() + ob.cap) return TFIDF_E_INVAL;
    const auto wall0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    /* the offsets on the host: checked here, by tfidf_transform's rules */
    std::vector<uint64_t> off_copy;
    const uint64_t* off = in.doc_off;
    if (dev && N) {
        off_copy.resize((size_t)N + 1);
        HIPCHK(hipMemcpyAsync(off_copy.data(), in.doc_off, ((size_t)N + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        off = off_copy.data();
    }
    for (uint32_t d = 0; d < N; ++d)
        if (off[d] > off[d + 1]) return TFIDF_E_INVAL;
    if (N && off[N] > in.nbytes) return TFIDF_E_INVAL;
    for (hipEvent_t& e : ctx->ev_an)
        if (!e) HIPCHK(hipEventCreate(&e));
    if (!ctx->ncu) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || n <= 0) n = 256;
        ctx->ncu = (uint32_t)n;
    }
    const hipMemcpyKind up = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    ENSURE(ctx->an_bytes[slot], in.nbytes + 64);
    ENSURE(ctx->an_off[slot], ((size_t)N + 1) * 8);
    if (in.doc_off) HIPCHK(hipMemcpyAsync(ctx->an_off[slot].p, in.doc_off, ((size_t)N + 1) * 8, up, s));
    else HIPCHK(hipMemsetAsync(ctx->an_off[slot].p, 0, 8, s));
    if (in.doc_ids && N) {
        ENSURE(ctx->an_ids[slot], (size_t)N * 4);
        HIPCHK(hipMemcpyAsync(ctx->an_ids[slot].p, in.doc_ids, (size_t)N * 4, up, s));
    }
    const uint8_t* d_in = in.bytes;
    if (!dev && in.nbytes) {
        ENSURE(ctx->an_in, in.nbytes + 64);
        HIPCHK(hipMemcpyAsync(ctx->an_in.p, in.bytes, in.nbytes, hipMemcpyHostToDevice, s));
        d_in = ctx->an_in.as<uint8_t>();
    }
    std::vector<uint32_t> blob(tfidf_an_table_bytes(an) / 4u);
    const uint32_t tab_bytes = tfidf_an_table_build(an, blob.data());
    ENSURE(ctx->an_tab, tab_bytes);
    ENSURE(ctx->an_cnt, 256);
    HIPCHK(hipMemcpyAsync(ctx->an_tab.p, blob.data(), tab_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(ctx->an_cnt.p, 0, 24, s));

    AnArgs a{};
    a.in = d_in;
    a.out = ctx->an_bytes[slot].as<uint8_t>();
    a.nbytes = in.nbytes;
    a.lo = N ? off[0] : 0;
    a.hi = N ? off[N] : 0;
    a.doc_off = ctx->an_off[slot].as<uint64_t>();
    a.ndocs = N;
    a.flags = an->flags;
    if (!(a.flags & (TFIDF_AN_LOWER | TFIDF_AN_PUNCT))) a.flags &= ~TFIDF_AN_UTF8;   /* alone it changes nothing */
    a.min_len = an->min_len;
    a.tab = ctx->an_tab.as<uint32_t>();
    a.tab_bytes = tab_bytes;
    a.blanked = ctx->an_cnt.as<unsigned long long>();
    a.stemmer = an->stemmer;
    const uint32_t lds = an_lds_bytes(a, an->nstop);
    const bool need_dstart = lds || (a.flags & TFIDF_AN_UTF8);   /* a document boundary cuts a sequence */
    if (need_dstart) {
        ENSURE(ctx->an_dstart, (size_t)(in.nbytes / 32u + 2u) * 4u);
        a.dstart = ctx->an_dstart.as<uint32_t>();
    }
    HIPCHK(hipEventRecord(ctx->ev_an[0], s));
    uint32_t grid = 0;
    if ((need_dstart && launch_an_docstarts(a, s)) || launch_analyze(a, an->nstop, ctx->ncu, ctx->an_grid, &grid, s)) {
        HIPCHK(hipGetLastError());
        return TFIDF_E_HIP;
    }
    HIPCHK(hipEventRecord(ctx->ev_an[1], s));
    unsigned long long counts[3] = {0, 0, 0};   /* tokens blanked, tokens stemmed, sequences changed */
    HIPCHK(hipMemcpyAsync(counts, ctx->an_cnt.p, 24, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));

    out->bytes = a.out;
    out->nbytes = in.nbytes;
    out->doc_off = a.doc_off;
    out->doc_ids = (in.doc_ids && N) ? ctx->an_ids[slot].as<uint32_t>() : nullptr;
    out->ndocs = N;
    out->flags = TFIDF_CORPUS_DEVICE;
    out->ndocs_total = in.ndocs_total;

    tfidf_analyze_info ai{};
    ai.nbytes = in.nbytes;
    ai.ndocs = N;
    ai.nstop = an->nstop;
    ai.table_slots = blob[0];
    ai.lds_bytes = lds;
    ai.tile_bytes = AN_TILE;
    ai.grid = grid;
    ai.blanked_tokens = counts[0];
    ai.stemmed_tokens = counts[1];
    ai.utf8_changed = counts[2];
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev_an[0], ctx->ev_an[1]);
    ai.ms_kernel = ms;
    ai.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    ctx->aninfo = ai;
    return TFIDF_OK;
}

extern "C" int tfidf_last_analyze_info(const tfidf_ctx* ctx, tfidf_analyze_info* info) {
    if (!ctx || !info || info->size < sizeof(uint64_t)) return TFIDF_E_INVAL;
    const uint64_t n = info->size < sizeof(tfidf_analyze_info) ? info->size : sizeof(tfidf_analyze_info);
    tfidf_analyze_info o = ctx->aninfo;
    o.size = n;
    memcpy(info, &o, (size_t)n);
    return TFIDF_OK;
}

/* ----------------------------------------------------------------- n-grams ----
 * include/tfidf.h, section "n-grams"; ngram.hip.  The check and the host definition are
 * ngram_host.c.  Like the analyzer the call stands beside a run: it reads and writes buffers of
 * its own and none of the run's state (the arena is scratch between runs, as for
 * tfidf_transform).  Two host round trips size the buffers: the tokens, then the output's bytes. */
extern "C" int tfidf_ngrams(tfidf_ctx* ctx, const tfidf_ngram_params* params, const tfidf_corpus* in_, uint32_t slot,
                            tfidf_corpus* out) {
    if (!ctx || !params || !in_ || !out || slot > 1u) return TFIDF_E_INVAL;
    const int prc = tfidf_ngram_check(params);
    if (prc) return prc;
    const tfidf_corpus in = *in_;   /* out may be the same struct */
    const uint32_t N = in.ndocs;
    if (N && !in.doc_off) return TFIDF_E_INVAL;
    if (in.nbytes && !in.bytes) return TFIDF_E_INVAL;
    const bool dev = (in.flags & TFIDF_CORPUS_DEVICE) != 0;
    DevBuf& ob = ctx->ng_bytes[slot];
    if (dev && ob.p && in.bytes >= ob.as<uint8_t>() && in.bytes < ob.as<uint8_t>() + ob.cap) return TFIDF_E_INVAL;
    const auto wall0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    /* the offsets on the host: checked here, by tfidf_transform's rules */
    std::vector<uint64_t> off_copy;
    const uint64_t* off = in.doc_off;
    if (dev && N) {
        off_copy.resize((size_t)N + 1);
        HIPCHK(hipMemcpyAsync(off_copy.data(), in.doc_off, ((size_t)N + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        off = off_copy.data();
    }
    for (uint32_t d = 0; d < N; ++d)
        if (off[d] > off[d + 1]) return TFIDF_E_INVAL;
    if (N && off[N] > in.nbytes) return TFIDF_E_INVAL;
    for (hipEvent_t& e : ctx->ev_ng)
        if (!e) HIPCHK(hipEventCreate(&e));
    const uint64_t b0 = N ? off[0] : 0, b1 = N ? off[N] : 0;
    const uint8_t* d_bytes = in.bytes;
    const uint64_t* d_off = in.doc_off;
    if (!dev && N) {   /* the window alone is staged, at its own offsets */
        ENSURE(ctx->ng_in, in.nbytes + 64);
        ENSURE(ctx->ng_inoff, ((size_t)N + 1) * 8);
        if (b1 > b0) HIPCHK(hipMemcpyAsync(ctx->ng_in.as<uint8_t>() + b0, in.bytes + b0, b1 - b0, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(ctx->ng_inoff.p, off, ((size_t)N + 1) * 8, hipMemcpyHostToDevice, s));
        d_bytes = ctx->ng_in.as<uint8_t>();
        d_off = ctx->ng_inoff.as<uint64_t>();
    }
    ENSURE(ctx->ng_off[slot], ((size_t)N + 1) * 8);
    if (in.doc_ids && N) {
        ENSURE(ctx->ng_ids[slot], (size_t)N * 4);
        HIPCHK(hipMemcpyAsync(ctx->ng_ids[slot].p, in.doc_ids, (size_t)N * 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    }

    tfidf_ngram_info ni{};
    ni.nbytes_in = in.nbytes;
    ni.ndocs = N;
    ni.tile_bytes = NG_TILE;
    uint64_t T = 0, nbytes_out = 0;
    unsigned long long ngrams = 0;
    HIPCHK(hipEventRecord(ctx->ev_ng[0], s));
    /* ---- token bounds: transform.hip's kernels over the whole window as one slice ---- */
    TrSlice sl{};
    size_t a_end = 0;
    if (b1 > b0) {
        sl.bytes = d_bytes;
        sl.nbytes = in.nbytes;
        sl.doc_off = d_off;
        sl.d0 = 0;
        sl.d1 = N;
        sl.b0 = b0;
        sl.b1 = b1;
        sl.p0 = (long long)b0 - (long long)(((uintptr_t)d_bytes + b0) & 15u);
        sl.ntiles = (uint64_t)((long long)b1 - sl.p0 + (TR_TILE - 1)) / TR_TILE;
        /* ng_a: status and the gram counter, the bitmap, the per-tile counts */
        const size_t a_dstart = 256, a_cs = al256(a_dstart + (size_t)(sl.ntiles * (TR_TILE / 32u) + 1u) * 4);
        const size_t a_ce = al256(a_cs + (size_t)(sl.ntiles + 1) * 8);
        a_end = al256(a_ce + (size_t)(sl.ntiles + 1) * 8);
        ENSURE(ctx->ng_a, a_end);
        uint8_t* A = ctx->ng_a.as<uint8_t>();
        sl.status = (uint32_t*)A;
        sl.dstart = (uint32_t*)(A + a_dstart);
        sl.cnt_s = (uint64_t*)(A + a_cs);
        sl.cnt_e = (uint64_t*)(A + a_ce);
        HIPCHK(hipMemsetAsync(A, 0, 256, s));   /* status, gram counter */
        ctx->arena.used = 0;   /* as tfidf_transform: nothing of a run's result lives in the arena */
        if (launch_tr_docstarts(sl, s) || launch_tr_count(sl, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        if (scan_excl_u64(sl.cnt_s, sl.cnt_s, sl.ntiles, ctx->arena, s) ||
            scan_excl_u64(sl.cnt_e, sl.cnt_e, sl.ntiles, ctx->arena, s)) {
            HIPCHK(hipGetLastError());
            return TFIDF_E_HIP;
        }
        uint64_t tot[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(&tot[0], sl.cnt_s + sl.ntiles, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&tot[1], sl.cnt_e + sl.ntiles, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        T = tot[0];
        if (tot[1] != T || T > tr_max_tokens(b1 - b0, N)) {
            fprintf(stderr, "tfidf: ngrams: %llu token starts, %llu ends in %llu bytes\n", (unsigned long long)tot[0],
                    (unsigned long long)tot[1], (unsigned long long)(b1 - b0));
            return TFIDF_E_STATE;
        }
        if (T > 0xFFFFFFFEull) return TFIDF_E_CAPACITY;
    }
    NgArgs na{};
    if (T) {
        /* ng_b: 24 bytes per token */
        const size_t b_ts = 0, b_te = al256(b_ts + (size_t)T * 8), b_so = al256(b_te + (size_t)T * 8);
        const size_t b_end = al256(b_so + ((size_t)T + 1) * 8);
        ENSURE(ctx->ng_b, b_end);
        {   /* the scans' block sums */
            const size_t want = (size_t)(T / 32) + (1u << 20);
            if (want > ctx->arena_buf.cap && arena_reset(ctx, want) != 0) return TFIDF_E_NOMEM;
            ctx->arena.used = 0;
        }
        uint8_t* B = ctx->ng_b.as<uint8_t>();
        sl.tok_start = (uint64_t*)(B + b_ts);
        sl.tok_end = (uint64_t*)(B + b_te);
        sl.tok_cap = T;
        if (launch_tr_write(sl, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_ng[1], s));
        /* ---- segment sizes, their scan, the output's size ---- */
        na.bytes = d_bytes;
        na.nbytes = in.nbytes;
        na.doc_off = d_off;
        na.ndocs = N;
        na.dstart = sl.dstart;
        na.p0 = sl.p0;
        na.min_n = params->min_n;
        na.max_n = params->max_n;
        na.joiner = params->joiner ? params->joiner : 0x5Fu;
        na.tok_start = sl.tok_start;
        na.tok_end = sl.tok_end;
        na.ntok = T;
        na.seg_off = (uint64_t*)(B + b_so);
        na.ngrams = (unsigned long long*)(ctx->ng_a.as<uint8_t>() + 8);
        if (launch_ng_sizes(na, s) || scan_excl_u64(na.seg_off, na.seg_off, T, ctx->arena, s)) {
            HIPCHK(hipGetLastError());
            return TFIDF_E_HIP;
        }
        uint32_t status = 0;
        HIPCHK(hipMemcpyAsync(&nbytes_out, na.seg_off + T, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&ngrams, na.ngrams, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&status, sl.status, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (status) {
            fprintf(stderr, "tfidf: ngrams: status 0x%x\n", status);
            return TFIDF_E_STATE;
        }
        ni.scratch_bytes = a_end + b_end;
    } else {
        HIPCHK(hipEventRecord(ctx->ev_ng[1], s));
    }
    ENSURE(ctx->ng_bytes[slot], nbytes_out + 64);
    if (nbytes_out) {
        na.out_off = ctx->ng_off[slot].as<uint64_t>();
        na.out = ctx->ng_bytes[slot].as<uint8_t>();
        na.nbytes_out = nbytes_out;
        na.ntiles = (nbytes_out + NG_TILE - 1) / NG_TILE;
        ENSURE(ctx->ng_tseg, (size_t)(na.ntiles + 1) * 4);
        na.tile_seg = ctx->ng_tseg.as<uint32_t>();
        ni.scratch_bytes += (size_t)(na.ntiles + 1) * 4;
        if (launch_ng_offsets(na, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_ng[2], s));
        if (launch_ng_write(na, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        ni.grid = (uint32_t)na.ntiles;
    } else {   /* no gram: every document is empty */
        HIPCHK(hipMemsetAsync(ctx->ng_off[slot].p, 0, ((size_t)N + 1) * 8, s));
        HIPCHK(hipEventRecord(ctx->ev_ng[2], s));
    }
    HIPCHK(hipEventRecord(ctx->ev_ng[3], s));
    HIPCHK(hipStreamSynchronize(s));

    out->bytes = ctx->ng_bytes[slot].as<uint8_t>();
    out->nbytes = nbytes_out;
    out->doc_off = ctx->ng_off[slot].as<uint64_t>();
    out->doc_ids = (in.doc_ids && N) ? ctx->ng_ids[slot].as<uint32_t>() : nullptr;
    out->ndocs = N;
    out->flags = TFIDF_CORPUS_DEVICE;
    out->ndocs_total = in.ndocs_total;

    ni.nbytes_out = nbytes_out;
    ni.ntokens = T;
    ni.ngrams = ngrams;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev_ng[0], ctx->ev_ng[1]);
    ni.ms_bounds = ms;
    (void)hipEventElapsedTime(&ms, ctx->ev_ng[1], ctx->ev_ng[2]);
    ni.ms_sizes = ms;
    (void)hipEventElapsedTime(&ms, ctx->ev_ng[2], ctx->ev_ng[3]);
    ni.ms_write = ms;
    ni.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    ctx->nginfo = ni;
    return TFIDF_OK;
}

extern "C" int tfidf_last_ngram_info(const tfidf_ctx* ctx, tfidf_ngram_info* info) {
    if (!ctx || !info || info->size < sizeof(uint64_t)) return TFIDF_E_INVAL;
    const uint64_t n = info->size < sizeof(tfidf_ngram_info) ? info->size : sizeof(tfidf_ngram_info);
    tfidf_ngram_info o = ctx->nginfo;
    o.size = n;
    memcpy(info, &o, (size_t)n);
    return TFIDF_OK;
}

/* ------------------------------------------------------------------- model ----
 * The model tfidf_transform reads, as an object (include/tfidf.h, model.hip; the host-only
 * check and file format are model_io.c).  Export gathers the term table on the device with the
 * keyword path's word gather (term metadata, a scan of the lengths, launch_terms_words over
 * every rank) and copies offsets, bytes and df.  Import builds what a run leaves behind from the
 * list: the slot table and rank_of_slot (launch_model_build), df by rank, the idf table in
 * run_post's two forms, V and N; the uploaded term bytes stand where the run's corpus does. */

namespace {
struct ModelGuard {   /* an error return leaves *out zeroed */
    tfidf_model* m;
    ~ModelGuard() { if (m) tfidf_model_free(m); }
};
}  // namespace

extern "C" int tfidf_model_export(tfidf_ctx* ctx, tfidf_model* out) {
    if (!ctx || !out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!ctx->have_model) return TFIDF_E_STATE;
    const auto wall0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint32_t V = ctx->V;
    ModelGuard guard{out};
    out->size = sizeof(tfidf_model);
    out->ndocs_total = ctx->ndocs_total;
    out->nterms = V;
    out->term_off = (uint64_t*)calloc((size_t)V + 1, 8);
    out->term_df = (uint32_t*)calloc((size_t)V + 1, 4);
    if (!out->term_off || !out->term_df) return TFIDF_E_NOMEM;
    const uint8_t* d_words = nullptr;
    if (ctx->model_only) {   /* the imported list is the table */
        if (V) HIPCHK(hipMemcpyAsync(out->term_off, ctx->m_off.p, ((size_t)V + 1) * 8, hipMemcpyDeviceToHost, s));
        d_words = ctx->m_blob.as<uint8_t>();
    } else if (V) {
        if (!ctx->tmeta_valid) {
            ENSURE(ctx->t_key, (size_t)V * 16 + 16);
            ENSURE(ctx->t_len, (size_t)V * 4 + 4);
            if (launch_term_meta(ctx->vkeys.as<uint4>(), ctx->vrep.as<uint64_t>(), ctx->slot_of_rank.as<uint32_t>(), V,
                                 ctx->t_key.as<uint4>(), ctx->t_len.as<uint32_t>(), s))
                return TFIDF_E_HIP;
            ctx->tmeta_valid = true;
        }
        ENSURE(ctx->tm_term, (size_t)V * 4 + 4);
        ENSURE(ctx->tm_woff, ((size_t)V + 1) * 8 + 16);
        uint64_t* d_woff = ctx->tm_woff.as<uint64_t>();
        if (launch_model_lens(ctx->t_len.as<uint32_t>(), V, ctx->tm_term.as<uint32_t>(), d_woff, s)) {
            HIPCHK(hipGetLastError());
            return TFIDF_E_HIP;
        }
        {
            const size_t want = scan_scratch(V) + 4096;
            if (want > ctx->arena_buf.cap && arena_reset(ctx, want) != 0) return TFIDF_E_NOMEM;
            ctx->arena.used = 0;   /* as format_prepare: nothing of the result lives in the arena */
        }
        const int sc = scan_excl_u64(d_woff, d_woff, V, ctx->arena, s);
        if (sc) { if (sc != -2) HIPCHK(hipGetLastError()); return sc == -2 ? TFIDF_E_NOMEM : TFIDF_E_HIP; }
        HIPCHK(hipMemcpyAsync(out->term_off, d_woff, ((size_t)V + 1) * 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    const uint64_t total = out->term_off[V];
    if (ctx->model_only && total != ctx->m_blob_bytes) return TFIDF_E_STATE;
    out->term_bytes = (uint8_t*)malloc((size_t)total + 1);
    if (!out->term_bytes) return TFIDF_E_NOMEM;
    if (!ctx->model_only && V) {
        ENSURE(ctx->tm_words, total + 16);
        TWordArgs wa{ctx->tm_term.as<uint32_t>(), ctx->tm_woff.as<uint64_t>(), V, ctx->t_key.as<uint4>(), V,
                     ctx->dev_bytes, ctx->corpus.nbytes, ctx->tm_words.as<uint8_t>()};
        if (launch_terms_words(wa, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        d_words = ctx->tm_words.as<uint8_t>();
    }
    if (total) HIPCHK(hipMemcpyAsync(out->term_bytes, d_words, (size_t)total, hipMemcpyDeviceToHost, s));
    if (V) HIPCHK(hipMemcpyAsync(out->term_df, df_of_run(ctx), (size_t)V * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    tfidf_model_info mi{};
    mi.nterms = V;
    mi.table_slots = ctx->vcap;
    mi.blob_bytes = total;
    mi.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    ctx->minfo = mi;
    guard.m = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_model_import(tfidf_ctx* ctx, const tfidf_model* m) {
    if (!ctx || !m) return TFIDF_E_INVAL;
    if (tfidf_model_check(m) != TFIDF_OK) return TFIDF_E_INVAL;
    const uint32_t V = m->nterms;
    const uint64_t Nt = m->ndocs_total;
    if (V && Nt > 0xFFFFFFFFull) return TFIDF_E_INVAL;   /* as tfidf_run: df and N are 32-bit */
    const auto wall0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint64_t base = V ? m->term_off[0] : 0, nbytes = V ? m->term_off[V] - base : 0;
    /* the table: the smallest size from the context's current one on that keeps V under the
     * run's load limits (run_local), chosen before anything is inserted */
    uint64_t cap = ctx->vcap;
    while (cap <= K1_VS_MAX_CAP &&
           (uint64_t)V * 100 > cap * (cap < VOCAB_LOW_LOAD_CAP ? ctx->vload_pct : ctx->vload_big_pct))
        cap *= 2;
    if (cap > K1_VS_MAX_CAP) return TFIDF_E_CAPACITY;
    for (hipEvent_t& e : ctx->ev_m)
        if (!e) HIPCHK(hipEventCreate(&e));
    /* from here on the previous result or model is gone */
    ctx->have_result = false;
    ctx->have_model = false;
    ctx->model_only = false;
    ctx->text_valid = false;
    ctx->tmeta_valid = false;
    ctx->norm_valid = false;
    ctx->bm25_L_valid = false;
    if (const int q = idf_pin_quiesce(ctx)) return q;
    ctx->vcap = cap;
    DevBuf& dfb = ctx->xp ? ctx->df_global : ctx->df_local;   /* df_of_run */
    ENSURE(ctx->vkeys, cap * 16);
    ENSURE(ctx->vrep, cap * 8);
    ENSURE(ctx->rank_of_slot, cap * 4);
    ENSURE(dfb, (size_t)V * 4 + 4);
    ENSURE(ctx->m_off, ((size_t)V + 1) * 8);
    ENSURE(ctx->m_blob, nbytes + 64);
    ENSURE(ctx->m_stat, 256);
    /* the device's offsets index the uploaded bytes from 0: the caller's own array when it
     * starts there (an exported or loaded model), else a rebased copy */
    std::vector<uint64_t> rebased;
    const uint64_t zero_off = 0;
    const uint64_t* h_off = V ? m->term_off : &zero_off;
    if (base) {
        rebased.resize((size_t)V + 1);
        for (uint32_t t = 0; t <= V; ++t) rebased[t] = m->term_off[t] - base;
        h_off = rebased.data();
    }
    uint64_t nlong = 0;
    for (uint32_t t = 0; t < V; ++t) nlong += (h_off[t + 1] - h_off[t]) >= 16u ? 1u : 0u;
    /* ---- idf: log(1.0 * N / df) on this host's libm, in run_post's forms.  Up to
     * IDF_FULL_MAX documents every df = 1..N, tabulated by the context's workers while the
     * device builds the table ---- */
    const bool full_lut = Nt <= IDF_FULL_MAX;
    IdfJoin idf_guard{ctx};
    if (V && full_lut) {
        const size_t n = (size_t)Nt + 1;
        if (ctx->idf_pin_n < n) {
            if (ctx->idf_pin) (void)hipHostFree(ctx->idf_pin);
            ctx->idf_pin = nullptr;
            ctx->idf_pin_n = 0;
            if (hipHostMalloc((void**)&ctx->idf_pin, n * 8, hipHostMallocDefault) != hipSuccess) return TFIDF_E_NOMEM;
            ctx->idf_pin_n = n;
        }
        ctx->idf_full_n = 0;
        ctx->idf_pin[0] = 0.0;
        idf_post(ctx, ctx->idf_pin, Nt, nullptr, Nt);
    }
    /* ---- upload, clear, build ---- */
    HIPCHK(hipMemcpyAsync(ctx->m_off.p, h_off, ((size_t)V + 1) * 8, hipMemcpyHostToDevice, s));
    if (nbytes) HIPCHK(hipMemcpyAsync(ctx->m_blob.p, m->term_bytes + base, (size_t)nbytes, hipMemcpyHostToDevice, s));
    if (V) HIPCHK(hipMemcpyAsync(dfb.p, m->term_df, (size_t)V * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(ctx->ev_m[0], s));
    {
        FillList fl{};
        fl.p[0] = ctx->vkeys.p;        fl.bytes[0] = cap * 16; fl.val[0] = 0xEEEEEEEEu;   /* KEY_EMPTY_HI */
        fl.p[1] = ctx->rank_of_slot.p; fl.bytes[1] = cap * 4;  fl.val[1] = 0xFFFFFFFFu;   /* QUERY_NO_TERM */
        fl.p[2] = ctx->m_stat.p;       fl.bytes[2] = 256;      fl.val[2] = 0u;
        fl.n = 3;
        if (launch_fill_multi(fl, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
    }
    ModelBuild mb{ctx->m_off.as<uint64_t>(), ctx->m_blob.as<uint8_t>(), nbytes, V, ctx->vkeys.as<uint4>(),
                  ctx->vrep.as<uint64_t>(), cap - 1, ctx->rank_of_slot.as<uint32_t>(), ctx->m_stat.as<uint32_t>()};
    if (launch_model_build(mb, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
    HIPCHK(hipEventRecord(ctx->ev_m[1], s));
    uint32_t st = 0;
    HIPCHK(hipMemcpyAsync(&st, ctx->m_stat.p, 4, hipMemcpyDeviceToHost, s));
    if (V && full_lut) {
        ENSURE(ctx->idf_vals, (size_t)(Nt + 1) * 8);
        idf_join(ctx);
        HIPCHK(hipMemcpyAsync(ctx->idf_vals.p, ctx->idf_pin, (size_t)(Nt + 1) * 8, hipMemcpyHostToDevice, s));
        ctx->idf_pin_busy = true;
        HIPCHK(hipStreamSynchronize(s));
        ctx->idf_pin_busy = false;
        ctx->idf_full_n = Nt;
    } else if (V) {   /* the distinct df values, listed on the device as run_post lists them */
        ctx->idf_full_n = 0;
        {
            const size_t want = (size_t)(Nt + 2) * 4 + scan_scratch(Nt + 1) + 8192;
            if (arena_reset(ctx, want > ctx->arena_buf.cap ? want : ctx->arena_buf.cap) != 0) return TFIDF_E_NOMEM;
        }
        Arena& ar = ctx->arena;
        ENSURE(ctx->present, (Nt + 2) * 4);
        uint32_t* present = ctx->present.as<uint32_t>();
        HIPCHK(hipMemsetAsync(present, 0, (Nt + 2) * 4, s));
        uint32_t* vals_dev = (uint32_t*)ar.get((size_t)(Nt + 2) * 4);
        if (!vals_dev) return TFIDF_E_NOMEM;
        if (launch_df_mark(dfb.as<uint32_t>(), V, present, s) || scan_excl_u32(present, present, Nt + 1, ar, s) ||
            launch_df_list(present, Nt + 1, vals_dev, s)) {
            HIPCHK(hipGetLastError());
            return TFIDF_E_HIP;
        }
        uint32_t K = 0;
        HIPCHK(hipMemcpyAsync(&K, present + Nt + 1, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (K == 0 || K > V) return TFIDF_E_STATE;
        std::vector<uint32_t> vals(K);
        HIPCHK(hipMemcpyAsync(vals.data(), vals_dev, (size_t)K * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        ENSURE(ctx->idf_vals, (size_t)K * 8 + 8);
        if (ctx->idf_pin_n < (size_t)K + 1) {
            if (ctx->idf_pin) (void)hipHostFree(ctx->idf_pin);
            ctx->idf_pin = nullptr;
            ctx->idf_pin_n = 0;
            if (hipHostMalloc((void**)&ctx->idf_pin, ((size_t)K + 1) * 8, hipHostMallocDefault) != hipSuccess)
                return TFIDF_E_NOMEM;
            ctx->idf_pin_n = (size_t)K + 1;
        }
        if (K < 2 * 16384) {
            for (uint32_t k = 0; k < K; ++k) ctx->idf_pin[k] = log(1.0 * (double)Nt / (double)vals[k]);
        } else {
            idf_post(ctx, ctx->idf_pin, Nt, vals.data(), K);
            idf_join(ctx);
        }
        HIPCHK(hipMemcpyAsync(ctx->idf_vals.p, ctx->idf_pin, (size_t)K * 8, hipMemcpyHostToDevice, s));
        ctx->idf_pin_busy = true;
        HIPCHK(hipStreamSynchronize(s));
        ctx->idf_pin_busy = false;
    } else {
        HIPCHK(hipStreamSynchronize(s));
    }
    /* the build's status, read as run_local reads K1's */
    if (st & ST_BOUNDS) {
        fprintf(stderr, "tfidf: model import: internal bounds check tripped (status 0x%x)\n", st);
        return TFIDF_E_STATE;
    }
    if (st & ST_LONG_COLLIDE) {   /* dev_vocab.h: reported, never merged */
        fprintf(stderr, "tfidf: two distinct terms of 16 bytes or more share their 120-bit identity key\n");
        return TFIDF_E_CAPACITY;
    }
    if (st & (ST_VOCAB_FULL | ST_VOCAB_SPIN | ST_TERM_LONG)) return TFIDF_E_CAPACITY;   /* not at these loads: no retry */
    if (st & ST_MODEL_DUP) return TFIDF_E_STATE;
    ctx->local_long = nlong != 0;
    ctx->V = V;
    ctx->Vg = V;
    ctx->ndocs_total = Nt;
    ctx->ndocs = 0;
    ctx->npairs = 0;
    ctx->info_npairs = 0;
    ctx->info_V = V;
    ctx->wt_tf = ctx->wt_idf = ctx->wt_norm = 0;   /* the model file records no scheme */
    ctx->rw_idf_mode = 0;
    ctx->corpus = tfidf_corpus{};
    ctx->corpus.nbytes = nbytes;   /* VocabRO.corpus_bytes: the blob stands where the corpus does */
    ctx->dev_bytes = ctx->m_blob.as<uint8_t>();
    ctx->dev_ids = nullptr;
    ctx->m_blob_bytes = nbytes;
    ctx->have_model = true;
    ctx->model_only = true;
    tfidf_model_info mi{};
    mi.nterms = V;
    mi.table_slots = cap;
    mi.blob_bytes = nbytes;
    mi.long_terms = nlong;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev_m[0], ctx->ev_m[1]);
    mi.ms_build = ms;
    mi.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    ctx->minfo = mi;
    return TFIDF_OK;
}

extern "C" int tfidf_last_model_info(const tfidf_ctx* ctx, tfidf_model_info* info) {
    if (!ctx || !info || info->size < sizeof(uint64_t)) return TFIDF_E_INVAL;
    const uint64_t n = info->size < sizeof(tfidf_model_info) ? info->size : sizeof(tfidf_model_info);
    tfidf_model_info o = ctx->minfo;
    o.size = n;
    memcpy(info, &o, (size_t)n);
    return TFIDF_OK;
}

/* ------------------------------------------------------------------- prune ----
 * Vocabulary pruning by document frequency over the resident result (prune.hip; the parameter
 * check and the model form are prune_host.c).  Select (flags, the max_features sort, bitmap, new
 * ranks), the term arrays, the pair pass.  Everything is written into spare buffers of the
 * context, which change places with the resident ones when every step has succeeded; only
 * rank_of_slot is rewritten in place, by the last launch.  idf_rank is the score stage's scratch
 * and has no reader after a run (transform reads the idf by df), so it is left alone. */

/* a spare as large as the buffer it will change places with: after the swap neither a run nor
 * the next prune has anything to grow */
static int ensure_spare(DevBuf& spare, const DevBuf& orig, size_t need) {
    const size_t want = orig.cap > need ? orig.cap : need;
    if (spare.p && spare.cap >= want) return 0;
    spare.release();
    if (tfidf_dev_malloc(&spare.p, want) != hipSuccess) {
        (void)hipGetLastError();
        spare.p = nullptr;
        return -1;
    }
    spare.cap = want;
    return 0;
}

extern "C" int tfidf_prune(tfidf_ctx* ctx, const tfidf_prune_params* params) {
    if (!ctx || tfidf_prune_check(params) != TFIDF_OK) return TFIDF_E_INVAL;
    if (!ctx->have_result || ctx->model_only) return TFIDF_E_STATE;
    if (ctx->xp && params->max_features) return TFIDF_E_INVAL;   /* the ranks share no term table */
    const auto wall0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    for (hipEvent_t& e : ctx->ev_pr)
        if (!e) HIPCHK(hipEventCreate(&e));
    if (!ctx->ncu) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || n <= 0) n = 256;
        ctx->ncu = (uint32_t)n;
    }
    const uint32_t V = ctx->V, N = ctx->ndocs, M = params->max_features;
    const uint64_t P = ctx->npairs, Nt = ctx->ndocs_total;
    const uint64_t ntiles = P / PR_TILE + 1u;
    const bool cut = M != 0u && M < V;   /* M >= V cannot remove a survivor */
    DevBuf& dfb = ctx->xp ? ctx->df_global : ctx->df_local;   /* df_of_run */
    ENSURE(ctx->pr_flag, ((size_t)V + 1) * 4 + 4);
    ENSURE(ctx->pr_bits, (((size_t)V + 63) / 64) * 8 + 16);
    ENSURE(ctx->pr_tcnt, (size_t)(ntiles + 1) * 8);
    ENSURE(ctx->pr_tdoc, (size_t)(ntiles + 1) * 4);
    ENSURE(ctx->pr_misc, 256);
    if (cut) {
        ENSURE(ctx->pr_k0, (size_t)V * 8 + 8);
        ENSURE(ctx->pr_k1, (size_t)V * 8 + 8);
        ENSURE(ctx->pr_v0, (size_t)V * 4 + 4);
        ENSURE(ctx->pr_v1, (size_t)V * 4 + 4);
    }
    if (ensure_spare(ctx->pr_sor, ctx->slot_of_rank, (size_t)V * 4 + 4) || ensure_spare(ctx->pr_df, dfb, (size_t)V * 4 + 4) ||
        ensure_spare(ctx->pr_term, ctx->out_term, (size_t)P * 4 + 4) || ensure_spare(ctx->pr_cnt, ctx->out_cnt, (size_t)P * 4 + 4) ||
        ensure_spare(ctx->pr_score, ctx->out_score, (size_t)P * 8 + 8) || ensure_spare(ctx->pr_off, ctx->out_off, ((size_t)N + 1) * 8))
        return TFIDF_E_NOMEM;
    {   /* the scans' block sums and the sort's histograms */
        const uint64_t nb = ((uint64_t)V + 2047) / 2048;
        const size_t want = scan_scratch((uint64_t)V + 1) + scan_scratch(ntiles + 1) +
                            (cut ? (size_t)(256 * nb + 1) * 4 + scan_scratch(256 * nb) : 0) + 8192;
        if (want > ctx->arena_buf.cap && arena_reset(ctx, want) != 0) return TFIDF_E_NOMEM;
        ctx->arena.used = 0;   /* as format_prepare: nothing of the result lives in the arena */
    }
    uint32_t* flag = ctx->pr_flag.as<uint32_t>();   /* the keep flags, then in place the new ranks */
    uint32_t* bits = ctx->pr_bits.as<uint32_t>();
    /* ---- select ---- */
    HIPCHK(hipEventRecord(ctx->ev_pr[0], s));
    if (launch_pr_range(df_of_run(ctx), V, Nt, params->min_df, params->max_df, flag,
                        cut ? ctx->pr_k0.as<uint64_t>() : nullptr, ctx->pr_v0.as<uint32_t>(), s)) {
        HIPCHK(hipGetLastError());
        return TFIDF_E_HIP;
    }
    uint64_t cut_keys[2] = {PR_KEY_DEAD, PR_KEY_DEAD};   /* the sorted keys at positions M - 1 and M */
    if (cut) {
        uint32_t byte_mask = 1u << 4;   /* PR_KEY_DEAD's bit; below it the bytes Nt - df can reach */
        for (int b = 0; b < 4; ++b)
            if ((Nt >> (8 * b)) != 0) byte_mask |= 1u << b;
        const int where = radix_sort_u64(ctx->pr_k0.as<uint64_t>(), ctx->pr_v0.as<uint32_t>(), ctx->pr_k1.as<uint64_t>(),
                                         ctx->pr_v1.as<uint32_t>(), V, byte_mask, ctx->arena, s);
        if (where < 0) { HIPCHK(hipGetLastError()); return where == -2 ? TFIDF_E_NOMEM : TFIDF_E_HIP; }
        const uint64_t* ks = where ? ctx->pr_k1.as<uint64_t>() : ctx->pr_k0.as<uint64_t>();
        const uint32_t* vs = where ? ctx->pr_v1.as<uint32_t>() : ctx->pr_v0.as<uint32_t>();
        if (launch_pr_take(ks, vs, V, M, flag, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipMemcpyAsync(cut_keys, ks + (M - 1u), 16, hipMemcpyDeviceToHost, s));   /* M < V: both exist */
    }
    if (launch_pr_bitmap(flag, V, bits, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
    {
        const int sc = scan_excl_u32(flag, flag, V, ctx->arena, s);
        if (sc) { if (sc != -2) HIPCHK(hipGetLastError()); return sc == -2 ? TFIDF_E_NOMEM : TFIDF_E_HIP; }
    }
    HIPCHK(hipEventRecord(ctx->ev_pr[1], s));
    uint32_t V2 = 0;
    HIPCHK(hipMemcpyAsync(&V2, flag + V, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (V2 > V) return TFIDF_E_STATE;
    tfidf_prune_info pi{};
    pi.nterms_before = V;
    pi.npairs_before = P;
    /* the cut removed a survivor of the range test exactly when position M holds one */
    if (cut && cut_keys[1] != PR_KEY_DEAD && cut_keys[0] <= Nt) pi.cut_df = (uint32_t)(Nt - cut_keys[0]);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev_pr[0], ctx->ev_pr[1]);
    pi.ms_select = ms;
    if (V2 == V) {   /* nothing to remove: every byte stays */
        pi.nterms_after = V;
        pi.npairs_after = P;
        pi.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        ctx->pinfo = pi;
        return TFIDF_OK;
    }
    /* ---- terms ---- */
    PrTerms ta{bits, flag, V, ctx->slot_of_rank.as<uint32_t>(), df_of_run(ctx), ctx->pr_sor.as<uint32_t>(),
               ctx->pr_df.as<uint32_t>()};
    if (launch_pr_terms(ta, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
    HIPCHK(hipEventRecord(ctx->ev_pr[2], s));
    /* ---- pairs ---- */
    HIPCHK(hipMemsetAsync(ctx->pr_misc.p, 0, 16, s));
    PrPairs pa{};
    pa.out_off = ctx->out_off.as<uint64_t>();
    pa.out_term = ctx->out_term.as<uint32_t>();
    pa.out_cnt = ctx->out_cnt.as<uint32_t>();
    pa.out_score = ctx->out_score.as<double>();
    pa.npairs = P;
    pa.ndocs = N;
    pa.V = V;
    pa.bits = bits;
    pa.new_rank = flag;
    pa.ntiles = ntiles;
    pa.tile_cnt = ctx->pr_tcnt.as<uint64_t>();
    pa.tile_doc = ctx->pr_tdoc.as<uint32_t>();
    pa.new_term = ctx->pr_term.as<uint32_t>();
    pa.new_cnt = ctx->pr_cnt.as<uint32_t>();
    pa.new_score = ctx->pr_score.as<double>();
    pa.new_off = ctx->pr_off.as<uint64_t>();
    pa.emptied = ctx->pr_misc.as<uint32_t>();
    if (launch_pr_tiledoc(pa, s) || launch_pr_count(pa, ctx->ncu, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
    {
        const int sc = scan_excl_u64(pa.tile_cnt, pa.tile_cnt, ntiles, ctx->arena, s);
        if (sc) { if (sc != -2) HIPCHK(hipGetLastError()); return sc == -2 ? TFIDF_E_NOMEM : TFIDF_E_HIP; }
    }
    if (launch_pr_write(pa, ctx->ncu, s) || launch_pr_emptied(pa, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
    HIPCHK(hipEventRecord(ctx->ev_pr[3], s));
    uint64_t P2 = 0;
    uint32_t emptied = 0;
    HIPCHK(hipMemcpyAsync(&P2, pa.tile_cnt + ntiles, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&emptied, pa.emptied, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));   /* every spare is written: from here on the call cannot fail half-way */
    if (P2 > P) return TFIDF_E_STATE;
    if (launch_pr_slots(ta, ctx->rank_of_slot.as<uint32_t>(), ctx->vcap, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
    HIPCHK(hipStreamSynchronize(s));
    std::swap(ctx->slot_of_rank, ctx->pr_sor);
    std::swap(dfb, ctx->pr_df);
    std::swap(ctx->out_term, ctx->pr_term);
    std::swap(ctx->out_cnt, ctx->pr_cnt);
    std::swap(ctx->out_score, ctx->pr_score);
    std::swap(ctx->out_off, ctx->pr_off);
    ctx->V = V2;
    ctx->npairs = P2;
    ctx->text_valid = false;
    ctx->tmeta_valid = false;
    ctx->norm_valid = false;   /* bm25_L stays: docSize is unchanged */
    pi.nterms_after = V2;
    pi.npairs_after = P2;
    pi.docs_emptied = emptied;
    (void)hipEventElapsedTime(&ms, ctx->ev_pr[1], ctx->ev_pr[2]);
    pi.ms_terms = ms;
    (void)hipEventElapsedTime(&ms, ctx->ev_pr[2], ctx->ev_pr[3]);
    pi.ms_pairs = ms;
    pi.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    ctx->pinfo = pi;
    return TFIDF_OK;
}

extern "C" int tfidf_last_prune_info(const tfidf_ctx* ctx, tfidf_prune_info* info) {
    if (!ctx || !info || info->size < sizeof(uint64_t)) return TFIDF_E_INVAL;
    const uint64_t n = info->size < sizeof(tfidf_prune_info) ? info->size : sizeof(tfidf_prune_info);
    tfidf_prune_info o = ctx->pinfo;
    o.size = n;
    memcpy(info, &o, (size_t)n);
    return TFIDF_OK;
}

/* --------------------------------------------------------------- weighting ----
 * Weighting schemes over the resident result (reweight.hip; the check, the formulas of the
 * tables and the host form are weight_host.c).  Tables (the scheme's idf in the layout of
 * idf_vals, the sublinear tf table, the idf by rank), then the pair pass into prune's spare
 * score buffer, which changes places with out_score when every step has succeeded.  idf_vals is
 * never written: the reference scheme reads it again. */

/* The scheme's idf for every df the run's table covers, in that table's layout, on the
 * context's workers; kept until the next run or import (a prune leaves the index a superset). */
static int rw_idf_table(tfidf_ctx* ctx, uint32_t mode, uint64_t* nlogs) {
    if (mode == TFIDF_IDF_REF || mode == TFIDF_IDF_NONE || ctx->rw_idf_mode == mode) return TFIDF_OK;
    const uint64_t Nt = ctx->ndocs_total;
    if (!ctx->V || !Nt) return TFIDF_OK;
    hipStream_t s = ctx->stream;
    if (const int q = idf_pin_quiesce(ctx)) return q;
    const double keep_host = ctx->ms_idf_host, keep_wait = ctx->ms_idf_wait;   /* the run's, in tfidf_last_run_info */
    std::vector<uint32_t> vals;
    uint64_t n = Nt + 1;   /* entries of the table */
    if (Nt > IDF_FULL_MAX) {   /* the distinct df values through the run's index, listed again */
        const size_t want = (size_t)(Nt + 2) * 4 + 8192;
        if (want > ctx->arena_buf.cap && arena_reset(ctx, want) != 0) return TFIDF_E_NOMEM;
        ctx->arena.used = 0;   /* as format_prepare: nothing of the result lives in the arena */
        uint32_t* vals_dev = (uint32_t*)ctx->arena.get((size_t)(Nt + 2) * 4);
        if (!vals_dev) return TFIDF_E_NOMEM;
        uint32_t* present = ctx->present.as<uint32_t>();
        if (!present || ctx->present.cap < (Nt + 2) * 4) return TFIDF_E_STATE;
        if (launch_df_list(present, Nt + 1, vals_dev, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        uint32_t K = 0;
        HIPCHK(hipMemcpyAsync(&K, present + Nt + 1, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (K == 0 || (uint64_t)K > Nt + 1) return TFIDF_E_STATE;
        vals.resize(K);
        HIPCHK(hipMemcpyAsync(vals.data(), vals_dev, (size_t)K * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        n = K;
    }
    ENSURE(ctx->rw_idf, (size_t)n * 8 + 8);
    if (ctx->idf_pin_n < (size_t)n + 1) {
        if (ctx->idf_pin) (void)hipHostFree(ctx->idf_pin);
        ctx->idf_pin = nullptr;
        ctx->idf_pin_n = 0;
        if (hipHostMalloc((void**)&ctx->idf_pin, ((size_t)n + 1) * 8, hipHostMallocDefault) != hipSuccess) return TFIDF_E_NOMEM;
        ctx->idf_pin_n = (size_t)n + 1;
    }
    if (vals.empty()) {
        ctx->idf_pin[0] = 0.0;   /* df >= 1 for every term that occurs */
        idf_post(ctx, ctx->idf_pin, Nt, nullptr, Nt, mode);
        *nlogs += Nt;
    } else {
        idf_post(ctx, ctx->idf_pin, Nt, vals.data(), n, mode);
        *nlogs += n;
    }
    idf_join(ctx);
    ctx->ms_idf_host = keep_host;
    ctx->ms_idf_wait = keep_wait;
    HIPCHK(hipMemcpyAsync(ctx->rw_idf.p, ctx->idf_pin, (size_t)n * 8, hipMemcpyHostToDevice, s));
    ctx->idf_pin_busy = true;
    HIPCHK(hipStreamSynchronize(s));
    ctx->idf_pin_busy = false;
    ctx->rw_idf_mode = mode;
    return TFIDF_OK;
}

/* sublinear tf, first half: the largest of n counts (n_dev: the total still on the device) and
 * the list of those above RW_LUT_MAX, into rw_misc[RWM_CMAX..] and rw_list */
static int rw_cmax_launch(tfidf_ctx* ctx, const uint32_t* count, uint64_t n, const uint32_t* n_dev) {
    ENSURE(ctx->rw_misc, 256);
    ENSURE(ctx->rw_list, (size_t)RW_LIST_MAX * 4);
    ENSURE(ctx->rw_lut, ((size_t)RW_LUT_MAX + 1) * 8);
    uint32_t* misc = ctx->rw_misc.as<uint32_t>();
    HIPCHK(hipMemsetAsync(misc + RWM_CMAX, 0, 8, ctx->stream));
    if (launch_rw_cmax(count, n, n_dev, misc + RWM_CMAX, ctx->rw_list.as<uint32_t>(), RW_LIST_MAX, ctx->stream)) {
        HIPCHK(hipGetLastError());
        return TFIDF_E_HIP;
    }
    return TFIDF_OK;
}
/* second half, with the two words on the host: the table fl(1 + log c) up to min(cmax,
 * RW_LUT_MAX) (grown, never rebuilt: its values do not depend on the run) and the listed
 * counts, sorted and distinct, with their values.  Synchronises the stream. */
static int rw_tf_finish(tfidf_ctx* ctx, uint32_t cmax, uint32_t nlist, uint32_t* nlisted, uint64_t* nlogs) {
    hipStream_t s = ctx->stream;
    *nlisted = 0;
    if (nlist > RW_LIST_MAX) return TFIDF_E_CAPACITY;   /* the list is bounded; nothing has been scored */
    const uint32_t need = cmax < RW_LUT_MAX ? cmax : RW_LUT_MAX;
    bool wait = false;
    if (need > ctx->rw_lut_n || ctx->rw_lut_host.empty()) {
        if (ctx->rw_lut_host.empty()) ctx->rw_lut_host.assign((size_t)RW_LUT_MAX + 1, 0.0);
        const uint32_t first = ctx->rw_lut_n + 1u;
        for (uint32_t c = first; c <= need; ++c) ctx->rw_lut_host[c] = tfidf_weight_tf_log(c);
        const uint32_t from = ctx->rw_lut_n ? first : 0u;
        if (need + 1u > from) {
            HIPCHK(hipMemcpyAsync(ctx->rw_lut.as<double>() + from, ctx->rw_lut_host.data() + from, (size_t)(need + 1u - from) * 8,
                                  hipMemcpyHostToDevice, s));
            wait = true;
        }
        if (need >= first) *nlogs += need - first + 1u;
    }
    if (nlist) {
        std::vector<uint32_t>& lc = ctx->rw_list_host;
        lc.resize(nlist);
        HIPCHK(hipMemcpyAsync(lc.data(), ctx->rw_list.p, (size_t)nlist * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        std::sort(lc.begin(), lc.end());
        lc.erase(std::unique(lc.begin(), lc.end()), lc.end());
        std::vector<double>& lv = ctx->rw_listv_host;
        lv.resize(lc.size());
        for (size_t i = 0; i < lc.size(); ++i) lv[i] = tfidf_weight_tf_log(lc[i]);
        ENSURE(ctx->rw_listv, lc.size() * 8 + 8);
        HIPCHK(hipMemcpyAsync(ctx->rw_list.p, lc.data(), lc.size() * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(ctx->rw_listv.p, lv.data(), lv.size() * 8, hipMemcpyHostToDevice, s));
        *nlisted = (uint32_t)lc.size();
        *nlogs += lc.size();
        wait = true;
    }
    if (wait) HIPCHK(hipStreamSynchronize(s));   /* the uploads read pageable host memory of the context */
    if (need > ctx->rw_lut_n) ctx->rw_lut_n = need;
    return TFIDF_OK;
}

/* the scheme-dependent members of a pair pass's arguments */
static void rw_scheme_args(tfidf_ctx* ctx, RwArgs& a, uint32_t tf, uint32_t norm, uint32_t nlisted) {
    a.tf_mode = tf;
    a.norm = norm;
    a.tf_lut = ctx->rw_lut.as<double>();
    a.lut_n = ctx->rw_lut_n;
    a.nlisted = nlisted;
    a.listed_c = ctx->rw_list.as<uint32_t>();
    a.listed_v = ctx->rw_listv.as<double>();
    a.big_list = ctx->rw_big.as<uint32_t>();
    a.misc = ctx->rw_misc.as<uint32_t>();
}

extern "C" int tfidf_reweight(tfidf_ctx* ctx, const tfidf_weighting* w) {
    if (!ctx || tfidf_weighting_check(w) != TFIDF_OK) return TFIDF_E_INVAL;
    if (!ctx->have_result && !ctx->have_model) return TFIDF_E_STATE;
    if (tfidf_weighting_check_n(w, ctx->ndocs_total) != TFIDF_OK) return TFIDF_E_INVAL;
    const auto wall0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    for (hipEvent_t& e : ctx->ev_rw)
        if (!e) HIPCHK(hipEventCreate(&e));
    if (!ctx->ncu) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || n <= 0) n = 256;
        ctx->ncu = (uint32_t)n;
    }
    const bool pairs = ctx->have_result && !ctx->model_only;
    const uint32_t V = ctx->V, N = pairs ? ctx->ndocs : 0u;
    const uint64_t P = pairs ? ctx->npairs : 0u, Nt = ctx->ndocs_total;
    tfidf_reweight_info ri{};
    ri.tf = w->tf;
    ri.idf = w->idf;
    ri.norm = w->norm;
    ri.npairs = P;
    ri.ndocs = N;
    if (w->tf == ctx->wt_tf && w->idf == ctx->wt_idf && w->norm == ctx->wt_norm) {   /* active already: no byte changes */
        ri.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        ctx->rwinfo = ri;
        return TFIDF_OK;
    }
    ri.changed = 1;
    HIPCHK(hipEventRecord(ctx->ev_rw[0], s));
    if (const int rc = rw_idf_table(ctx, w->idf, &ri.nlogs)) return rc;
    if (P && N) {
        if (ensure_spare(ctx->pr_score, ctx->out_score, (size_t)P * 8 + 8)) return TFIDF_E_NOMEM;
        ENSURE(ctx->rw_misc, 256);
        ENSURE(ctx->rw_big, (size_t)N * 4 + 4);
        uint32_t nlisted = 0;
        if (w->tf == TFIDF_TF_LOG) {
            if (const int rc = rw_cmax_launch(ctx, ctx->out_cnt.as<uint32_t>(), P, nullptr)) return rc;
            uint32_t cw[2] = {0, 0};
            HIPCHK(hipMemcpyAsync(cw, ctx->rw_misc.as<uint32_t>() + RWM_CMAX, 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (const int rc = rw_tf_finish(ctx, cw[0], cw[1], &nlisted, &ri.nlogs)) return rc;
            ri.max_count = cw[0];
            ri.listed_counts = nlisted;
        }
        RwArgs a{};
        a.off = ctx->out_off.as<uint64_t>();
        a.npairs = P;
        a.ndocs = N;
        a.order = ctx->order;
        a.doc_size = ctx->doc_size.as<uint32_t>();
        a.count = ctx->out_cnt.as<uint32_t>();
        a.key = ctx->out_term.as<uint32_t>();
        a.key_n = V;
        if (w->idf != TFIDF_IDF_NONE) {   /* the idf by rank: one 8-byte gather per pair in the pair pass */
            ENSURE(ctx->idf_rank, (size_t)V * 8 + 8);
            const double* tab = w->idf == TFIDF_IDF_REF ? ctx->idf_vals.as<double>() : ctx->rw_idf.as<double>();
            const uint32_t* idx = Nt <= IDF_FULL_MAX ? nullptr : ctx->present.as<uint32_t>();
            if (launch_rw_idf_rank(df_of_run(ctx), V, tab, idx, Nt + 1, ctx->idf_rank.as<double>(), s)) {
                HIPCHK(hipGetLastError());
                return TFIDF_E_HIP;
            }
            a.idf = ctx->idf_rank.as<double>();
        }
        a.score = ctx->pr_score.as<double>();
        rw_scheme_args(ctx, a, w->tf, w->norm, nlisted);
        HIPCHK(hipEventRecord(ctx->ev_rw[1], s));
        if (launch_rw_pairs(a, ctx->ncu, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_rw[2], s));
        uint32_t mw[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(mw, ctx->rw_misc.as<uint32_t>() + RWM_BIG, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));   /* the spare is written: from here on the call cannot fail */
        std::swap(ctx->out_score, ctx->pr_score);
        ctx->text_valid = false;
        ctx->norm_valid = false;   /* bm25_L stays: docSize is unchanged */
        ri.big_docs = mw[0] < N ? mw[0] : N;
        ri.zero_norm_docs = mw[1];
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ctx->ev_rw[0], ctx->ev_rw[1]);
        ri.ms_tables = ms;
        (void)hipEventElapsedTime(&ms, ctx->ev_rw[1], ctx->ev_rw[2]);
        ri.ms_pairs = ms;
    }
    ctx->wt_tf = w->tf;
    ctx->wt_idf = w->idf;
    ctx->wt_norm = w->norm;
    ri.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    ctx->rwinfo = ri;
    return TFIDF_OK;
}

extern "C" int tfidf_weighting_get(const tfidf_ctx* ctx, tfidf_weighting* out) {
    if (!ctx || !out || out->size < sizeof(tfidf_weighting)) return TFIDF_E_INVAL;
    out->tf = ctx->wt_tf;
    out->idf = ctx->wt_idf;
    out->norm = ctx->wt_norm;
    out->reserved = 0;
    return TFIDF_OK;
}

extern "C" int tfidf_last_reweight_info(const tfidf_ctx* ctx, tfidf_reweight_info* info) {
    if (!ctx || !info || info->size < sizeof(uint64_t)) return TFIDF_E_INVAL;
    const uint64_t n = info->size < sizeof(tfidf_reweight_info) ? info->size : sizeof(tfidf_reweight_info);
    tfidf_reweight_info o = ctx->rwinfo;
    o.size = n;
    memcpy(info, &o, (size_t)n);
    return TFIDF_OK;
}

/* ---------------------------------------------------------------- keywords ----
 * Per-document top-k terms over the resident result (terms.hip).  The rows (every output
 * position, or the positions of the requested ids) are cut into batches whose device result
 * buffers stay under the context's budget; a batch is one selection pass, a scan of the
 * selected words' lengths and a gather of their bytes, copied straight into the caller's
 * arrays.  Nothing of the run's result is written. */

extern "C" void tfidf_doc_terms_free(tfidf_doc_terms* t) {
    if (!t) return;
    free(t->doc); free(t->pos); free(t->npairs); free(t->nterms); free(t->term); free(t->count);
    free(t->score); free(t->pair); free(t->word_off); free(t->word_bytes);
    memset(t, 0, sizeof(*t));
}

extern "C" int tfidf_top_terms(tfidf_ctx* ctx, const uint32_t* doc_ids, uint32_t ndocs, uint32_t k, tfidf_doc_terms* out) {
    if (!ctx || !out) return TFIDF_E_INVAL;
    if (k == 0 || k > TFIDF_TERMS_MAX_K) return TFIDF_E_INVAL;
    if (!ctx->have_result) return TFIDF_E_STATE;
    const auto wall0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    for (hipEvent_t& e : ctx->ev_t)
        if (!e) HIPCHK(hipEventCreate(&e));
    if (!ctx->ncu) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || n <= 0) n = 256;
        ctx->ncu = (uint32_t)n;
    }
    const uint32_t N = ctx->ndocs, V = ctx->V;
    const uint32_t R = doc_ids ? ndocs : N;
    const size_t RK = (size_t)R * k;
    memset(out, 0, sizeof(*out));
    out->ndocs = R;
    out->k = k;
    out->doc = (uint32_t*)calloc((size_t)R + 1, 4);
    out->pos = (uint32_t*)calloc((size_t)R + 1, 4);
    out->npairs = (uint64_t*)calloc((size_t)R + 1, 8);
    out->nterms = (uint32_t*)calloc((size_t)R + 1, 4);
    out->term = (uint32_t*)calloc(RK + 1, 4);
    out->count = (uint32_t*)calloc(RK + 1, 4);
    out->score = (double*)calloc(RK + 1, 8);
    out->pair = (uint64_t*)calloc(RK + 1, 8);
    out->word_off = (uint64_t*)calloc(RK + 1, 8);
    out->word_bytes = (uint8_t*)calloc(1, 1);
    struct TermsGuard {   /* an error return leaves *out zeroed */
        tfidf_doc_terms* t;
        ~TermsGuard() { if (t) tfidf_doc_terms_free(t); }
    } guard{out};
    if (!out->doc || !out->pos || !out->npairs || !out->nterms || !out->term || !out->count || !out->score ||
        !out->pair || !out->word_off || !out->word_bytes)
        return TFIDF_E_NOMEM;
    tfidf_terms_info ti{};
    ti.ndocs = R;
    ti.k = k;
    float ms = 0;

    /* ---- the selected words' lengths and byte sources: the formatter's term metadata ---- */
    if (V && !ctx->tmeta_valid) {
        ENSURE(ctx->t_key, (size_t)V * 16 + 16);
        ENSURE(ctx->t_len, (size_t)V * 4 + 4);
        if (launch_term_meta(ctx->vkeys.as<uint4>(), ctx->vrep.as<uint64_t>(), ctx->slot_of_rank.as<uint32_t>(), V,
                             ctx->t_key.as<uint4>(), ctx->t_len.as<uint32_t>(), s))
            return TFIDF_E_HIP;
        ctx->tmeta_valid = true;
    }

    /* ---- lookup: one lane per requested id ---- */
    const uint32_t* d_pos = nullptr;
    if (doc_ids && R) {
        ENSURE(ctx->tm_ids, (size_t)R * 8 + 8);
        uint32_t* d_ids = ctx->tm_ids.as<uint32_t>();
        HIPCHK(hipMemcpyAsync(d_ids, doc_ids, (size_t)R * 4, hipMemcpyHostToDevice, s));
        TLookupArgs la{d_ids, R, ctx->order, ctx->dev_ids, N, d_ids + R};
        HIPCHK(hipEventRecord(ctx->ev_t[0], s));
        if (launch_terms_lookup(la, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_t[1], s));
        HIPCHK(hipMemcpyAsync(out->pos, d_ids + R, (size_t)R * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        (void)hipEventElapsedTime(&ms, ctx->ev_t[0], ctx->ev_t[1]);
        ti.ms_lookup = ms;
        d_pos = d_ids + R;
        ti.out_bytes += (uint64_t)R * 4;
    } else {
        for (uint32_t r = 0; r < R; ++r) out->pos[r] = r;
    }

    /* ---- batches of rows under the budget: 32 bytes per entry, 20 per row ---- */
    const uint64_t per_row = (uint64_t)k * 32 + 20;
    uint64_t B = ctx->terms_bytes / per_row;
    B = B < 1 ? 1 : B;
    if (B > R) B = R;
    const size_t BK = (size_t)B * k;
    if (R) {
        ENSURE(ctx->tm_rows, (size_t)B * 16 + 16);
        ENSURE(ctx->tm_score, BK * 8 + 8);
        ENSURE(ctx->tm_pair, BK * 8 + 8);
        ENSURE(ctx->tm_term, BK * 4 + 4);
        ENSURE(ctx->tm_cnt, BK * 4 + 4);
        ENSURE(ctx->tm_woff, BK * 8 + 16);
        ENSURE(ctx->tm_big, (size_t)B * 4 + 16);
    }
    std::vector<uint64_t> h_woff(BK + 1);
    std::vector<uint32_t> h_doc(B);
    uint64_t wbase = 0;
    for (uint64_t r0 = 0; r0 < R; r0 += B) {
        const uint32_t nb = (uint32_t)(R - r0 < B ? R - r0 : B);
        const size_t nbk = (size_t)nb * k;
        ++ti.nbatches;
        TSelArgs sa{};
        sa.out_off = ctx->out_off.as<uint64_t>();
        sa.out_term = ctx->out_term.as<uint32_t>();
        sa.out_cnt = ctx->out_cnt.as<uint32_t>();
        sa.out_score = ctx->out_score.as<double>();
        sa.order = ctx->order;
        sa.doc_ids = ctx->dev_ids;
        sa.tlen = ctx->t_len.as<uint32_t>();
        sa.ndocs = N;
        sa.nterms = V;
        sa.npairs = ctx->npairs;
        sa.pos = d_pos;
        sa.row0 = (uint32_t)r0;
        sa.nrows = nb;
        sa.k = k;
        sa.rnpairs = ctx->tm_rows.as<uint64_t>();
        sa.rnterms = (uint32_t*)(sa.rnpairs + B);
        sa.rdoc = sa.rnterms + B;
        sa.score = ctx->tm_score.as<uint64_t>();
        sa.pair = ctx->tm_pair.as<uint64_t>();
        sa.term = ctx->tm_term.as<uint32_t>();
        sa.cnt = ctx->tm_cnt.as<uint32_t>();
        sa.wlen = ctx->tm_woff.as<uint64_t>();
        sa.big_list = ctx->tm_big.as<uint32_t>();
        sa.big_count = sa.big_list + B;
        HIPCHK(hipEventRecord(ctx->ev_t[0], s));
        if (launch_terms_select(sa, ctx->ncu, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_t[1], s));
        /* word lengths -> offsets inside the batch, in place; [nbk] = the batch's word bytes */
        ctx->arena.used = 0;   /* as format_prepare: nothing of the result lives in the arena */
        const int sc = scan_excl_u64(sa.wlen, sa.wlen, nbk, ctx->arena, s);
        if (sc) { if (sc != -2) HIPCHK(hipGetLastError()); return sc == -2 ? TFIDF_E_NOMEM : TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_t[2], s));
        uint32_t nbig = 0;
        HIPCHK(hipMemcpyAsync(h_woff.data(), sa.wlen, (nbk + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&nbig, sa.big_count, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const uint64_t wtotal = h_woff[nbk];
        ENSURE(ctx->tm_words, wtotal + 16);
        TWordArgs wa{sa.term, sa.wlen, nbk, ctx->t_key.as<uint4>(), V, ctx->dev_bytes, ctx->corpus.nbytes,
                     ctx->tm_words.as<uint8_t>()};
        HIPCHK(hipEventRecord(ctx->ev_t[3], s));
        if (launch_terms_words(wa, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_t[4], s));
        uint8_t* wb = (uint8_t*)realloc(out->word_bytes, (size_t)(wbase + wtotal) + 1);
        if (!wb) return TFIDF_E_NOMEM;
        out->word_bytes = wb;
        const size_t e0 = (size_t)r0 * k;
        HIPCHK(hipMemcpyAsync(out->npairs + r0, sa.rnpairs, (size_t)nb * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->nterms + r0, sa.rnterms, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_doc.data(), sa.rdoc, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->score + e0, sa.score, nbk * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->pair + e0, sa.pair, nbk * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->term + e0, sa.term, nbk * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->count + e0, sa.cnt, nbk * 4, hipMemcpyDeviceToHost, s));
        if (wtotal) HIPCHK(hipMemcpyAsync(wb + wbase, ctx->tm_words.p, wtotal, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        (void)hipEventElapsedTime(&ms, ctx->ev_t[0], ctx->ev_t[1]);
        ti.ms_select += ms;
        (void)hipEventElapsedTime(&ms, ctx->ev_t[1], ctx->ev_t[2]);
        ti.ms_words += ms;
        (void)hipEventElapsedTime(&ms, ctx->ev_t[3], ctx->ev_t[4]);
        ti.ms_words += ms;
        ti.big_docs += nbig < nb ? nbig : nb;
        ti.out_bytes += (uint64_t)nb * 16 + nbk * 32 + wtotal;
        for (uint32_t i = 0; i < nb; ++i) out->doc[r0 + i] = doc_ids ? doc_ids[r0 + i] : h_doc[i];
        for (size_t i = 0; i < nbk; ++i) out->word_off[e0 + i] = wbase + h_woff[i];
        wbase += wtotal;
    }
    out->word_off[RK] = wbase;
    ti.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    ctx->tinfo = ti;
    guard.t = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_last_terms_info(const tfidf_ctx* ctx, tfidf_terms_info* info) {
    if (!ctx || !info || info->size < sizeof(uint64_t)) return TFIDF_E_INVAL;
    const uint64_t n = info->size < sizeof(tfidf_terms_info) ? info->size : sizeof(tfidf_terms_info);
    tfidf_terms_info o = ctx->tinfo;
    o.size = n;
    memcpy(info, &o, (size_t)n);
    return TFIDF_OK;
}

/* ----------------------------------------------------------------- similar ----
 * Top-k similar documents over the resident result (similar.hip).  The norms are computed by
 * the first call after a run.  The rows (every output position, or the positions of the
 * requested ids) are cut into groups of up to SG_MAX under the accumulator budget; a group is
 * a postings table (masks, offsets, weights) built on the device from the rows' vectors, one scan of the pairs that
 * leaves sim and the shared-term count per (row, output position), the top-k rounds of
 * tfidf_query over them, and a lookup of the neighbours' positions for their shared counts.
 * Nothing of the run's result is written. */

extern "C" void tfidf_neighbors_free(tfidf_neighbors* n) {
    if (!n) return;
    free(n->doc); free(n->pos); free(n->npairs); free(n->norm); free(n->nmatch); free(n->nnb);
    free(n->nb_doc); free(n->nb_shared); free(n->nb_score);
    memset(n, 0, sizeof(*n));
}

static int neighbors_alloc(tfidf_neighbors* out, uint32_t R, uint32_t k) {
    const size_t RK = (size_t)R * k;
    memset(out, 0, sizeof(*out));
    out->ndocs = R;
    out->k = k;
    out->doc = (uint32_t*)calloc((size_t)R + 1, 4);
    out->pos = (uint32_t*)calloc((size_t)R + 1, 4);
    out->npairs = (uint64_t*)calloc((size_t)R + 1, 8);
    out->norm = (double*)calloc((size_t)R + 1, 8);
    out->nmatch = (uint64_t*)calloc((size_t)R + 1, 8);
    out->nnb = (uint32_t*)calloc((size_t)R + 1, 4);
    out->nb_doc = (uint32_t*)calloc(RK + 1, 4);
    out->nb_shared = (uint32_t*)calloc(RK + 1, 4);
    out->nb_score = (double*)calloc(RK + 1, 8);
    if (!out->doc || !out->pos || !out->npairs || !out->norm || !out->nmatch || !out->nnb || !out->nb_doc ||
        !out->nb_shared || !out->nb_score) {
        tfidf_neighbors_free(out);
        return TFIDF_E_NOMEM;
    }
    return TFIDF_OK;
}

namespace {
struct NeighborsGuard {   /* an error return leaves *out zeroed */
    tfidf_neighbors* n;
    ~NeighborsGuard() { if (n) tfidf_neighbors_free(n); }
};
/* the call's rows on the device (sm_rows) */
struct SimCall {
    uint32_t R = 0;
    uint64_t* rb = nullptr;
    uint64_t* re = nullptr;
    double* rnorm = nullptr;
    double* rsq = nullptr;
    uint32_t* rpos = nullptr;
    uint32_t* rid = nullptr;
};
}  // namespace

static int sim_begin(tfidf_ctx* ctx) {
    HIPCHK(hipSetDevice(ctx->device));
    for (hipEvent_t& e : ctx->ev_s)
        if (!e) HIPCHK(hipEventCreate(&e));
    if (!ctx->ncu) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || n <= 0) n = 256;
        ctx->ncu = (uint32_t)n;
    }
    return TFIDF_OK;
}

static int sim_layout(tfidf_ctx* ctx, uint32_t R, SimCall& c) {
    ENSURE(ctx->sm_rows, (size_t)R * 40 + 64);
    c.R = R;
    c.rb = ctx->sm_rows.as<uint64_t>();
    c.re = c.rb + R;
    c.rnorm = (double*)(c.re + R);
    c.rsq = c.rnorm + R;
    c.rpos = (uint32_t*)(c.rsq + R);
    c.rid = c.rpos + R;
    return TFIDF_OK;
}

/* sq and norm by output position, once per run */
static int sim_norms(tfidf_ctx* ctx, tfidf_similar_info& si) {
    if (ctx->norm_valid) return TFIDF_OK;
    hipStream_t s = ctx->stream;
    const uint32_t N = ctx->ndocs;
    ENSURE(ctx->sm_norm, (size_t)N * 16 + 16);
    HIPCHK(hipEventRecord(ctx->ev_s[4], s));
    if (launch_sim_norms(ctx->out_off.as<uint64_t>(), ctx->out_score.as<double>(), N, ctx->npairs,
                         ctx->sm_norm.as<double>(), ctx->sm_norm.as<double>() + N, s)) {
        HIPCHK(hipGetLastError());
        return TFIDF_E_HIP;
    }
    HIPCHK(hipEventRecord(ctx->ev_s[5], s));
    HIPCHK(hipStreamSynchronize(s));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev_s[4], ctx->ev_s[5]);
    si.ms_norms = ms;
    ctx->norm_valid = true;
    return TFIDF_OK;
}

/* requested ids -> output positions at `d_pos` (k_terms_lookup) */
static int sim_lookup_ids(tfidf_ctx* ctx, const uint32_t* ids, uint32_t R, uint32_t* d_pos) {
    hipStream_t s = ctx->stream;
    ENSURE(ctx->sm_ids, (size_t)R * 4 + 8);
    uint32_t* d_ids = ctx->sm_ids.as<uint32_t>();
    HIPCHK(hipMemcpyAsync(d_ids, ids, (size_t)R * 4, hipMemcpyHostToDevice, s));
    TLookupArgs la{d_ids, R, ctx->order, ctx->dev_ids, ctx->ndocs, d_pos};
    if (launch_terms_lookup(la, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
    return TFIDF_OK;
}

/* the rows of a call from the resident result: positions (ids looked up, or every position),
 * vector ranges, norms, ids; copied to the host arrays (R entries each) */
static int sim_resident_rows(tfidf_ctx* ctx, const uint32_t* doc_ids, uint32_t R, SimCall& c, uint64_t* h_rb,
                             uint64_t* h_re, double* h_norm, uint32_t* h_pos, uint32_t* h_id) {
    hipStream_t s = ctx->stream;
    int rc = sim_layout(ctx, R, c);
    if (rc) return rc;
    if (!R) return TFIDF_OK;
    if (doc_ids) {
        rc = sim_lookup_ids(ctx, doc_ids, R, c.rpos);
        if (rc) return rc;
    }
    SimRowArgs ra{};
    ra.out_off = ctx->out_off.as<uint64_t>();
    ra.order = ctx->order;
    ra.doc_ids = ctx->dev_ids;
    ra.sq = ctx->sm_norm.as<double>();
    ra.norm = ra.sq + ctx->ndocs;
    ra.ndocs = ctx->ndocs;
    ra.npairs = ctx->npairs;
    ra.pos = doc_ids ? c.rpos : nullptr;   /* read and rewritten by the same thread */
    ra.nrows = R;
    ra.rb = c.rb;
    ra.re = c.re;
    ra.rnorm = c.rnorm;
    ra.rsq = c.rsq;
    ra.rpos = c.rpos;
    ra.rid = c.rid;
    if (launch_sim_rows(ra, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
    HIPCHK(hipMemcpyAsync(h_rb, c.rb, (size_t)R * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_re, c.re, (size_t)R * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_norm, c.rnorm, (size_t)R * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_pos, c.rpos, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_id, c.rid, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return TFIDF_OK;
}

/* the groups of a call: row i's vector is entries [h_rb[i], h_re[i]) of d_term / d_score
 * (nentries of them; terms >= V are words this shard does not hold).  Fills nmatch, nnb and
 * nb_* of `out`. */
static int similar_groups(tfidf_ctx* ctx, const SimCall& c, uint32_t k, const uint32_t* d_term, const double* d_score,
                          uint64_t nentries, const uint64_t* h_rb, const uint64_t* h_re, tfidf_neighbors* out,
                          tfidf_similar_info& si) {
    hipStream_t s = ctx->stream;
    const uint32_t N = ctx->ndocs, V = ctx->V, R = c.R;
    const TopkPlan plan = topk_plan(N, k, R, ctx->query_acc_bytes);
    const uint64_t G = plan.G;
    si.group_rows = (uint32_t)G;
    si.acc_bytes = G * plan.per_q;
    if (!N || !V || !R) return TFIDF_OK;
    uint64_t maxP = 0;   /* the largest group's postings */
    for (uint32_t g0 = 0; g0 < R; g0 += (uint32_t)G) {
        uint64_t pg = 0;
        for (uint32_t i = g0; i < R && i < g0 + G; ++i) pg += h_re[i] - h_rb[i];
        if (pg > maxP) maxP = pg;
    }
    if (maxP > 0x7FFFFFFFull) return TFIDF_E_CAPACITY;
    if (!maxP) return TFIDF_OK;   /* every row is empty */
    const int erc = topk_ensure(ctx, plan, N);
    if (erc) return erc;
    ENSURE(ctx->sm_mask, ((size_t)V + 2) * 8);
    ENSURE(ctx->sm_cnt, ((size_t)V + 2) * 4);
    ENSURE(ctx->sm_off, ((size_t)V + 2) * 4);
    ENSURE(ctx->sm_pw, (size_t)maxP * 8 + 16);
    ENSURE(ctx->sm_res, (size_t)G * k * 8 + 16);
    std::vector<uint64_t> h_s((size_t)G * k), h_nm(G);
    std::vector<uint32_t> h_id((size_t)G * k), h_sh((size_t)G * k), h_n(G);
    uint32_t* res_pos = ctx->sm_res.as<uint32_t>();
    uint32_t* res_sh = res_pos + (size_t)G * k;
    for (uint32_t g0 = 0; g0 < R; g0 += (uint32_t)G) {
        const uint32_t gn = R - g0 < G ? R - g0 : (uint32_t)G;
        uint64_t pg = 0;
        for (uint32_t i = g0; i < g0 + gn; ++i) pg += h_re[i] - h_rb[i];
        if (!pg) continue;   /* empty rows: no neighbours */
        ++si.ngroups;
        /* ---- the group's table ---- */
        SimTabArgs ta{};
        ta.term = d_term;
        ta.score = d_score;
        ta.rb = c.rb + g0;
        ta.re = c.re + g0;
        ta.nentries = nentries;
        ta.nrows = gn;
        ta.V = V;
        ta.mask = ctx->sm_mask.as<uint64_t>();
        ta.cnt = ctx->sm_cnt.as<uint32_t>();
        ta.post_off = ctx->sm_off.as<uint32_t>();
        ta.post_w = ctx->sm_pw.as<double>();
        ta.post_cap = (uint32_t)maxP;
        HIPCHK(hipEventRecord(ctx->ev_s[0], s));
        HIPCHK(hipMemsetAsync(ta.mask, 0, ((size_t)V + 1) * 8, s));
        if (launch_sim_mark(ta, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        ctx->arena.used = 0;   /* as format_prepare: nothing of the result lives in the arena */
        const int sc = scan_excl_u32(ta.cnt, ctx->sm_off.as<uint32_t>(), V, ctx->arena, s);
        if (sc) { if (sc != -2) HIPCHK(hipGetLastError()); return sc == -2 ? TFIDF_E_NOMEM : TFIDF_E_HIP; }
        if (launch_sim_fill(ta, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_s[1], s));
        /* ---- one scan of the pairs ---- */
        unsigned long long* d_nm = ctx->q_misc.as<unsigned long long>();
        HIPCHK(hipMemsetAsync(d_nm, 0, (size_t)G * 8, s));
        SimScoreArgs sa{};
        sa.out_off = ctx->out_off.as<uint64_t>();
        sa.out_term = ctx->out_term.as<uint32_t>();
        sa.out_score = ctx->out_score.as<double>();
        sa.ndocs = N;
        sa.npairs = ctx->npairs;
        sa.V = V;
        sa.mask = ta.mask;
        sa.post_off = ta.post_off;
        sa.post_w = ta.post_w;
        sa.post_cap = ta.post_cap;
        sa.nq = gn;
        sa.rnorm = c.rnorm + g0;
        sa.rpos = c.rpos + g0;
        sa.dnorm = ctx->sm_norm.as<double>() + N;
        sa.acc = ctx->q_acc.as<double>();
        sa.cnt = ctx->q_cnt.as<uint32_t>();
        sa.big_list = ctx->q_big.as<uint32_t>();
        sa.big_count = (uint32_t*)(d_nm + G);
        if (launch_sim_score(sa, ctx->ncu, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_s[2], s));
        /* ---- top-k rounds (tfidf_query's) ---- */
        TopkCand res{};
        int rc = topk_rounds(ctx, plan, sa.acc, sa.cnt, N, k, gn, d_nm, &res);
        if (rc) return rc;
        /* ---- the neighbours' positions and shared-term counts ---- */
        TLookupArgs la{res.id, gn * k, ctx->order, ctx->dev_ids, N, res_pos};
        if (launch_terms_lookup(la, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        if (launch_sim_shared(sa.cnt, res_pos, res.n, gn, k, N, res_sh, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_s[3], s));
        uint32_t nbig = 0;
        HIPCHK(hipMemcpyAsync(h_sh.data(), res_sh, (size_t)gn * k * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&nbig, sa.big_count, 4, hipMemcpyDeviceToHost, s));
        rc = topk_read_back(ctx, res, d_nm, gn, k, h_s.data(), h_id.data(), h_n.data(), h_nm.data());
        if (rc) return rc;
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ctx->ev_s[0], ctx->ev_s[1]);
        si.ms_table += ms;
        (void)hipEventElapsedTime(&ms, ctx->ev_s[1], ctx->ev_s[2]);
        si.ms_score += ms;
        (void)hipEventElapsedTime(&ms, ctx->ev_s[2], ctx->ev_s[3]);
        si.ms_topk += ms;
        si.big_docs = nbig < N ? nbig : N;
        for (uint32_t q = 0; q < gn; ++q) {
            const uint32_t n = h_n[q] < k ? h_n[q] : k;
            out->nnb[g0 + q] = n;
            out->nmatch[g0 + q] = h_nm[q];
            for (uint32_t i = 0; i < n; ++i) {
                const size_t o = (size_t)(g0 + q) * k + i, e = (size_t)q * k + i;
                out->nb_doc[o] = h_id[e];
                out->nb_shared[o] = h_sh[e];
                memcpy(&out->nb_score[o], &h_s[e], 8);
            }
        }
    }
    return TFIDF_OK;
}

extern "C" int tfidf_similar(tfidf_ctx* ctx, const uint32_t* doc_ids, uint32_t ndocs, uint32_t k, tfidf_neighbors* out) {
    if (!ctx || !out) return TFIDF_E_INVAL;
    if (k == 0 || k > TFIDF_SIMILAR_MAX_K) return TFIDF_E_INVAL;
    if (!ctx->have_result) return TFIDF_E_STATE;
    const auto wall0 = std::chrono::steady_clock::now();
    int rc = sim_begin(ctx);
    if (rc) return rc;
    const uint32_t R = doc_ids ? ndocs : ctx->ndocs;
    rc = neighbors_alloc(out, R, k);
    if (rc) return rc;
    NeighborsGuard guard{out};
    tfidf_similar_info si{};
    si.rows = R;
    si.k = k;
    rc = sim_norms(ctx, si);
    if (rc) return rc;
    SimCall c;
    std::vector<uint64_t> h_rb((size_t)R + 1), h_re((size_t)R + 1);
    std::vector<uint32_t> h_id((size_t)R + 1);
    rc = sim_resident_rows(ctx, doc_ids, R, c, h_rb.data(), h_re.data(), out->norm, out->pos, h_id.data());
    if (rc) return rc;
    for (uint32_t i = 0; i < R; ++i) {
        out->doc[i] = doc_ids ? doc_ids[i] : h_id[i];
        out->npairs[i] = h_re[i] - h_rb[i];
    }
    rc = similar_groups(ctx, c, k, ctx->out_term.as<uint32_t>(), ctx->out_score.as<double>(), ctx->npairs, h_rb.data(),
                        h_re.data(), out, si);
    if (rc) return rc;
    si.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    ctx->sinfo = si;
    guard.n = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_last_similar_info(const tfidf_ctx* ctx, tfidf_similar_info* info) {
    if (!ctx || !info || info->size < sizeof(uint64_t)) return TFIDF_E_INVAL;
    const uint64_t n = info->size < sizeof(tfidf_similar_info) ? info->size : sizeof(tfidf_similar_info);
    tfidf_similar_info o = ctx->sinfo;
    o.size = n;
    memcpy(info, &o, (size_t)n);
    return TFIDF_OK;
}

/* the rows' vectors as (word bytes, score): the word gather of tfidf_top_terms over every pair
 * of the rows' documents (short terms from their key, long terms from the corpus) */
int tfidf_ctx_similar_export(tfidf_ctx* ctx, const uint32_t* doc_ids, uint32_t ndocs, SimExport* e) {
    if (!ctx || !e) return TFIDF_E_INVAL;
    if (!ctx->have_result) return TFIDF_E_STATE;
    int rc = sim_begin(ctx);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    const uint32_t V = ctx->V;
    const uint32_t R = doc_ids ? ndocs : ctx->ndocs;
    tfidf_similar_info si{};
    rc = sim_norms(ctx, si);
    if (rc) return rc;
    if (V && !ctx->tmeta_valid) {
        ENSURE(ctx->t_key, (size_t)V * 16 + 16);
        ENSURE(ctx->t_len, (size_t)V * 4 + 4);
        if (launch_term_meta(ctx->vkeys.as<uint4>(), ctx->vrep.as<uint64_t>(), ctx->slot_of_rank.as<uint32_t>(), V,
                             ctx->t_key.as<uint4>(), ctx->t_len.as<uint32_t>(), s))
            return TFIDF_E_HIP;
        ctx->tmeta_valid = true;
    }
    SimCall c;
    std::vector<uint64_t> h_rb((size_t)R + 1), h_re((size_t)R + 1);
    e->id.assign((size_t)R + 1, 0);
    e->pos.assign((size_t)R + 1, 0);
    e->norm.assign((size_t)R + 1, 0.0);
    e->npairs.assign((size_t)R + 1, 0);
    e->voff.assign((size_t)R + 1, 0);
    rc = sim_resident_rows(ctx, doc_ids, R, c, h_rb.data(), h_re.data(), e->norm.data(), e->pos.data(), e->id.data());
    if (rc) return rc;
    for (uint32_t i = 0; i < R; ++i) {
        if (doc_ids) e->id[i] = doc_ids[i];
        e->npairs[i] = h_re[i] - h_rb[i];
        e->voff[i + 1] = e->voff[i] + e->npairs[i];
    }
    const uint64_t P = e->voff[R];
    e->woff.assign((size_t)P + 1, 0);
    e->score.assign((size_t)P + 1, 0.0);
    e->wbytes.clear();
    if (!P) return TFIDF_OK;
    ENSURE(ctx->sm_xoff, ((size_t)R + 1) * 8);
    ENSURE(ctx->sm_xterm, (size_t)P * 4 + 16);
    ENSURE(ctx->sm_xscore, (size_t)P * 8 + 16);
    ENSURE(ctx->sm_xwoff, (size_t)P * 8 + 16);
    HIPCHK(hipMemcpyAsync(ctx->sm_xoff.p, e->voff.data(), ((size_t)R + 1) * 8, hipMemcpyHostToDevice, s));
    SimExportArgs xa{};
    xa.out_term = ctx->out_term.as<uint32_t>();
    xa.out_score = ctx->out_score.as<double>();
    xa.tlen = ctx->t_len.as<uint32_t>();
    xa.V = V;
    xa.rb = c.rb;
    xa.re = c.re;
    xa.eoff = ctx->sm_xoff.as<uint64_t>();
    xa.nrows = R;
    xa.term = ctx->sm_xterm.as<uint32_t>();
    xa.score = ctx->sm_xscore.as<double>();
    xa.wlen = ctx->sm_xwoff.as<uint64_t>();
    if (launch_sim_export(xa, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
    ctx->arena.used = 0;
    const int sc = scan_excl_u64(xa.wlen, xa.wlen, P, ctx->arena, s);   /* lengths -> offsets, in place */
    if (sc) { if (sc != -2) HIPCHK(hipGetLastError()); return sc == -2 ? TFIDF_E_NOMEM : TFIDF_E_HIP; }
    HIPCHK(hipMemcpyAsync(e->woff.data(), xa.wlen, ((size_t)P + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(e->score.data(), xa.score, (size_t)P * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const uint64_t wtotal = e->woff[P];
    e->wbytes.assign((size_t)wtotal + 1, 0);
    ENSURE(ctx->sm_xwords, (size_t)wtotal + 16);
    TWordArgs wa{xa.term, xa.wlen, P, ctx->t_key.as<uint4>(), V, ctx->dev_bytes, ctx->corpus.nbytes,
                 ctx->sm_xwords.as<uint8_t>()};
    if (launch_terms_words(wa, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
    if (wtotal) HIPCHK(hipMemcpyAsync(e->wbytes.data(), ctx->sm_xwords.p, (size_t)wtotal, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return TFIDF_OK;
}

int tfidf_ctx_similar_ext(tfidf_ctx* ctx, const SimExport* rows, uint32_t k, tfidf_neighbors* out) {
    if (!ctx || !rows || !out) return TFIDF_E_INVAL;
    if (k == 0 || k > TFIDF_SIMILAR_MAX_K || rows->voff.empty()) return TFIDF_E_INVAL;
    if (!ctx->have_result) return TFIDF_E_STATE;
    const auto wall0 = std::chrono::steady_clock::now();
    int rc = sim_begin(ctx);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    const uint32_t R = (uint32_t)(rows->voff.size() - 1);
    const uint64_t P = rows->voff[R];
    if (rows->id.size() < R || rows->norm.size() < R || rows->woff.size() < P + 1 || rows->score.size() < P ||
        rows->wbytes.size() < rows->woff[P])
        return TFIDF_E_INVAL;
    if (P > 0xFFFFFFFFull) return TFIDF_E_CAPACITY;   /* one lookup lane per exported word */
    rc = neighbors_alloc(out, R, k);
    if (rc) return rc;
    NeighborsGuard guard{out};
    tfidf_similar_info si{};
    si.rows = R;
    si.k = k;
    rc = sim_norms(ctx, si);
    if (rc) return rc;
    SimCall c;
    rc = sim_layout(ctx, R, c);
    if (rc) return rc;
    for (uint32_t i = 0; i < R; ++i) out->doc[i] = rows->id[i];
    if (R && P && ctx->ndocs && ctx->V) {
        /* the rows' own documents by id (another shard's: no position here) */
        rc = sim_lookup_ids(ctx, rows->id.data(), R, c.rpos);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(c.rb, rows->voff.data(), (size_t)R * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(c.re, rows->voff.data() + 1, (size_t)R * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(c.rnorm, rows->norm.data(), (size_t)R * 8, hipMemcpyHostToDevice, s));
        /* the words -> this shard's term ranks (k_query_lookup; QUERY_NO_TERM: not in its vocabulary) */
        const size_t offb = ((size_t)P + 1) * 8;
        const uint64_t wtotal = rows->woff[P];
        ENSURE(ctx->q_terms, offb + wtotal + 16);
        ENSURE(ctx->q_rank, (size_t)P * 4 + 4);
        ENSURE(ctx->sm_escore, (size_t)P * 8 + 16);
        HIPCHK(hipMemcpyAsync(ctx->q_terms.p, rows->woff.data(), offb, hipMemcpyHostToDevice, s));
        if (wtotal)
            HIPCHK(hipMemcpyAsync(ctx->q_terms.as<uint8_t>() + offb, rows->wbytes.data(), wtotal, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(ctx->sm_escore.p, rows->score.data(), (size_t)P * 8, hipMemcpyHostToDevice, s));
        QLookupArgs la{};
        la.tbytes = ctx->q_terms.as<uint8_t>() + offb;
        la.toff = ctx->q_terms.as<uint64_t>();
        la.nterms = (uint32_t)P;
        la.vkeys = ctx->vkeys.as<uint4>();
        la.vrep = ctx->vrep.as<uint64_t>();
        la.mask = ctx->vcap - 1;
        la.home = ~1ull;
        la.rank_of_slot = ctx->rank_of_slot.as<uint32_t>();
        la.corpus = ctx->dev_bytes;
        la.corpus_bytes = ctx->corpus.nbytes;
        la.V = ctx->V;
        la.rank_out = ctx->q_rank.as<uint32_t>();
        if (launch_query_lookup(la, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipStreamSynchronize(s));   /* the host arrays are the caller's */
        rc = similar_groups(ctx, c, k, ctx->q_rank.as<uint32_t>(), ctx->sm_escore.as<double>(), P, rows->voff.data(),
                            rows->voff.data() + 1, out, si);
        if (rc) return rc;
    }
    si.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    ctx->sinfo = si;
    guard.n = nullptr;
    return TFIDF_OK;
}

/* ---------------------------------------------------------------- clusters ----
 * Spherical k-means over the resident result (kmeans.hip).  The norms are tfidf_similar's.  The
 * host validates the seeds against the documents' ids and norms (copied once), then loops over
 * the passes: an assignment, a 4-byte copy of the changed-label count, and unless the loop
 * stops an update.  Labels, sims and sizes come to the host once, after the last pass; the
 * matrix never does: the clusters' top terms are selected on the device and their words
 * gathered by the keyword path's k_terms_words.  Nothing of the run's result is written. */

extern "C" void tfidf_clusters_free(tfidf_clusters* c) {
    if (!c) return;
    free(c->doc); free(c->label); free(c->sim); free(c->size); free(c->seed); free(c->nterms); free(c->term);
    free(c->weight); free(c->word_off); free(c->word_bytes);
    memset(c, 0, sizeof(*c));
}

extern "C" int tfidf_kmeans(tfidf_ctx* ctx, const tfidf_kmeans_params* params, tfidf_clusters* out) {
    if (!ctx || !params || !out) return TFIDF_E_INVAL;
    if (params->size < sizeof(tfidf_kmeans_params)) return TFIDF_E_INVAL;
    const uint32_t K = params->k, T = params->nterms;
    const uint32_t max_iter = params->max_iter ? params->max_iter : TFIDF_KMEANS_DEFAULT_ITER;
    if (K == 0 || K > TFIDF_KMEANS_MAX_K || T > TFIDF_KMEANS_MAX_TERMS) return TFIDF_E_INVAL;
    if (params->seeds && params->nseeds != K) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!ctx->have_result) return TFIDF_E_STATE;
    const uint32_t N = ctx->ndocs, V = ctx->V;
    const uint64_t matrix = (uint64_t)K * V * 8;
    const uint64_t work = (uint64_t)N * 24 + (uint64_t)K * 24 + 64;
    if (matrix + work > ctx->kmeans_bytes) return TFIDF_E_CAPACITY;
    const auto wall0 = std::chrono::steady_clock::now();
    int rc = sim_begin(ctx);
    if (rc) return rc;
    for (hipEvent_t& e : ctx->ev_k)
        if (!e) HIPCHK(hipEventCreate(&e));
    hipStream_t s = ctx->stream;
    tfidf_kmeans_info ki{};
    ki.ndocs = N;
    ki.k = K;
    ki.matrix_bytes = matrix;
    ki.work_bytes = work;
    tfidf_similar_info si{};
    rc = sim_norms(ctx, si);
    if (rc) return rc;
    ki.ms_norms = si.ms_norms;
    ENSURE(ctx->km_work, work);
    ENSURE(ctx->km_C, matrix + 64);

    KmArgs a{};
    a.out_off = ctx->out_off.as<uint64_t>();
    a.out_term = ctx->out_term.as<uint32_t>();
    a.out_score = ctx->out_score.as<double>();
    a.norm = ctx->sm_norm.as<double>() + N;
    a.ndocs = N;
    a.npairs = ctx->npairs;
    a.V = V;
    a.K = K;
    a.C = ctx->km_C.as<double>();
    a.sim = ctx->km_work.as<double>();
    a.cnorm = a.sim + N;
    uint32_t* d_ids = (uint32_t*)(a.cnorm + K);
    uint32_t* d_lab[2] = {d_ids + N, d_ids + 2 * (size_t)N};
    a.members = d_ids + 3 * (size_t)N;
    a.size = a.members + N;
    a.moff = a.size + K;
    uint32_t* d_seedpos = a.moff + K + 1;
    a.seedpos = d_seedpos;
    a.changed = d_seedpos + K;

    /* ---- ids and norms by output position: the seeds are checked on the host ---- */
    std::vector<uint32_t> h_id((size_t)N + 1);
    std::vector<double> h_norm((size_t)N + 1);
    if (N) {
        if (launch_km_docs(ctx->order, ctx->dev_ids, N, d_ids, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipMemcpyAsync(h_id.data(), d_ids, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_norm.data(), a.norm, (size_t)N * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    std::vector<uint32_t> clus;   /* the clusterable positions, ascending */
    for (uint32_t j = 0; j < N; ++j)
        if (h_norm[j] > 0.0) clus.push_back(j);
    const uint64_t M = clus.size();
    ki.clusterable = (uint32_t)M;
    if (K > M) return TFIDF_E_INVAL;
    std::vector<uint32_t> h_seedpos(K), h_seed(K);
    if (params->seeds) {
        std::unordered_map<uint32_t, uint32_t> pos_of;
        pos_of.reserve((size_t)N * 2);
        for (uint32_t j = 0; j < N; ++j) pos_of.emplace(h_id[j], j);
        std::unordered_map<uint32_t, int> seen;
        for (uint32_t c = 0; c < K; ++c) {
            const uint32_t id = params->seeds[c];
            const auto it = pos_of.find(id);
            if (it == pos_of.end() || !(h_norm[it->second] > 0.0) || !seen.emplace(id, 1).second) return TFIDF_E_INVAL;
            h_seedpos[c] = it->second;
            h_seed[c] = id;
        }
    } else {
        for (uint32_t c = 0; c < K; ++c) {
            h_seedpos[c] = clus[(size_t)((uint64_t)c * M / K)];
            h_seed[c] = h_id[h_seedpos[c]];
        }
    }

    const size_t KT = (size_t)K * T;
    out->ndocs = N;
    out->k = K;
    out->t = T;
    out->doc = (uint32_t*)calloc((size_t)N + 1, 4);
    out->label = (uint32_t*)calloc((size_t)N + 1, 4);
    out->sim = (double*)calloc((size_t)N + 1, 8);
    out->size = (uint32_t*)calloc((size_t)K + 1, 4);
    out->seed = (uint32_t*)calloc((size_t)K + 1, 4);
    out->nterms = (uint32_t*)calloc((size_t)K + 1, 4);
    out->term = (uint32_t*)calloc(KT + 1, 4);
    out->weight = (double*)calloc(KT + 1, 8);
    out->word_off = (uint64_t*)calloc(KT + 1, 8);
    out->word_bytes = (uint8_t*)calloc(1, 1);
    struct ClustersGuard {   /* an error return leaves *out zeroed */
        tfidf_clusters* c;
        ~ClustersGuard() { if (c) tfidf_clusters_free(c); }
    } guard{out};
    if (!out->doc || !out->label || !out->sim || !out->size || !out->seed || !out->nterms || !out->term || !out->weight ||
        !out->word_off || !out->word_bytes)
        return TFIDF_E_NOMEM;
    memcpy(out->doc, h_id.data(), (size_t)N * 4);
    memcpy(out->seed, h_seed.data(), (size_t)K * 4);

    /* ---- centroid 0 ---- */
    HIPCHK(hipMemcpyAsync(d_seedpos, h_seedpos.data(), (size_t)K * 4, hipMemcpyHostToDevice, s));
    if (launch_km_seed(a, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }

    /* ---- the passes ---- */
    uint32_t split = ctx->kmeans_split;
    if (!split) {
        split = (2u * ctx->ncu + K - 1) / K;
        split = split < 1u ? 1u : (split > 64u ? 64u : split);
    }
    ki.split = split;
    float ms = 0;
    int cur = 0;
    bool update_pending = false;
    for (uint32_t it = 1; it <= max_iter; ++it) {
        a.label = d_lab[cur];
        a.prev = it > 1 ? d_lab[cur ^ 1] : nullptr;
        uint32_t changed = 0;
        HIPCHK(hipEventRecord(ctx->ev_k[0], s));
        if (launch_km_assign(a, ctx->ncu, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_k[1], s));
        HIPCHK(hipMemcpyAsync(&changed, a.changed, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        (void)hipEventElapsedTime(&ms, ctx->ev_k[0], ctx->ev_k[1]);
        ki.ms_assign += ms;
        if (update_pending) {
            (void)hipEventElapsedTime(&ms, ctx->ev_k[2], ctx->ev_k[3]);
            ki.ms_update += ms;
            update_pending = false;
        }
        ki.passes = it;
        if (it > 1 && changed == 0) { out->converged = 1; break; }
        if (it == max_iter) break;
        HIPCHK(hipEventRecord(ctx->ev_k[2], s));
        if (launch_km_update(a, split, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_k[3], s));
        ++ki.updates;
        update_pending = true;
        cur ^= 1;
    }
    out->iterations = ki.passes;
    if (N) {
        HIPCHK(hipMemcpyAsync(out->label, a.label, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->sim, a.sim, (size_t)N * 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipMemcpyAsync(out->size, a.size, (size_t)K * 4, hipMemcpyDeviceToHost, s));

    /* ---- the clusters' best terms and their words ---- */
    if (T) {
        if (V && !ctx->tmeta_valid) {
            ENSURE(ctx->t_key, (size_t)V * 16 + 16);
            ENSURE(ctx->t_len, (size_t)V * 4 + 4);
            if (launch_term_meta(ctx->vkeys.as<uint4>(), ctx->vrep.as<uint64_t>(), ctx->slot_of_rank.as<uint32_t>(), V,
                                 ctx->t_key.as<uint4>(), ctx->t_len.as<uint32_t>(), s))
                return TFIDF_E_HIP;
            ctx->tmeta_valid = true;
        }
        ENSURE(ctx->km_top, (size_t)K * KM_TOP_SLICES * 16 + (size_t)K * 16 + KT * 8 + (KT + 1) * 8 + KT * 4 + (size_t)K * 4 + 64);
        KmTopArgs ta{};
        ta.C = a.C;
        ta.V = V;
        ta.K = K;
        ta.T = T;
        ta.tlen = ctx->t_len.as<uint32_t>();
        ta.part = ctx->km_top.as<uint64_t>();
        ta.prev = ta.part + (size_t)K * KM_TOP_SLICES * 2;
        ta.weight = ta.prev + (size_t)K * 2;
        ta.wlen = ta.weight + KT;
        ta.term = (uint32_t*)(ta.wlen + KT + 1);
        ta.n = ta.term + KT;
        HIPCHK(hipEventRecord(ctx->ev_k[0], s));
        if (launch_km_top(ta, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        ctx->arena.used = 0;   /* as tfidf_top_terms: nothing of the result lives in the arena */
        const int sc = scan_excl_u64(ta.wlen, ta.wlen, KT, ctx->arena, s);   /* lengths -> offsets, in place */
        if (sc) { if (sc != -2) HIPCHK(hipGetLastError()); return sc == -2 ? TFIDF_E_NOMEM : TFIDF_E_HIP; }
        HIPCHK(hipMemcpyAsync(out->word_off, ta.wlen, (KT + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const uint64_t wtotal = out->word_off[KT];
        ENSURE(ctx->km_words, wtotal + 16);
        TWordArgs wa{ta.term, ta.wlen, KT, ctx->t_key.as<uint4>(), V, ctx->dev_bytes, ctx->corpus.nbytes,
                     ctx->km_words.as<uint8_t>()};
        if (launch_terms_words(wa, s)) { HIPCHK(hipGetLastError()); return TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_k[1], s));
        uint8_t* wb = (uint8_t*)realloc(out->word_bytes, (size_t)wtotal + 1);
        if (!wb) return TFIDF_E_NOMEM;
        out->word_bytes = wb;
        HIPCHK(hipMemcpyAsync(out->term, ta.term, KT * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->weight, ta.weight, KT * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->nterms, ta.n, (size_t)K * 4, hipMemcpyDeviceToHost, s));
        if (wtotal) HIPCHK(hipMemcpyAsync(wb, ctx->km_words.p, wtotal, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        (void)hipEventElapsedTime(&ms, ctx->ev_k[0], ctx->ev_k[1]);
        ki.ms_terms = ms;
    } else {
        HIPCHK(hipStreamSynchronize(s));
    }
    ki.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    ctx->kinfo = ki;
    guard.c = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_last_kmeans_info(const tfidf_ctx* ctx, tfidf_kmeans_info* info) {
    if (!ctx || !info || info->size < sizeof(uint64_t)) return TFIDF_E_INVAL;
    const uint64_t n = info->size < sizeof(tfidf_kmeans_info) ? info->size : sizeof(tfidf_kmeans_info);
    tfidf_kmeans_info o = ctx->kinfo;
    o.size = n;
    memcpy(info, &o, (size_t)n);
    return TFIDF_OK;
}
