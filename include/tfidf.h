/*
 * tfidf.h — C-ABI of the MI355X-native TF-IDF engine (libtfidf_hip.so).
 *
 * The reference (ndas7/Parallel-Systems-MPI-TFIDF, TFIDF.c) has no library API: the
 * whole path is one monolithic main() (TFIDF.c:52-287) whose seams are
 *   ingest      input/docN bytes            TFIDF.c:98-110, 130-147
 *   count       wordCount / docSize / df    TFIDF.c:141-196, 291-326
 *   score       tf * log(N/df)              TFIDF.c:202, 243-244
 *   emit        "docN@word\t%.16f", qsort   TFIDF.c:245, 273-282
 * Every entry point below names the reference lines it replaces.  Plain C types only:
 * pointers + sizes, no torch or HIP types.  Every function returns 0 or a negative
 * TFIDF_E* code (never exit()s, unlike TFIDF.c:102,122,137,277).  A context is used
 * by one host thread at a time.
 */
#ifndef TFIDF_H
#define TFIDF_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: tfidf_run_info starts with its own size (set by the caller), the experimental K1 run
 *    flags are gone */
#define TFIDF_ABI_VERSION 2

enum tfidf_status {
    TFIDF_OK = 0,
    TFIDF_E_INVAL = -1,     /* bad argument */
    TFIDF_E_NOMEM = -2,     /* host or device allocation failed */
    TFIDF_E_HIP = -3,       /* HIP runtime error */
    TFIDF_E_RCCL = -4,      /* RCCL error */
    TFIDF_E_NODEV = -5,     /* no usable gfx950 device */
    TFIDF_E_NOINPUT = -6,   /* ./input cannot be opened        (TFIDF.c:100-103) */
    TFIDF_E_NODOC = -7,     /* input/docN cannot be opened     (TFIDF.c:134-138) */
    TFIDF_E_OUTPUT = -8,    /* output.txt cannot be written    (TFIDF.c:274-278) */
    TFIDF_E_CAPACITY = -9,  /* an internal table could not be grown, or a term (a token's bytes
                               up to its first NUL) is 16 MiB or longer: its offset/length
                               word holds 24 length bits, or two distinct terms of 16 bytes or
                               more share their 120-bit identity key (compared byte by byte on
                               every key match: reported, never merged) */
    TFIDF_E_STATE = -10,    /* call out of order (e.g. fetch before run) */
    TFIDF_E_PEER = -11,     /* another rank of the DF exchange failed (this rank did not) */
    TFIDF_E_MODEL = -12     /* a model file cannot be read or does not hold a valid model */
};

/* ---------------------------------------------------------------- corpus ---- */

#define TFIDF_CORPUS_DEVICE 1u   /* bytes/doc_off/doc_ids are device pointers on the ctx's GPU */

/* One shard of documents.  Replaces the reference's per-rank fopen/fscanf ingest
 * (TFIDF.c:130-147): document i (0-based, local) is bytes[doc_off[i], doc_off[i+1]).
 * Document boundaries are token boundaries.  Tokens follow fscanf("%s") in the C
 * locale: maximal runs of bytes not in {0x20,0x09..0x0D}; a term is the token's bytes
 * up to its first NUL (strcmp semantics, TFIDF.c:152,172).
 * The documents are a window of the buffer: doc_off[0] may be greater than 0 and
 * doc_off[ndocs] less than nbytes.  Bytes outside [doc_off[0], doc_off[ndocs]) belong
 * to no document and never join a token, whatever they hold (several shards may pass
 * the same bytes / nbytes with doc_off pointing into one shared offsets array).
 * A device `bytes` pointer (TFIDF_CORPUS_DEVICE) of any alignment is accepted; one
 * that is not 16-byte aligned is tokenised by the general kernel (TFIDF_RUN_K1_VS
 * clear in tfidf_run_info.flags), the result is the same. */
typedef struct tfidf_corpus {
    const uint8_t*  bytes;
    uint64_t        nbytes;
    const uint64_t* doc_off;      /* ndocs + 1 entries, non-decreasing, doc_off[ndocs] <= nbytes */
    const uint32_t* doc_ids;      /* global 1-based ids ("docN"); NULL means 1..ndocs */
    uint32_t        ndocs;        /* documents in this shard */
    uint32_t        flags;        /* TFIDF_CORPUS_* */
    uint64_t        ndocs_total;  /* N of log(N/df) (TFIDF.c:98-115,243); 0 means ndocs */
} tfidf_corpus;

/* ---------------------------------------------------------------- result ---- */

/* Host-side result, pairs in output order: the strcmp order of the reference's
 * "docN@word\t%.16f" lines (TFIDF.c:245,273).  Arrays are owned by the library and
 * released by tfidf_result_free(). */
typedef struct tfidf_result {
    uint64_t  npairs;       /* unique (doc, term) pairs in this shard = output lines */
    uint32_t  ndocs;        /* documents in this shard */
    uint32_t  nterms;       /* distinct terms in this shard */
    uint64_t  ndocs_total;  /* N used for idf */
    /* per pair (output order) */
    uint32_t* pair_doc;     /* global doc id (TFIDF.c:132 "doc%d") */
    uint32_t* pair_term;    /* index into the term table below */
    uint32_t* pair_count;   /* wordCount     (TFIDF.c:154,163) */
    uint32_t* pair_docsize; /* docSize       (TFIDF.c:141-143) */
    uint32_t* pair_df;      /* numDocsWithWord over ALL shards (TFIDF.c:169-188,215-234) */
    double*   pair_score;   /* tf * log(N/df) (TFIDF.c:202,243-244) */
    /* per local document, input order */
    uint32_t* doc_id;
    uint32_t* doc_size;
    /* term table: this shard's terms in strcmp("word\t") order */
    uint64_t* term_off;     /* nterms + 1 */
    uint8_t*  term_bytes;
    uint32_t* term_df;      /* global df of each term */
} tfidf_result;

/* ---------------------------------------------------------------- context --- */

typedef struct tfidf_ctx tfidf_ctx;

/* Opens device `device` (HIP ordinal).  Fails with TFIDF_E_NODEV unless it is gfx950. */
int tfidf_open(int device, tfidf_ctx** out);
/* Number of visible HIP devices (0 when there is none). */
int tfidf_device_count(void);
void tfidf_close(tfidf_ctx* ctx);
const char* tfidf_strerror(int status);
int tfidf_abi_version(void);

/* ---- multi-GPU: one process per GPU; replaces MPI_Init/Comm_size/Comm_rank
 *      (TFIDF.c:82,91-92) and the DF combine MPI_Reduce(CustomReduce)+MPI_Bcast
 *      (TFIDF.c:209-222,291-326) with RCCL collectives over xGMI, in one of two forms
 *      chosen alike by every rank from the agreed per-rank term counts:
 *        dense (every rank's V <= 2^17, the default for c2/c3/c5-size shards): the ranks'
 *          term keys are all-gathered, numbered identically on every rank, and ONE
 *          ncclAllReduce (sum) of a u32 df vector over those numbers gives the global df;
 *        hash-owner (larger V, e.g. 10^7 terms): each term's df is summed by an owner rank
 *          (a hash of the term) after an all-to-all of (term, df) and returned by a second
 *          all-to-all (grouped ncclSend / ncclRecv).
 *      TFIDF_XCHG=dense|owner|dense_table forces a form. */
#define TFIDF_UNIQUE_ID_BYTES 128
int tfidf_comm_unique_id(uint8_t id[TFIDF_UNIQUE_ID_BYTES]);
/* Attaches an RCCL communicator rank (ncclCommInitRankConfig).  From then on every tfidf_run
 * of this context is collective: all ranks call it, each on its own shard (contiguous
 * ranges of the "docN@" order, ndocs_total = N of the whole corpus).  Capacity retries
 * are agreed between the ranks (all repeat or none does); a rank whose run fails makes
 * the others return TFIDF_E_PEER instead of waiting.
 * Abort contract: the communicator is created non-blocking (a peer that never joins makes
 * this call return TFIDF_E_PEER after TFIDF_COMM_TIMEOUT_S seconds, default 600, 0 = no
 * limit), and every RCCL call and every wait for a collective's kernels is polled.  A
 * failure agreed before the exchange's collectives (a local error, a capacity retry) needs
 * nothing from the caller.  A rank-local failure AFTER the agreement aborts this rank's
 * communicator; a peer process waiting for it gives up at the same deadline (or when RCCL
 * reports the peer's failure) and aborts its own.  A context whose communicator was aborted
 * returns TFIDF_E_PEER from then on: close and reopen it. */
int tfidf_comm_init(tfidf_ctx* ctx, const uint8_t id[TFIDF_UNIQUE_ID_BYTES], int rank, int nranks);   /* nranks <= 1024 */

/* ---- one process, several shards: the drop-in for `mpirun -np P ./TFIDF`
 *      (TFIDF.c:82-92 process group, :125-130 document -> rank assignment, :253-273
 *      gather + sort).  Rank r runs on devices[r] (NULL: device r).  When every rank has
 *      its own GPU the ranks are one RCCL clique (non-blocking communicators created in one
 *      ncclGroupStart/End); when a device is listed more than once (or TFIDF_GROUP_LOCAL is
 *      set) they exchange through device copies in this process — same engine code, same
 *      results.  An error on one rank inside the exchange sets the clique's abort flag: every
 *      rank, wherever it waits (inside an RCCL call, for a collective's kernels, or at its
 *      next call), aborts its own communicator at its next poll, so no peer stays blocked; the
 *      other ranks return TFIDF_E_PEER.  An RCCL group is unusable after such an abort (close
 *      and reopen it); an in-process group starts its next tfidf_group_run afresh. */
#define TFIDF_GROUP_LOCAL 1u
typedef struct tfidf_group tfidf_group;
int tfidf_group_open(int nranks, const int* devices, uint32_t flags, tfidf_group** out);
int tfidf_group_size(const tfidf_group* g);
tfidf_ctx* tfidf_group_ctx(tfidf_group* g, int rank);
/* tfidf_run on every rank at once (one host thread per rank); shards[nranks].  Returns
 * the lowest rank's own error, else TFIDF_E_PEER, else 0. */
int tfidf_group_run(tfidf_group* g, const tfidf_corpus* shards);
/* every rank formats its lines on its GPU, then output.txt = the texts in rank order */
int tfidf_group_write_output(tfidf_group* g, const char* path);
void tfidf_group_close(tfidf_group* g);

/* Runs the whole hot path on this shard: tokenize -> per-document TF counts ->
 * vocabulary -> DF (all-reduced across ranks when a communicator is attached) ->
 * tf*log(N/df) -> output order.  Replaces TFIDF.c:130-273.  Results stay in HBM
 * until tfidf_fetch().  Host-pointer corpora are copied to HBM first. */
int tfidf_run(tfidf_ctx* ctx, const tfidf_corpus* corpus);

/* Copies the last run's results to host memory. */
int tfidf_fetch(tfidf_ctx* ctx, tfidf_result* out);
void tfidf_result_free(tfidf_result* r);

/* Counters of the last run (sizes, for roofline accounting).  The caller sets `size` to
 * sizeof(tfidf_run_info) as it was compiled; the library writes no byte past it (a
 * caller built against an older, shorter struct gets its prefix), and sets `size` to the
 * bytes it wrote.  TFIDF_E_INVAL when size < 16. */
typedef struct tfidf_run_info {
    uint64_t size;            /* in: sizeof(tfidf_run_info) of the caller; out: bytes written */
    uint64_t nbytes;          /* C */
    uint64_t ntokens;         /* T */
    uint64_t npairs;          /* P */
    uint32_t nterms;          /* V (this shard) */
    uint32_t nterms_global;   /* V over all ranks */
    uint64_t nchunks;         /* tokenize+count work units */
    uint64_t partial_records; /* (doc, term) records of documents split across work units */
    uint32_t ndocs;
    uint32_t vocab_capacity;
    double   ms_total;        /* device time of the whole run (HIP events) */
    double   ms_tokcount;     /* device time of the tokenize+count kernels (HIP events) */
    double   ms_stage[16];    /* per-stage device times, see tfidf_stage_name() */
    uint32_t nstages;
    uint32_t flags;           /* TFIDF_RUN_* */
    /* device (re)allocations made by this library in this process since it was loaded
     * (hipMalloc of the engine's buffers, cumulative, all contexts): a caller timing
     * steady-state runs reads them before and after and expects no change */
    uint64_t device_allocs;
    uint64_t device_alloc_bytes;
    /* the run's idf table, log(N/df) on the host's libm (TFIDF.c:243): up to 2^18 documents
     * every df = 1..N is tabulated by the context's host worker threads while the device runs
     * the stages before the score; beyond that only the run's distinct df values, after the DF
     * stage (one host round trip) */
    uint64_t idf_logs;        /* libm log() calls made for this run's table (every run builds its own) */
    double   ms_idf_host;     /* wall time of those calls (host threads) */
    double   ms_idf_wait;     /* time the run waited for them before the score stage */
    /* the grid of the run's last tokenize+count launch: min(nchunks, CUs x 4) persistent
     * workgroups (CUs: tfidf_grid_cus), nchunks for the general kernel, 0 when none was
     * launched (an empty corpus) */
    uint32_t k1_workgroups;
    uint32_t reserved2;
} tfidf_run_info;
#define TFIDF_RUN_K1_VS   2u  /* slot-keyed tokenize+count kernel (the default path; the general
                                 kernel of TFIDF_K1=general or an unaligned corpus leaves it clear) */
#define TFIDF_RUN_K1_ST   4u  /* retired: round 3's k_tokcount_st (removed in round 5), never set */
#define TFIDF_RUN_K1_SL   8u  /* ... run as k_tokcount_sl (the default, vocabulary table <= 32M slots);
                                 neither ST nor SL with VS set: k_tokcount_vs (larger tables) */
#define TFIDF_RUN_REC_PACK 32u  /* K1 emitted packed records: one word (count, slot) per complete
                                   document's record (k_tokcount_sl, table <= 4M slots, env TFIDF_REC_PACK
                                   not 0) */
#define TFIDF_RUN_REC_PACK_KEPT 64u  /* ... and they stayed one word through DF and the score kernels
                                        (V <= 65536, ranks no wider than the slot field); clear: unpacked
                                        after K1 */
#define TFIDF_RUN_XCHG_DENSE 16u  /* multi-rank: the DF exchange used the dense all-reduce form
                                     (else the hash-owner all-to-all; single rank: no exchange) */
int tfidf_last_run_info(tfidf_ctx* ctx, tfidf_run_info* info);
/* Sums over the successful runs since the last reset (a caller timing many runs reads them
 * once instead of querying every run): runs, K1 ms, whole-run ms (HIP events: 0 while
 * timing is off), idf logs, idf host ms, idf wait ms.  reset != 0 zeroes them after the read. */
typedef struct tfidf_run_totals {
    uint64_t runs;
    double ms_tokcount, ms_total;
    uint64_t idf_logs;
    double ms_idf_host, ms_idf_wait;
} tfidf_run_totals;
int tfidf_run_totals_get(tfidf_ctx* ctx, tfidf_run_totals* out, int reset);
/* The same device-allocation counters without a run (process-wide, cumulative). */
int tfidf_alloc_stats(uint64_t* allocs, uint64_t* bytes);
/* The engine's device allocations that are still held: allocations minus frees, and their bytes
 * (process-wide).  Equal before tfidf_open and after tfidf_close of every context and group: a
 * closed context leaves no device memory behind. */
int tfidf_alloc_live(uint64_t* allocs, uint64_t* bytes);
/* The CU count the context sizes its launches over the resident result by (tfidf_query,
 * _query_bm25, _top_terms, _similar, _kmeans, _prune, _reweight, _transform's row norm, _minhash,
 * _near_dups; tfidf_analyze's tile kernel too): each takes min(work, CUs x a per-kernel constant)
 * workgroups that stride over the work.  The device's count, or env TFIDF_GRID_CUS (1..4096,
 * read at tfidf_open; anything else: the device's), which exists so that tests reach the second
 * and later trips of those loops on a small corpus.  No result depends on it.  The run's own
 * persistent kernels follow it as well: the tokenize+count kernels (CUs x 4 workgroups that claim
 * chunks; tfidf_run_info.k1_workgroups reports the grid), the score stage, and the formatter
 * behind tfidf_format / tfidf_write_output_gpu (CUs x 8 workgroups, a wave per document).
 * TFIDF_E_INVAL: a NULL argument. */
int tfidf_grid_cus(tfidf_ctx* ctx, uint32_t* ncu);
const char* tfidf_stage_name(int stage);
/* HIP event timing of a run's stages (tfidf_run_info.ms_stage / ms_tokcount / ms_total):
 * enable 0 none, 1 every stage (the default; ten event records per run), 2 the tokenize+count
 * kernel and the whole run only (four records; each record costs the stream ~5 us). */
int tfidf_set_timing(tfidf_ctx* ctx, int enable);
/* Diagnostics: per-phase cycle sums of the fast tokenize+count kernel, available only
 * from the diagnostic build lib/libtfidf_hip_stamps.so with TFIDF_STAMPS=1 set before
 * tfidf_open.  Returns the number of values written (phases + workgroup count). */
int tfidf_debug_k1_stamps(tfidf_ctx* ctx, uint64_t* out, int n);

/* Diagnostics: measured HBM streaming peaks on this device (SURVEY §8d's "fraction of a
 * measured copy-kernel peak"): GB/s of a read-only stream over nbytes and of an nbytes
 * copy (2 x nbytes moved), each averaged over `iters` passes after a warm-up. */
int tfidf_hbm_probe(tfidf_ctx* ctx, uint64_t nbytes, int iters, double* read_gbps, double* copy_gbps);

/* ---------------------------------------------------------------- emission -- */

/* GPU emission (the default output path): formats the last run's lines
 * "docN@word\t%.16f\n" (TFIDF.c:245,281) in output order into one text in HBM.  %.16f
 * is computed exactly (integer significand x 10^16, 128-bit, ties to even: glibc
 * printf's result).  The corpus of the run must still be valid (long terms' bytes are
 * read from it).  *nbytes = the text's size. */
int tfidf_format(tfidf_ctx* ctx, uint64_t* nbytes);
/* Copies bytes [off, off + n) of the formatted text to host memory. */
int tfidf_copy_text(tfidf_ctx* ctx, uint64_t off, void* dst, uint64_t n);
/* tfidf_format + D2H + write to `path` (TFIDF.c:274-282); append != 0 appends (a shard
 * after the previous ones).  An unformatted result is formatted in document groups whose
 * D2H copies overlap the next group's formatting; the copies go through the context's
 * ring of pinned 16 MB buffers (kept across calls) and a regular file is written by
 * several threads at their blocks' offsets (pwrite).  TFIDF_E_OUTPUT when the file
 * cannot be opened or written. */
int tfidf_write_output_gpu(tfidf_ctx* ctx, const char* path, int append);
/* Timings of the last tfidf_write_output_gpu (the caller sets `size` = sizeof). */
typedef struct tfidf_output_info {
    uint64_t size;
    uint64_t text_bytes;      /* bytes written */
    uint32_t writers;         /* host writer threads (1: not a regular file) */
    uint32_t formatted;       /* 1: this call formatted the text (0: it was already) */
    double   ms_prepare;      /* length pass + text size (0 when already formatted) */
    double   ms_d2h_busy;     /* host wall time from the first copy issued to the last copy done */
    double   ms_write;        /* summed host time inside write/pwrite (over writer threads) */
    double   ms_total;        /* the whole call */
} tfidf_output_info;
int tfidf_last_output_info(const tfidf_ctx* ctx, tfidf_output_info* info);
/* The device %.16f formatter on n host doubles: out = n 32-byte slots, NUL-padded.
 * TFIDF_E_INVAL for values outside [0, 2^63/10^16) (scores are < 23). */
int tfidf_format_f64(tfidf_ctx* ctx, const double* vals, uint64_t n, char* out);

/* Host emission from a fetched result (glibc snprintf; kept for callers that already
 * hold a tfidf_result): writes the same lines to `path`. */
int tfidf_write_output(const tfidf_result* r, const char* path);
/* Prints the debug TF Job / IDF Job blocks (TFIDF.c:199-205,236-239) to stdout,
 * one block pair for this shard, pairs in output order. */
int tfidf_print_jobs(const tfidf_result* r);

/* ---------------------------------------------------------------- query ----- */

/* Batched top-k document retrieval over the resident result of the last run.  The reference
 * ends at the sorted lines (TFIDF.c:245,273-282); ranking reads the scores it prints
 * (TFIDF.c:202,243-244) where tfidf_run left them, without tfidf_fetch's copy of every pair.
 *
 * Query q is bytes[q_off[q], q_off[q + 1]) (host pointers), tokenised like a document
 * (tfidf_corpus above; TFIDF.c:141-147,152): tokens are maximal runs of bytes not in
 * {0x20,0x09..0x0D}, a term is the token's bytes up to its first NUL.  w(q,t) = the tokens
 * of q whose term is t.  A term outside this shard's vocabulary contributes nothing; a term
 * of >= 16 bytes matches a vocabulary term only when the bytes are equal (the 120-bit key
 * alone does not decide: the rule of TFIDF_E_CAPACITY above and TFIDF.c:152,172's strcmp).
 *   score(q,d)   = (..((+0.0 + fl(w1*s1)) + fl(w2*s2)) + ..) in IEEE binary64, round to
 *                  nearest, every product rounded before its add (never fused), over the
 *                  terms t1 < t2 < .. of q that occur in d in term-table order (the order of
 *                  tfidf_result.pair_term inside a document), s = the run's pair_score
 *   hits of q    = the documents holding >= 1 term of q (a score of 0.0 is a hit: df = N
 *                  gives idf 0, TFIDF.c:243), ordered by score descending, then global
 *                  document id ascending numerically (not the "docN@" strcmp order of the
 *                  lines, TFIDF.c:273); the first k are returned. */
#define TFIDF_QUERY_MAX_K 1024u
#define TFIDF_QUERY_MAX_QUERIES 65536u
typedef struct tfidf_queries {
    const uint8_t*  bytes;
    uint64_t        nbytes;
    const uint64_t* q_off;       /* nqueries + 1 entries, non-decreasing, q_off[nqueries] <= nbytes */
    uint32_t        nqueries;
} tfidf_queries;
/* Arrays are owned by the library and released by tfidf_hits_free(). */
typedef struct tfidf_hits {
    uint32_t  nqueries, k;
    uint32_t* nhits;        /* per query, <= k */
    uint64_t* nmatch;       /* per query: documents holding >= 1 query term (all hits, before the cut) */
    uint32_t* nterms_found; /* per query: distinct query terms present in the vocabulary */
    uint32_t* doc;          /* nqueries * k, row q at q * k: global doc ids ("docN", TFIDF.c:132) */
    double*   score;        /* same layout */
} tfidf_hits;
/* Ranks this context's documents for every query of the batch.  TFIDF_E_STATE before a
 * successful tfidf_run; TFIDF_E_INVAL for a NULL argument, k == 0, k > TFIDF_QUERY_MAX_K,
 * nqueries > TFIDF_QUERY_MAX_QUERIES, a non-monotone q_off or q_off[nqueries] > nbytes.
 * nqueries == 0 and empty queries are valid (nhits = nmatch = 0).  The run's result is not
 * disturbed (tfidf_fetch / tfidf_format / tfidf_write_output_gpu give the same bytes after
 * the call), and the run's corpus must still be valid, as for tfidf_format (long terms are
 * compared with it).  With a communicator attached (tfidf_comm_init) the call is local, not
 * collective: it ranks this shard's documents with the run's global-df scores
 * (TFIDF.c:209-222).  The batch is scored in groups of queries, one pass over the pairs per
 * group, whose per-(query, document) accumulators stay under TFIDF_QUERY_ACC_MB (read at
 * tfidf_open, default 1024) MiB; the buffers belong to the context, so a repeated call
 * allocates nothing (tfidf_alloc_stats). */
int tfidf_query(tfidf_ctx* ctx, const tfidf_queries* queries, uint32_t k, tfidf_hits* out);
void tfidf_hits_free(tfidf_hits* hits);
/* The same over every shard of a group (tfidf_group_run; the gather + sort of
 * TFIDF.c:253-273 for hits instead of lines): every rank ranks its shard on its own host
 * thread, the host merges the ranks' rows by the same order (the shards partition the
 * documents, so this is the exact top-k), nmatch sums over the ranks and nterms_found
 * counts the distinct query terms found in at least one rank's vocabulary. */
int tfidf_group_query(tfidf_group* g, const tfidf_queries* queries, uint32_t k, tfidf_hits* out);
/* Counters of the last tfidf_query (the caller sets `size` = sizeof, as tfidf_run_info). */
typedef struct tfidf_query_info {
    uint64_t size;
    uint32_t nqueries, k;
    uint32_t nterms;          /* distinct terms of the batch */
    uint32_t nterms_found;    /* ... present in the vocabulary */
    uint32_t ngroups;         /* scoring passes over the pairs */
    uint32_t group_queries;   /* queries per group the budget allowed */
    uint64_t acc_bytes;       /* accumulator + candidate bytes of the largest group */
    double   ms_lookup;       /* device times (HIP events), summed over the groups */
    double   ms_score;
    double   ms_topk;
    double   ms_total;        /* host wall time of the whole call */
} tfidf_query_info;
int tfidf_last_query_info(const tfidf_ctx* ctx, tfidf_query_info* info);

/* ---------------------------------------------------------------- BM25 ------ */

/* tfidf_query with Okapi BM25 as the ranking function, over the same resident result: term
 * frequency saturates (k1), length normalisation is soft (b), and a word of every document
 * still counts.  Queries are tokenised exactly as for tfidf_query (tokens, terms cut at their
 * first NUL, terms of >= 16 bytes matched by their bytes); w(q,t) = the tokens of q whose
 * term is t.
 *
 * All arithmetic is IEEE binary64, round to nearest; every operation below rounds on its own
 * (fl() marks each rounding; no product is fused into an add).
 *   N          the run's ndocs_total; df(t) the run's global df (tfidf_result.term_df)
 *   idf(t)     log( fl(1.0 + fl( fl((double)(N - df) + 0.5) / fl((double)df + 0.5) )) ), the
 *              host's libm log, once per distinct found term of the batch (the Lucene form:
 *              always > 0, so a df = N word counts, unlike tfidf_query)
 *   W(q,t)     fl( (double)w(q,t) * idf(t) )
 *   avgdl      params.avgdl when it is > 0; when it is 0, fl( (double)L / (double)n ) with L the
 *              u64 sum of docSize over this context's documents and n the number of documents
 *              the context holds (L = 0: there are no pairs and every row is empty)
 *   K(d)       fl( k1 * fl( fl(1.0 - b) + fl( b * fl( (double)docSize(d) / avgdl ) ) ) )
 *   sat(d,t)   fl( fl( (double)c * fl(k1 + 1.0) ) / fl( (double)c + K(d) ) ), c = the pair's
 *              wordCount (tfidf_result.pair_count; c >= 1, so the divisor is >= 1)
 *   score(q,d) ((+0.0 + fl(W1 * sat1)) + fl(W2 * sat2)) + .. over the terms of q that occur in
 *              d, in pair order (term-table order, the order of tfidf_result.pair_term)
 *   hits of q  the documents holding >= 1 term of q, ordered by score descending, then global
 *              document id ascending numerically; the first k are returned.
 * All scores are >= +0.0 and finite.  The result does not depend on grid, group size, budget
 * or number of shards.
 *
 * Parameters: k1 >= 0, 0 <= b <= 1, avgdl >= 0, all finite; anything else, NaN included, is
 * TFIDF_E_INVAL.  So that no intermediate can become inf/inf or 0*inf (K(d) may overflow to +inf:
 * sat is then +0.0 and the score stays finite), k1 above TFIDF_BM25_MAX_K1 and an avgdl in
 * (0, TFIDF_BM25_MIN_AVGDL) are TFIDF_E_INVAL too.  `size` is set by the caller to
 * sizeof(tfidf_bm25_params); a smaller one is TFIDF_E_INVAL.  A NULL params pointer means
 * the defaults k1 = 1.2, b = 0.75, avgdl = 0. */
#define TFIDF_BM25_DEFAULT_K1 1.2
#define TFIDF_BM25_DEFAULT_B  0.75
#define TFIDF_BM25_MAX_K1     0x1p+900
#define TFIDF_BM25_MIN_AVGDL  0x1p-900
typedef struct tfidf_bm25_params {
    uint64_t size;
    double   k1, b, avgdl;
} tfidf_bm25_params;
/* Errors, state rules and buffers are tfidf_query's: TFIDF_E_STATE before a successful
 * tfidf_run; TFIDF_E_INVAL for a NULL ctx / queries / out, k == 0, k > TFIDF_QUERY_MAX_K, a bad
 * batch or bad parameters; the run's result is not disturbed; the run's corpus must still be
 * valid (long terms); with a communicator attached the call is local to this shard.  The
 * accumulators and candidate lists are tfidf_query's own buffers under TFIDF_QUERY_ACC_MB, so
 * a repeated call allocates nothing and tfidf_query after it returns its own bits.  L is
 * summed once per run.  The rows are freed with tfidf_hits_free. */
int tfidf_query_bm25(tfidf_ctx* ctx, const tfidf_queries* queries, uint32_t k, const tfidf_bm25_params* params,
                     tfidf_hits* out);
/* The same over every shard of a group, merged like tfidf_group_query.  With avgdl = 0 the
 * host sums L and n over the ranks (exact integers, one division) and hands every rank the
 * same avgdl; global df and N are shared by the run, so the merged result is bit-identical to
 * a single-shard run of the same corpus.  A multi-process caller that attached its own
 * communicator (tfidf_comm_init) has no group: its tfidf_query_bm25 calls are local, avgdl = 0
 * would be each shard's own average, so it passes the corpus-wide avgdl itself. */
int tfidf_group_query_bm25(tfidf_group* g, const tfidf_queries* queries, uint32_t k, const tfidf_bm25_params* params,
                           tfidf_hits* out);
/* Counters of the last tfidf_query_bm25: tfidf_query_info's fields and the avgdl used (the
 * caller sets `size` = sizeof). */
typedef struct tfidf_bm25_info {
    uint64_t size;
    uint32_t nqueries, k;
    uint32_t nterms;
    uint32_t nterms_found;
    uint32_t ngroups;
    uint32_t group_queries;
    uint64_t acc_bytes;
    double   ms_lookup;       /* includes the gather of the found terms' df */
    double   ms_score;
    double   ms_topk;
    double   ms_total;
    double   avgdl;           /* the value the scores were computed with (0: L = 0, no pairs) */
} tfidf_bm25_info;
int tfidf_last_bm25_info(const tfidf_ctx* ctx, tfidf_bm25_info* info);

/* ---------------------------------------------------------------- clauses --- */

/* tfidf_query / tfidf_query_bm25 with must, should and must-not clauses.  Query q has three
 * texts, `must`, `should` and `must_not`, each tokenised exactly as a tfidf_query text (tokens
 * are maximal runs of bytes outside {0x20,0x09..0x0D}, a term is the token up to its first NUL,
 * terms of >= 16 bytes are matched by their bytes).
 *   M(q), S(q), X(q)  the sets of distinct terms of the three texts
 *   w(q,t)            the tokens of t in the must text plus those in the should text (a u32
 *                     that saturates, as tfidf_query's)
 *   scoring terms     M(q) u S(q)
 *   m(q)              min_should[q], or 0 without the array
 * Document d is a hit of q exactly when
 *   (a) every term of M(q) occurs in d,
 *   (b) no term of X(q) occurs in d,
 *   (c) at least m(q) terms of S(q) occur in d (a term that is also in M counts here too),
 *   (d) d holds at least one scoring term.
 *   score(q,d)        tfidf_query's sum (TFIDF_RANK_TFIDF) or tfidf_query_bm25's (TFIDF_RANK_BM25,
 *                     W = fl(w * idf)) over the scoring terms that occur in d, in pair order,
 *                     every product rounded before its add: the same fixed sequence of IEEE
 *                     operations.  A term that is only in X contributes no product.
 *   order and cut     score descending, then global document id ascending; the first k
 *   nmatch[q]         the documents that satisfy (a)-(d), counted before the cut
 *   nterms_found[q]   the distinct scoring terms present in the vocabulary
 * Consequences:
 *   1. with empty must and must_not texts and m = 0 every field equals tfidf_query /
 *      tfidf_query_bm25 of the should text, bit for bit;
 *   2. in general the hits are the OR ranking of the text must + " " + should restricted to the
 *      documents that pass (a)-(c); no score bit differs;
 *   3. a must term outside the vocabulary gives no hits;
 *   4. a term in both M and X gives no hits;
 *   5. m(q) > |S(q)| gives no hits;
 *   6. a query with only a must_not text has no hits;
 *   7. an X term outside the vocabulary is ignored;
 *   8. the result does not depend on grid, group size, budget or number of shards (every
 *      condition is decided per document).
 * Limits, checked on the host (TFIDF_E_INVAL): at most TFIDF_CLAUSE_MAX_TERMS distinct terms in one
 * query's must text and the same in its should text, at most TFIDF_CLAUSE_MAX_NOT in its must_not
 * text, min_should[q] <= TFIDF_CLAUSE_MAX_TERMS: the 12 + 12 + 8 bits of one count word per
 * (query, document). */
#define TFIDF_RANK_TFIDF 0u
#define TFIDF_RANK_BM25  1u
#define TFIDF_CLAUSE_MAX_TERMS 4095u
#define TFIDF_CLAUSE_MAX_NOT   255u
typedef struct tfidf_clauses {
    uint64_t size;                       /* sizeof(tfidf_clauses), set by the caller */
    uint32_t nqueries, ranking;          /* TFIDF_RANK_TFIDF / TFIDF_RANK_BM25 */
    const tfidf_queries *must, *should, *must_not;   /* NULL: that text is empty in every query;
                                                        otherwise ->nqueries == nqueries */
    const uint32_t* min_should;          /* nqueries entries, or NULL */
    const tfidf_bm25_params* bm25;       /* BM25: NULL = the defaults; must be NULL for TFIDF_RANK_TFIDF */
} tfidf_clauses;
/* Every rule above on the host, without a GPU: TFIDF_E_INVAL for NULL, a short `size`, an
 * unknown ranking, nqueries > TFIDF_QUERY_MAX_QUERIES, a batch with another nqueries or a bad
 * q_off, bm25 set under TFIDF_RANK_TFIDF or bad BM25 parameters, and the limits. */
int tfidf_clauses_check(const tfidf_clauses* clauses);
/* Errors, state rules and buffers are tfidf_query's: TFIDF_E_STATE before a successful tfidf_run
 * and on a model-only context, *out zeroed on error, the run's result is not disturbed, the call
 * is local with a communicator attached, the buffers belong to the context (a repeated call
 * allocates nothing), and the call follows tfidf_prune / tfidf_reweight as tfidf_query does.
 * tfidf_last_query_info and tfidf_last_bm25_info keep what the last tfidf_query /
 * tfidf_query_bm25 left.  The rows are freed with tfidf_hits_free. */
int tfidf_query_clauses(tfidf_ctx* ctx, const tfidf_clauses* clauses, uint32_t k, tfidf_hits* out);
/* The same over every shard of a group, merged like tfidf_group_query (BM25 with avgdl = 0: the
 * average over every shard, as tfidf_group_query_bm25).  The conditions are per document and the
 * shards partition the documents, so the result is the single-shard one. */
int tfidf_group_query_clauses(tfidf_group* g, const tfidf_clauses* clauses, uint32_t k, tfidf_hits* out);
/* Counters of the last tfidf_query_clauses: tfidf_bm25_info's fields (avgdl 0 under
 * TFIDF_RANK_TFIDF) and two more (the caller sets `size` = sizeof). */
typedef struct tfidf_clause_info {
    uint64_t size;
    uint32_t nqueries, k;
    uint32_t nterms;          /* distinct terms of the batch, the three texts together */
    uint32_t nterms_found;
    uint32_t ngroups;
    uint32_t group_queries;
    uint64_t acc_bytes;
    double   ms_lookup;
    double   ms_score;
    double   ms_topk;
    double   ms_total;
    double   avgdl;
    uint32_t nq_unsatisfiable; /* queries dropped on the host: a must term outside this shard's
                                  vocabulary, a term in both M and X, or m > |S| */
    uint32_t ngroups_tab_lds;  /* groups whose table the scoring kernels staged in LDS */
} tfidf_clause_info;
int tfidf_last_clause_info(const tfidf_ctx* ctx, tfidf_clause_info* info);

/* ---------------------------------------------------------------- keywords -- */

/* Per-document top-k keyword extraction over the resident result of the last run: the k
 * best-scoring words of each document, read where tfidf_run left the scores.
 *
 * The keywords of document d are its pairs (TFIDF.c:202,243-245), one per distinct term of d.
 *   order        score descending, then term ascending in term-table order: the strcmp order
 *                of "word\t" (TFIDF.c:245,273), which is the order of tfidf_result.pair_term
 *                inside a document, so it equals pair position ascending
 *   cut          the first k pairs are returned
 *   zero scores  a pair with score +0.0 (df = N, TFIDF.c:243) is a pair like any other and
 *                sorts last
 *   scores       the run's pair_score, bit for bit: no arithmetic
 * Scores are >= +0.0 and finite, so their bit patterns order like the values, and a term
 * occurs at most once in a document (TFIDF.c:154,163 count it): the order is total and the
 * result unique.  Equal scores at the cut are the normal case (same count and df). */
#define TFIDF_TERMS_MAX_K 1024u
/* Arrays are owned by the library and released by tfidf_doc_terms_free(). */
typedef struct tfidf_doc_terms {
    uint32_t  ndocs, k;      /* rows, row stride */
    uint32_t* doc;           /* per row: global document id */
    uint32_t* pos;           /* per row: the document's output position (index into the "docN@" order); UINT32_MAX: not in this shard */
    uint64_t* npairs;        /* per row: pairs of the document (all, before the cut) */
    uint32_t* nterms;        /* per row: min(k, npairs) */
    uint32_t* term;          /* ndocs * k, row r at r * k: term rank = tfidf_result.pair_term */
    uint32_t* count;         /* wordCount (TFIDF.c:154,163) */
    double*   score;
    uint64_t* pair;          /* index of the pair in output order (tfidf_result.pair_*) */
    uint64_t* word_off;      /* ndocs * k + 1: entry r * k + j is bytes [word_off[..], word_off[.. + 1]); unused entries empty */
    uint8_t*  word_bytes;    /* the selected words' bytes, gathered on the device */
} tfidf_doc_terms;
/* doc_ids == NULL: ndocs is ignored; one row per document of this context in output order
 * ("docN@" order), empty documents included.  doc_ids != NULL: one row per entry in the
 * caller's order, duplicates allowed; an id this shard does not hold gives pos = UINT32_MAX
 * and npairs = nterms = 0.  TFIDF_E_STATE before a successful tfidf_run; TFIDF_E_INVAL for a
 * NULL ctx or out, k == 0 or k > TFIDF_TERMS_MAX_K.  The run's result is not disturbed, and the
 * run's corpus must still be valid, as for tfidf_format (long terms' bytes are read from it).
 * With a communicator attached the call is local to the context.  Rows are processed in
 * batches whose device result buffers (32 bytes per entry; the gathered words come on top)
 * stay under TFIDF_TERMS_MB (read at tfidf_open, default 256) MiB; the buffers belong to the
 * context, so a repeated identical call allocates nothing (tfidf_alloc_stats). */
int tfidf_top_terms(tfidf_ctx* ctx, const uint32_t* doc_ids, uint32_t ndocs, uint32_t k, tfidf_doc_terms* out);
void tfidf_doc_terms_free(tfidf_doc_terms* t);
/* The same over every shard of a group (tfidf_group_run).  NULL list: the ranks' rows in rank
 * order, which is the global "docN@" order for the contiguous shards tfidf_group_run
 * requires.  Id list: every rank looks the ids up on its own host thread and each row comes
 * from the rank that holds the id; an id that no rank holds stays UINT32_MAX.  pos and pair
 * count from the first rank's first document and pair (the concatenated output); term is the
 * rank in the holding shard's own term table. */
int tfidf_group_top_terms(tfidf_group* g, const uint32_t* doc_ids, uint32_t ndocs, uint32_t k, tfidf_doc_terms* out);
/* Counters of the last tfidf_top_terms (the caller sets `size` = sizeof, as tfidf_query_info). */
typedef struct tfidf_terms_info {
    uint64_t size;
    uint32_t ndocs, k;
    uint32_t nbatches;        /* batches of rows */
    uint32_t big_docs;        /* rows of documents over 4096 pairs (the workgroup kernel) */
    uint64_t out_bytes;       /* bytes copied to the host */
    double   ms_lookup;       /* device times (HIP events), summed over the batches */
    double   ms_select;
    double   ms_words;
    double   ms_total;        /* host wall time of the whole call */
} tfidf_terms_info;
int tfidf_last_terms_info(const tfidf_ctx* ctx, tfidf_terms_info* info);

/* ----------------------------------------------------------------- similar -- */

/* Top-k similar-document search over the resident result of the last run: the nearest
 * neighbours of a document under the cosine similarity of the TF-IDF vectors, read where
 * tfidf_run left the scores.
 *
 * All arithmetic is IEEE binary64, round to nearest, and no product is fused into an add.
 *   vector      document d's pairs (t, s(d,t)), s = the run's pair_score, terms in term-table
 *               order, which is pair order
 *   sq(d)       ((+0.0 + fl(s1*s1)) + fl(s2*s2)) + ... over d's pairs in pair order
 *   norm(d)     sqrt(sq(d)), correctly rounded
 *   dot(q,d)    ((+0.0 + fl(s(q,t1)*s(d,t1))) + fl(s(q,t2)*s(d,t2))) + ... over the terms q
 *               and d share, in term-table order: the strcmp order of the words, the same in
 *               every shard, so dot(q,d) and dot(d,q) have the same bits
 *   sim(q,d)    fl(dot(q,d) / fl(norm(q)*norm(d))); +0.0 when that denominator is 0 (every
 *               pair of q or of d has df = N, TFIDF.c:243)
 *   neighbours  the documents other than q itself that share at least one term with q (a
 *               similarity of +0.0 still counts)
 *   order       sim descending, then global document id ascending numerically; the first k
 *               are returned
 * All values are >= +0.0 and finite, so their bit patterns order like the values (the argument
 * of tfidf_query).  The result does not depend on grid, group size, budget or number of
 * shards. */
#define TFIDF_SIMILAR_MAX_K 1024u
/* Arrays are owned by the library and released by tfidf_neighbors_free(). */
typedef struct tfidf_neighbors {
    uint32_t  ndocs, k;      /* rows, row stride */
    uint32_t* doc;           /* per row: global document id */
    uint32_t* pos;           /* per row: the document's output position; UINT32_MAX: not in this shard */
    uint64_t* npairs;        /* per row: pairs of the document */
    double*   norm;          /* per row: norm(d) */
    uint64_t* nmatch;        /* per row: all neighbours, before the cut */
    uint32_t* nnb;           /* per row: min(k, nmatch) */
    uint32_t* nb_doc;        /* ndocs * k, row r at r * k: the neighbours' global document ids */
    uint32_t* nb_shared;     /* terms the row's document and the neighbour share */
    double*   nb_score;      /* sim */
} tfidf_neighbors;
/* The row rules are tfidf_top_terms's.  doc_ids == NULL: ndocs is ignored; one row per document
 * of this context in output order (all pairs of documents: ceil(N / group) scans of the pairs).
 * doc_ids != NULL: one row per entry in the caller's order, duplicates allowed; an id this
 * shard does not hold gives pos = UINT32_MAX and an empty row.  An empty document has no
 * neighbours.  TFIDF_E_STATE before a successful tfidf_run; TFIDF_E_INVAL for a NULL ctx or out,
 * k == 0 or k > TFIDF_SIMILAR_MAX_K.  The run's result is not disturbed.  With a communicator
 * attached the call is local to the context: it searches this shard's documents.  The norms
 * are computed by the first call after a run and kept until the next tfidf_run (16 bytes per
 * document).  The rows are scored in groups of up to 64, one scan of the pairs per group,
 * whose dense per-(row, document) accumulators and top-k candidates stay under
 * TFIDF_QUERY_ACC_MB (they are tfidf_query's buffers); all buffers belong to the context, so a
 * repeated identical call allocates nothing (tfidf_alloc_stats). */
int tfidf_similar(tfidf_ctx* ctx, const uint32_t* doc_ids, uint32_t ndocs, uint32_t k, tfidf_neighbors* out);
void tfidf_neighbors_free(tfidf_neighbors* n);
/* The same over every shard of a group (tfidf_group_run): the exact global top-k, bit-identical
 * to a single-shard run of the same corpus.  The rank that holds a row's document exports its
 * vector as (word bytes, score) and its norm; every rank resolves the words in its own
 * vocabulary, scores its shard and the host merges the ranks' rows by the same order (the
 * shards partition the documents).  nmatch sums over the ranks; pos counts from the first
 * rank's first document.  The vectors of the rows pass through host memory: the all-documents
 * form moves every pair's word and score once per rank. */
int tfidf_group_similar(tfidf_group* g, const uint32_t* doc_ids, uint32_t ndocs, uint32_t k, tfidf_neighbors* out);
/* Counters of the last tfidf_similar (the caller sets `size` = sizeof, as tfidf_query_info). */
typedef struct tfidf_similar_info {
    uint64_t size;
    uint32_t rows, k;
    uint32_t ngroups;         /* scans of the pairs */
    uint32_t group_rows;      /* rows per group the budget allowed */
    uint64_t acc_bytes;       /* accumulator + candidate bytes of the largest group */
    uint32_t big_docs;        /* documents over 4096 pairs (the workgroup kernel), per scan */
    uint32_t reserved;
    double   ms_norms;        /* device times (HIP events), summed over the groups; 0 when cached */
    double   ms_table;
    double   ms_score;
    double   ms_topk;
    double   ms_total;        /* host wall time of the whole call */
} tfidf_similar_info;
int tfidf_last_similar_info(const tfidf_ctx* ctx, tfidf_similar_info* info);

/* ---------------------------------------------------------------- clusters -- */

/* Spherical k-means over the resident result of the last run: which groups the documents fall
 * into under the cosine similarity of their TF-IDF vectors, and what each group is about.
 *
 * All arithmetic is IEEE binary64, round to nearest; fl() marks every rounding and no product
 * is fused into an add.  Documents are taken in output order (the "docN@" order, position j).
 *   norm(d)      tfidf_similar's, the same bits as tfidf_neighbors.norm
 *   unclustered  a document with norm(d) == 0 (no pairs, or every pair has df = N): label
 *                TFIDF_NO_CLUSTER, sim +0.0; it takes part in nothing
 *   u(d,t)       fl(s(d,t) / norm(d)) over d's pairs, s = the run's pair_score
 *   seeds        K global document ids; centroid 0 is C[c][t] = u(seed_c, t) on the seed's
 *                terms and +0.0 elsewhere, not renormalised.  An id this context does not hold,
 *                a seed with norm 0 and a repeated id are TFIDF_E_INVAL; two different
 *                documents with equal bytes are both valid.  seeds == NULL: the clusterable
 *                documents at indices floor(c * M / K), c = 0..K-1, M = the number of clusterable
 *                documents counted in output order.  K > M is TFIDF_E_INVAL.
 *   sim(d,c)     ((+0.0 + fl(u(d,t1) * C[c][t1])) + fl(u(d,t2) * C[c][t2])) + .. over all of
 *                d's pairs in pair order (a zero centroid entry adds +0.0)
 *   label(d)     the c with the largest sim(d,c), the lowest c among equals
 *   update       for a cluster c with at least one member:
 *                S[t] = ((+0.0 + u(d1,t)) + u(d2,t)) + .. over the members holding t, in
 *                ascending output position;
 *                sq = ((+0.0 + fl(S[t1]*S[t1])) + fl(S[t2]*S[t2])) + .. over the terms with
 *                S[t] != 0 in ascending term rank; nrm = sqrt(sq), correctly rounded;
 *                C[c][t] = fl(S[t] / nrm).  A cluster without members keeps its centroid.
 *   loop         pass it = 1..max_iter: assign against the current centroids; if it > 1 and
 *                every label equals the pass before's, stop (converged = 1); if it == max_iter,
 *                stop (converged = 0); otherwise update.  The reported centroids are the ones
 *                the returned labels and sims were computed against; max_iter = 1 is nearest seed.
 *   top terms    per cluster its nterms <= min(T, number of non-zero weights) best terms, by
 *                weight descending, then term rank ascending
 * Everything is >= +0.0 and finite, so bit patterns order like values.  The result does not
 * depend on grid, launch shape or budget. */
#define TFIDF_KMEANS_MAX_K      256u
#define TFIDF_KMEANS_MAX_TERMS  64u
#define TFIDF_KMEANS_DEFAULT_ITER 20u
#define TFIDF_NO_CLUSTER        0xFFFFFFFFu
/* `size` is set by the caller to sizeof(tfidf_kmeans_params); a smaller one is TFIDF_E_INVAL. */
typedef struct tfidf_kmeans_params {
    uint64_t size;
    uint32_t k;              /* 1..TFIDF_KMEANS_MAX_K */
    uint32_t max_iter;       /* >= 1; 0: TFIDF_KMEANS_DEFAULT_ITER */
    uint32_t nterms;         /* T, 0..TFIDF_KMEANS_MAX_TERMS */
    uint32_t nseeds;         /* with seeds: == k */
    const uint32_t* seeds;   /* NULL: the default seeds */
} tfidf_kmeans_params;
/* Arrays are owned by the library and released by tfidf_clusters_free(). */
typedef struct tfidf_clusters {
    uint32_t  ndocs, k;
    uint32_t  iterations;    /* passes (assignments) made */
    uint32_t  converged;
    uint32_t  t, reserved;   /* row stride of the term arrays (params.nterms) */
    uint32_t* doc;           /* per output position: global document id */
    uint32_t* label;         /* per output position: cluster, or TFIDF_NO_CLUSTER */
    double*   sim;           /* per output position: sim to its own centroid */
    uint32_t* size;          /* per cluster: members */
    uint32_t* seed;          /* per cluster: the seed id used */
    uint32_t* nterms;        /* per cluster: entries of its row below */
    uint32_t* term;          /* k * t, cluster c at c * t: term rank; unused entries UINT32_MAX */
    double*   weight;        /* C[c][term]; unused entries +0.0 */
    uint64_t* word_off;      /* k * t + 1, laid out as in tfidf_doc_terms; unused entries empty */
    uint8_t*  word_bytes;
} tfidf_clusters;
/* TFIDF_E_INVAL for a NULL ctx / params / out, a short params.size, k == 0 or above
 * TFIDF_KMEANS_MAX_K, nterms above TFIDF_KMEANS_MAX_TERMS, seeds with nseeds != k, bad seeds, or
 * k > M.  TFIDF_E_STATE before a successful tfidf_run and on a context that holds only an
 * imported model.  The run's result is not disturbed; the run's corpus must still be valid
 * (long terms' bytes are read from it); with a communicator attached the call is local to the
 * shard.  The dense centroid matrix takes k * V * 8 bytes (the update's sums are built in it)
 * and, with 24 bytes per document and the per-cluster words, must fit under TFIDF_KMEANS_MB MiB
 * (read at tfidf_open, default 1024: a guess, nobody has measured what a caller needs); over it
 * the call returns TFIDF_E_CAPACITY before any device work.  TFIDF_KMEANS_SPLIT (read at
 * tfidf_open) sets the update's workgroups per cluster; the result does not depend on it.  All
 * buffers belong to the context, so a repeated identical call allocates nothing
 * (tfidf_alloc_stats).  On an error *out is zeroed. */
int tfidf_kmeans(tfidf_ctx* ctx, const tfidf_kmeans_params* params, tfidf_clusters* out);
void tfidf_clusters_free(tfidf_clusters* c);
/* Counters of the last tfidf_kmeans (the caller sets `size` = sizeof, as tfidf_query_info). */
typedef struct tfidf_kmeans_info {
    uint64_t size;
    uint32_t ndocs, k;
    uint32_t passes;          /* assignments */
    uint32_t updates;
    uint32_t clusterable;     /* M */
    uint32_t split;           /* update workgroups per cluster */
    uint64_t matrix_bytes;    /* k * V * 8 */
    uint64_t work_bytes;      /* the other buffers counted against the budget */
    double   ms_norms;        /* device times (HIP events), summed over the passes; norms 0 when cached */
    double   ms_assign;
    double   ms_update;
    double   ms_terms;
    double   ms_total;        /* host wall time of the whole call */
} tfidf_kmeans_info;
int tfidf_last_kmeans_info(const tfidf_ctx* ctx, tfidf_kmeans_info* info);

/* --------------------------------------------------------------- transform -- */

/* Fit/transform: scores documents the run has not seen against the resident model of the last
 * run: its vocabulary, its global df, its N and its own idf table, all read-only.  The
 * reference has one pass over one corpus (TFIDF.c:130-247); appending a document and running
 * again would change N and every df.
 *
 * The batch is a tfidf_corpus and follows that struct's rules: document r (0-based, batch
 * order) is bytes[doc_off[r], doc_off[r + 1]), windows are allowed (doc_off[0] > 0, trailing
 * bytes after the last document), document boundaries are token boundaries, and a host pointer
 * or a TFIDF_CORPUS_DEVICE pointer of any alignment is accepted (for a device batch doc_off is
 * a device pointer too).  doc_ids and ndocs_total are ignored.  Tokens and terms are the run's
 * (TFIDF.c:141-147,152): maximal runs of bytes not in {0x20,0x09..0x0D}; a term is the token's
 * bytes up to its first NUL, and the empty term is a term.  A term of >= 16 bytes matches a
 * vocabulary term only when the bytes are equal (the 120-bit key alone never decides: the rule
 * of tfidf_query and TFIDF_E_CAPACITY above).  A token whose term is 16 MiB or longer is
 * outside every vocabulary (a run refuses it); here it is out of vocabulary, not an error.
 *   doc_size(r)  every token of the document (TFIDF.c:141-143), those outside the vocabulary
 *                included: they lower tf, they are not dropped from the denominator
 *   pairs of r   one per distinct vocabulary term of r, in ascending term rank: the
 *                strcmp("word\t") order of tfidf_result.pair_term inside a document
 *   score        fl( fl((double)count / (double)doc_size) * idf(t) ), IEEE binary64, two
 *                roundings per pair (TFIDF.c:202,243-244); idf(t) is the double the run itself
 *                used for t, log(1.0 * N / df) on the host's libm, read from the run's table.  A
 *                score of +0.0 (df = N) is a pair like any other.
 * Consequence: a batch document that is byte-equal to a document of the run gets that
 * document's pairs bit for bit (term, count, df, score) and doc_oov = 0.  No floating-point
 * atomics, no reciprocal: the result does not depend on grid, slices or budget.
 * Arrays are owned by the library and released by tfidf_rows_free(). */
typedef struct tfidf_rows {
    uint32_t  ndocs;      /* rows = the batch's documents, in batch order */
    uint32_t  reserved;
    uint64_t  npairs;     /* all rows */
    uint64_t  ntokens;    /* all rows, out-of-vocabulary tokens included */
    uint64_t* row_off;    /* ndocs + 1: row r = pairs [row_off[r], row_off[r+1]) */
    uint32_t* doc_size;   /* per row: every token of the document (TFIDF.c:141-143) */
    uint32_t* doc_oov;    /* per row: tokens whose term the vocabulary does not hold */
    uint32_t* term;       /* per pair: term rank = index into this context's term table */
    uint32_t* count;      /* wordCount of the term in the document */
    uint32_t* df;         /* the run's global df of the term */
    double*   score;
    uint64_t* word_off;   /* offset into the BATCH's bytes of the term's first token in this document */
    uint32_t* word_len;   /* the term's length (token bytes up to its first NUL) */
} tfidf_rows;
/* TFIDF_E_STATE before a successful tfidf_run or tfidf_model_import (section "model": an imported
 * model stands for the run's, with its own copy of the term bytes in the corpus's place);
 * TFIDF_E_INVAL for a NULL ctx, batch or out, a
 * non-monotone doc_off or doc_off[ndocs] > nbytes.  ndocs == 0 and empty documents are valid.
 * The state rules are tfidf_query's: the run's result is not disturbed (tfidf_fetch,
 * tfidf_format, tfidf_query and the others give the same bytes afterwards), the run's corpus
 * must still be valid (long terms are compared with it), and with a communicator attached the
 * call is local to this shard's vocabulary (with the run's global df and N).
 * The batch is processed in slices cut at document boundaries.  A slice's device scratch
 * (boundary bitmap and counts, token records, the sort's ping-pong buffers, pairs) is bounded
 * before its tokens are known, by one token per two bytes, and slices are cut so that this
 * bound stays under TFIDF_TRANSFORM_MB MiB (read at tfidf_open); a single document larger than
 * that is a slice of its own and the buffers grow for it.  The default of 512 is a guess:
 * nobody has measured which budget serves which batch best.  The buffers belong to the
 * context, so a repeated identical call allocates nothing (tfidf_alloc_stats). */
int tfidf_transform(tfidf_ctx* ctx, const tfidf_corpus* batch, tfidf_rows* out);
/* NULL or an all-zero struct: no-op. */
void tfidf_rows_free(tfidf_rows* r);
/* The same over every shard of a group (tfidf_group_run).  Host batches only: a
 * TFIDF_CORPUS_DEVICE batch is TFIDF_E_INVAL.  Every rank transforms the whole batch against
 * its own vocabulary on its own host thread; the host merges each row across the ranks in
 * strcmp("word\t") order of the words (read from the batch bytes; every rank's row is already
 * in that order).  A pair several ranks found is kept once: equal word_off identifies it, and
 * the ranks agree on count, df and score because df and N are global.  doc_oov = doc_size
 * minus the merged counts.  term is UINT32_MAX (the shards share no term table).  The merged
 * result is bit-identical to a single-shard run of the same corpus. */
int tfidf_group_transform(tfidf_group* g, const tfidf_corpus* batch, tfidf_rows* out);
/* Counters of the last tfidf_transform (the caller sets `size` = sizeof, as tfidf_query_info). */
typedef struct tfidf_transform_info {
    uint64_t size;
    uint32_t ndocs;
    uint32_t nslices;
    uint64_t ntokens;
    uint64_t npairs;
    uint64_t noov;            /* tokens outside the vocabulary */
    uint64_t scratch_bytes;   /* device scratch of the largest slice */
    double   ms_tokens;       /* device times (HIP events), summed over the slices: token boundaries */
    double   ms_resolve;      /* rows, terms, vocabulary probes */
    double   ms_sort;         /* the (row, term) sort */
    double   ms_pairs;        /* run heads, counts, scores, row offsets */
    double   ms_total;        /* host wall time of the whole call */
} tfidf_transform_info;
int tfidf_last_transform_info(const tfidf_ctx* ctx, tfidf_transform_info* info);

/* ------------------------------------------------------------------- model -- */

/* The model tfidf_transform scores against, as an object of its own: the term table in
 * strcmp("word\t") order (the order of tfidf_result.term_off), the global df of every term and
 * N.  It is exported from a fitted context or a whole group, written to a file, read back and
 * imported into a fresh context, which then answers tfidf_transform bit for bit as the fitted
 * context would, with no corpus anywhere.  The reference keeps none of this past its one pass
 * (TFIDF.c:130-247).
 * idf is never part of a model: the importing host's libm computes log(1.0 * N / df)
 * (TFIDF.c:243), the rule of a run. */
typedef struct tfidf_model {
    uint64_t  size;          /* sizeof(tfidf_model), set by whoever fills the struct */
    uint64_t  ndocs_total;   /* N of log(N/df) */
    uint32_t  nterms;        /* V */
    uint32_t  reserved;
    uint64_t* term_off;      /* nterms + 1; term t = term_bytes[term_off[t], term_off[t+1]) */
    uint8_t*  term_bytes;
    uint32_t* term_df;       /* global df */
} tfidf_model;
/* Host only.  TFIDF_E_INVAL unless: size >= sizeof(tfidf_model); term_off is non-decreasing;
 * every term is shorter than 16 MiB and holds no NUL and none of the separator bytes
 * {0x20,0x09..0x0D} (no token contains them); the terms are strictly ascending compared as
 * word + "\t" with strcmp on unsigned bytes (which also rules out duplicates); 1 <= df <= N for
 * every term; nterms < 2^32 - 1.  The empty term is a term; nterms == 0 is valid for any N. */
int tfidf_model_check(const tfidf_model* m);
/* The context's term table, global df and N: byte for byte tfidf_fetch's term_off, term_bytes,
 * term_df and ndocs_total, without the pairs.  The words are gathered on the device (short
 * terms from their keys, long terms from the run's corpus, which must still be valid, or from
 * the imported model's own bytes) and come back in three copies.  TFIDF_E_STATE unless the
 * context holds a model, from a run or from an import.  With a communicator attached the call
 * is local: this shard's vocabulary with the global df.  The arrays are owned by the library
 * and released by tfidf_model_free(). */
int tfidf_model_export(tfidf_ctx* ctx, tfidf_model* out);
/* The model of a whole group (tfidf_group_run): every rank exports on its own host thread and
 * the host k-way merges the sorted term tables in the same order.  A word several ranks hold is
 * kept once; ranks that disagree on its df make the call return TFIDF_E_STATE.  Byte-identical
 * to a single-shard export of the same corpus. */
int tfidf_group_model_export(tfidf_group* g, tfidf_model* out);
/* Checks the model (TFIDF_E_INVAL; the context is then left as it was) and puts the context
 * into a model-only state: tfidf_transform and tfidf_model_export work, everything that needs
 * pairs (tfidf_fetch, tfidf_format, tfidf_write_output_gpu, tfidf_query*, tfidf_top_terms,
 * tfidf_similar) returns TFIDF_E_STATE.  A previous run's result is discarded; a later tfidf_run
 * replaces the imported model as it replaces a previous run.  The context builds what a run
 * leaves behind (the slot table, the ranks, df, the idf table of this host's libm) from its own
 * device copy of the term bytes: the caller may free `m` as soon as the call returns.  The table
 * has the smallest power-of-two size, not below the context's current one, that keeps V under
 * the run's load limits; more than 2^28 slots is TFIDF_E_CAPACITY, as are two distinct terms of
 * 16 bytes or more that share their 120-bit identity key.  The buffers belong to the context:
 * a repeated import of the same model allocates nothing (tfidf_alloc_stats). */
int tfidf_model_import(tfidf_ctx* ctx, const tfidf_model* m);
/* Host only.  The file is little-endian without padding and depends on the model alone:
 *   0  "TFIDFMDL"   8  u32 version = 1   12  u32 nterms   16  u64 ndocs_total
 *   24 u64 nbytes = term_off[V] - term_off[0]
 *   32 u64 FNV-1a-64 (offset basis 0xcbf29ce484222325, prime 0x100000001b3) of every byte from 40 on
 *   40 u64 term_off[V + 1] rebased to term_off[0] = 0, then u32 term_df[V], then the term bytes
 * save: TFIDF_E_INVAL for a model that fails tfidf_model_check, TFIDF_E_OUTPUT when the file
 * cannot be written.  load: TFIDF_E_MODEL when the file cannot be opened, is shorter or longer
 * than its header implies, has a wrong magic, version or checksum, or holds arrays that fail
 * tfidf_model_check; TFIDF_E_NOMEM; *out is zeroed on every error, else released by
 * tfidf_model_free(). */
int tfidf_model_save(const tfidf_model* m, const char* path);
int tfidf_model_load(const char* path, tfidf_model* out);
/* NULL or an all-zero struct: no-op.  Only for models the library filled. */
void tfidf_model_free(tfidf_model* m);
/* Counters of the last tfidf_model_import or tfidf_model_export (the caller sets `size` =
 * sizeof, as tfidf_query_info). */
typedef struct tfidf_model_info {
    uint64_t size;
    uint32_t nterms;
    uint32_t reserved;
    uint64_t table_slots;     /* the vocabulary table's slots */
    uint64_t blob_bytes;      /* term bytes */
    uint64_t long_terms;      /* terms of >= 16 bytes (import; 0 after an export) */
    double   ms_build;        /* import: device time of the table's clear + build (HIP events); export: 0 */
    double   ms_total;        /* host wall time of the whole call */
} tfidf_model_info;
int tfidf_last_model_info(const tfidf_ctx* ctx, tfidf_model_info* info);

/* ---------------------------------------------------------------- analyzer -- */

/* A byte-to-byte analyzer in front of the counter: case folding, punctuation stripping, a
 * minimum token length, a stop-word list and a Porter stemmer.  The reference tokenises with
 * fscanf("%s") and compares with strcmp (TFIDF.c:141-152): "The", "the", "the," and "(the" are
 * four terms.  The analyzer rewrites a corpus (or a batch, or the lines of a query batch: bytes plus offsets)
 * into one of the same length with the same offsets, so tfidf_run and everything after it stay
 * as they are.  Everything is byte-exact.
 *
 * For every document window [off[i], off[i + 1]):
 *   1. byte map, each byte on its own
 *        TFIDF_AN_LOWER   0x41..0x5A become b + 0x20
 *        TFIDF_AN_PUNCT   every ASCII byte that is not a letter, a digit or one of the six
 *                         separators {0x20,0x09..0x0D} becomes 0x20: 0x00..0x08, 0x0E..0x1F,
 *                         0x21..0x2F, 0x3A..0x40, 0x5B..0x60, 0x7B..0x7F (60 values, NUL among
 *                         them: with this flag a token equals its term)
 *        everything else is unchanged: bytes >= 0x80 (UTF-8 passes through, unless
 *        TFIDF_AN_UTF8 is set: 1b) and the separators themselves ('\n' stays '\n')
 *   1b. sequence map, with TFIDF_AN_UTF8, beside the byte map.  Two tables of code points
 *      >= U+0080, frozen at the Unicode version csrc/analyze_utf8_tab.h records (13.0.0):
 *        FOLD    cp whose lowercase is exactly one code point L(cp) != cp with a UTF-8 form of
 *                the same length (1342 code points; the 25 whose lowercase changes length, such
 *                as U+0130, U+023A, U+1E9E, U+2126, U+212A, U+212B, are not in it)
 *        BLANK   cp of general category P*, S* or Z* (8348 code points: NBSP, U+2003, the
 *                typographic quotes and dashes, U+2026, currency signs, emoji)
 *      A sequence is an occurrence of the bytes UTF-8(cp), cp in a table, that lies wholly
 *      inside the document window; occurrences never overlap.  This equals decoding the document
 *      as UTF-8 with every undecodable byte passed through.  Malformed bytes (overlong forms,
 *      encoded surrogates, stray continuations, truncated leads) are never touched, nor is a
 *      sequence that a document boundary, a window edge or the buffer's end cuts: shards and
 *      batches analyze separately and must agree.
 *        TFIDF_AN_PUNCT | TFIDF_AN_UTF8   every byte of a BLANK sequence becomes 0x20
 *        TFIDF_AN_LOWER | TFIDF_AN_UTF8   a FOLD sequence becomes UTF-8(L(cp))
 *      U+24B6..U+24CF are in both tables: with both flags the blank wins, as in ASCII.
 *      TFIDF_AN_UTF8 alone is valid and changes nothing.  Cf (U+200B, U+00AD, U+FEFF), Mn
 *      (combining marks) and Cc (C1 controls) are in neither table.  No special casing: U+03A3
 *      always becomes U+03C3.  Steps 2 and 3 run on the mapped bytes: min_len and
 *      TFIDF_AN_MAX_WORD count bytes, stop words are compared verbatim (the caller supplies the
 *      folded form), and the stemmer takes tokens of a..z only.  L(L(cp)) does not exist, so the
 *      analyzer without a stemmer stays idempotent.
 *   2. token filter, on the mapped bytes: tokens are the maximal runs of non-separator bytes
 *      inside the document (a document boundary ends a token, as for tfidf_corpus).  A token is
 *      blanked (every one of its bytes becomes 0x20) when its length in bytes is < min_len, or
 *      when its bytes equal a stop word.  The comparison takes the whole token, not the term cut
 *      at a NUL: stop words hold no NUL, so without TFIDF_AN_PUNCT a token that contains a NUL
 *      never matches.  Stop words are compared verbatim with the mapped tokens: the caller
 *      supplies them already folded.
 *   3. stemmer (stemmer = TFIDF_STEM_PORTER), on the bytes that 1 and 2 produced.  A token that
 *      survived the filter is stemmed when its length L is 3..TFIDF_AN_MAX_WORD and every one of
 *      its bytes is in 0x61..0x7A.  Every other token is unchanged: one with a digit, a byte
 *      >= 0x80, an upper-case letter (without TFIDF_AN_LOWER) or a NUL, and one of 1, 2 or more
 *      than 64 bytes.  Leaving tokens of 1 or 2 bytes alone is the one departure from the paper;
 *      it is the guard Porter's own C implementation has.  With S the stem's length,
 *      1 <= S <= L, bytes [0, S) of the token become the stem and bytes [S, L) become 0x20.
 *      min_len and the stop list see the UNSTEMMED token (the order of Lucene's stop filter and
 *      stem filter): with "running" in the list, "running" is blanked and "run" is not; with
 *      "run" in the list, "running" becomes "run" and stays.  A document boundary ends a token
 *      as before: "runn|ing" split by off is two tokens, "runn" and "ing".
 *
 *      The algorithm is Porter 1980 exactly as published (no logi -> log; abli -> able, not
 *      bli -> ble).  A consonant is a letter other than a, e, i, o, u and other than a y
 *      preceded by a consonant; a y at the start or after a vowel is a consonant.  m is the
 *      number of VC sequences in [C](VC)^m[V].  *v*: the stem contains a vowel.  *d: the stem
 *      ends in a double consonant.  *o: the stem ends consonant-vowel-consonant with the last
 *      letter not w, x or y.  Conditions apply to the stem in front of the suffix.  In every
 *      step the longest matching suffix is chosen; if its condition fails, the step does
 *      nothing ("feed" matches EED, has m = 0 and is left alone; ED is not tried).
 *        1a  SSES -> SS, IES -> I, SS -> SS, S -> ""
 *        1b  (m>0) EED -> EE; (*v*) ED -> ""; (*v*) ING -> "".  After the second or third rule
 *            fired, the first of these that applies: AT -> ATE, BL -> BLE, IZ -> IZE; *d and
 *            not ending in l, s or z -> drop the last letter; m=1 and *o -> append E
 *        1c  (*v*) Y -> I
 *        2   (m>0) ATIONAL -> ATE, TIONAL -> TION, ENCI -> ENCE, ANCI -> ANCE, IZER -> IZE,
 *            ABLI -> ABLE, ALLI -> AL, ENTLI -> ENT, ELI -> E, OUSLI -> OUS, IZATION -> IZE,
 *            ATION -> ATE, ATOR -> ATE, ALISM -> AL, IVENESS -> IVE, FULNESS -> FUL,
 *            OUSNESS -> OUS, ALITI -> AL, IVITI -> IVE, BILITI -> BLE
 *        3   (m>0) ICATE -> IC, ATIVE -> "", ALIZE -> AL, ICITI -> IC, ICAL -> IC, FUL -> "",
 *            NESS -> ""
 *        4   (m>1) removed: AL, ANCE, ENCE, ER, IC, ABLE, IBLE, ANT, EMENT, MENT, ENT, ION (only
 *            when the stem ends in s or t), OU, ISM, ATE, ITI, OUS, IVE, IZE
 *        5a  (m>1) E -> ""; (m=1 and not *o) E -> ""
 *        5b  (m>1 and *d and ending in l) -> drop the last letter
 * Bytes of [0, nbytes) outside [off[0], off[n]) are copied unchanged.
 * Consequences: without a stemmer the analyzer is idempotent, with one it is not (Porter is
 * not: "agreed" -> "agre" -> "agr"); stemming is independent of TFIDF_AN_LOWER (an upper-case
 * letter that was not folded makes its token ineligible); with flags = 0, min_len <= 1, no stop
 * words and no stemmer the output equals the input; a token longer than TFIDF_AN_MAX_WORD bytes
 * is never blanked or stemmed (it matches no stop word and is not shorter than min_len).
 * The analyzer is not part of a model (tfidf_model, the model file), its stemmer included:
 * whoever scores batches against a saved model passes the same analyzer again. */
#define TFIDF_AN_LOWER 1u
#define TFIDF_AN_PUNCT 2u
#define TFIDF_AN_UTF8 16u                /* 4u and 8u are unknown flag bits */
#define TFIDF_STEM_NONE   0u
#define TFIDF_STEM_PORTER 1u
#define TFIDF_AN_MAX_WORD 64u            /* longest stop word, largest min_len */
#define TFIDF_AN_MAX_STOP 4096u          /* stop words */
#define TFIDF_AN_MAX_STOP_BYTES 32768u   /* all stop words together */
typedef struct tfidf_analyzer {
    uint64_t size;               /* sizeof(tfidf_analyzer), set by the caller */
    uint32_t flags;              /* TFIDF_AN_* */
    uint32_t min_len;
    const uint8_t*  stop_bytes;  /* stop word i = stop_bytes[stop_off[i], stop_off[i + 1]) */
    const uint64_t* stop_off;    /* nstop + 1 */
    uint32_t nstop;
    uint32_t stemmer;            /* TFIDF_STEM_*.  This was `reserved` and unchecked until the stemmer
                                    came; same offset and size, and every in-tree caller zeroed it */
} tfidf_analyzer;
/* Host only.  TFIDF_E_INVAL for: NULL; size < sizeof(tfidf_analyzer); unknown flag bits;
 * a stemmer other than TFIDF_STEM_NONE and TFIDF_STEM_PORTER; min_len > TFIDF_AN_MAX_WORD;
 * nstop > TFIDF_AN_MAX_STOP; nstop > 0 with a NULL stop_bytes or
 * stop_off; a non-monotone stop_off; more than TFIDF_AN_MAX_STOP_BYTES bytes of stop words; a
 * stop word that is empty, longer than TFIDF_AN_MAX_WORD, or holds a NUL or a separator.
 * Duplicates in the list are allowed. */
int tfidf_analyzer_check(const tfidf_analyzer* an);
/* Host only, plain C: the definition above.  Document i is bytes[off[i], off[i + 1]); out
 * receives nbytes bytes and may equal bytes (in place).  TFIDF_E_INVAL for an analyzer that
 * fails the check, a NULL bytes or out with nbytes > 0, a NULL off with n > 0, a non-monotone
 * off or off[n] > nbytes.  Stop words are looked up in the same open-addressed table the device
 * kernel probes (csrc/analyze_tab.h). */
int tfidf_analyze_host(const tfidf_analyzer* an, const uint8_t* bytes, uint64_t nbytes,
                       const uint64_t* off, uint32_t n, uint8_t* out);
/* Host only, plain C: step 3 on one word, byte by byte, for a stop list or a query term.
 * Returns the stem's length S and rewrites word[0, S); word[S, len) is left as it is.  Returns
 * len and writes nothing for an ineligible word (len < 3, len > TFIDF_AN_MAX_WORD, a byte
 * outside 0x61..0x7A); TFIDF_E_INVAL for NULL with len > 0. */
int tfidf_stem_porter(uint8_t* word, uint32_t len);

/* The same on the device (analyze.hip), where tfidf_ingest_dir_device leaves the bytes.
 * in: a host corpus (staged in a context buffer first) or a TFIDF_CORPUS_DEVICE corpus at any
 * alignment of bytes, windows allowed: the context's own ingest or synth buffer, or a caller's.
 * *out: a device corpus in buffers owned by the context (slot `slot`), valid until the next
 * tfidf_analyze with the same slot on this context or tfidf_close; out->bytes is 16-byte aligned
 * whatever the input's alignment (a run takes its default kernel), doc_off and doc_ids are the
 * context's own device copies, nbytes / ndocs / ndocs_total are the input's.
 * Two slots, because a run's corpus must stay valid while batches are analyzed (emission,
 * keywords, query and transform read long terms from it): the corpus goes to slot 0, batches
 * to slot 1.
 * TFIDF_E_INVAL: a NULL argument, slot > 1, an analyzer that fails the check, bad offsets (the
 * rules of tfidf_transform), in->bytes inside the same slot's buffer.  ndocs == 0, nbytes == 0
 * and empty documents are valid.  The kernels read no byte outside in->bytes[0, nbytes) and
 * write none outside the slot's [0, nbytes).  The result does not depend on grid, tile or list
 * order.  All buffers belong to the context: a repeated identical call allocates nothing
 * (tfidf_alloc_stats).  The call neither needs nor disturbs a run's result and works before any
 * tfidf_run.  There is no group entry point: analyze each shard on tfidf_group_ctx(g, r) before
 * tfidf_group_run. */
#define TFIDF_AN_SLOT_CORPUS 0u
#define TFIDF_AN_SLOT_BATCH  1u
int tfidf_analyze(tfidf_ctx* ctx, const tfidf_analyzer* an, const tfidf_corpus* in,
                  uint32_t slot, tfidf_corpus* out);
/* Counters of the last tfidf_analyze (the caller sets `size` = sizeof, as tfidf_query_info). */
typedef struct tfidf_analyze_info {
    uint64_t size;
    uint64_t nbytes;
    uint32_t ndocs;
    uint32_t nstop;           /* stop words of the list, duplicates included */
    uint32_t table_slots;     /* slots of the stop-word table (0: no list) */
    uint32_t lds_bytes;       /* LDS of a workgroup: table, word bytes, tile and halos (0: the
                                 pure byte map, which uses none) */
    uint32_t tile_bytes;      /* bytes a workgroup owns per step */
    uint32_t grid;            /* persistent workgroups of the tile kernel (0: the pure byte map);
                                 env TFIDF_AN_GRID, read at tfidf_open, caps it (0 or unset: the
                                 GPU's resident workgroups).  The result does not depend on it */
    uint64_t blanked_tokens;  /* tokens blanked (an integer atomic counter, one add per workgroup) */
    double   ms_kernel;       /* device time of the kernels (HIP events) */
    double   ms_total;        /* host wall time of the whole call */
    uint64_t stemmed_tokens;  /* tokens whose bytes the stemmer changed, counted like blanked_tokens */
    uint64_t utf8_changed;    /* TFIDF_AN_UTF8: sequences whose bytes changed, each counted where its
                                 first byte lies, like blanked_tokens */
} tfidf_analyze_info;
int tfidf_last_analyze_info(const tfidf_ctx* ctx, tfidf_analyze_info* info);

/* ----------------------------------------------------------------- n-grams -- */

/* Word n-grams (shingles) in front of the counter: the one stage that is not bytes-to-bytes of
 * the same length.  It turns a corpus into a corpus of another size whose tokens are the grams;
 * tfidf_run, query, BM25, keywords, similar, clusters, transform and the model work on its
 * output as on any corpus.  Byte-exact everywhere.
 *
 * Parameters: min_n and max_n with 1 <= min_n <= max_n <= TFIDF_NGRAM_MAX_N, and a joiner byte J
 * (0: the default 0x5F '_'; any byte except NUL and the six separators 0x20, 0x09..0x0D).  After
 * TFIDF_AN_PUNCT no token holds '_', so the grams are unambiguous.
 *
 * The tokens t_0..t_{m-1} of every document window [off[i], off[i + 1]) are the maximal runs of
 * non-separator bytes inside the document; a document boundary ends a token, as for
 * tfidf_corpus.  The output document is, position-major,
 *
 *     for p in 0..m-1:  for n in min_n..max_n:  if p + n <= m:
 *         t_p J t_{p+1} J .. J t_{p+n-1}  0x20
 *
 * every gram followed by exactly one blank.  Tokens are copied verbatim, NUL bytes included; the
 * run's own "term = bytes up to the first NUL" rule then applies to the gram.  The output corpus
 * is the concatenation of the output documents: out_off[0] = 0, nbytes_out = out_off[ndocs];
 * bytes outside [off[0], off[ndocs]) are dropped; a document with fewer than min_n tokens
 * becomes an empty document; doc_ids and ndocs_total pass through; with (1, 1) the output is the
 * input's tokens separated by single blanks.
 *
 * Example: b"XXnew  york\ncityrunning onYY" with off = [2, 16, 20, 26] ("runn|ing" is cut by a
 * document boundary and no gram crosses it):
 *     (1, 2)  b"new new_york york york_city city runn ing ing_on on "   out_off [0, 33, 38, 52]
 *     (2, 3)  b"new_york new_york_city york_city ing_on "               out_off [0, 33, 33, 40]
 *
 * Consequences: docSize of a run of the output counts grams, not words.  The stage runs after
 * the analyzer, so grams skip over blanked stop words, as in scikit-learn.  Like the analyzer it
 * is not recorded in a model file: whoever serves from a model passes the same options again.  A
 * gram of 16 MiB or more is refused by the run itself (TFIDF_E_CAPACITY), not here. */
#define TFIDF_NGRAM_MAX_N 8u
typedef struct tfidf_ngram_params {
    uint64_t size;               /* sizeof(tfidf_ngram_params), set by the caller */
    uint32_t min_n, max_n;
    uint8_t  joiner;             /* 0: '_' */
    uint8_t  reserved[7];        /* 0 */
} tfidf_ngram_params;
/* Host only.  TFIDF_E_INVAL for: NULL; size < sizeof(tfidf_ngram_params); min_n == 0;
 * max_n < min_n; max_n > TFIDF_NGRAM_MAX_N; a joiner that is a separator; non-zero reserved
 * bytes. */
int tfidf_ngram_check(const tfidf_ngram_params* params);
/* Host only, plain C: the definition above.  Document i is bytes[off[i], off[i + 1]).
 * *out_bytes (*out_nbytes bytes; at least one byte is allocated) and *out_off (n + 1 entries)
 * are malloc'd and released with tfidf_free.  TFIDF_E_INVAL for parameters that fail the check,
 * a NULL output pointer, a NULL bytes with nbytes > 0, a NULL off with n > 0, a non-monotone off
 * or off[n] > nbytes; TFIDF_E_NOMEM.  On an error the three outputs are zeroed. */
int tfidf_ngrams_host(const tfidf_ngram_params* params, const uint8_t* bytes, uint64_t nbytes,
                      const uint64_t* off, uint32_t n, uint8_t** out_bytes, uint64_t* out_nbytes,
                      uint64_t** out_off);

/* The same on the device (ngram.hip).  in: a host corpus (staged in a context buffer first) or a
 * TFIDF_CORPUS_DEVICE corpus at any alignment of bytes, windows allowed.  *out: a device corpus
 * in buffers owned by the context (slot `slot`), valid until the next tfidf_ngrams with the same
 * slot on this context or tfidf_close; out->bytes is 16-byte aligned, doc_off (the new offsets)
 * and doc_ids are the context's own device copies, ndocs / ndocs_total are the input's.
 * Two slots of its own, separate from the analyzer's: the corpus goes to slot 0, batches to
 * slot 1.  The usual chain is ingest -> tfidf_analyze slot 0 -> tfidf_ngrams slot 0 ->
 * tfidf_run.
 * TFIDF_E_INVAL: a NULL argument, slot > 1, parameters that fail the check, bad offsets (the
 * rules of tfidf_transform), in->bytes inside the same n-gram slot's buffer.  ndocs == 0,
 * nbytes == 0 and empty documents are valid.  TFIDF_E_CAPACITY: 2^32 - 1 tokens or more.  The
 * kernels read no byte outside in->bytes[0, nbytes).  The result does not depend on grid or
 * tile.  All buffers belong to the context: a repeated identical call allocates nothing
 * (tfidf_alloc_stats).  The call neither needs nor disturbs a run's result and works before any
 * tfidf_run.  There is no group entry point: shingle each shard on tfidf_group_ctx(g, r) before
 * tfidf_group_run.
 * The whole input is handled in one piece, without slicing: beside the output the call holds 24
 * bytes of scratch per token (start, end, segment offset) plus the boundary bitmap and per-tile
 * counts of the input (about nbytes / 8 + nbytes / 256) and 4 bytes per 4096 output bytes.  What
 * a caller needs in practice has not been measured. */
#define TFIDF_NG_SLOT_CORPUS 0u
#define TFIDF_NG_SLOT_BATCH  1u
int tfidf_ngrams(tfidf_ctx* ctx, const tfidf_ngram_params* params, const tfidf_corpus* in,
                 uint32_t slot, tfidf_corpus* out);
/* Counters of the last tfidf_ngrams (the caller sets `size` = sizeof, as tfidf_query_info). */
typedef struct tfidf_ngram_info {
    uint64_t size;
    uint64_t nbytes_in;       /* in->nbytes */
    uint64_t nbytes_out;
    uint64_t ntokens;         /* tokens of the input's documents */
    uint64_t ngrams;          /* grams written */
    uint32_t ndocs;
    uint32_t tile_bytes;      /* output bytes a workgroup of the write kernel owns */
    uint32_t grid;            /* workgroups of the write kernel (0: nothing to write) */
    uint32_t reserved;
    uint64_t scratch_bytes;   /* device scratch beside the output: bitmap, counts, 24 bytes per token */
    double   ms_bounds;       /* token bounds (HIP events, like the next two) */
    double   ms_sizes;        /* segment sizes, their scan, the document offsets */
    double   ms_write;        /* the write kernel */
    double   ms_total;        /* host wall time of the whole call */
} tfidf_ngram_info;
int tfidf_last_ngram_info(const tfidf_ctx* ctx, tfidf_ngram_info* info);

/* ------------------------------------------------------------------- prune -- */

/* Vocabulary pruning by document frequency: min_df, max_df and max_features over the resident
 * result of the last run.  tfidf_prune removes terms, and with them their pairs, from what the
 * run left in HBM; it never changes a number that stays.  The reference keeps every word
 * (TFIDF.c:152-188); a second run over a filtered corpus would change docSize and every score.
 *
 *   kept set    term t survives the range test when
 *                 (min_df <= 1 || df(t) >= min_df) && (max_df == 0 || df(t) <= max_df),
 *               df = the run's global df (tfidf_result.term_df).  With max_features = M > 0 only
 *               the first M survivors of the range test are kept, in the order df descending,
 *               then term rank ascending (term rank = the strcmp("word\t") order of the term
 *               table).  M >= the number of survivors removes nothing more.  The ranking is by
 *               df, not by collection frequency (the sum of the counts): the df is resident by
 *               rank, and (df, rank) is a total order, so the cut is unique.
 *   terms       the kept terms keep their relative order; their new ranks are 0..V'-1
 *   pairs       a pair survives exactly when its term does; the surviving pairs of a document
 *               keep their order
 *   unchanged   count, df and score of a surviving pair are the run's bits: nothing is
 *               recomputed.  docSize, N, ndocs, the document ids and the output order of the
 *               documents are unchanged.  The tokens of a pruned word still count in docSize,
 *               exactly as out-of-vocabulary tokens do in tfidf_transform.  A document may end
 *               with no pairs.
 * Consequences:
 *   - tfidf_fetch after the call equals the fetch before it with the pruned terms and their
 *     pairs removed and pair_term renumbered;
 *   - the formatted text is the old text minus the lines of pruned words, in the same order;
 *   - tfidf_transform of the run's own corpus against the pruned context gives the pruned pairs
 *     bit for bit; a pruned word is out of vocabulary (it counts in doc_oov and doc_size);
 *   - tfidf_query, _query_bm25, _top_terms, _similar, _kmeans and _model_export answer as they
 *     would on a result that never held the pruned terms.  BM25's L and avgdl are unchanged,
 *     because docSize is; the norms of tfidf_similar are recomputed;
 *   - prune(a) then prune(b) on df ranges equals one prune with the intersected range;
 *   - a prune that removes nothing leaves every byte as it was.
 * After the call tfidf_last_run_info still describes the run.  A later tfidf_run or
 * tfidf_model_import replaces everything as before: a run after a prune gives the unpruned
 * result again.
 * `size` is set by the caller to sizeof(tfidf_prune_params). */
typedef struct tfidf_prune_params {
    uint64_t size;
    uint32_t min_df;         /* 0 or 1: no lower bound */
    uint32_t max_df;         /* 0: no upper bound */
    uint32_t max_features;   /* 0: no cut */
    uint32_t reserved;       /* 0 */
} tfidf_prune_params;
/* Host only.  TFIDF_E_INVAL for: NULL; size < sizeof(tfidf_prune_params); non-zero reserved;
 * max_df != 0 && min_df > max_df. */
int tfidf_prune_check(const tfidf_prune_params* params);
/* TFIDF_E_INVAL for a NULL ctx or parameters that fail the check.  TFIDF_E_STATE before a
 * successful tfidf_run and on a context that holds only an imported model (prune the model on
 * the host with tfidf_model_prune before importing it).  With a communicator attached the call
 * is local and df is global, so min_df / max_df select the same words on every rank;
 * max_features != 0 is TFIDF_E_INVAL there (the ranks share no term table; a cut over all
 * ranks is not provided).  A failed call leaves the result exactly as it was: the new arrays
 * are written into spare buffers of the context and swapped in when every step has succeeded.
 * The run's corpus must still be valid afterwards, as before (long terms).  All buffers belong
 * to the context: a repeated run -> prune sequence allocates nothing after the first
 * (tfidf_alloc_stats).  The spares are as large as the arrays they stand in for: a context
 * that prunes holds the pair arrays (16 bytes per pair) and the two term arrays twice.  Integer kernels only, no atomics on results: the outcome does not
 * depend on grid or tile size. */
int tfidf_prune(tfidf_ctx* ctx, const tfidf_prune_params* params);
/* The same on every rank of a group at once (one host thread per rank).  max_features != 0 is
 * TFIDF_E_INVAL at every group size.  After it tfidf_group_write_output, _query, _similar,
 * _transform and _model_export equal a pruned single-shard run of the same corpus.  Returns the
 * lowest rank's error; a rank that failed keeps its unpruned result while the others are
 * pruned, so run again after an error. */
int tfidf_group_prune(tfidf_group* g, const tfidf_prune_params* params);
/* Counters of the last tfidf_prune (the caller sets `size` = sizeof, as tfidf_query_info). */
typedef struct tfidf_prune_info {
    uint64_t size;
    uint32_t nterms_before, nterms_after;
    uint64_t npairs_before, npairs_after;
    uint32_t docs_emptied;    /* documents that held pairs before the call and hold none after */
    uint32_t cut_df;          /* the df of the last term max_features kept when the cut removed a
                                 survivor of the range test; 0 when it removed none */
    double   ms_select;       /* device times (HIP events): the keep mask and the new ranks */
    double   ms_terms;        /* the term arrays */
    double   ms_pairs;        /* the pair pass: count, scan, write, document offsets */
    double   ms_total;        /* host wall time of the whole call */
} tfidf_prune_info;
int tfidf_last_prune_info(const tfidf_ctx* ctx, tfidf_prune_info* info);
/* Host only, plain C: the same definition on a model struct, for which df and the term order
 * are all it needs.  *out is owned by the library and released with tfidf_model_free; its
 * term_off starts at 0.  TFIDF_E_INVAL for a NULL argument, parameters that fail the check or a
 * model that fails tfidf_model_check; TFIDF_E_NOMEM; *out is zeroed on every error.  This is
 * how a saved model is pruned with no GPU, before tfidf_model_import.  A pruned model needs no
 * options when it is served: the options are not recorded in the model file. */
int tfidf_model_prune(const tfidf_model* in, const tfidf_prune_params* params, tfidf_model* out);

/* --------------------------------------------------------------- weighting -- */

/* Weighting schemes over the resident result of the last run: sublinear tf, smooth idf and L1 /
 * L2 row norms.  tfidf_run always computes the reference's fl(fl(count / docSize) * log(N / df))
 * (TFIDF.c:202,243-244); tfidf_reweight replaces the scores of the resident pairs by another
 * scheme, computed from the integers (count, docSize, df, N), never from the scores it finds.
 *
 * All arithmetic is IEEE binary64, round to nearest; fl() marks every rounding; no product is
 * fused into an add; log is the host's libm log and is never evaluated on the device (the rule
 * the run's idf table follows); (double) of an integer rounds to nearest.
 *
 *   tf(c, ds)   TFIDF_TF_RATIO   fl((double)c / (double)ds)                    TFIDF.c:202
 *               TFIDF_TF_RAW     (double)c
 *               TFIDF_TF_LOG     fl(1.0 + log((double)c))                      sublinear tf
 *               TFIDF_TF_BINARY  1.0
 *   idf(df)     TFIDF_IDF_REF    log(1.0 * N / df): the run's own table entry, its bits
 *               TFIDF_IDF_SMOOTH fl(log(fl(fl((double)N + 1.0) / fl((double)df + 1.0))) + 1.0)
 *               TFIDF_IDF_PLUS1  fl(log(1.0 * N / df) + 1.0)
 *               TFIDF_IDF_NONE   1.0
 *   w(d, t)     fl(tf * idf)
 *   norm        TFIDF_NORM_NONE  score = w
 *               TFIDF_NORM_L2    sq = ((+0.0 + fl(w1*w1)) + fl(w2*w2)) + .. over d's resident pairs
 *                                in pair order (tfidf_similar's sq(d) applied to w); n = sqrt(sq),
 *                                correctly rounded; score = fl(w / n); n == 0: the scores stay w
 *               TFIDF_NORM_L1    s = ((+0.0 + w1) + w2) + ..; score = fl(w / s); s == 0: the
 *                                scores stay w
 * c, ds and df are the resident pair's wordCount, its document's docSize and the run's global df:
 * the integers tfidf_fetch returns; N is the run's ndocs_total.  Every score is >= +0.0 and
 * finite, so bit patterns still order like values (tfidf_query, tfidf_top_terms).  Two static
 * limits keep every score inside the "%.16f" formatter's range [0, 2^63 / 10^16):
 *   - TFIDF_TF_RAW with TFIDF_NORM_NONE is TFIDF_E_INVAL (a raw count times an idf has no bound);
 *   - TFIDF_TF_LOG with TFIDF_NORM_NONE and N >= 2^48 is TFIDF_E_INVAL: below that N the product
 *     stays under (1 + ln 2^32) * (ln 2^48 + 1) < 23.2 * 34.3 < 922; the others stay under 46.
 * `size` is set by the caller to sizeof(tfidf_weighting). */
enum { TFIDF_TF_RATIO = 0, TFIDF_TF_RAW = 1, TFIDF_TF_LOG = 2, TFIDF_TF_BINARY = 3 };
enum { TFIDF_IDF_REF = 0, TFIDF_IDF_SMOOTH = 1, TFIDF_IDF_PLUS1 = 2, TFIDF_IDF_NONE = 3 };
enum { TFIDF_NORM_NONE = 0, TFIDF_NORM_L2 = 1, TFIDF_NORM_L1 = 2 };
typedef struct tfidf_weighting {
    uint64_t size;
    uint32_t tf, idf, norm, reserved;
} tfidf_weighting;
/* Host only.  TFIDF_E_INVAL for: NULL; size < sizeof(tfidf_weighting); an unknown tf, idf or norm
 * value; non-zero reserved; TFIDF_TF_RAW with TFIDF_NORM_NONE.  The limit that depends on N is
 * checked where N is known (tfidf_reweight, tfidf_result_reweight). */
int tfidf_weighting_check(const tfidf_weighting* w);
/* Replaces the scores of the resident pairs by the scheme's.
 *   - reweight(a) then reweight(b) equals reweight(b); {RATIO, REF, NONE} restores the run's bits
 *     exactly; a call whose scheme is already active changes no byte (the formatted text stays
 *     valid);
 *   - tfidf_fetch after the call equals the fetch before it with pair_score replaced; the
 *     formatted text has the same lines with new digits; out_off, terms, counts, df, docSize and
 *     N are untouched; BM25 is unaffected; the norms of tfidf_similar are recomputed;
 *   - the scheme is part of the context's state until the next tfidf_run or tfidf_model_import,
 *     which both reset it to the reference (a run after a prune gives the unpruned result
 *     likewise);
 *   - tfidf_transform follows the active scheme, so transforming the run's own corpus still
 *     reproduces the resident pairs bit for bit: the same tf, idf and w, the norm over the row's
 *     in-vocabulary pairs in pair order; out-of-vocabulary tokens count in doc_size as before;
 *   - on a context that holds only an imported model the call sets the scheme for
 *     tfidf_transform (there are no pairs to rewrite).  The model file does not record the
 *     scheme, as it does not record the analyzer: whoever serves from a model passes it again;
 *   - with tfidf_prune the L1 / L2 norm runs over the pairs resident at the time of the call:
 *     prune then reweight normalises over the kept words (what a vectoriser with a limited
 *     vocabulary does), reweight then prune keeps the bits of the unpruned norm.
 * TFIDF_E_INVAL for a NULL ctx, parameters that fail the check, or TFIDF_TF_LOG with
 * TFIDF_NORM_NONE on N >= 2^48.  TFIDF_E_STATE only when the context holds neither a run nor a
 * model.  TFIDF_E_CAPACITY (TFIDF_TF_LOG) when more than 2^20 pairs hold a count above the
 * tabulated range of 2^16: their list is bounded; no score has been written then.  A failed call
 * leaves the scores as they were: the new ones go into a spare buffer of the context (the one
 * tfidf_prune uses) that changes places with the resident one when every step has succeeded.
 * A repeated run -> reweight sequence allocates nothing after the first (tfidf_alloc_stats).
 * With a communicator attached the call is local: N and df are global and a document's pairs live
 * in one shard, so every shard computes what a single shard would.  No floating-point atomics:
 * the outcome does not depend on the grid or on which of the two launches takes a document. */
int tfidf_reweight(tfidf_ctx* ctx, const tfidf_weighting* params);
/* The active scheme ({RATIO, REF, NONE} after a run or an import).  `out->size` is set by the
 * caller.  TFIDF_E_INVAL for NULL or a short size. */
int tfidf_weighting_get(const tfidf_ctx* ctx, tfidf_weighting* out);
/* The same on every rank of a group at once (one host thread per rank).  After it
 * tfidf_group_write_output, _query, _similar and _transform equal a reweighted single-shard run
 * of the same corpus.  Under a norm tfidf_group_transform lets the ranks transform with the norm
 * off (a rank sees only its own vocabulary's part of a row) and normalises each merged row on the
 * host by the definition above.  Returns the lowest rank's error. */
int tfidf_group_reweight(tfidf_group* g, const tfidf_weighting* params);
/* Counters of the last tfidf_reweight (the caller sets `size` = sizeof, as tfidf_query_info). */
typedef struct tfidf_reweight_info {
    uint64_t size;
    uint32_t tf, idf, norm;   /* the scheme of the call */
    uint32_t changed;         /* 0: the scheme was already active, nothing was written */
    uint64_t npairs;          /* pairs rewritten */
    uint32_t ndocs;
    uint32_t zero_norm_docs;  /* documents that hold pairs and whose L1 / L2 norm is 0 */
    uint64_t nlogs;           /* distinct logs the host computed for this call (idf and tf tables) */
    uint32_t max_count;       /* TFIDF_TF_LOG: the largest wordCount (0 otherwise) */
    uint32_t listed_counts;   /* TFIDF_TF_LOG: distinct counts above the tabulated range */
    uint32_t big_docs;        /* documents the one-workgroup-per-document launch took */
    uint32_t reserved;
    double   ms_tables;       /* device times (HIP events): count maximum, tables, idf by rank */
    double   ms_pairs;        /* the pair pass */
    double   ms_total;        /* host wall time of the whole call */
} tfidf_reweight_info;
int tfidf_last_reweight_info(const tfidf_ctx* ctx, tfidf_reweight_info* info);
/* Host only, plain C (weight_host.c): the same definition on a fetched result.  Rewrites
 * r->pair_score in place from pair_count, pair_docsize, pair_df and ndocs_total; a document is a
 * maximal run of equal pair_doc.  It serves a caller that already holds a fetched result and is
 * the second opinion on the device.  TFIDF_E_INVAL for a NULL argument, parameters that fail the
 * check, the N limit above, or a pair with count, docsize or df of 0 or df > N; the scores are
 * untouched then. */
int tfidf_result_reweight(tfidf_result* r, const tfidf_weighting* w);

/* ---------------------------------------------------------- near duplicates -- */

/* Which documents of the resident result are copies or near-copies of one another: min-wise
 * hashing over each document's term set, LSH bands to propose candidate pairs, and an exact
 * Jaccard verification of every candidate.  With word shingles in front of the run
 * (tfidf_ngrams) a document's set is its shingle set.  All of it is integer arithmetic plus one
 * correctly rounded division; all integers are unsigned and wrap at their width.
 *
 *   mix64(z)    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 *               z ^= z >> 31
 *   S(d)        the terms of document d's resident pairs (after tfidf_prune: the kept words);
 *               counts and scores play no part (tfidf_reweight has no effect); n(d) = |S(d)|
 *   documents   in output order (the "docN@" order, position pos), as in tfidf_kmeans.  A
 *               document with n(d) = 0 takes part in nothing: its signature is all 0xFFFFFFFF,
 *               it is in no candidate pair and it is a group of one
 *   h0(t)       mix64(FNV-1a-64(term bytes)), offset basis 0xCBF29CE484222325 and prime
 *               0x100000001B3 (the model file's): a function of the bytes alone, the same in
 *               every shard and on an imported model
 *   family      from a u64 seed: s = seed; next() = mix64(s += 0x9E3779B97F4A7C15); for
 *               i = 0..H-1 in this order a_i = next() | 1, b_i = (u32)(next() >> 32);
 *               g_i(x) = (u32)((a_i * x mod 2^64) >> 32) + b_i mod 2^32
 *   signature   sig[d][i] = min over t in S(d) of g_i(h0(t)), a u32; 1 <= H <= 256
 *   bands       r rows each, r >= 1, r divides H, b = H / r.  Band key of (d, j), j = 0..b-1:
 *               k = mix64(j + 1); for i = j*r .. j*r + r - 1 in order k = mix64(k ^ sig[d][i])
 *   candidates  for every band j the documents with n(d) >= 1 are ordered by (band key, pos);
 *               each two consecutive documents with equal keys give the candidate
 *               (pos_a, pos_b), pos_a < pos_b: a chain, so m equal documents give m - 1
 *               candidates, never m^2.  C = the union over the bands, as a set; ncand = |C|
 *   verify      for every candidate: shared = the terms S(a) and S(b) have in common (by term
 *               rank), uni = n(a) + n(b) - shared, jaccard = fl((double)shared / (double)uni) (one IEEE binary64 division),
 *               same = the number of i with sig[a][i] == sig[b][i] (same / H is the estimate).
 *               A candidate is kept when jaccard >= threshold (a plain double compare).  The
 *               kept edges are ordered by (pos_a, pos_b)
 *   groups      the connected components of the kept edges over the positions; group[pos] is
 *               the lowest position of its component (the document's own when it is alone)
 *
 * Consequences: every reported pair is exact.  Which pairs become candidates is a deterministic
 * function of (result, H, r, seed).  The chance that a pair of Jaccard s shares a band is the
 * textbook 1 - (1 - s^r)^b; chaining links a bucket's members in position order, and a stranger
 * that collides into a bucket splits the chain, it does not remove it.  Nothing depends on grid,
 * launch shape or budget.  With the defaults (H = 128, r = 4) the S-curve's midpoint is
 * (1/32)^(1/4) ~ 0.42 and a pair at 0.8 is missed with probability (1 - 0.8^4)^32 < 1e-7: that
 * follows from the formula; nothing of it is measured.
 *
 * `size` is set by the caller to sizeof(tfidf_dedup_params).  nhashes == 0 selects the defaults
 * H = 128, r = 4, seed = 1 (rows and seed are ignored then). */
#define TFIDF_MINHASH_MAX_H      256u
#define TFIDF_DEDUP_DEFAULT_H    128u
#define TFIDF_DEDUP_DEFAULT_ROWS 4u
#define TFIDF_DEDUP_DEFAULT_SEED 1ull
typedef struct tfidf_dedup_params {
    uint64_t size;
    uint32_t nhashes;     /* H; 0: the defaults */
    uint32_t rows;        /* r */
    uint64_t seed;
    double   threshold;   /* in [0, 1]; tfidf_minhash checks and ignores it */
} tfidf_dedup_params;
/* Host only.  TFIDF_E_INVAL for: NULL; size < sizeof(tfidf_dedup_params); H > 256; with H != 0
 * r == 0 or r not dividing H; a threshold outside [0, 1] or NaN. */
int tfidf_dedup_check(const tfidf_dedup_params* params);

/* Signatures, row-major ndocs * nhashes, documents in output order.  Arrays are owned by the
 * library and released by tfidf_signatures_free(). */
typedef struct tfidf_signatures {
    uint32_t  ndocs;
    uint32_t  nhashes;
    uint32_t* doc;        /* global id by position */
    uint32_t* npairs;     /* n(d) by position */
    uint32_t* sig;        /* ndocs * nhashes */
} tfidf_signatures;
typedef struct tfidf_dups {
    uint32_t  ndocs;
    uint32_t  ngroups;    /* components of two or more documents */
    uint64_t  ncand;      /* |C| */
    uint64_t  nedges;     /* kept candidates */
    uint32_t* doc;        /* ndocs: global id by position */
    uint32_t* group;      /* ndocs: the lowest position of the document's component */
    /* per kept edge, ordered by (a_pos, b_pos) */
    uint32_t* a_pos;
    uint32_t* b_pos;
    uint32_t* a_doc;
    uint32_t* b_doc;
    uint32_t* shared;
    uint32_t* uni;
    uint32_t* same;
    double*   jaccard;
} tfidf_dups;
/* Over the resident result of the last run, one shard (there is no group form yet; h0 is defined
 * on bytes so that one can be bit-identical).  The result is not disturbed.  The run's corpus
 * must still be valid: the bytes of terms of 16 bytes and more are read from it.  With a
 * communicator attached the call is local.  All device buffers belong to the context: a
 * repeated identical call allocates nothing (tfidf_alloc_stats).  The per-term h0 table (8 bytes
 * per term) is kept until the next tfidf_run, tfidf_prune or tfidf_model_import.
 * TFIDF_E_INVAL: NULL arguments or parameters that fail the check.  TFIDF_E_STATE: before a
 * successful run, and on a context that holds only an imported model.  TFIDF_E_CAPACITY, before
 * any device work: when ndocs * H * 4 (the signatures) plus the bound b * (M - 1) * 16 on the
 * candidate scratch (M = the documents with pairs) exceeds TFIDF_DEDUP_MB MiB (environment, read
 * by tfidf_open; default 1024, a guess that no measurement stands behind), or when b * M does
 * not fit 32 bits.  On an error *out is zeroed. */
int tfidf_minhash(tfidf_ctx* ctx, const tfidf_dedup_params* params, tfidf_signatures* out);
void tfidf_signatures_free(tfidf_signatures* s);
int tfidf_near_dups(tfidf_ctx* ctx, const tfidf_dedup_params* params, tfidf_dups* out);
void tfidf_dups_free(tfidf_dups* d);
/* Counters of the last tfidf_minhash or tfidf_near_dups (the caller sets `size` = sizeof, as
 * tfidf_query_info).  tfidf_minhash leaves the candidate counters and their times 0. */
typedef struct tfidf_dedup_info {
    uint64_t size;
    uint32_t ndocs;
    uint32_t nhashes;
    uint32_t rows;
    uint32_t clusterable;   /* M: documents with n(d) >= 1 */
    uint64_t ncand;
    uint64_t nedges;
    uint32_t ngroups;
    uint32_t big_docs;      /* documents the one-workgroup-per-document signature launch took */
    uint64_t sig_bytes;     /* ndocs * H * 4 */
    uint64_t work_bytes;    /* device scratch of the band and verify stages */
    double   ms_hash;       /* device times (HIP events): the h0 table (0 when it was kept) */
    double   ms_sig;        /* the signature pass */
    double   ms_bands;      /* band keys, sorts, candidates */
    double   ms_verify;     /* the exact intersection */
    double   ms_total;      /* host wall time of the whole call */
} tfidf_dedup_info;
int tfidf_last_dedup_info(const tfidf_ctx* ctx, tfidf_dedup_info* info);
/* Host only, plain C (dedup_host.c): the same definition on a fetched result, the second opinion
 * on the device.  A document's set is the pair_term of its pairs (a document is a maximal run of
 * equal pair_doc); the documents are r->doc_id in "docN@" order, so a document without pairs is
 * there with n(d) = 0; a term's bytes come from the term table.  TFIDF_E_INVAL for NULL
 * arguments, parameters that fail the check, a pair_term outside the term table or a pair_doc
 * that is not among doc_id; *out is zeroed then. */
int tfidf_result_minhash(const tfidf_result* r, const tfidf_dedup_params* params, tfidf_signatures* out);
int tfidf_result_near_dups(const tfidf_result* r, const tfidf_dedup_params* params, tfidf_dups* out);
/* Host only: group[pos] = the lowest position of pos's component under the n edges
 * (a_pos[i], b_pos[i]) over positions 0..ndocs-1, and *ngroups = the components of two or more.
 * The union-find both paths end with.  TFIDF_E_INVAL for a NULL array that is needed or an edge
 * outside the positions. */
int tfidf_dedup_groups(uint32_t ndocs, const uint32_t* a_pos, const uint32_t* b_pos, uint64_t n, uint32_t* group,
                       uint32_t* ngroups);

/* ---------------------------------------------------------------- classify -- */

/* Naive Bayes text classification over the resident result: a fit on the documents the caller
 * labels, then the label of resident documents or of the rows of a tfidf_transform.  Multinomial
 * NB and the complement variant (Rennie et al. 2003).  The features are the pairs' counts, so the
 * sums are integers, exact in any order; every logarithm is the host's libm.  All floating-point
 * arithmetic is IEEE binary64, round to nearest; fl() marks every rounding; no product is fused
 * into an add.  The reference has no such pass.
 *
 *   classes      0..K-1, 1 <= K <= TFIDF_NB_MAX_CLASSES.  The labelled documents are the
 *                (global doc id, class) entries of the parameters; the context's other documents
 *                are unlabelled and take no part in the fit
 *   x(d,t)       the pair's wordCount (TFIDF_NB_COUNT) or 1 (TFIDF_NB_BINARY)
 *   counts       u64, exact: FC[c][t] = the sum of x(d,t) over the documents labelled c;
 *                T[c] = sum_t FC[c][t]; F[t] = sum_c FC[c][t]; Ttot = sum_c T[c];
 *                n_c = the documents labelled c (empty ones included), n = sum_c n_c
 *   smoothing    V = the context's current term count (after a tfidf_prune: the kept terms);
 *                aV = fl(alpha * (double)V)
 *   multinomial  W[c][t] = fl( log(fl((double)FC[c][t] + alpha)) - log(fl((double)T[c] + aV)) )
 *                prior(c) = fl( log((double)n_c) - log((double)n) ), or +0.0 with uniform_prior
 *   complement   W[c][t] = fl( log(fl((double)(Ttot - T[c]) + aV))
 *                             - log(fl((double)(F[t] - FC[c][t]) + alpha)) );  prior(c) = +0.0
 *   score(d,c)   ((prior(c) + fl((double)x1 * W[c][t1])) + fl((double)x2 * W[c][t2])) + ..
 *                over d's pairs in pair order (term-table order); a document without pairs
 *                scores prior(c)
 *   label(d)     the c with the largest score(d,c) by value, the lowest c among equals.  Scores
 *                are finite and of either sign
 * Consequence: a fixed sequence of IEEE operations per (document, class); nothing depends on grid,
 * launch shape or budget, and the device equals the plain-C twin below bit for bit.
 *
 * `size` is set by the caller to sizeof(tfidf_nb_params).  alpha == 0 selects the default 1.0;
 * otherwise it must be finite, > 0 and <= TFIDF_NB_MAX_ALPHA, so that every log argument is
 * positive and finite. */
#define TFIDF_NB_MAX_CLASSES 256u    /* four accumulators per lane of the owner wave, as k-means */
#define TFIDF_NB_MAX_ALPHA   0x1p+900
#define TFIDF_NB_MULTINOMIAL 0u
#define TFIDF_NB_COMPLEMENT  1u
#define TFIDF_NB_COUNT       0u
#define TFIDF_NB_BINARY      1u
#define TFIDF_NB_ALL_SCORES  1u      /* predict flag: also every class's score per row */
#define TFIDF_NO_CLASS       0xFFFFFFFFu
typedef struct tfidf_nb_params {
    uint64_t size;
    uint32_t nclasses;        /* K */
    uint32_t variant;         /* TFIDF_NB_MULTINOMIAL / TFIDF_NB_COMPLEMENT */
    uint32_t feature;         /* TFIDF_NB_COUNT / TFIDF_NB_BINARY */
    uint32_t uniform_prior;   /* non-zero: prior(c) = +0.0 (multinomial; the complement's always is) */
    double   alpha;           /* 0: 1.0 */
    uint64_t nlabelled;
    const uint32_t* doc;      /* nlabelled global document ids */
    const uint32_t* label;    /* nlabelled classes */
} tfidf_nb_params;
/* Host only, no GPU.  TFIDF_E_INVAL for: NULL; size < sizeof(tfidf_nb_params); K == 0 or
 * K > TFIDF_NB_MAX_CLASSES; an unknown variant or feature; an alpha that is NaN, infinite,
 * negative or > TFIDF_NB_MAX_ALPHA; nlabelled >= 2^32, or > 0 with a NULL doc or label; a label
 * >= K; a repeated id; a class without a labelled document. */
int tfidf_nb_check(const tfidf_nb_params* params);

/* The fitted model on the host.  The matrices are term-major like the device's: entry (t, c) is
 * at t * nclasses + c, t = term rank.  Arrays are owned by the library and released by
 * tfidf_nb_model_free(). */
typedef struct tfidf_nb_model {
    uint64_t  size;
    uint32_t  nclasses;       /* K */
    uint32_t  nterms;         /* V */
    uint32_t  variant;
    uint32_t  feature;
    uint32_t  uniform_prior;
    uint32_t  reserved;
    double    alpha;          /* the value used (1.0 for the default) */
    uint64_t  nlabelled;      /* n */
    uint64_t* class_docs;     /* K: n_c */
    uint64_t* class_total;    /* K: T[c] */
    uint64_t* feature_count;  /* V * K: FC */
    double*   prior;          /* K */
    double*   weight;         /* V * K: W */
} tfidf_nb_model;
void tfidf_nb_model_free(tfidf_nb_model* m);

/* Per row the label and its score; with TFIDF_NB_ALL_SCORES scores[r * nclasses + c] as well
 * (NULL otherwise).  A row of a document the context does not hold has pos = UINT32_MAX, label
 * TFIDF_NO_CLASS and scores of +0.0.  Arrays are owned by the library and released by
 * tfidf_nb_labels_free(). */
typedef struct tfidf_nb_labels {
    uint32_t  ndocs;
    uint32_t  nclasses;
    uint32_t* doc;            /* per row: global document id (tfidf_nb_predict); the row's index (the row calls) */
    uint32_t* pos;            /* per row: output position, as tfidf_doc_terms.pos; the row's index (the row calls) */
    uint32_t* label;
    double*   score;          /* score(d, label(d)) */
    double*   scores;         /* ndocs * nclasses, or NULL */
} tfidf_nb_labels;
void tfidf_nb_labels_free(tfidf_nb_labels* l);

/* Fits the model over the resident result of the last run, in HBM; it stays in the context until
 * the next tfidf_run, tfidf_prune or tfidf_model_import (term ranks change there) or the next
 * tfidf_nb_fit.  tfidf_reweight keeps it: the model reads counts only.  One shard; with a
 * communicator attached the call is local.  The run's result is not disturbed.
 * TFIDF_E_INVAL: NULL arguments, parameters that fail tfidf_nb_check, an id the context does not
 * hold.  TFIDF_E_STATE: before a successful run, and on a context that holds only an imported
 * model.  TFIDF_E_CAPACITY, before any device work: when the two dense matrices (FC as u64, W as
 * f64, both [V][K] with 64-bit offsets) and the per-term and per-class words exceed TFIDF_NB_MB
 * MiB (environment, read by tfidf_open; default 1024, a guess that nobody has measured).  All
 * device buffers belong to the context: a repeated identical call allocates nothing
 * (tfidf_alloc_stats).  A call refused by the check, the state or the budget leaves an earlier
 * model in place; one that fails later (an id the context does not hold, a device error) leaves
 * the context without a model. */
int tfidf_nb_fit(tfidf_ctx* ctx, const tfidf_nb_params* params);
/* Labels of resident documents, with the row rules of tfidf_top_terms: doc_ids == NULL gives one
 * row per document in output order (ndocs is ignored); otherwise one row per entry in the
 * caller's order, duplicates allowed.  TFIDF_E_STATE without a fitted model; TFIDF_E_INVAL for
 * NULL ctx or out or unknown flag bits.  On an error *out is zeroed. */
int tfidf_nb_predict(tfidf_ctx* ctx, const uint32_t* doc_ids, uint32_t ndocs, uint32_t flags, tfidf_nb_labels* out);
/* Labels of the rows of a tfidf_transform of this context: row_off, term and count are uploaded
 * (the call is independent of transform's slices); df, score and the words are not read.
 * TFIDF_E_INVAL for a non-monotone row_off, row_off[0] != 0, row_off[ndocs] != npairs or a term >= V (a merged
 * tfidf_group_transform carries UINT32_MAX and is refused). */
int tfidf_nb_predict_rows(tfidf_ctx* ctx, const tfidf_rows* rows, uint32_t flags, tfidf_nb_labels* out);
/* The fitted model copied to the host.  TFIDF_E_STATE without one. */
int tfidf_nb_export(tfidf_ctx* ctx, tfidf_nb_model* out);
/* Counters of the last tfidf_nb_fit, with the times of the last predict call added (the caller
 * sets `size` = sizeof, as tfidf_query_info). */
typedef struct tfidf_nb_info {
    uint64_t size;
    uint32_t nclasses;
    uint32_t nterms;
    uint64_t nlabelled;
    uint64_t matrix_bytes;    /* FC + W */
    uint64_t nlogs;           /* log() calls of the fit, all on the host */
    uint64_t nlisted;         /* distinct log arguments above the table (the sorted list) */
    uint32_t predict_rows;    /* rows of the last predict call */
    uint32_t reserved;
    double   ms_logs_host;    /* host time of the fit's logs */
    double   ms_count;        /* device times (HIP events): the count pass and its reductions */
    double   ms_weights;      /* the weight pass */
    double   ms_predict;      /* the last predict call's kernel */
    double   ms_total;        /* host wall time of the fit */
} tfidf_nb_info;
int tfidf_last_nb_info(const tfidf_ctx* ctx, tfidf_nb_info* info);
/* Host only, plain C (nb_host.c): the same definition, the second opinion on the device.
 * tfidf_result_nb_fit reads a fetched result: a document is a maximal run of equal pair_doc, its
 * feature values pair_count, V = r->nterms, the documents r->doc_id.  TFIDF_E_INVAL for NULL
 * arguments, parameters that fail the check, a labelled id that is not among doc_id, a pair_term
 * outside the term table or a pair_doc that is not among doc_id; *out is zeroed then.
 * tfidf_nb_model_predict scores nrows rows (row r = pairs [row_off[r], row_off[r + 1]) of term and
 * count) against a model, from tfidf_nb_export or tfidf_result_nb_fit; doc and pos of the answer
 * are the row's index.  TFIDF_E_INVAL for NULL arguments, a model without its arrays, a
 * non-monotone row_off or a term >= nterms. */
int tfidf_result_nb_fit(const tfidf_result* r, const tfidf_nb_params* params, tfidf_nb_model* out);
int tfidf_nb_model_predict(const tfidf_nb_model* m, uint32_t nrows, const uint64_t* row_off, const uint32_t* term,
                           const uint32_t* count, uint32_t flags, tfidf_nb_labels* out);

/* ------------------------------------------------------------ term matching -- */

/* Fuzzy and prefix matching of patterns against the resident term dictionary: the term
 * expansion a retrieval engine answers `recieve` and `connect*` with.  A pattern is matched
 * against every term of the context's table; its best few matches, by edit distance and then by
 * document frequency, are returned with their words and can stand in for it in an ordinary
 * query.  The reference has no such pass.  Everything is integer arithmetic on BYTES: there are
 * no code points here, a two-byte UTF-8 letter is two bytes of distance.
 *
 *   pattern      p = bytes[p_off[p], p_off[p + 1]) (host pointers), 1..TFIDF_MATCH_MAX_PATTERN
 *                bytes of any value; kind[p] is TFIDF_MATCH_FUZZY or TFIDF_MATCH_PREFIX;
 *                max_edits[p] <= TFIDF_MATCH_MAX_EDITS is the budget of a fuzzy pattern and is
 *                ignored for a prefix pattern
 *   prefix       term t matches when len(t) >= len(p) and t's first len(p) bytes equal p;
 *                dist = 0
 *   fuzzy        term t matches when the first min(fixed_prefix, len(p)) bytes of p equal t's
 *                (so t has at least that many) and dist(p, t) <= max_edits[p]
 *   dist         the Levenshtein distance (insert, delete, substitute one byte); with
 *                TFIDF_MATCH_TRANSPOSE in flags the optimal-string-alignment distance: an
 *                adjacent transposition is one edit too, and no substring is edited twice.
 *                "ab" -> "ba" is 1 with the flag and 2 without; "ca" -> "abc" is 3 with it
 *                (not the 2 of the unrestricted Damerau distance)
 *   empty term   a term like any other: it matches a fuzzy pattern of length <= max_edits[p]
 *   order        dist ascending, then df descending (the global df), then term-table order
 *                ascending (= rank ascending = strcmp of "word\t").  Ranks are unique: the order
 *                is total and the result unique
 *   cut          the first max_expansions matches are returned
 * Nothing depends on grid, pattern grouping, batch cut or list capacity. */
#define TFIDF_MATCH_MAX_PATTERN    64u      /* bytes */
#define TFIDF_MATCH_MAX_EDITS      2u
#define TFIDF_MATCH_MAX_EXPANSIONS 1024u
#define TFIDF_MATCH_MAX_PATTERNS   65536u
#define TFIDF_MATCH_FUZZY  0u
#define TFIDF_MATCH_PREFIX 1u
#define TFIDF_MATCH_TRANSPOSE 1u            /* flags: an adjacent transposition is one edit */
typedef struct tfidf_patterns {
    const uint8_t*  bytes;
    uint64_t        nbytes;
    const uint64_t* p_off;       /* npatterns + 1 entries, non-decreasing, p_off[npatterns] <= nbytes */
    uint32_t        npatterns;
    const uint8_t*  kind;        /* npatterns: TFIDF_MATCH_FUZZY / TFIDF_MATCH_PREFIX */
    const uint8_t*  max_edits;   /* npatterns: 0..TFIDF_MATCH_MAX_EDITS (fuzzy patterns) */
} tfidf_patterns;
typedef struct tfidf_match_params {
    uint64_t size;               /* sizeof(tfidf_match_params), set by the caller */
    uint32_t max_expansions;     /* E: 1..TFIDF_MATCH_MAX_EXPANSIONS */
    uint32_t flags;              /* TFIDF_MATCH_TRANSPOSE or 0 */
    uint32_t fixed_prefix;       /* 0..TFIDF_MATCH_MAX_PATTERN: leading bytes a fuzzy match must share */
    uint32_t reserved;
    uint64_t list_records;       /* capacity of the device match list in records; 0: the default
                                    (262144), else >= 1024.  A field, not an environment knob */
} tfidf_match_params;
/* Rows laid out like tfidf_doc_terms.  Arrays are owned by the library and released by
 * tfidf_term_matches_free(). */
typedef struct tfidf_term_matches {
    uint32_t  npatterns, k;  /* rows, row stride (= max_expansions) */
    uint64_t* nmatch;        /* per pattern: matching terms (all, before the cut) */
    uint32_t* nterms;        /* per pattern: min(k, nmatch) */
    uint32_t* term;          /* npatterns * k, row p at p * k: term rank (UINT32_MAX from a group) */
    uint8_t*  dist;          /* same layout */
    uint32_t* df;            /* same layout: global df */
    uint64_t* word_off;      /* npatterns * k + 1: entry p * k + j is bytes [word_off[..], word_off[.. + 1]); unused entries empty */
    uint8_t*  word_bytes;    /* the matched words' bytes, gathered on the device */
} tfidf_term_matches;
/* Host only, no GPU.  TFIDF_E_INVAL for: a NULL argument; params->size < sizeof(tfidf_match_params);
 * max_expansions == 0 or > TFIDF_MATCH_MAX_EXPANSIONS; unknown flag bits; fixed_prefix >
 * TFIDF_MATCH_MAX_PATTERN; list_records in 1..1023; npatterns > TFIDF_MATCH_MAX_PATTERNS;
 * with npatterns > 0 a NULL p_off, kind or max_edits, a non-monotone p_off or
 * p_off[npatterns] > nbytes; a pattern of 0 or more than TFIDF_MATCH_MAX_PATTERN bytes; an
 * unknown kind; a fuzzy pattern's max_edits > TFIDF_MATCH_MAX_EDITS. */
int tfidf_match_check(const tfidf_patterns* patterns, const tfidf_match_params* params);
/* Matches every pattern against the context's term table in HBM: the table of the last run (after
 * a tfidf_prune: the kept terms and their df) or of an imported model (the call needs the
 * dictionary alone, so it works on a model-only context).  TFIDF_E_INVAL for NULL arguments or
 * what tfidf_match_check refuses; TFIDF_E_STATE when the context holds neither a result nor a
 * model; on an error *out is zeroed.  npatterns == 0 is valid.  The result is not disturbed;
 * the run's corpus must still be valid, as for tfidf_format (long terms' bytes are read from
 * it).  With a communicator attached the call is local: this shard's table with the global df.
 * The patterns are scanned in groups of 64, one pass over the table per group; matches go to a
 * device list of list_records records (40 bytes each).  A group whose matches exceed it is
 * scanned again in batches of patterns whose exact counts fit, and for one pattern with more
 * matches than the capacity the list grows once to that count, which is at most V.  The
 * buffers belong to the context: a repeated identical call allocates nothing
 * (tfidf_alloc_stats). */
int tfidf_match_terms(tfidf_ctx* ctx, const tfidf_patterns* patterns, const tfidf_match_params* params,
                      tfidf_term_matches* out);
void tfidf_term_matches_free(tfidf_term_matches* m);
/* The same over every shard of a group (tfidf_group_run): every rank matches its own table on its
 * own host thread, the host merges the ranks' rows by (dist, df descending, "word\t" ascending)
 * and keeps a word several ranks hold once.  A term has the same dist and the same global df in
 * every shard that holds it, so the merged first E of the ranks' first E are the first E of the
 * corpus-wide dictionary.  term is UINT32_MAX (there is no common table); nmatch[p] is the
 * largest of the ranks' counts, a lower bound of the corpus-wide count that is exact with one
 * shard (with several, the merged row may hold more words than one rank counted: nterms[p] is the
 * row's length, at most E). */
int tfidf_group_match_terms(tfidf_group* g, const tfidf_patterns* patterns, const tfidf_match_params* params,
                            tfidf_term_matches* out);
/* Host only, plain C (match_host.c): the same definition over a model struct, the second opinion
 * on the device; term is the index into the model's table.  TFIDF_E_INVAL for NULL arguments,
 * what tfidf_match_check refuses or a model that fails tfidf_model_check; *out is zeroed then. */
int tfidf_model_match_terms(const tfidf_model* m, const tfidf_patterns* patterns, const tfidf_match_params* params,
                            tfidf_term_matches* out);
/* Counters of the last tfidf_match_terms (the caller sets `size` = sizeof, as tfidf_query_info). */
typedef struct tfidf_match_info {
    uint64_t size;
    uint32_t npatterns, k;
    uint32_t ngroups;         /* scans of the table (a group that overflowed is scanned again per batch) */
    uint32_t nbatches;        /* selections: a sort of the list, the cut and the word gather */
    uint64_t nrecords;        /* matches written to the list by the scans that were selected from */
    uint64_t list_records;    /* the capacity the call ended with */
    double   ms_scan;         /* device times (HIP events), summed */
    double   ms_select;
    double   ms_words;
    double   ms_total;        /* host wall time of the whole call */
} tfidf_match_info;
int tfidf_last_match_info(const tfidf_ctx* ctx, tfidf_match_info* info);

/* ---------------------------------------------------------------- snippets -- */

/* Best passage and match marks for (query, document) jobs: where in a hit the query matched, and
 * the window of W tokens a result page would show.  The run's corpus is still resident (the term
 * table points into it), so positions are found on demand in the documents that were hit; the run
 * stores none and there is no inverted index.  The reference has no such pass.  Everything is a
 * comparison of bytes and integer arithmetic: the result is defined exactly.
 *
 *   tokens       a document's tokens t_0 .. t_{T-1} are those of tfidf_corpus: maximal runs of
 *                bytes not in {0x20,0x09..0x0D} inside the document (a document boundary is a token
 *                boundary); a token's term is its bytes up to its first NUL; a token beginning with
 *                NUL has the empty term, which is a term.  T = the run's doc_size of the document
 *   query terms  query q is tokenised as tfidf_query does.  U(q) = its distinct terms in order of
 *                first occurrence; the first TFIDF_SNIP_MAX_TERMS are used, and when there are more
 *                every job of q carries TFIDF_SNIP_TRUNCATED.  A term of U is found when the
 *                resident vocabulary holds it (a term of >= 16 bytes only when the bytes are equal,
 *                the rule of tfidf_query); only found terms match, so a word removed by tfidf_prune
 *                no longer marks.  A term's slot is its index in U, found or not: the result does
 *                not depend on which shard holds the document
 *   jobs         njobs <= TFIDF_SNIP_MAX_JOBS pairs (job_query[j], job_doc[j]), the second a global
 *                document id; any order, repeats allowed.  A document this context does not hold
 *                gives the job TFIDF_SNIP_NO_DOC and zeros in every other field
 *   matches      token i matches when its term equals a found u_s; then slot(i) = s
 *   window       W = params.window.  For a start s the window is the tokens [s, min(s + W, T));
 *                cover(s) = the distinct slots among its matches, hits(s) = its matches.  The
 *                candidates are the match positions (any window can be moved right to its first
 *                match without losing one).  The chosen start maximises (cover, hits), cover first;
 *                ties go to the smallest s
 *   centring     last = the chosen window's last match position, span = last - s + 1,
 *                slack = W - span: s' = s - min(s, slack / 2) (integer division),
 *                e' = min(s' + W, T).  The final window is [s', e'); cover and hits are counted
 *                again over it (centring can bring in a match on the left).  A document without a
 *                match gets s' = 0, e' = min(W, T), cover = hits = 0; T = 0 gives zeros
 *   win_byte     offsets relative to the document's first byte: the first byte of token s', and the
 *                first byte of token e' or, when e' = T, the document's length (the text may end in
 *                whitespace; trimming is the caller's)
 *   marks        the first min(max_marks, hits) matches of the final window in position order, each
 *                (byte offset relative to the document, the term's length, slot)
 *   text         with TFIDF_SNIP_TEXT the window's bytes, as the counter saw them
 * Nothing depends on grid, batch cut or scratch budget. */
#define TFIDF_SNIP_MAX_TERMS  256u
#define TFIDF_SNIP_MAX_JOBS   (1u << 20)
#define TFIDF_SNIP_MAX_WINDOW 1024u
#define TFIDF_SNIP_MAX_MARKS  1024u
#define TFIDF_SNIP_TEXT       1u            /* params.flags: copy the windows' bytes */
#define TFIDF_SNIP_NO_DOC     1u            /* job flags: the context does not hold the document */
#define TFIDF_SNIP_TRUNCATED  2u            /* job flags: the query has more than TFIDF_SNIP_MAX_TERMS distinct terms */
#define TFIDF_SNIP_MIN_SCRATCH 65536ull
typedef struct tfidf_snippet_params {
    uint64_t size;               /* sizeof(tfidf_snippet_params), set by the caller */
    uint32_t window;             /* W: 1..TFIDF_SNIP_MAX_WINDOW */
    uint32_t max_marks;          /* M: 0..TFIDF_SNIP_MAX_MARKS */
    uint32_t flags;              /* TFIDF_SNIP_TEXT or 0 */
    uint32_t reserved;
    uint64_t scratch_bytes;      /* device scratch of a batch of jobs (tile words + match records);
                                    0: the default (256 MiB), else >= TFIDF_SNIP_MIN_SCRATCH.  A
                                    field, not an environment knob */
} tfidf_snippet_params;
/* Arrays are owned by the library and released by tfidf_snippets_free(). */
typedef struct tfidf_snippets {
    uint32_t  njobs, nqueries;
    /* per job */
    uint32_t* flags;           /* TFIDF_SNIP_NO_DOC | TFIDF_SNIP_TRUNCATED */
    uint32_t* ntokens;         /* T */
    uint32_t* nmatch;          /* matches in the whole document */
    uint32_t* nterms_matched;  /* distinct slots in the whole document */
    uint32_t* win_tok;         /* 2 * njobs: (s', e') */
    uint64_t* win_byte;        /* 2 * njobs */
    uint32_t* cover;           /* of the final window */
    uint32_t* hits;
    uint64_t* mark_off;        /* njobs + 1: job j's marks are [mark_off[j], mark_off[j + 1]) */
    uint64_t* mark_byte;
    uint32_t* mark_len;
    uint32_t* mark_slot;
    uint64_t* text_off;        /* njobs + 1 (all 0 without TFIDF_SNIP_TEXT) */
    uint8_t*  text;
    /* per query: its used terms, U(q) cut at TFIDF_SNIP_MAX_TERMS; a term's slot is its index here */
    uint64_t* qterm_off;       /* nqueries + 1 */
    uint64_t* qterm_pos;       /* the term's offset inside the query's bytes */
    uint32_t* qterm_len;
    uint8_t*  qterm_found;
} tfidf_snippets;
void tfidf_snippets_free(tfidf_snippets* s);
/* Host only, no GPU.  TFIDF_E_INVAL for: NULL; size < sizeof(tfidf_snippet_params); window == 0 or
 * > TFIDF_SNIP_MAX_WINDOW; max_marks > TFIDF_SNIP_MAX_MARKS; unknown flag bits; scratch_bytes in
 * 1..TFIDF_SNIP_MIN_SCRATCH-1. */
int tfidf_snippets_check(const tfidf_snippet_params* params);
/* Snippets of njobs jobs over the resident corpus of the last run.  TFIDF_E_STATE before a
 * successful tfidf_run and on a model-only context (it has no corpus); TFIDF_E_INVAL for a NULL
 * argument (job arrays may be NULL when njobs == 0), what tfidf_snippets_check refuses, bad queries
 * as tfidf_query, njobs > TFIDF_SNIP_MAX_JOBS or a job_query[j] >= nqueries; on an error *out is
 * zeroed.  The resident result is not disturbed and the run's corpus must still be valid, as for
 * tfidf_query.  With a communicator attached the call is local.  The documents are scanned in
 * tiles of 4096 bytes, so one long document spreads over the whole GPU; jobs go in batches whose
 * tile words and match records fit scratch_bytes (one job larger than that grows the buffer once
 * to its size).  The buffers belong to the context: a repeated identical call allocates nothing
 * (tfidf_alloc_stats). */
int tfidf_snippet(tfidf_ctx* ctx, const tfidf_queries* queries, const uint32_t* job_query, const uint32_t* job_doc,
                  uint32_t njobs, const tfidf_snippet_params* params, tfidf_snippets* out);
/* The same over every shard of a group (tfidf_group_run): every rank gets the whole job list on its
 * own host thread and answers TFIDF_SNIP_NO_DOC for what it does not hold; the host takes each job
 * from the rank that held it.  Slots index U(q), so the merged result equals a single shard's field
 * for field; a query term counts as found when any rank found it. */
int tfidf_group_snippet(tfidf_group* g, const tfidf_queries* queries, const uint32_t* job_query, const uint32_t* job_doc,
                        uint32_t njobs, const tfidf_snippet_params* params, tfidf_snippets* out);
/* Host only, plain C (snippet_host.c): the definition over a fetched result and the host corpus the
 * run had (host pointers; doc_ids NULL means 1..ndocs), the second opinion on the device.  A term
 * is found by binary search in the result's term table.  Errors as tfidf_snippet, without the
 * state checks. */
int tfidf_result_snippet(const tfidf_result* r, const tfidf_corpus* host_corpus, const tfidf_queries* queries,
                         const uint32_t* job_query, const uint32_t* job_doc, uint32_t njobs,
                         const tfidf_snippet_params* params, tfidf_snippets* out);
/* Counters of the last tfidf_snippet (the caller sets `size` = sizeof, as tfidf_query_info). */
typedef struct tfidf_snippet_info {
    uint64_t size;
    uint32_t njobs;
    uint32_t nbatches;        /* count passes (batches of jobs by tiles) */
    uint32_t nsubbatches;     /* write / select / emit passes (cuts by match records) */
    uint32_t nbig;            /* jobs whose candidates took more than one select slice */
    uint64_t ntiles;
    uint64_t nbytes;          /* document bytes scanned by the count passes */
    uint64_t ntokens;
    uint64_t nmatches;
    uint64_t scratch_bytes;   /* the budget the call ended with (grown for one job larger than it) */
    double   ms_lookup;       /* device times (HIP events), summed */
    double   ms_count;
    double   ms_write;
    double   ms_select;
    double   ms_emit;
    double   ms_total;        /* host wall time of the whole call */
} tfidf_snippet_info;
int tfidf_last_snippet_info(const tfidf_ctx* ctx, tfidf_snippet_info* info);

/* ---------------------------------------------------------------- ingest ---- */

/* Reference input contract (TFIDF.c:98-110,130-147): N = number of entries of `dir`
 * other than "." and ".."; documents are dir/doc1 .. dir/docN.  Reads them into one
 * malloc'd buffer with doc_off[N+1].  Returns TFIDF_E_NOINPUT / TFIDF_E_NODOC
 * (with *bad_doc set) like the reference's error exits. */
int tfidf_ingest_dir(const char* dir, uint8_t** bytes, uint64_t* nbytes,
                     uint64_t** doc_off, uint32_t* ndocs, uint32_t* bad_doc);
void tfidf_free(void* p);

/* Streaming ingest into HBM (replaces TFIDF.c:98-110,130-147): the
 * same contract as tfidf_ingest_dir (N = entries of `dir` other than "." and "..";
 * documents dir/doc1..docN; TFIDF_E_NOINPUT / TFIDF_E_NODOC with *bad_doc = the smallest
 * document that cannot be read), but the files are pread() by `nthreads` host threads
 * (0: OMP_NUM_THREADS, at most 16) into a ring of pinned 8 MiB segments whose H2D copies
 * overlap the reads.  *out is a device corpus (TFIDF_CORPUS_DEVICE, doc ids 1..N) owned
 * by the context, valid until the next ingest, host-corpus tfidf_run or tfidf_close.
 * `info` (optional) receives sizes and host wall times. */
typedef struct tfidf_ingest_info {
    uint64_t nbytes;      /* corpus bytes */
    uint64_t segments;    /* 8 MiB staging segments copied */
    uint32_t ndocs;       /* N */
    uint32_t threads;     /* reader threads used */
    double   ms_scan;     /* directory count + open/fstat of every document */
    double   ms_read;     /* reads + overlapped H2D, until the last copy completed */
    double   ms_total;
} tfidf_ingest_info;
int tfidf_ingest_dir_device(tfidf_ctx* ctx, const char* dir, int nthreads, tfidf_corpus* out,
                            uint32_t* bad_doc, tfidf_ingest_info* info);

/* Byte-balanced shard plan of an input directory (replaces the round-robin
 * document -> rank deal of TFIDF.c:125-130).  One scan gives N (every entry but "." and
 * "..", TFIDF.c:98-110) and the sizes of doc1..docN (TFIDF.c:130-138 error contract:
 * TFIDF_E_NOINPUT, TFIDF_E_NODOC with *bad_doc = the smallest missing id).  Documents are
 * ordered by "docN@" (the output's strcmp order, TFIDF.c:49,273) and cut into nshards
 * contiguous ranges at the cuts nearest to r * total / nshards, so every shard holds at
 * most total / nshards + the largest document and the shards' outputs concatenate in
 * shard order.  Release with tfidf_plan_free. */
typedef struct tfidf_dir_plan {
    uint32_t  ndocs;         /* N */
    uint32_t  nshards;
    uint32_t* doc_ids;       /* N document ids in "docN@" order */
    uint64_t* doc_bytes;     /* their sizes */
    uint32_t* shard_first;   /* nshards + 1: shard r = doc_ids[shard_first[r] .. shard_first[r + 1]) */
    uint64_t* shard_bytes;   /* nshards */
} tfidf_dir_plan;
int tfidf_plan_dir(const char* dir, uint32_t nshards, int nthreads, tfidf_dir_plan* plan, uint32_t* bad_doc);
void tfidf_plan_free(tfidf_dir_plan* plan);
/* Streams shard `shard` of the plan into the context's HBM like tfidf_ingest_dir_device;
 * the corpus carries the documents' global ids (device) and ndocs_total = N. */
int tfidf_ingest_shard_device(tfidf_ctx* ctx, const char* dir, const tfidf_dir_plan* plan, uint32_t shard,
                              int nthreads, tfidf_corpus* out, uint32_t* bad_doc, tfidf_ingest_info* info);
/* The plan's pieces on their own (host only): ids 1..n in "docN@" order, and the
 * byte-balanced cut of a sequence of sizes (first[nshards + 1]). */
int tfidf_doc_name_order(uint32_t n, uint32_t* ids);
int tfidf_shard_split(const uint64_t* bytes, uint32_t n, uint32_t nshards, uint32_t* first);

/* ---------------------------------------------------------------- synthetic - */

/* Synthetic Zipfian corpus (generator in csrc/synth.h).  ntok[i] tokens
 * in local document i whose global id is doc_ids[i]; cdf = Zipf CDF over V ranks
 * (zipf mode) or NULL (mode 1: config-1 "4 words per doc").  Host version fills
 * caller-provided buffers (query the size first with bytes == NULL). */
int tfidf_synth_host(uint64_t seed, uint32_t V, uint32_t mode, const double* cdf,
                     const uint32_t* doc_ids, const uint64_t* ntok, uint32_t ndocs,
                     uint8_t* bytes, uint64_t* nbytes, uint64_t* doc_off);
/* Device version: generates straight into HBM buffers owned by the ctx and returns a
 * device corpus (flags = TFIDF_CORPUS_DEVICE) valid until the next synth call or
 * tfidf_close. */
int tfidf_synth_device(tfidf_ctx* ctx, uint64_t seed, uint32_t V, uint32_t mode,
                       const double* cdf, const uint32_t* doc_ids, const uint64_t* ntok,
                       uint32_t ndocs, uint64_t ndocs_total, tfidf_corpus* out);

#ifdef __cplusplus
}
#endif
#endif /* TFIDF_H */
