/*
 * xport.h — the collectives of the DF exchange, behind one small interface.
 *
 * The reference combines per-rank DF with MPI_Reduce(CustomReduce) + MPI_Bcast
 * (TFIDF.c:209-222,291-326) between OS processes.  Here a context (one GPU shard) talks
 * to its peers through an Xport:
 *
 *   RcclXport   ncclAllGather / ncclAllReduce / grouped ncclSend-ncclRecv over xGMI: one
 *               communicator rank per GPU,
 *               either one process per GPU (tfidf_comm_init, torch.distributed launch) or
 *               one process driving every GPU (tfidf_group_open, ncclCommInitAll).
 *   LocalXport  contexts of one process that share a device (tfidf_group_open with a
 *               device listed twice, e.g. K shards on the 1-GPU test box): the same
 *               operations as device-to-device copies between the contexts' buffers, with
 *               host barriers.  The engine code above the interface is identical, so the
 *               owner partition / aggregate / reply kernels and the status agreement run
 *               unchanged with K > 1 ranks on one GPU.
 *
 * Every operation is collective: all ranks call it in the same order.  `words` is the
 * host-level agreement step (status + sizes), the device operations are stream-ordered.
 */
#ifndef TFIDF_XPORT_H
#define TFIDF_XPORT_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

struct tfidf_ctx;
struct tfidf_queries;
struct tfidf_hits;

struct Xport {
    int rank = 0, nranks = 1;
    virtual ~Xport() {}
    /* host all-gather of two u64 per rank: all[2 * r + k] = rank r's mine[k] */
    virtual int words(const uint64_t mine[2], uint64_t* all, hipStream_t s) = 0;
    /* device all-gather: recv[r * bytes ...] = rank r's send[0 .. bytes) */
    virtual int allgather(const void* send, void* recv, size_t bytes, hipStream_t s) = 0;
    /* device all-to-all with per-peer counts of `eb`-byte elements (host arrays of nranks):
     * this rank's elements for peer p are send[so[p] .. so[p] + scnt[p]) and peer p's for
     * this rank land at recv[ro[p] ..), so, ro the exclusive prefix sums of scnt, rcnt
     * (rcnt[p] must equal peer p's scnt[rank]) */
    virtual int alltoallv(const void* send, const uint64_t* scnt, void* recv, const uint64_t* rcnt, size_t eb,
                          hipStream_t s) = 0;
    /* device all-reduce (sum) of n u32 in place: the dense DF exchange's one collective */
    virtual int allreduce_u32(uint32_t* buf, size_t n, hipStream_t s) = 0;
    /* waits for the stream's work, collectives among it.  RcclXport polls, so that an abort
     * of the clique releases a rank waiting for a failed peer's part (TFIDF_E_PEER) */
    virtual int wait(hipStream_t s) { return hipStreamSynchronize(s) == hipSuccess ? 0 : -3 /* TFIDF_E_HIP */; }
    /* a rank failed between collectives: release the peers (they return errors) */
    virtual void abort() = 0;
    virtual const char* name() const = 0;
};

/* engine.cpp: attach (and take ownership of) an Xport; nullptr detaches */
int tfidf_ctx_attach_xport(tfidf_ctx* ctx, Xport* xp);
int tfidf_ctx_device(const tfidf_ctx* ctx);
hipStream_t tfidf_ctx_stream(const tfidf_ctx* ctx);
/* engine_query.cpp: tfidf_query that also reports which query terms the shard's vocabulary holds:
 * found[found_off[q] + i] for the i-th distinct term of query q in first-occurrence order
 * (the same numbering on every rank: tfidf_group_query counts a term found by any rank once) */
struct Bm25Call;
struct ClausePlan;
int tfidf_ctx_query(tfidf_ctx* ctx, const tfidf_queries* queries, uint32_t k, tfidf_hits* out,
                    std::vector<uint8_t>* found, std::vector<uint64_t>* found_off, const Bm25Call* bm = nullptr,
                    const ClausePlan* clauses = nullptr);
/* engine_query.cpp: tfidf_query_clauses is tfidf_ctx_query with a clause plan (`queries` is then
 * unused): the three texts of a checked tfidf_clauses.  The numbering behind found / found_off is
 * per query the must text's terms, then the should text's, then the terms that are only in the
 * must_not text (never found: they are no scoring terms).  The counters go to
 * tfidf_last_clause_info. */
struct ClausePlan {
    uint32_t nqueries;
    const tfidf_queries *must, *should, *must_not;   /* null: empty in every query */
    const uint32_t* min_should;                      /* or null */
};
/* the plan and the BM25 call (*has_bm) of checked clauses; TFIDF_E_INVAL as tfidf_clauses_check */
int tfidf_clause_plan(const tfidf_clauses* c, ClausePlan* plan, Bm25Call* bm, bool* has_bm);
/* engine_query.cpp: tfidf_query_bm25 is tfidf_ctx_query with validated parameters (bm non-null: the
 * scoring pass is bm25.hip's, the counters go to tfidf_last_bm25_info).  avgdl 0: this
 * context's own average */
struct Bm25Call {
    double k1, b, avgdl;
};
/* TFIDF_E_INVAL unless params (NULL: the defaults) are as include/tfidf.h requires */
int tfidf_bm25_params_check(const tfidf_bm25_params* params, Bm25Call* out);
/* L = the exact sum of docSize over the context's documents, n = the documents it holds */
int tfidf_ctx_bm25_lengths(tfidf_ctx* ctx, uint64_t* L, uint64_t* n);

/* engine_similar.cpp: the two halves of tfidf_group_similar on one shard.  Export: the rows' documents
 * as this shard holds them (pos UINT32_MAX: it does not; the row is empty): row i's vector is
 * entries [voff[i], voff[i + 1]) of (word, score), word x = wbytes[woff[x], woff[x + 1]), in
 * term-table order.  Search: this shard's neighbours of rows given that way (id, norm, voff,
 * woff, wbytes, score): the words are resolved in the shard's own vocabulary, the row's own
 * document is found by its id; fills nmatch, nnb and nb_* of `out` (rows in the given order). */
struct SimExport {
    std::vector<uint32_t> id, pos;
    std::vector<uint64_t> npairs, voff, woff;
    std::vector<double> norm, score;
    std::vector<uint8_t> wbytes;
};
int tfidf_ctx_similar_export(tfidf_ctx* ctx, const uint32_t* doc_ids, uint32_t ndocs, SimExport* e);
int tfidf_ctx_similar_ext(tfidf_ctx* ctx, const SimExport* rows, uint32_t k, tfidf_neighbors* out);

/* weight_host.c (plain C): the pieces of the weighting definition the engine's tables and the
 * group transform share with tfidf_result_reweight */
extern "C" {
int tfidf_weighting_check_n(const tfidf_weighting* w, uint64_t ndocs_total);   /* the check plus the limit that needs N */
double tfidf_weight_tf_log(uint32_t c);                                        /* fl(1.0 + log((double)c)) */
double tfidf_weight_idf(uint32_t mode, uint64_t N, uint32_t df);
int tfidf_weight_normalize(double* w, uint64_t n, uint32_t norm);              /* one row in place; 1: the norm is 0 */
}
/* engine_transform.cpp: tfidf_transform is tfidf_ctx_transform with norm = true.  norm = false leaves the
 * active scheme's row norm out (w is returned): tfidf_group_transform normalises the merged rows */
struct tfidf_corpus;
struct tfidf_rows;
int tfidf_ctx_transform(tfidf_ctx* ctx, const tfidf_corpus* batch, tfidf_rows* out, bool norm);

/* group.cpp */
/* a process-per-GPU rank: non-blocking ncclCommInitRankConfig with the job's unique id */
int rccl_init_rank(const void* unique_id, int rank, int nranks, int device, Xport** out);

#endif
