/*
 * bm25.hip — the scoring pass of tfidf_query_bm25 (include/tfidf.h): Okapi BM25 over the
 * resident result of a run.  The pass is docscan.h's scan, the one tfidf_query runs, with the
 * BM25 policy below.  Term lookup and the top-k rounds are query.hip's own kernels
 * (launch_query_lookup, launch_query_topk).
 *
 * What the policy supplies:
 *   weights   the posting table carries W(q,t) = fl(w * idf) as binary64 (the host computes
 *             them with its libm log); in the table's one block the doubles follow the u32
 *             words at an even word, so the LDS copy keeps them 8-byte aligned.
 *   inputs    a match reads the pair's count (out_cnt) and nothing else; a pair that misses
 *             the filter costs its term load and one LDS bit test, as for tfidf_query.
 *   K(d)      fl(k1 * fl(fl(1 - b) + fl(b * fl(docSize / avgdl)))), computed by the owner
 *             when its document shows a first match (one division per matching document;
 *             docSize is loaded through the output order with the document's first terms).
 *   sat       fl(fl(c * fl(k1 + 1)) / fl(c + K(d))) per match: the lanes that hold a round's
 *             matches divide at once, the owner then adds fl(W * sat) in pair order.
 *
 * Every operation rounds on its own: docscan.h turns contraction off for the rest of this file.
 */
#include "docscan.h"

namespace {

/* the found terms' global df, next to their ranks (a few u32 for the host's idf) */
__global__ void k_bm25_df(const uint32_t* rank, uint32_t n, const uint32_t* df, uint32_t V, uint32_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = rank[i];
    out[i] = r < V ? df[r] : 0u;
}

struct Bm25Score {
    using Args = BScoreArgs;
    using W = double;
    struct Doc {
        uint32_t dsz;   /* docSize */
        double K;
        bool haveK;     /* wave-uniform */
    };
    /* docSize of the document at output position j: two dependent loads */
    static __device__ __forceinline__ Doc doc_begin(const Args& a, uint32_t j) {
        const uint32_t d = gload(a.order + j);
        return Doc{d < a.ndocs ? gload(a.doc_size + d) : 0u, 0.0, false};
    }
    static __device__ __forceinline__ void doc_ready(const Args& a, Doc& d) {
        if (d.haveK) return;
        const double rel = (double)d.dsz / a.avgdl;
        const double bl = a.b * rel;
        const double nrm = a.one_minus_b + bl;
        d.K = a.k1 * nrm;
        d.haveK = true;
    }
    /* sat of the pair at pp in a document of normaliser K */
    static __device__ __forceinline__ double value(const Args& a, const Doc& d, uint64_t pp) {
        const uint32_t c = gload(a.out_cnt + pp);
        const double num = (double)c * a.k1_plus_1;
        const double den = (double)c + d.K;
        return num / den;
    }
};

/* the same with clauses: a match adds its posting's increment to the document's count word */
struct Bm25ClauseScore : Bm25Score {
    using Args = BClauseArgs;
    static constexpr bool POST_INC = true;
};

}  // namespace

int launch_bm25_df(const uint32_t* rank, uint32_t n, const uint32_t* df, uint32_t V, uint32_t* out, hipStream_t s) {
    if (!n) return 0;
    k_bm25_df<<<grid_for(n, 64), 64, 0, s>>>(rank, n, df, V, out);
    return ok();
}

int launch_bm25_score(const BScoreArgs& a, uint32_t ncu, hipStream_t s) { return docscan::launch_score<Bm25Score>(a, ncu, s); }

int launch_bm25_score_clauses(const BClauseArgs& a, uint32_t ncu, hipStream_t s) {
    if (!a.post_inc) return -1;
    return docscan::launch_score<Bm25ClauseScore>(a, ncu, s);
}
