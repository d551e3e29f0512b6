/*
 * query.hip — batched top-k document retrieval over the resident result of a run
 * (include/tfidf.h: tfidf_query).  The reference stops at the sorted "docN@word\t%.16f"
 * lines (TFIDF.c:245,273-282); ranking documents for a query reads the same scores
 * (TFIDF.c:202,243-244) where the run left them in HBM.
 *
 *   lookup   one lane per distinct query term: the term's identity key (dev_common.h), a
 *            read-only probe of the run's vocabulary table from the key's home slot, a byte
 *            compare for terms of >= 16 bytes (the rule of long_term_differs, dev_vocab.h),
 *            then rank_of_slot.
 *   score    one pass over out_term / out_score per group of <= QG_MAX queries: docscan.h's
 *            scan (filter, search, owner wave per document, a workgroup per document over
 *            QS_BIG pairs), which tfidf_query_bm25 shares, with the TF-IDF policy below:
 *            u32 weights, a match's value is the pair's score, no per-document state.
 *   top-k    dense (query, output position) accumulators -> per-slice top-k in LDS
 *            (compaction of the hits, bitonic sort under (score descending, document id
 *            ascending)) -> the same kernel over the slices' lists until one slice is left.
 */
#include "docscan.h"
#include "dev_vocab.h"

namespace {

constexpr int NT = 256;

/* ------------------------------------------------------------------ lookup -- */

__global__ void k_query_lookup(const QLookupArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nterms) return;
    const uint64_t t0 = a.toff[i], n = a.toff[i + 1] - t0;
    const uint8_t* p = a.tbytes + t0;
    uint64_t klo = 0, khi = 0;
    if (n < 16u) {
        uint64_t lo = 0, hi = 0;
        for (uint32_t b = 0; b < (uint32_t)n; ++b) {
            const uint64_t c = p[b];
            if (b < 8u) lo |= c << (8u * b);
            else hi |= c << (8u * (b - 8u));
        }
        make_short_key(lo, hi, (uint32_t)n, &klo, &khi);
    } else {
        make_long_key(p, n, &klo, &khi);
    }
    const VocabRO v{a.vkeys, a.vrep, a.mask, a.home, a.rank_of_slot, a.corpus, a.corpus_bytes, a.V};
    a.rank_out[i] = vocab_find_rank(v, klo, khi, p, n);
}

/* ------------------------------------------------------------------- score -- */

/* docscan.h's pass with the TF-IDF values: a match adds fl(w * score), w = the term's count in
 * the query.  No per-document state. */
struct TfidfScore {
    using Args = QScoreArgs;
    using W = uint32_t;
    struct Doc {};
    static __device__ __forceinline__ Doc doc_begin(const Args&, uint32_t) { return {}; }
    static __device__ __forceinline__ void doc_ready(const Args&, Doc&) {}
    static __device__ __forceinline__ double value(const Args& a, const Doc&, uint64_t pp) { return gload(a.out_score + pp); }
};

/* the same with clauses: a match adds its posting's increment to the document's count word */
struct TfidfClauseScore : TfidfScore {
    using Args = QClauseArgs;
    static constexpr bool POST_INC = true;
};

/* ------------------------------------------------------------------- top-k -- */

/* the first round's test of a document's count word.  Without clauses: any match.  With them
 * (CLAUSES, n = need[q] = |M| << 12 | min_should): no must_not term, every must term, enough
 * should terms, and at least one scoring term.  A template parameter of the kernel, so that the
 * rounds of tfidf_query, tfidf_query_bm25 and tfidf_similar are the code they were. */
template <bool CLAUSES>
__device__ __forceinline__ bool hit_valid(uint32_t cnt, uint32_t n) {
    if (!CLAUSES) return cnt != 0u;
    return (cnt >> 24) == 0u && ((cnt >> 12) & CL_FIELD) == (n >> 12) && (cnt & CL_FIELD) >= (n & CL_FIELD) &&
           (cnt & 0xFFFFFFu) != 0u;
}

/* a before b: score descending, then document id ascending.  Keys are the scores' bit
 * patterns + 1 (scores are >= +0.0 and finite: the patterns order like the values and the
 * increment cannot wrap); 0 pads the sort to a power of two and sorts last. */
__device__ __forceinline__ bool hit_before(uint64_t sa, uint32_t ia, uint64_t sb, uint32_t ib) {
    return sa > sb || (sa == sb && ia < ib);
}

template <bool CLAUSES>
__global__ __launch_bounds__(NT) void k_query_topk(const QTopkArgs a) {
    __shared__ uint64_t ls[QT_SLICE];
    __shared__ uint32_t lid[QT_SLICE];
    __shared__ uint32_t lcount;
    const uint32_t slice = blockIdx.x, q = blockIdx.y;
    if (threadIdx.x == 0) lcount = 0u;
    __syncthreads();
    const uint32_t need = CLAUSES ? a.need[q] : 0u;
    const uint64_t e0 = (uint64_t)slice * QT_SLICE;
    const uint64_t e1 = e0 + QT_SLICE < a.n_in ? e0 + QT_SLICE : a.n_in;
    for (uint64_t e = e0 + threadIdx.x; e < e1; e += NT) {
        bool valid;
        uint64_t s = 0;
        uint32_t id = 0;
        const uint64_t at = (uint64_t)q * a.n_in + e;
        if (a.acc) {   /* first round: the dense accumulators, e = output position */
            valid = hit_valid<CLAUSES>(a.cnt[at], need);
            if (valid) {
                s = (uint64_t)__double_as_longlong(a.acc[at]);
                id = doc_id_at(a.order, a.doc_ids, (uint32_t)e);
            }
        } else {       /* the previous round's lists: in_slices lists of kk entries */
            const uint32_t sl = (uint32_t)(e / a.kk), r = (uint32_t)(e % a.kk);
            valid = r < a.in_n[(uint64_t)q * a.in_slices + sl];
            if (valid) { s = a.in_s[at]; id = a.in_id[at]; }
        }
        if (valid) {
            const uint32_t pos = atomicAdd(&lcount, 1u);   /* any order: the sort follows */
            ls[pos] = s + 1ull;
            lid[pos] = id;
        }
    }
    __syncthreads();
    const uint32_t c = lcount;   /* <= QT_SLICE */
    const uint64_t orow = ((uint64_t)q * a.out_slices + slice);
    if (threadIdx.x == 0) {
        a.out_n[orow] = c < a.kk ? c : a.kk;
        if (a.acc && c) atomicAdd(a.nmatch + q, (unsigned long long)c);
    }
    if (c == 0u) return;
    uint32_t m = 2u;
    while (m < c) m <<= 1;
    for (uint32_t i = c + threadIdx.x; i < m; i += NT) { ls[i] = 0ull; lid[i] = 0xFFFFFFFFu; }
    __syncthreads();
    for (uint32_t k2 = 2u; k2 <= m; k2 <<= 1) {
        for (uint32_t jj = k2 >> 1; jj > 0u; jj >>= 1) {
            for (uint32_t i = threadIdx.x; i < m; i += NT) {
                const uint32_t x = i ^ jj;
                if (x > i) {
                    const uint64_t si = ls[i], sx = ls[x];
                    const uint32_t ii = lid[i], ix = lid[x];
                    const bool up = (i & k2) == 0u;   /* best first in this run */
                    if (up ? hit_before(sx, ix, si, ii) : hit_before(si, ii, sx, ix)) {
                        ls[i] = sx; lid[i] = ix;
                        ls[x] = si; lid[x] = ii;
                    }
                }
            }
            __syncthreads();
        }
    }
    const uint32_t nout = c < a.kk ? c : a.kk;
    for (uint32_t i = threadIdx.x; i < nout; i += NT) {
        a.out_s[orow * a.kk + i] = ls[i] - 1ull;
        a.out_id[orow * a.kk + i] = lid[i];
    }
}

}  // namespace

int launch_query_lookup(const QLookupArgs& a, hipStream_t s) {
    if (!a.nterms) return 0;
    k_query_lookup<<<grid_for(a.nterms, 64), 64, 0, s>>>(a);
    return ok();
}

int launch_query_score(const QScoreArgs& a, uint32_t ncu, hipStream_t s) { return docscan::launch_score<TfidfScore>(a, ncu, s); }

int launch_query_score_clauses(const QClauseArgs& a, uint32_t ncu, hipStream_t s) {
    if (!a.post_inc) return -1;
    return docscan::launch_score<TfidfClauseScore>(a, ncu, s);
}

int launch_query_topk(const QTopkArgs& a, uint32_t nq, hipStream_t s) {
    if (!nq || !a.out_slices) return 0;
    if (a.acc && a.need) k_query_topk<true><<<dim3(a.out_slices, nq), NT, 0, s>>>(a);
    else k_query_topk<false><<<dim3(a.out_slices, nq), NT, 0, s>>>(a);
    return ok();
}
