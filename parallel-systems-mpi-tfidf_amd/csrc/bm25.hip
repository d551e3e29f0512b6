/*
 * bm25.hip — the scoring pass of tfidf_query_bm25 (include/tfidf.h): Okapi BM25 over the
 * resident result of a run.  The pass has the shape of query.hip's (k_query_score /
 * k_query_score_big): an LDS bit filter over the group's term ranks, a binary search in the
 * group's sorted term list for the pairs that pass, one owner wave per document adding its
 * matches in pair order into one accumulator per query, a workgroup per document over
 * QS_BIG pairs.  Term lookup and the top-k rounds are query.hip's own kernels
 * (launch_query_lookup, launch_query_topk).
 *
 * What differs:
 *   weights   the posting table carries W(q,t) = fl(w * idf) as binary64 (the host computes
 *             them with its libm log); in the table's one block the doubles follow the u32
 *             words at an even word, so the LDS copy keeps them 8-byte aligned.
 *   inputs    a match reads the pair's count (out_cnt) and nothing else; a pair that misses
 *             the filter costs its term load and one LDS bit test, as in query.hip.
 *   K(d)      fl(k1 * fl(fl(1 - b) + fl(b * fl(docSize / avgdl)))), computed by the owner
 *             when its document shows a first match (one division per matching document;
 *             docSize is loaded through the output order with the document's first terms).
 *   sat       fl(fl(c * fl(k1 + 1)) / fl(c + K(d))) per match: the lanes that hold a round's
 *             matches divide at once, the owner then adds fl(W * sat) in pair order.
 *
 * Every operation rounds on its own: contraction is off for the whole file (hipcc fuses
 * a * b + c by default, through __dmul_rn / __dadd_rn as well), and `/` on doubles is the
 * correctly rounded expansion (the build has no fast-math flag).  No floating-point atomics.
 *
 * filter / gterm_find / doc_range / wave_lds_order are query.hip's helpers, repeated here
 * over this file's argument struct so that query.hip stays as it is.
 */
#include "kernels.h"
#include "dev_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
int ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

constexpr uint32_t QF_BITS = 1u << 18;          /* LDS filter: 32 KiB */
constexpr uint32_t QF_WORDS = QF_BITS / 32u;
constexpr uint32_t QTAB_WORDS = 4096u;          /* a group's table staged in LDS when it fits (16 KiB) */

/* the found terms' global df, next to their ranks (a few u32 for the host's idf) */
__global__ void k_bm25_df(const uint32_t* rank, uint32_t n, const uint32_t* df, uint32_t V, uint32_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = rank[i];
    out[i] = r < V ? df[r] : 0u;
}

__device__ __forceinline__ uint32_t gterm_find(const uint32_t* gterm, uint32_t n, uint32_t t) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (gterm[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && gterm[lo] == t) ? lo : QUERY_NO_TERM;
}

__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct GTab {
    const uint32_t* gterm;
    const uint32_t* post_off;
    const uint32_t* post_q;
    const double* post_w;
};
/* no barrier of its own: filter_build's barriers follow.  lds is 8-byte aligned and the
 * host put post_w at an even word of the block. */
__device__ __forceinline__ GTab tab_stage(const BScoreArgs& a, uint32_t* lds) {
    GTab t{a.gterm, a.post_off, a.post_q, a.post_w};
    if (a.tab_words != 0u && a.tab_words <= QTAB_WORDS) {
        for (uint32_t i = threadIdx.x; i < a.tab_words; i += NT) lds[i] = a.gterm[i];
        t.gterm = lds;
        t.post_off = lds + (a.post_off - a.gterm);
        t.post_q = lds + (a.post_q - a.gterm);
        t.post_w = (const double*)(lds + ((const uint32_t*)a.post_w - a.gterm));
    }
    return t;
}

__device__ __forceinline__ void filter_build(const BScoreArgs& a, uint32_t* filt) {
    for (uint32_t w = threadIdx.x; w < QF_WORDS; w += NT) filt[w] = 0u;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < a.ngterm; i += NT) {
        const uint32_t b = a.gterm[i] & (QF_BITS - 1u);
        atomicOr(&filt[b >> 5], 1u << (b & 31u));
    }
    __syncthreads();
}
__device__ __forceinline__ bool filter_has(const uint32_t* filt, uint32_t t) {
    const uint32_t b = t & (QF_BITS - 1u);
    return (filt[b >> 5] >> (b & 31u)) & 1u;
}

__device__ __forceinline__ void doc_range(const BScoreArgs& a, uint32_t j, uint64_t& b, uint64_t& e) {
    b = a.out_off[j];
    e = a.out_off[j + 1];
    if (e > a.npairs) e = a.npairs;
    if (b > e) b = e;
}

/* docSize of the document at output position j */
__device__ __forceinline__ uint32_t doc_len(const BScoreArgs& a, uint32_t j) {
    const uint32_t d = gload(a.order + j);
    return d < a.ndocs ? gload(a.doc_size + d) : 0u;
}

/* K(d) of a document of dsz tokens */
__device__ __forceinline__ double doc_K(const BScoreArgs& a, uint32_t dsz) {
    const double rel = (double)dsz / a.avgdl;
    const double bl = a.b * rel;
    const double nrm = a.one_minus_b + bl;
    return a.k1 * nrm;
}

/* sat of a pair with count c in a document of normaliser K */
__device__ __forceinline__ double pair_sat(const BScoreArgs& a, uint32_t c, double K) {
    const double num = (double)c * a.k1_plus_1;
    const double den = (double)c + K;
    return num / den;
}

/* one match added by its owner wave: lane x takes posting x of the term (a term's postings
 * name distinct queries, so the lanes of one pass never share an accumulator) */
__device__ __forceinline__ void add_match(const BScoreArgs& a, const GTab& g, uint32_t ti, double sat, double* wacc,
                                          uint32_t* wcnt, uint32_t lane) {
    const uint32_t p0 = g.post_off[ti], p1 = g.post_off[ti + 1];
    for (uint32_t x = p0 + lane; x < p1; x += 64u) {
        const uint32_t q = g.post_q[x];
        if (q < a.nq) {
            const double prod = g.post_w[x] * sat;
            wacc[q] = wacc[q] + prod;
            wcnt[q] += 1u;
        }
    }
    wave_lds_order();
}

__device__ __forceinline__ void write_doc(const BScoreArgs& a, uint32_t j, const double* wacc, const uint32_t* wcnt,
                                          uint32_t lane) {
    wave_lds_order();
    if (lane < a.nq) {
        a.acc[(uint64_t)lane * a.ndocs + j] = wacc[lane];
        a.cnt[(uint64_t)lane * a.ndocs + j] = wcnt[lane];
    }
}

/* waves stride over the output positions; a wave owns its document */
__global__ __launch_bounds__(NT) void k_bm25_score(const BScoreArgs a) {
    __shared__ uint32_t filt[QF_WORDS];
    __shared__ double acc_s[NT / 64][QG_MAX];
    __shared__ uint32_t cnt_s[NT / 64][QG_MAX];
    __shared__ double tab_s[QTAB_WORDS / 2];
    const GTab g = tab_stage(a, (uint32_t*)tab_s);
    filter_build(a, filt);
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    double* wacc = acc_s[wv];
    uint32_t* wcnt = cnt_s[wv];
    const uint32_t nwaves = gridDim.x * (NT / 64);
    for (uint32_t j = blockIdx.x * (NT / 64) + wv; j < a.ndocs; j += nwaves) {
        uint64_t b, e;
        doc_range(a, j, b, e);
        if (e - b > QS_BIG) {   /* the second launch's: one workgroup per such document */
            if (lane == 0) {
                const uint32_t at = atomicAdd(a.big_count, 1u);
                if (at < a.ndocs) a.big_list[at] = j;
            }
            continue;
        }
        wacc[lane] = 0.0;
        wcnt[lane] = 0u;
        wave_lds_order();
        const uint32_t dsz = doc_len(a, j);   /* two dependent loads, in flight with the first terms' */
        bool haveK = false;   /* wave-uniform */
        double K = 0.0;
        for (uint64_t p = b; p < e; p += 256u) {
            uint32_t t[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {   /* four rounds' terms in flight */
                const uint64_t pp = p + 64u * u + lane;
                t[u] = pp < e ? gload(a.out_term + pp) : QUERY_NO_TERM;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint64_t pp = p + 64u * u + lane;
                uint32_t ti = QUERY_NO_TERM;
                if (pp < e && filter_has(filt, t[u])) ti = gterm_find(g.gterm, a.ngterm, t[u]);
                uint64_t m = __ballot(ti != QUERY_NO_TERM);
                if (m == 0ull) continue;
                if (!haveK) { K = doc_K(a, dsz); haveK = true; }   /* the document's first match */
                double sat = 0.0;
                if (ti != QUERY_NO_TERM) sat = pair_sat(a, gload(a.out_cnt + pp), K);   /* the round's matches divide at once */
                while (m) {   /* the round's matches in pair order */
                    const int l = __builtin_ctzll(m);
                    m &= m - 1ull;
                    add_match(a, g, (uint32_t)__shfl((int)ti, l, 64), __shfl(sat, l, 64), wacc, wcnt, lane);
                }
            }
        }
        write_doc(a, j, wacc, wcnt, lane);
    }
}

/* documents over QS_BIG pairs: workgroups stride over the first launch's list */
__global__ __launch_bounds__(NT) void k_bm25_score_big(const BScoreArgs a) {
    __shared__ uint32_t filt[QF_WORDS];
    __shared__ double acc_s[QG_MAX];
    __shared__ uint32_t cnt_s[QG_MAX];
    __shared__ uint32_t m_ti[NT];
    __shared__ double m_s[NT];
    __shared__ uint32_t wsum[NT / 64];
    __shared__ double tab_s[QTAB_WORDS / 2];
    const GTab g = tab_stage(a, (uint32_t*)tab_s);
    filter_build(a, filt);
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t nbig = *a.big_count;
    if (nbig > a.ndocs) nbig = a.ndocs;
    for (uint32_t k = blockIdx.x; k < nbig; k += gridDim.x) {
        const uint32_t j = a.big_list[k];
        if (j >= a.ndocs) continue;
        uint64_t b, e;
        doc_range(a, j, b, e);
        const double K = doc_K(a, doc_len(a, j));   /* one division per long document, the same in every thread */
        if (threadIdx.x < QG_MAX) { acc_s[threadIdx.x] = 0.0; cnt_s[threadIdx.x] = 0u; }
        __syncthreads();
        for (uint64_t p = b; p < e; p += NT) {
            const uint64_t pp = p + threadIdx.x;
            uint32_t ti = QUERY_NO_TERM;
            if (pp < e) {
                const uint32_t t = gload(a.out_term + pp);
                if (filter_has(filt, t)) ti = gterm_find(g.gterm, a.ngterm, t);
            }
            const uint32_t hit = ti != QUERY_NO_TERM ? 1u : 0u;
            if (__syncthreads_count((int)hit) == 0) continue;   /* uniform: every thread sees the count */
            uint32_t total = 0;
            const uint32_t at = block_excl_scan<NT>(hit, wsum, &total);   /* pair order */
            if (hit) { m_ti[at] = ti; m_s[at] = pair_sat(a, gload(a.out_cnt + pp), K); }
            __syncthreads();
            if (wv == 0)
                for (uint32_t x = 0; x < total; ++x) add_match(a, g, m_ti[x], m_s[x], acc_s, cnt_s, lane);
            __syncthreads();
        }
        if (wv == 0) write_doc(a, j, acc_s, cnt_s, lane);
        __syncthreads();
    }
}

}  // namespace

int launch_bm25_df(const uint32_t* rank, uint32_t n, const uint32_t* df, uint32_t V, uint32_t* out, hipStream_t s) {
    if (!n) return 0;
    k_bm25_df<<<(n + 63u) / 64u, 64, 0, s>>>(rank, n, df, V, out);
    return ok();
}

int launch_bm25_score(const BScoreArgs& a, uint32_t ncu, hipStream_t s) {
    if (!a.ndocs || !a.nq || a.nq > QG_MAX) return a.nq > QG_MAX ? -1 : 0;
    if (hipMemsetAsync(a.big_count, 0, 4, s) != hipSuccess) return -1;
    /* every workgroup builds the filter once: no more of them than stay resident */
    const uint32_t cap = (ncu ? ncu : 256u) * 3u;   /* ~52 KiB of LDS each: three per CU */
    const uint32_t want = (a.ndocs + (NT / 64) - 1) / (NT / 64);
    k_bm25_score<<<want < cap ? want : cap, NT, 0, s>>>(a);
    if (ok()) return -1;
    k_bm25_score_big<<<want < 256u ? want : 256u, NT, 0, s>>>(a);
    return ok();
}
