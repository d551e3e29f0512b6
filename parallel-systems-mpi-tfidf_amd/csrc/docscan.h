/*
 * docscan.h — the one scoring pass behind tfidf_query (query.hip) and tfidf_query_bm25
 * (bm25.hip): a scan of the resident pairs for a group of <= QG_MAX queries.
 *
 * A pair's term is tested against the group's terms in an LDS bit filter indexed by the rank's
 * low bits (exact while V <= QF_BITS), so a pair that misses costs no second memory access; a
 * pair that passes is located in the group's sorted term list by binary search.  One wave owns
 * a document and adds its matches in pair order into one accumulator per query, each product
 * rounded before its add: the sum is a fixed sequence of IEEE operations, whatever the grid.
 * Documents over QS_BIG pairs are handed to a second launch, one workgroup each: every tile of
 * 256 pairs is compacted in pair order into LDS and wave 0 adds the compacted matches.
 *
 * A ranking function is a policy type P that supplies only what differs:
 *   P::Args          DocScanArgs plus the policy's own inputs
 *   P::W             the type of a posting's weight; a match adds fl((double)w * value)
 *   P::Doc           per-document state (empty when there is none)
 *   P::doc_begin     issues the state's loads, before the document's pair loop
 *   P::doc_ready     completes the state: at the document's first match in the wave kernel
 *                    (wave-uniform), once per document in the workgroup kernel
 *   P::value         a matching pair's value, by the lane or thread that holds the match
 *   P::POST_INC      optional, true: a match adds its posting's increment to the count word
 *
 * No product may be fused into an add and every operation rounds on its own: hipcc contracts
 * a * b + c by default, through __dmul_rn / __dadd_rn as well (they compiled to v_fmac_f64
 * here).  Contraction is off from here to the end of the including file, so for the policies
 * too; `/` on doubles is the correctly rounded expansion (the build has no fast-math flag).
 * No floating-point atomics.
 */
#ifndef TFIDF_DOCSCAN_H
#define TFIDF_DOCSCAN_H

#include "kernels.h"
#include "dev_common.h"
#include "launch_util.h"

#pragma clang fp contract(off)

namespace docscan {

constexpr int NT = 256;
constexpr uint32_t QF_BITS = 1u << 18;          /* LDS filter: 32 KiB */
constexpr uint32_t QF_WORDS = QF_BITS / 32u;

/* P::POST_INC (a static constexpr bool, absent = false): a match adds its posting's post_inc word
 * to the count instead of 1 (the clause policies: one field of the word per clause kind); P::Args
 * then has the member post_inc, an array inside the table's block */
template <class P, class = void>
struct post_inc_of { static constexpr bool value = false; };
template <class P>
struct post_inc_of<P, decltype((void)P::POST_INC)> { static constexpr bool value = P::POST_INC; };

/* index of term t in the group's sorted list, or QUERY_NO_TERM */
__device__ __forceinline__ uint32_t gterm_find(const uint32_t* gterm, uint32_t n, uint32_t t) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (gterm[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && gterm[lo] == t) ? lo : QUERY_NO_TERM;
}

/* orders one wave's LDS accesses across its lanes (the accumulators are read and written by
 * different lanes of the owner wave; the hardware runs a wave's LDS instructions in order) */
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* the group's table as the kernels read it: in LDS when it fits (a match then costs no
 * dependent global load: with frequent query words most documents hold many matches),
 * else where the host put it */
template <class W>
struct GTab {
    const uint32_t* gterm;
    const uint32_t* post_off;
    const uint32_t* post_q;
    const W* post_w;
    const uint32_t* post_inc;
};
/* no barrier of its own: filter_build's barriers follow.  lds is 8-byte aligned and the host
 * put binary64 weights at an even word of the block. */
template <class P>
__device__ __forceinline__ GTab<typename P::W> tab_stage(const typename P::Args& a, uint32_t* lds) {
    using W = typename P::W;
    GTab<W> t{a.gterm, a.post_off, a.post_q, (const W*)a.post_w, nullptr};
    if constexpr (post_inc_of<P>::value) t.post_inc = a.post_inc;
    if (a.tab_words != 0u && a.tab_words <= QTAB_WORDS) {
        for (uint32_t i = threadIdx.x; i < a.tab_words; i += NT) lds[i] = a.gterm[i];
        t.gterm = lds;
        t.post_off = lds + (a.post_off - a.gterm);
        t.post_q = lds + (a.post_q - a.gterm);
        t.post_w = (const W*)(lds + (a.post_w - a.gterm));
        if constexpr (post_inc_of<P>::value) t.post_inc = lds + (a.post_inc - a.gterm);
    }
    return t;
}

/* one match added by its owner wave: lane x takes posting x of the term (a term's postings
 * name distinct queries, so the lanes of one pass never share an accumulator) */
template <bool INC, class W>
__device__ __forceinline__ void add_match(const DocScanArgs& a, const GTab<W>& g, uint32_t ti, double v, double* wacc,
                                          uint32_t* wcnt, uint32_t lane) {
    const uint32_t p0 = g.post_off[ti], p1 = g.post_off[ti + 1];
    for (uint32_t x = p0 + lane; x < p1; x += 64u) {
        const uint32_t q = g.post_q[x];
        if (q < a.nq) {
            const double prod = (double)g.post_w[x] * v;
            wacc[q] = wacc[q] + prod;
            wcnt[q] += INC ? g.post_inc[x] : 1u;
        }
    }
    wave_lds_order();
}

__device__ __forceinline__ void filter_build(const DocScanArgs& a, uint32_t* filt) {
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

__device__ __forceinline__ void write_doc(const DocScanArgs& a, uint32_t j, const double* wacc, const uint32_t* wcnt,
                                          uint32_t lane) {
    wave_lds_order();
    if (lane < a.nq) {
        a.acc[(uint64_t)lane * a.ndocs + j] = wacc[lane];
        a.cnt[(uint64_t)lane * a.ndocs + j] = wcnt[lane];
    }
}

/* waves stride over the output positions; a wave owns its document */
template <class P>
__global__ __launch_bounds__(NT) void k_doc_score(const typename P::Args a) {
    __shared__ uint32_t filt[QF_WORDS];
    __shared__ double acc_s[NT / 64][QG_MAX];
    __shared__ uint32_t cnt_s[NT / 64][QG_MAX];
    __shared__ uint32_t tab_s[QTAB_WORDS] __attribute__((aligned(8)));
    const GTab<typename P::W> g = tab_stage<P>(a, tab_s);
    filter_build(a, filt);
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    double* wacc = acc_s[wv];
    uint32_t* wcnt = cnt_s[wv];
    const uint32_t nwaves = gridDim.x * (NT / 64);
    for (uint32_t j = blockIdx.x * (NT / 64) + wv; j < a.ndocs; j += nwaves) {
        uint64_t b, e;
        pair_range(a.out_off, a.npairs, j, b, e);
        if (e - b > QS_BIG) {   /* the second launch's: one workgroup per such document */
            if (lane == 0) hand_to_big(a.big_list, a.big_count, a.ndocs, j);
            continue;
        }
        wacc[lane] = 0.0;
        wcnt[lane] = 0u;
        wave_lds_order();
        typename P::Doc d = P::doc_begin(a, j);   /* its loads are in flight with the first terms' */
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
                P::doc_ready(a, d);   /* wave-uniform */
                double v = 0.0;
                if (ti != QUERY_NO_TERM) v = P::value(a, d, pp);   /* the round's matches at once */
                while (m) {   /* the round's matches in pair order */
                    const int l = __builtin_ctzll(m);
                    m &= m - 1ull;
                    add_match<post_inc_of<P>::value>(a, g, (uint32_t)__shfl((int)ti, l, 64), __shfl(v, l, 64), wacc, wcnt, lane);
                }
            }
        }
        write_doc(a, j, wacc, wcnt, lane);
    }
}

/* documents over QS_BIG pairs: workgroups stride over the first launch's list */
template <class P>
__global__ __launch_bounds__(NT) void k_doc_score_big(const typename P::Args a) {
    __shared__ uint32_t filt[QF_WORDS];
    __shared__ double acc_s[QG_MAX];
    __shared__ uint32_t cnt_s[QG_MAX];
    __shared__ uint32_t m_ti[NT];
    __shared__ double m_v[NT];
    __shared__ uint32_t wsum[NT / 64];
    __shared__ uint32_t tab_s[QTAB_WORDS] __attribute__((aligned(8)));
    const GTab<typename P::W> g = tab_stage<P>(a, tab_s);
    filter_build(a, filt);
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t nbig = *a.big_count;
    if (nbig > a.ndocs) nbig = a.ndocs;
    for (uint32_t k = blockIdx.x; k < nbig; k += gridDim.x) {
        const uint32_t j = a.big_list[k];
        if (j >= a.ndocs) continue;
        uint64_t b, e;
        pair_range(a.out_off, a.npairs, j, b, e);
        typename P::Doc d = P::doc_begin(a, j);
        P::doc_ready(a, d);   /* once per long document, the same in every thread */
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
            if (hit) { m_ti[at] = ti; m_v[at] = P::value(a, d, pp); }
            __syncthreads();
            if (wv == 0)
                for (uint32_t x = 0; x < total; ++x) add_match<post_inc_of<P>::value>(a, g, m_ti[x], m_v[x], acc_s, cnt_s, lane);
            __syncthreads();
        }
        if (wv == 0) write_doc(a, j, acc_s, cnt_s, lane);
        __syncthreads();
    }
}

template <class P>
int launch_score(const typename P::Args& a, uint32_t ncu, hipStream_t s) {
    if (!a.ndocs || !a.nq || a.nq > QG_MAX) return a.nq > QG_MAX ? -1 : 0;
    if (hipMemsetAsync(a.big_count, 0, 4, s) != hipSuccess) return -1;
    /* every workgroup builds the filter once: no more of them than stay resident */
    const uint32_t want = (a.ndocs + (NT / 64) - 1) / (NT / 64);
    k_doc_score<P><<<cu_grid(want, ncu, QS_WG_PER_CU), NT, 0, s>>>(a);   /* ~52 KiB of LDS each: three per CU */
    if (ok()) return -1;
    k_doc_score_big<P><<<big_grid(want, ncu), NT, 0, s>>>(a);
    return ok();
}

}  // namespace docscan

#endif
