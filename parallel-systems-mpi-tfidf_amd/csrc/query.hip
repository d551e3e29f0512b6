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
 *   score    one pass over out_term / out_score per group of <= QG_MAX queries.  A pair's
 *            term is tested against the group's terms in an LDS bit filter indexed by the
 *            rank's low bits (exact while V <= QF_BITS), so a pair that misses costs no
 *            second memory access; a pair that passes is located in the group's sorted
 *            term list by binary search.  One wave owns a document and adds its matches in
 *            pair order into one accumulator per query, each product rounded before its
 *            add (no fused multiply-add): the sum is a fixed sequence of IEEE operations,
 *            whatever the grid.  Documents over QS_BIG pairs are handed to a second launch,
 *            one workgroup each: every tile of 256 pairs is compacted in pair order into
 *            LDS and wave 0 adds the compacted matches.
 *   top-k    dense (query, output position) accumulators -> per-slice top-k in LDS
 *            (compaction of the hits, bitonic sort under (score descending, document id
 *            ascending)) -> the same kernel over the slices' lists until one slice is left.
 */
#include "kernels.h"
#include "dev_common.h"
#include "dev_vocab.h"

namespace {

constexpr int NT = 256;
inline unsigned grid_for(uint64_t n, int nt = NT) { return n ? (unsigned)((n + nt - 1) / nt) : 1u; }
int ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

constexpr uint32_t QF_BITS = 1u << 18;          /* LDS filter: 32 KiB */
constexpr uint32_t QF_WORDS = QF_BITS / 32u;
constexpr uint32_t QTAB_WORDS = 4096u;          /* a group's term table staged in LDS when it fits (16 KiB) */

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
struct GTab {
    const uint32_t* gterm;
    const uint32_t* post_off;
    const uint32_t* post_q;
    const uint32_t* post_w;
};
/* no barrier of its own: filter_build's barriers follow */
__device__ __forceinline__ GTab tab_stage(const QScoreArgs& a, uint32_t* lds) {
    GTab t{a.gterm, a.post_off, a.post_q, a.post_w};
    if (a.tab_words != 0u && a.tab_words <= QTAB_WORDS) {   /* the host's layout is one block from gterm on */
        for (uint32_t i = threadIdx.x; i < a.tab_words; i += NT) lds[i] = a.gterm[i];
        t.gterm = lds;
        t.post_off = lds + (a.post_off - a.gterm);
        t.post_q = lds + (a.post_q - a.gterm);
        t.post_w = lds + (a.post_w - a.gterm);
    }
    return t;
}

/* one match added by its owner wave: lane x takes posting x of the term (a term's postings
 * name distinct queries, so the lanes of one pass never share an accumulator) */
__device__ __forceinline__ void add_match(const QScoreArgs& a, const GTab& g, uint32_t ti, double s, double* wacc, uint32_t* wcnt,
                                          uint32_t lane) {
/* hipcc contracts a * b + c by default, through __dmul_rn / __dadd_rn as well (they compiled
 * to v_fmac_f64 here): the product must round on its own */
#pragma clang fp contract(off)
    const uint32_t p0 = g.post_off[ti], p1 = g.post_off[ti + 1];
    for (uint32_t x = p0 + lane; x < p1; x += 64u) {
        const uint32_t q = g.post_q[x];
        if (q < a.nq) {
            const double prod = (double)g.post_w[x] * s;
            wacc[q] = wacc[q] + prod;
            wcnt[q] += 1u;
        }
    }
    wave_lds_order();
}

__device__ __forceinline__ void filter_build(const QScoreArgs& a, uint32_t* filt) {
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

/* a document's pair range, clamped to the run's pair total */
__device__ __forceinline__ void doc_range(const QScoreArgs& a, uint32_t j, uint64_t& b, uint64_t& e) {
    b = a.out_off[j];
    e = a.out_off[j + 1];
    if (e > a.npairs) e = a.npairs;
    if (b > e) b = e;
}

__device__ __forceinline__ void write_doc(const QScoreArgs& a, uint32_t j, const double* wacc, const uint32_t* wcnt,
                                          uint32_t lane) {
    wave_lds_order();
    if (lane < a.nq) {
        a.acc[(uint64_t)lane * a.ndocs + j] = wacc[lane];
        a.cnt[(uint64_t)lane * a.ndocs + j] = wcnt[lane];
    }
}

/* waves stride over the output positions; a wave owns its document */
__global__ __launch_bounds__(NT) void k_query_score(const QScoreArgs a) {
    __shared__ uint32_t filt[QF_WORDS];
    __shared__ double acc_s[NT / 64][QG_MAX];
    __shared__ uint32_t cnt_s[NT / 64][QG_MAX];
    __shared__ uint32_t tab_s[QTAB_WORDS];
    const GTab g = tab_stage(a, tab_s);
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
                const double s = ti != QUERY_NO_TERM ? gload(a.out_score + pp) : 0.0;
                while (m) {   /* the round's matches in pair order */
                    const int l = __builtin_ctzll(m);
                    m &= m - 1ull;
                    add_match(a, g, (uint32_t)__shfl((int)ti, l, 64), __shfl(s, l, 64), wacc, wcnt, lane);
                }
            }
        }
        write_doc(a, j, wacc, wcnt, lane);
    }
}

/* documents over QS_BIG pairs: workgroups stride over the first launch's list */
__global__ __launch_bounds__(NT) void k_query_score_big(const QScoreArgs a) {
    __shared__ uint32_t filt[QF_WORDS];
    __shared__ double acc_s[QG_MAX];
    __shared__ uint32_t cnt_s[QG_MAX];
    __shared__ uint32_t m_ti[NT];
    __shared__ double m_s[NT];
    __shared__ uint32_t wsum[NT / 64];
    __shared__ uint32_t tab_s[QTAB_WORDS];
    const GTab g = tab_stage(a, tab_s);
    filter_build(a, filt);
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t nbig = *a.big_count;
    if (nbig > a.ndocs) nbig = a.ndocs;
    for (uint32_t k = blockIdx.x; k < nbig; k += gridDim.x) {
        const uint32_t j = a.big_list[k];
        if (j >= a.ndocs) continue;
        uint64_t b, e;
        doc_range(a, j, b, e);
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
            if (hit) { m_ti[at] = ti; m_s[at] = gload(a.out_score + pp); }
            __syncthreads();
            if (wv == 0)
                for (uint32_t x = 0; x < total; ++x) add_match(a, g, m_ti[x], m_s[x], acc_s, cnt_s, lane);
            __syncthreads();
        }
        if (wv == 0) write_doc(a, j, acc_s, cnt_s, lane);
        __syncthreads();
    }
}

/* ------------------------------------------------------------------- top-k -- */

/* a before b: score descending, then document id ascending.  Keys are the scores' bit
 * patterns + 1 (scores are >= +0.0 and finite: the patterns order like the values and the
 * increment cannot wrap); 0 pads the sort to a power of two and sorts last. */
__device__ __forceinline__ bool hit_before(uint64_t sa, uint32_t ia, uint64_t sb, uint32_t ib) {
    return sa > sb || (sa == sb && ia < ib);
}

__global__ __launch_bounds__(NT) void k_query_topk(const QTopkArgs a) {
    __shared__ uint64_t ls[QT_SLICE];
    __shared__ uint32_t lid[QT_SLICE];
    __shared__ uint32_t lcount;
    const uint32_t slice = blockIdx.x, q = blockIdx.y;
    if (threadIdx.x == 0) lcount = 0u;
    __syncthreads();
    const uint64_t e0 = (uint64_t)slice * QT_SLICE;
    const uint64_t e1 = e0 + QT_SLICE < a.n_in ? e0 + QT_SLICE : a.n_in;
    for (uint64_t e = e0 + threadIdx.x; e < e1; e += NT) {
        bool valid;
        uint64_t s = 0;
        uint32_t id = 0;
        const uint64_t at = (uint64_t)q * a.n_in + e;
        if (a.acc) {   /* first round: the dense accumulators, e = output position */
            valid = a.cnt[at] != 0u;
            if (valid) {
                s = (uint64_t)__double_as_longlong(a.acc[at]);
                const uint32_t d = a.order[e];
                id = a.doc_ids ? a.doc_ids[d] : d + 1u;
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

int launch_query_score(const QScoreArgs& a, uint32_t ncu, hipStream_t s) {
    if (!a.ndocs || !a.nq || a.nq > QG_MAX) return a.nq > QG_MAX ? -1 : 0;
    if (hipMemsetAsync(a.big_count, 0, 4, s) != hipSuccess) return -1;
    /* every workgroup builds the filter once: no more of them than stay resident */
    const uint32_t cap = (ncu ? ncu : 256u) * 3u;   /* ~52 KiB of LDS each: three per CU */
    const uint32_t want = (a.ndocs + (NT / 64) - 1) / (NT / 64);
    k_query_score<<<want < cap ? want : cap, NT, 0, s>>>(a);
    if (ok()) return -1;
    k_query_score_big<<<want < 256u ? want : 256u, NT, 0, s>>>(a);
    return ok();
}

int launch_query_topk(const QTopkArgs& a, uint32_t nq, hipStream_t s) {
    if (!nq || !a.out_slices) return 0;
    k_query_topk<<<dim3(a.out_slices, nq), NT, 0, s>>>(a);
    return ok();
}
