/*
 * reweight.hip — weighting schemes over the resident result of a run (include/tfidf.h, section
 * "weighting": tfidf_reweight) and over the rows of tfidf_transform under a scheme.  The reference
 * has the one formula fl(fl(count / docSize) * log(N / df)) (TFIDF.c:202,243-244), which the
 * run's score kernels compute; here the scores are computed again from the integers the run left
 * in HBM, by another tf, another idf and an L1 or L2 norm per document.
 *
 *   cmax     sublinear tf needs log(c) for the counts that occur and the device evaluates no
 *            log: one pass gives the largest count and lists the counts above RW_LUT_MAX (there
 *            are at most tokens / RW_LUT_MAX of them); the host tabulates fl(1 + log c) for
 *            c = 1..min(Cmax, RW_LUT_MAX) and for the listed counts, sorted.
 *   idf      the scheme's idf lives in a table in the layout of the run's own (by df, or through
 *            the run's index of distinct df values), filled by the host; one lane per term
 *            gathers it by rank, so that the pair pass reads one 8-byte value per pair.
 *   pairs    document-major.  One wave owns a document: 64 pairs at once get their w = fl(tf *
 *            idf); under a norm the 64 terms (w, or fl(w * w)) are added in pair order, one
 *            lane's after the other, into one sum that every lane carries (k_sim_norms' shape:
 *            the chain of one add per pair is the definition), sqrt is the correctly rounded
 *            one, and every lane divides its own w.  Up to RW_KEEP pairs the w stay in registers
 *            between the sum and the division; beyond, a lane reloads what it wrote.  Documents
 *            over RW_BIG pairs are handed to a second launch, one workgroup each: 256 pairs get
 *            their w at once, wave 0 adds the tile's terms from LDS in pair order.  Either way
 *            a document's result is a fixed sequence of IEEE operations: it depends neither on
 *            the grid nor on which launch took it.  No floating-point atomics.
 *
 * No product may be fused into an add in this file (hipcc contracts a * b + c by default, and
 * through __dmul_rn / __dadd_rn as well: similar.hip, docscan.h). */
#include "kernels.h"
#include "dev_common.h"
#include "launch_util.h"
#include "../../include/tfidf.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
static_assert(RW_KEEP == 256u, "four rounds of 64 pairs in registers");

/* ------------------------------------------------------------------- tables -- */

__global__ __launch_bounds__(NT) void k_rw_cmax(const uint32_t* count, uint64_t n, const uint32_t* n_dev, uint32_t* cmax,
                                                uint32_t* list, uint32_t list_cap) {
    if (n_dev && (uint64_t)*n_dev < n) n = *n_dev;
    uint32_t m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * NT) {
        const uint32_t c = gload(count + i);
        m = c > m ? c : m;
        if (c > RW_LUT_MAX) {
            const uint32_t at = atomicAdd(cmax + 1, 1u);
            if (at < list_cap) list[at] = c;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t x = (uint32_t)__shfl_xor((int)m, o, 64);
        m = x > m ? x : m;
    }
    if ((threadIdx.x & 63u) == 0u && m) atomicMax(cmax, m);
}

__global__ __launch_bounds__(NT) void k_rw_idf_rank(const uint32_t* df, uint32_t V, const double* idf, const uint32_t* idf_idx,
                                                    uint64_t idf_n, double* idf_rank) {
    const uint32_t r = blockIdx.x * NT + threadIdx.x;
    if (r >= V) return;
    const uint32_t d = df[r];
    double v = 1.0;   /* a df outside the table: never with a valid run */
    if ((uint64_t)d < idf_n) v = idf_idx ? idf[idf_idx[d]] : idf[d];
    idf_rank[r] = v;
}

/* -------------------------------------------------------------------- pairs -- */

__device__ __forceinline__ double rw_tf(const RwArgs& a, uint32_t c, double dsd) {
#pragma clang fp contract(off)
    switch (a.tf_mode) {   /* uniform */
    case TFIDF_TF_RATIO:
        return (double)c / dsd;   /* TFIDF.c:202 */
    case TFIDF_TF_RAW:
        return (double)c;
    case TFIDF_TF_LOG: {
        if (c <= a.lut_n) return a.tf_lut[c];
        uint32_t lo = 0, hi = a.nlisted;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.listed_c[mid] < c) lo = mid + 1;
            else hi = mid;
        }
        return (lo < a.nlisted && a.listed_c[lo] == c) ? a.listed_v[lo] : 0.0;   /* listed by k_rw_cmax: always found */
    }
    default:
        return 1.0;
    }
}

/* w(d, t) = fl(tf * idf) of a pair with count c and key k */
__device__ __forceinline__ double rw_w_ck(const RwArgs& a, uint32_t c, uint32_t k, double dsd) {
#pragma clang fp contract(off)
    const double tf = rw_tf(a, c, dsd);
    double idf = 1.0;
    if (a.idf && (uint64_t)k < a.key_n) idf = a.idf_idx ? a.idf[a.idf_idx[k]] : a.idf[k];
    return tf * idf;
}
__device__ __forceinline__ double rw_w(const RwArgs& a, uint64_t p, double dsd) {
    return rw_w_ck(a, gload(a.count + p), a.idf ? gload(a.key + p) : 0u, dsd);
}

/* w of the wave's pairs p0 + 64 u + lane, u < 4, below e (0.0 beyond): the four rounds' counts and
 * keys are in flight before the first table is read */
__device__ __forceinline__ void rw_w4(const RwArgs& a, uint64_t p0, uint64_t e, uint32_t lane, double dsd, double (&w)[4]) {
    uint32_t c[4], k[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) {
        const uint64_t pp = p0 + 64u * u + lane;
        c[u] = pp < e ? gload(a.count + pp) : 0u;
        k[u] = (pp < e && a.idf) ? gload(a.key + pp) : 0u;
    }
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) w[u] = p0 + 64u * u + lane < e ? rw_w_ck(a, c[u], k[u], dsd) : 0.0;
}

__device__ __forceinline__ double rw_doc_size(const RwArgs& a, uint32_t j) {
    return (double)a.doc_size[a.order ? a.order[j] : j];
}

/* the norm's term of a pair */
template <int NORM>
__device__ __forceinline__ double rw_term(double w) {
#pragma clang fp contract(off)
    return NORM == TFIDF_NORM_L2 ? w * w : w;
}

/* adds the first n (<= 64) lanes' x to sum in lane order; every lane carries the sum */
__device__ __forceinline__ double rw_chain(double sum, double x, int n) {
#pragma clang fp contract(off)
    for (int l = 0; l < n; ++l) sum = sum + bcast_f64(x, l);
    return sum;
}

template <int NORM>
__device__ __forceinline__ double rw_divisor(double sum) {
    return NORM == TFIDF_NORM_L2 ? __dsqrt_rn(sum) : sum;
}

/* waves stride over the documents; a wave owns its document */
template <int NORM>
__global__ __launch_bounds__(NT) void k_rw_docs(const RwArgs a) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nwaves = gridDim.x * (NT / 64);
    for (uint32_t j = blockIdx.x * (NT / 64) + (threadIdx.x >> 6); j < a.ndocs; j += nwaves) {
        uint64_t b, e;
        pair_range(a.off, a.npairs, j, b, e);
        if (b == e) continue;   /* wave-uniform, as every branch on b and e below */
        if (e - b > RW_BIG) {   /* the second launch's: one workgroup per such document */
            if (lane == 0) hand_to_big(a.big_list, a.misc, a.ndocs, j);
            continue;
        }
        const double dsd = rw_doc_size(a, j);
        if (NORM == TFIDF_NORM_NONE) {   /* a pure stream */
            /* one round per step: four rounds in flight (rw_w4) measured 8 % slower here, 10 % faster below */
            for (uint64_t p = b + lane; p < e; p += 64u) a.score[p] = rw_w(a, p, dsd);
            continue;
        }
        double sum = 0.0;
        if (e - b <= RW_KEEP) {
            double w[RW_KEEP / 64];
            rw_w4(a, b, e, lane, dsd, w);
#pragma unroll
            for (uint32_t u = 0; u < RW_KEEP / 64; ++u) {
                const uint64_t p = b + 64u * u;
                if (p < e) sum = rw_chain(sum, rw_term<NORM>(w[u]), e - p < 64u ? (int)(e - p) : 64);
            }
            const double d = rw_divisor<NORM>(sum);
            if (d == 0.0 && lane == 0) atomicAdd(a.misc + 1, 1u);
#pragma unroll
            for (uint32_t u = 0; u < RW_KEEP / 64; ++u) {
                const uint64_t pp = b + 64u * u + lane;
                if (pp < e) a.score[pp] = d == 0.0 ? w[u] : w[u] / d;
            }
            continue;
        }
        for (uint64_t p = b; p < e; p += 64u) {
            const uint64_t pp = p + lane;
            double w = 0.0;
            if (pp < e) {
                w = rw_w(a, pp, dsd);
                a.score[pp] = w;
            }
            sum = rw_chain(sum, rw_term<NORM>(w), e - p < 64u ? (int)(e - p) : 64);
        }
        const double d = rw_divisor<NORM>(sum);
        if (d == 0.0) {   /* the scores stay w */
            if (lane == 0) atomicAdd(a.misc + 1, 1u);
            continue;
        }
        for (uint64_t pp = b + lane; pp < e; pp += 64u) a.score[pp] = a.score[pp] / d;   /* this lane's own stores */
    }
}

/* documents over RW_BIG pairs: workgroups stride over the first launch's list */
template <int NORM>
__global__ __launch_bounds__(NT) void k_rw_docs_big(const RwArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_x[NT];
    __shared__ double s_d;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t nbig = a.misc[0];
    if (nbig > a.ndocs) nbig = a.ndocs;
    for (uint32_t k = blockIdx.x; k < nbig; k += gridDim.x) {
        const uint32_t j = a.big_list[k];
        if (j >= a.ndocs) continue;
        uint64_t b, e;
        pair_range(a.off, a.npairs, j, b, e);
        const double dsd = rw_doc_size(a, j);
        double sum = 0.0;   /* wave 0's */
        for (uint64_t p = b; p < e; p += NT) {
            const uint64_t pp = p + threadIdx.x;
            double w = 0.0;
            if (pp < e) {
                w = rw_w(a, pp, dsd);
                a.score[pp] = w;
            }
            if (NORM == TFIDF_NORM_NONE) continue;
            s_x[threadIdx.x] = rw_term<NORM>(w);
            __syncthreads();
            if (wv == 0) {
                const uint32_t n = e - p < (uint64_t)NT ? (uint32_t)(e - p) : (uint32_t)NT;
                for (uint32_t c = 0; c < n; c += 64u) sum = rw_chain(sum, s_x[c + lane], n - c < 64u ? (int)(n - c) : 64);
            }
            __syncthreads();
        }
        if (NORM == TFIDF_NORM_NONE) continue;
        if (threadIdx.x == 0) {
            const double d = rw_divisor<NORM>(sum);
            s_d = d;
            if (d == 0.0) atomicAdd(a.misc + 1, 1u);
        }
        __syncthreads();
        const double d = s_d;
        if (d != 0.0)
            for (uint64_t pp = b + threadIdx.x; pp < e; pp += NT) a.score[pp] = a.score[pp] / d;   /* this thread's own stores */
        __syncthreads();   /* s_d is rewritten by the next document */
    }
}

template <int NORM>
int rw_launch(const RwArgs& a, uint32_t ncu, hipStream_t s) {
    const uint32_t want = (a.ndocs + (NT / 64) - 1) / (NT / 64);
    k_rw_docs<NORM><<<cu_grid(want, ncu, RW_WG_PER_CU), NT, 0, s>>>(a);
    if (ok()) return -1;
    k_rw_docs_big<NORM><<<big_grid(want, ncu), NT, 0, s>>>(a);
    return ok();
}

}  // namespace

int launch_rw_cmax(const uint32_t* count, uint64_t n, const uint32_t* n_dev, uint32_t* cmax, uint32_t* list,
                   uint32_t list_cap, hipStream_t s) {
    if (!n) return 0;
    const uint64_t g = (n + NT - 1) / NT;
    k_rw_cmax<<<(unsigned)(g < 2048u ? g : 2048u), NT, 0, s>>>(count, n, n_dev, cmax, list, list_cap);
    return ok();
}

int launch_rw_idf_rank(const uint32_t* df, uint32_t V, const double* idf, const uint32_t* idf_idx, uint64_t idf_n,
                       double* idf_rank, hipStream_t s) {
    if (!V) return 0;
    k_rw_idf_rank<<<grid_for(V, NT), NT, 0, s>>>(df, V, idf, idf_idx, idf_n, idf_rank);
    return ok();
}

int launch_rw_pairs(const RwArgs& a, uint32_t ncu, hipStream_t s) {
    if (hipMemsetAsync(a.misc, 0, 8, s) != hipSuccess) return -1;
    if (!a.ndocs || !a.npairs) return 0;
    switch (a.norm) {
    case TFIDF_NORM_NONE: return rw_launch<TFIDF_NORM_NONE>(a, ncu, s);
    case TFIDF_NORM_L2: return rw_launch<TFIDF_NORM_L2>(a, ncu, s);
    case TFIDF_NORM_L1: return rw_launch<TFIDF_NORM_L1>(a, ncu, s);
    default: return -1;
    }
}
