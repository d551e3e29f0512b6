/*
 * similar.hip — top-k similar documents over the resident result of a run (include/tfidf.h:
 * tfidf_similar): nearest neighbours under the cosine similarity of the TF-IDF vectors.  The
 * reference stops at the sorted "docN@word\t%.16f" lines (TFIDF.c:245,273-282); the vectors
 * are the same scores (TFIDF.c:202,243-244) where the run left them in HBM, document-major,
 * terms ascending inside a document.
 *
 *   norms    one wave per document: 64 scores are loaded and squared at once (each product
 *            rounded on its own), then added in pair order, one lane's product after the
 *            other, into one sum that every lane carries; sqrt is the correctly rounded one.
 *   table    a group of <= SG_MAX rows becomes a term -> postings table indexed directly by
 *            term rank: mask[t] has bit r set when row r holds term t (64-bit atomic OR), the
 *            exclusive scan (prims.hip) of the masks' popcounts gives post_off, and row r's
 *            weight for t is post_w[post_off[t] + popcount(mask[t] below bit r)]: every
 *            posting's place is a function of the masks, so the fill needs no cursor and the
 *            table's layout is the same in every run.  The rows' vectors are read where they
 *            are: the resident pairs, or (vectors another shard exported) the ranks
 *            k_query_lookup found with the exported scores.
 *   score    one scan of out_term / out_score per group.  One wave owns a document; lane r
 *            owns row r's sum in a register.  A pair's term indexes mask / post_off directly
 *            (no filter, no search: the table is thousands of terms wide and the frequent
 *            terms are all in it).  The pairs whose mask is not empty are taken in pair order,
 *            four at a time: mask, offset and score are broadcast from the pair's lane, every
 *            lane whose bit is set loads its weight, and only then are the four products
 *            added, each rounded before its add: per (row, document) a fixed sequence of IEEE
 *            operations, whatever the grid, and no accumulator is shared between lanes (no
 *            LDS, no atomics).  Documents over QS_BIG pairs are handed to a second launch, one
 *            workgroup each, which compacts every tile of 256 pairs in pair order into LDS
 *            (docscan.h's scheme) for wave 0 to add.  The owner turns the sums into
 *            similarities as it writes them: dot / (norm * norm), +0.0 for a zero
 *            denominator, and the row's own position gets count 0.
 *   top-k    k_query_topk over the dense (row, output position) arrays, then the neighbours'
 *            positions (k_terms_lookup) and their shared-term counts.
 *
 * No product may be fused into an add in this file (hipcc contracts a * b + c by default, and
 * through __dmul_rn / __dadd_rn as well: docscan.h). */
#include "kernels.h"
#include "dev_common.h"
#include "launch_util.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;

/* ------------------------------------------------------------------- norms -- */

__global__ __launch_bounds__(NT) void k_sim_norms(const uint64_t* out_off, const double* out_score, uint32_t ndocs,
                                                  uint64_t npairs, double* sq, double* norm) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t j = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (j >= ndocs) return;   /* wave-uniform */
    uint64_t b, e;
    pair_range(out_off, npairs, j, b, e);
    double sum = 0.0;
    for (uint64_t p = b; p < e; p += 64u) {
        const uint64_t pp = p + lane;
        const double s = pp < e ? gload(out_score + pp) : 0.0;
        const double prod = s * s;
        const int n = e - p < 64u ? (int)(e - p) : 64;
        for (int l = 0; l < n; ++l) sum = sum + bcast_f64(prod, l);
    }
    if (lane == 0) {
        sq[j] = sum;
        norm[j] = __dsqrt_rn(sum);
    }
}

/* -------------------------------------------------------------------- rows -- */

__global__ void k_sim_rows(const SimRowArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nrows) return;
    const uint32_t j = a.pos ? a.pos[i] : i;
    uint64_t b = 0, e = 0;
    double n = 0.0, q = 0.0;
    uint32_t id = 0;
    if (j < a.ndocs) {
        pair_range(a.out_off, a.npairs, j, b, e);
        n = a.norm[j];
        q = a.sq[j];
        id = doc_id_at(a.order, a.doc_ids, j);
    }
    a.rb[i] = b;
    a.re[i] = e;
    a.rnorm[i] = n;
    a.rsq[i] = q;
    a.rpos[i] = j < a.ndocs ? j : 0xFFFFFFFFu;
    a.rid[i] = id;
}

/* ------------------------------------------------------------------- table -- */

/* a workgroup per row */
__global__ __launch_bounds__(NT) void k_sim_mark(const SimTabArgs a) {
    const uint32_t r = blockIdx.x;
    if (r >= a.nrows || r >= SG_MAX) return;
    uint64_t b = a.rb[r], e = a.re[r];
    if (e > a.nentries) e = a.nentries;
    for (uint64_t p = b + threadIdx.x; p < e; p += NT) {
        const uint32_t t = gload(a.term + p);
        if (t < a.V) atomicOr((unsigned long long*)a.mask + t, 1ull << r);
    }
}

__global__ void k_sim_popc(const uint64_t* mask, uint32_t V, uint32_t* cnt) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < V) cnt[t] = (uint32_t)__popcll(mask[t]);
}

__global__ __launch_bounds__(NT) void k_sim_fill(const SimTabArgs a) {
    const uint32_t r = blockIdx.x;
    if (r >= a.nrows || r >= SG_MAX) return;
    uint64_t b = a.rb[r], e = a.re[r];
    if (e > a.nentries) e = a.nentries;
    for (uint64_t p = b + threadIdx.x; p < e; p += NT) {
        const uint32_t t = gload(a.term + p);
        if (t >= a.V) continue;
        const uint64_t x = (uint64_t)a.post_off[t] + (uint32_t)__popcll(a.mask[t] & ((1ull << r) - 1ull));
        if (x < a.post_cap) a.post_w[x] = gload(a.score + p);
    }
}

/* ------------------------------------------------------------------- score -- */

/* a pair's table entry: the rows holding its term and where their weights start */
__device__ __forceinline__ void term_entry(const SimScoreArgs& a, uint32_t t, uint64_t& M, uint32_t& o) {
    M = 0ull;
    o = 0u;
    if (t < a.V) {
        M = gload(a.mask + t);
        o = gload(a.post_off + t);
    }
}

/* lane r's weight for a term with rows M whose weights start at o (valid when bit r is set) */
__device__ __forceinline__ double weight_of(const SimScoreArgs& a, uint64_t M, uint32_t o, uint32_t lane) {
    const uint64_t x = (uint64_t)o + (uint32_t)__popcll(M & ((1ull << lane) - 1ull));
    return x < a.post_cap ? gload(a.post_w + x) : 0.0;
}

/* lane r's sum -> the similarity of row r and the document at position j */
__device__ __forceinline__ void write_doc(const SimScoreArgs& a, uint32_t j, double dot, uint32_t c, uint32_t lane) {
#pragma clang fp contract(off)
    if (lane < a.nq) {
        const double den = a.rnorm[lane] * a.dnorm[j];
        if (a.rpos[lane] == j) c = 0u;   /* the row's own document is no neighbour */
        a.acc[(uint64_t)lane * a.ndocs + j] = den == 0.0 ? 0.0 : dot / den;
        a.cnt[(uint64_t)lane * a.ndocs + j] = c;
    }
}

constexpr int MU = 4;   /* matches whose weights are in flight before the first is added */

/* waves stride over the output positions; a wave owns its document, lane r row r's sum */
__global__ __launch_bounds__(NT) void k_sim_score(const SimScoreArgs a) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t nwaves = gridDim.x * (NT / 64);
    for (uint32_t j = blockIdx.x * (NT / 64) + wv; j < a.ndocs; j += nwaves) {
        uint64_t b, e;
        pair_range(a.out_off, a.npairs, j, b, e);
        if (e - b > QS_BIG) {   /* the second launch's: one workgroup per such document */
            if (lane == 0) hand_to_big(a.big_list, a.big_count, a.ndocs, j);
            continue;
        }
        double acc = 0.0;
        uint32_t cnt = 0u;
        for (uint64_t p = b; p < e; p += 256u) {
            uint32_t t[4], o[4];
            uint64_t M[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {   /* four rounds' terms in flight */
                const uint64_t pp = p + 64u * u + lane;
                t[u] = pp < e ? gload(a.out_term + pp) : QUERY_NO_TERM;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) term_entry(a, t[u], M[u], o[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint64_t pp = p + 64u * u + lane;
                const bool hit = M[u] != 0ull;
                uint64_t m = __ballot(hit);
                if (m == 0ull) continue;
                const double s = hit ? gload(a.out_score + pp) : 0.0;
                while (m) {   /* the round's matches in pair order, MU at a time */
                    double w[MU], sv[MU];
                    bool h[MU];
#pragma unroll
                    for (int i = 0; i < MU; ++i) {
                        h[i] = false;
                        w[i] = 0.0;
                        sv[i] = 0.0;
                        if (m) {   /* uniform */
                            const int l = __builtin_ctzll(m);
                            m &= m - 1ull;
                            const uint64_t Ml = bcast_u64(M[u], l);
                            const uint32_t ol = (uint32_t)__builtin_amdgcn_readlane((int)o[u], l);
                            sv[i] = bcast_f64(s, l);
                            h[i] = (Ml >> lane) & 1ull;
                            if (h[i]) w[i] = weight_of(a, Ml, ol, lane);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < MU; ++i) {
                        if (h[i]) {
                            const double prod = w[i] * sv[i];
                            acc = acc + prod;
                            cnt += 1u;
                        }
                    }
                }
            }
        }
        write_doc(a, j, acc, cnt, lane);
    }
}

/* documents over QS_BIG pairs: workgroups stride over the first launch's list */
__global__ __launch_bounds__(NT) void k_sim_score_big(const SimScoreArgs a) {
#pragma clang fp contract(off)
    __shared__ uint64_t m_M[NT];
    __shared__ uint32_t m_o[NT];
    __shared__ double m_s[NT];
    __shared__ uint32_t wsum[NT / 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t nbig = *a.big_count;
    if (nbig > a.ndocs) nbig = a.ndocs;
    for (uint32_t k = blockIdx.x; k < nbig; k += gridDim.x) {
        const uint32_t j = a.big_list[k];
        if (j >= a.ndocs) continue;
        uint64_t b, e;
        pair_range(a.out_off, a.npairs, j, b, e);
        double acc = 0.0;      /* wave 0's lanes: row r's sum */
        uint32_t cnt = 0u;
        for (uint64_t p = b; p < e; p += NT) {
            const uint64_t pp = p + threadIdx.x;
            uint64_t M = 0ull;
            uint32_t o = 0u;
            if (pp < e) term_entry(a, gload(a.out_term + pp), M, o);
            const uint32_t hit = M != 0ull ? 1u : 0u;
            if (__syncthreads_count((int)hit) == 0) continue;   /* uniform: every thread sees the count */
            uint32_t total = 0;
            const uint32_t at = block_excl_scan<NT>(hit, wsum, &total);   /* pair order */
            if (hit) { m_M[at] = M; m_o[at] = o; m_s[at] = gload(a.out_score + pp); }
            __syncthreads();
            if (wv == 0) {
                for (uint32_t x0 = 0; x0 < total; x0 += MU) {
                    double w[MU], sv[MU];
                    bool h[MU];
#pragma unroll
                    for (int i = 0; i < MU; ++i) {
                        h[i] = false;
                        w[i] = 0.0;
                        sv[i] = 0.0;
                        if (x0 + i < total) {
                            const uint64_t Ml = m_M[x0 + i];
                            sv[i] = m_s[x0 + i];
                            h[i] = (Ml >> lane) & 1ull;
                            if (h[i]) w[i] = weight_of(a, Ml, m_o[x0 + i], lane);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < MU; ++i) {
                        if (h[i]) {
                            const double prod = w[i] * sv[i];
                            acc = acc + prod;
                            cnt += 1u;
                        }
                    }
                }
            }
            __syncthreads();
        }
        if (wv == 0) write_doc(a, j, acc, cnt, lane);
    }
}

/* ------------------------------------------------------------------ shared -- */

__global__ void k_sim_shared(const uint32_t* cnt, const uint32_t* pos, const uint32_t* n_of_row, uint32_t nrows,
                             uint32_t k, uint32_t ndocs, uint32_t* shared) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (uint64_t)nrows * k) return;
    const uint32_t row = (uint32_t)(e / k), i = (uint32_t)(e % k);
    uint32_t v = 0u;
    if (i < n_of_row[row]) {
        const uint32_t j = pos[e];
        if (j < ndocs) v = cnt[(uint64_t)row * ndocs + j];
    }
    shared[e] = v;
}

/* ------------------------------------------------------------------ export -- */

__global__ __launch_bounds__(NT) void k_sim_export(const SimExportArgs a) {
    const uint32_t r = blockIdx.x;
    if (r >= a.nrows) return;
    const uint64_t b = a.rb[r], e = a.re[r], o = a.eoff[r];
    for (uint64_t x = threadIdx.x; x < e - b; x += NT) {
        const uint32_t t = gload(a.out_term + b + x);
        a.term[o + x] = t;
        a.score[o + x] = gload(a.out_score + b + x);
        a.wlen[o + x] = t < a.V ? a.tlen[t] : 0u;
    }
}

}  // namespace

int launch_sim_norms(const uint64_t* out_off, const double* out_score, uint32_t ndocs, uint64_t npairs, double* sq,
                     double* norm, hipStream_t s) {
    if (!ndocs) return 0;
    k_sim_norms<<<grid_for(ndocs, NT / 64), NT, 0, s>>>(out_off, out_score, ndocs, npairs, sq, norm);
    return ok();
}

int launch_sim_rows(const SimRowArgs& a, hipStream_t s) {
    if (!a.nrows) return 0;
    k_sim_rows<<<grid_for(a.nrows), NT, 0, s>>>(a);
    return ok();
}

int launch_sim_mark(const SimTabArgs& a, hipStream_t s) {
    if (!a.nrows) return 0;
    if (a.nrows > SG_MAX) return -1;
    k_sim_mark<<<a.nrows, NT, 0, s>>>(a);
    if (ok()) return -1;
    k_sim_popc<<<grid_for(a.V), NT, 0, s>>>(a.mask, a.V, a.cnt);
    return ok();
}

int launch_sim_fill(const SimTabArgs& a, hipStream_t s) {
    if (!a.nrows) return 0;
    if (a.nrows > SG_MAX) return -1;
    k_sim_fill<<<a.nrows, NT, 0, s>>>(a);
    return ok();
}

int launch_sim_score(const SimScoreArgs& a, uint32_t ncu, hipStream_t s) {
    if (!a.ndocs || !a.nq || a.nq > SG_MAX) return a.nq > SG_MAX ? -1 : 0;
    if (hipMemsetAsync(a.big_count, 0, 4, s) != hipSuccess) return -1;
    const uint32_t want = (a.ndocs + (NT / 64) - 1) / (NT / 64);
    k_sim_score<<<cu_grid(want, ncu, SM_WG_PER_CU), NT, 0, s>>>(a);   /* no LDS: the waves a CU holds */
    if (ok()) return -1;
    k_sim_score_big<<<big_grid(want, ncu), NT, 0, s>>>(a);
    return ok();
}

int launch_sim_shared(const uint32_t* cnt, const uint32_t* pos, const uint32_t* n_of_row, uint32_t nrows, uint32_t k,
                      uint32_t ndocs, uint32_t* shared, hipStream_t s) {
    if (!nrows || !k) return 0;
    k_sim_shared<<<grid_for((uint64_t)nrows * k), NT, 0, s>>>(cnt, pos, n_of_row, nrows, k, ndocs, shared);
    return ok();
}

int launch_sim_export(const SimExportArgs& a, hipStream_t s) {
    if (!a.nrows) return 0;
    k_sim_export<<<a.nrows, NT, 0, s>>>(a);
    return ok();
}
