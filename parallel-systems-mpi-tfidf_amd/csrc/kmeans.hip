/*
 * kmeans.hip — spherical k-means over the resident result of a run (include/tfidf.h:
 * tfidf_kmeans).  The vectors are the run's scores where it left them in HBM, document-major,
 * terms ascending inside a document; a document's unit vector u(d,t) = s(d,t) / norm(d) is
 * recomputed at every use (one division, the same bits every time).  The centroids are one
 * dense matrix C[V][K]: a term's K weights are one contiguous row, so the lanes of a wave read a
 * row with one coalesced load.  Offsets into it are 64-bit (t * K + c passes 2^32).
 *
 *   assign   one wave owns a document; lane l owns the sums of clusters l, l + 64, .. (NA <= 4
 *            registers).  64 pairs are loaded at once (term, u), then taken in pair order: term
 *            and u are broadcast from the pair's lane, every lane loads its clusters' weights
 *            of that row, MU rows in flight, and only then are the products added, each rounded
 *            before its add.  Per (document, cluster) a fixed sequence of IEEE operations,
 *            whatever the grid; no accumulator is shared between lanes.  The argmax is a
 *            butterfly over (sim bits, cluster): a maximum under a total order, so the order of
 *            the exchange does not matter.  Lane 0 writes label and sim and counts the
 *            cluster's size and the changed labels (integer atomics: exact in any order).
 *   update   the positions are partitioned by label, stably: the sizes' scan gives each
 *            cluster's place, and a workgroup per cluster compacts the positions that carry its
 *            label in ascending order (block scan per tile).  Then `split` workgroups per
 *            cluster walk the cluster's members in that order; each owns a range of term ranks
 *            and adds the member's pairs inside its range, one pair per thread.  A term occurs
 *            once in a document, so no two threads of a member touch the same sum, a barrier
 *            separates the members, and a sum belongs to exactly one workgroup: S[t] is added
 *            in member order without atomics.  The sums are built in the matrix itself (the
 *            columns of clusters with members are cleared first; the others keep their
 *            centroid).  The squared norm is a sequential sum in rank order, one lane per
 *            cluster (the zero entries add +0.0 and change nothing), then one division per entry.
 *   top      the T best entries of every column, one per round: lanes own clusters, waves and
 *            workgroups own term slices, each finds its best entry after the round before's
 *            under (weight descending, rank ascending), a second kernel merges the slices.
 *
 * No product may be fused into an add in this file (similar.hip). */
#include "kernels.h"
#include "dev_common.h"
#include "launch_util.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;

__global__ void k_km_docs(const uint32_t* order, const uint32_t* doc_ids, uint32_t ndocs, uint32_t* id) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ndocs) return;
    id[j] = doc_id_at(order, doc_ids, j);
}

/* -------------------------------------------------------------------- seed -- */

/* a workgroup per cluster */
__global__ __launch_bounds__(NT) void k_km_seed(const KmArgs a) {
#pragma clang fp contract(off)
    const uint32_t c = blockIdx.x;
    if (c >= a.K) return;
    const uint32_t j = a.seedpos[c];
    if (j >= a.ndocs) return;
    uint64_t b, e;
    pair_range(a.out_off, a.npairs, j, b, e);
    const double nrm = a.norm[j];
    if (!(nrm > 0.0)) return;
    for (uint64_t p = b + threadIdx.x; p < e; p += NT) {
        const uint32_t t = gload(a.out_term + p);
        if (t < a.V) a.C[(uint64_t)t * a.K + c] = gload(a.out_score + p) / nrm;
    }
}

/* ------------------------------------------------------------------ assign -- */

constexpr int MU = 4;   /* rows whose weights are in flight before the first is added */

/* waves stride over the output positions; a wave owns its document, lane l the sums of the
 * clusters l + 64 * i, i < NA */
template <int NA>
__global__ __launch_bounds__(NT) void k_km_assign(const KmArgs a) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t nwaves = gridDim.x * (NT / 64);
    for (uint32_t j = blockIdx.x * (NT / 64) + wv; j < a.ndocs; j += nwaves) {
        uint64_t b, e;
        pair_range(a.out_off, a.npairs, j, b, e);
        const double nrm = a.norm[j];
        uint32_t lab = KM_NO_CLUSTER;
        uint64_t best = 0ull;
        if (nrm > 0.0) {   /* wave-uniform */
            double acc[NA];
#pragma unroll
            for (int i = 0; i < NA; ++i) acc[i] = 0.0;
            for (uint64_t p = b; p < e; p += 64u) {
                const uint64_t pp = p + lane;
                uint32_t t = pp < e ? gload(a.out_term + pp) : 0u;
                double u = pp < e ? gload(a.out_score + pp) / nrm : 0.0;
                if (t >= a.V) { t = 0u; u = 0.0; }   /* never in a valid result: adds +0.0 */
                const int n = e - p < 64u ? (int)(e - p) : 64;
                for (int l0 = 0; l0 < n; l0 += MU) {
                    double w[MU][NA], uv[MU];
#pragma unroll
                    for (int m = 0; m < MU; ++m) {
                        const int l = l0 + m < n ? l0 + m : n - 1;   /* uniform; the tail's copies are not added */
                        const uint32_t tl = (uint32_t)__builtin_amdgcn_readlane((int)t, l);
                        uv[m] = bcast_f64(u, l);
                        const double* row = a.C + (uint64_t)tl * a.K;
#pragma unroll
                        for (int i = 0; i < NA; ++i) {
                            const uint32_t c = lane + 64u * i;
                            w[m][i] = c < a.K ? gload(row + c) : 0.0;
                        }
                    }
#pragma unroll
                    for (int m = 0; m < MU; ++m) {
                        if (l0 + m < n) {   /* uniform */
#pragma unroll
                            for (int i = 0; i < NA; ++i) {
                                const double prod = uv[m] * w[m][i];
                                acc[i] = acc[i] + prod;
                            }
                        }
                    }
                }
            }
            /* this lane's best: clusters ascending, a later one only when strictly larger */
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const uint32_t c = lane + 64u * i;
                const uint64_t bits = (uint64_t)__double_as_longlong(acc[i]);
                if (c < a.K && (lab == KM_NO_CLUSTER || bits > best)) { best = bits; lab = c; }
            }
            /* the wave's: the largest sim, the lowest cluster among equals */
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const uint32_t olo = (uint32_t)__shfl_xor((int)(uint32_t)best, o, 64);
                const uint32_t ohi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), o, 64);
                const uint32_t oc = (uint32_t)__shfl_xor((int)lab, o, 64);
                const uint64_t ob = ((uint64_t)ohi << 32) | olo;
                if (ob > best || (ob == best && oc < lab)) { best = ob; lab = oc; }
            }
        }
        if (lane == 0) {
            a.label[j] = lab;
            a.sim[j] = __longlong_as_double((long long)best);
            if (lab < a.K) atomicAdd(a.size + lab, 1u);
            if (a.prev && a.prev[j] != lab) atomicAdd(a.changed, 1u);
        }
    }
}

/* ------------------------------------------------------------------ update -- */

/* moff = the exclusive scan of size (K <= 256: one workgroup) */
__global__ __launch_bounds__(NT) void k_km_moff(const KmArgs a) {
    __shared__ uint32_t wsum[NT / 64];
    const uint32_t v = threadIdx.x < a.K ? a.size[threadIdx.x] : 0u;
    uint32_t total = 0;
    const uint32_t at = block_excl_scan<NT>(v, wsum, &total);
    if (threadIdx.x < a.K) a.moff[threadIdx.x] = at;
    if (threadIdx.x == 0) a.moff[a.K] = total;
}

/* a workgroup per cluster: the positions carrying its label, ascending */
__global__ __launch_bounds__(NT) void k_km_members(const KmArgs a) {
    __shared__ uint32_t wsum[NT / 64];
    const uint32_t c = blockIdx.x;
    if (c >= a.K) return;
    uint32_t base = a.moff[c];
    for (uint32_t j0 = 0; j0 < a.ndocs; j0 += NT) {   /* uniform trip count */
        const uint32_t j = j0 + threadIdx.x;
        const uint32_t hit = j < a.ndocs && a.label[j] == c ? 1u : 0u;
        uint32_t total = 0;
        const uint32_t at = block_excl_scan<NT>(hit, wsum, &total);
        if (hit && base + at < a.ndocs) a.members[base + at] = j;
        base += total;
    }
}

/* the columns of the clusters with members: 0 */
__global__ void k_km_clear(const KmArgs a) {
    const uint64_t n = (uint64_t)a.V * a.K;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (a.size[(uint32_t)(i % a.K)]) a.C[i] = 0.0;
}

/* workgroup (c, g): cluster c's members in order, the pairs whose rank is in range g */
__global__ __launch_bounds__(NT) void k_km_accum(const KmArgs a) {
#pragma clang fp contract(off)
    const uint32_t c = blockIdx.x, g = blockIdx.y, G = gridDim.y;
    if (c >= a.K) return;
    const uint32_t n = a.size[c], m0 = a.moff[c];
    const uint32_t tlo = (uint32_t)((uint64_t)a.V * g / G), thi = (uint32_t)((uint64_t)a.V * (g + 1u) / G);
    if (tlo >= thi) return;   /* uniform */
    for (uint32_t m = 0; m < n; ++m) {
        if (m0 + m >= a.ndocs) break;   /* uniform */
        const uint32_t j = a.members[m0 + m];
        if (j < a.ndocs) {
            uint64_t b, e;
            pair_range(a.out_off, a.npairs, j, b, e);
            const double nrm = a.norm[j];
            if (G > 1u && e - b > 4u * NT) {   /* a long document: start at the range's first pair */
                uint64_t lo = b, hi = e;
                while (lo < hi) {
                    const uint64_t mid = lo + (hi - lo) / 2;
                    if (gload(a.out_term + mid) < tlo) lo = mid + 1; else hi = mid;
                }
                b = lo;
            }
            if (nrm > 0.0) {
                for (uint64_t p = b + threadIdx.x; p < e; p += NT) {
                    const uint32_t t = gload(a.out_term + p);
                    if (t >= thi) break;   /* terms ascend inside a document */
                    if (t >= tlo) {
                        double* x = a.C + (uint64_t)t * a.K + c;
                        *x = *x + gload(a.out_score + p) / nrm;
                    }
                }
            }
        }
        __syncthreads();   /* the next member's adds come after this one's */
    }
}

/* lane = cluster: the column's squares added in rank order */
__global__ __launch_bounds__(64) void k_km_cnorm(const KmArgs a) {
#pragma clang fp contract(off)
    const uint32_t c = blockIdx.x * 64u + threadIdx.x;
    if (c >= a.K || !a.size[c]) return;
    double sum = 0.0;
    for (uint32_t t = 0; t < a.V; t += 8u) {
        double x[8];
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) x[i] = t + i < a.V ? gload(a.C + (uint64_t)(t + i) * a.K + c) : 0.0;
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) {
            const double prod = x[i] * x[i];
            sum = sum + prod;
        }
    }
    a.cnorm[c] = __dsqrt_rn(sum);
}

__global__ void k_km_scale(const KmArgs a) {
#pragma clang fp contract(off)
    const uint64_t n = (uint64_t)a.V * a.K;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t c = (uint32_t)(i % a.K);
        if (a.size[c]) a.C[i] = a.C[i] / a.cnorm[c];
    }
}

/* --------------------------------------------------------------- top terms -- */

constexpr uint32_t TOP_NONE = 0xFFFFFFFFu;

__global__ void k_km_top_init(const KmTopArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.K) {
        a.prev[2 * i] = ~0ull;   /* above every weight's bits */
        a.prev[2 * i + 1] = 0ull;
        a.n[i] = 0u;
    }
    if (i < a.K * a.T) {
        a.term[i] = TOP_NONE;
        a.weight[i] = 0ull;
    }
}

/* workgroup (cluster group, slice): lane = cluster, the four waves interleave the slice's terms;
 * the best entry after prev[c] under (weight descending, rank ascending) */
__global__ __launch_bounds__(NT) void k_km_top_part(const KmTopArgs a) {
    __shared__ uint64_t sb[NT];
    __shared__ uint32_t st[NT];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x * 64u + lane, s = blockIdx.y;
    const uint32_t lo = (uint32_t)((uint64_t)a.V * s / KM_TOP_SLICES), hi = (uint32_t)((uint64_t)a.V * (s + 1u) / KM_TOP_SLICES);
    uint64_t bb = 0ull;
    uint32_t bt = TOP_NONE;
    if (c < a.K) {
        const uint64_t pb = a.prev[2 * c];
        const uint32_t pt = (uint32_t)a.prev[2 * c + 1];
        for (uint32_t t = lo + wv; t < hi; t += NT / 64) {
            const uint64_t bits = (uint64_t)__double_as_longlong(gload(a.C + (uint64_t)t * a.K + c));
            const bool cand = bits != 0ull && (bits < pb || (bits == pb && t > pt));
            if (cand && (bt == TOP_NONE || bits > bb)) { bb = bits; bt = t; }   /* t ascends: the first of equals stays */
        }
    }
    sb[threadIdx.x] = bb;
    st[threadIdx.x] = bt;
    __syncthreads();
    if (wv == 0 && c < a.K) {
        for (uint32_t w = 1; w < NT / 64; ++w) {
            const uint64_t ob = sb[w * 64 + lane];
            const uint32_t ot = st[w * 64 + lane];
            if (ot != TOP_NONE && (bt == TOP_NONE || ob > bb || (ob == bb && ot < bt))) { bb = ob; bt = ot; }
        }
        a.part[2 * ((uint64_t)s * a.K + c)] = bb;
        a.part[2 * ((uint64_t)s * a.K + c) + 1] = bt;
    }
}

/* a thread per cluster: the slices' best -> entry r of the cluster's list */
__global__ void k_km_top_merge(const KmTopArgs a, uint32_t r) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.K || r >= a.T) return;
    uint64_t bb = 0ull;
    uint32_t bt = TOP_NONE;
    for (uint32_t s = 0; s < KM_TOP_SLICES; ++s) {   /* slices ascend in rank */
        const uint64_t ob = a.part[2 * ((uint64_t)s * a.K + c)];
        const uint32_t ot = (uint32_t)a.part[2 * ((uint64_t)s * a.K + c) + 1];
        if (ot != TOP_NONE && (bt == TOP_NONE || ob > bb)) { bb = ob; bt = ot; }
    }
    if (bt != TOP_NONE) {
        a.term[(uint64_t)c * a.T + r] = bt;
        a.weight[(uint64_t)c * a.T + r] = bb;
        a.n[c] = r + 1u;
        a.prev[2 * c] = bb;
        a.prev[2 * c + 1] = bt;
    } else {
        a.prev[2 * c] = 0ull;   /* nothing is below +0.0: the list is complete */
        a.prev[2 * c + 1] = TOP_NONE;
    }
}

__global__ void k_km_wlen(const KmTopArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = a.K * a.T;
    if (i > n) return;
    uint64_t len = 0;
    if (i < n) {
        const uint32_t t = a.term[i];
        if (t < a.V) len = a.tlen[t];
    }
    a.wlen[i] = len;
}

}  // namespace

int launch_km_docs(const uint32_t* order, const uint32_t* doc_ids, uint32_t ndocs, uint32_t* id, hipStream_t s) {
    if (!ndocs) return 0;
    k_km_docs<<<grid_for(ndocs), NT, 0, s>>>(order, doc_ids, ndocs, id);
    return ok();
}

int launch_km_seed(const KmArgs& a, hipStream_t s) {
    if (!a.K || a.K > KM_MAX_K || !a.V) return a.K > KM_MAX_K ? -1 : 0;
    if (hipMemsetAsync(a.C, 0, (size_t)a.V * a.K * 8, s) != hipSuccess) return -1;
    k_km_seed<<<a.K, NT, 0, s>>>(a);
    return ok();
}

int launch_km_assign(const KmArgs& a, uint32_t ncu, hipStream_t s) {
    if (!a.K || a.K > KM_MAX_K) return -1;
    if (hipMemsetAsync(a.changed, 0, 4, s) != hipSuccess) return -1;
    if (hipMemsetAsync(a.size, 0, (size_t)a.K * 4, s) != hipSuccess) return -1;
    if (!a.ndocs) return 0;
    const uint32_t want = (a.ndocs + (NT / 64) - 1) / (NT / 64);
    const uint32_t grid = cu_grid(want, ncu, KM_WG_PER_CU);   /* no LDS: the waves a CU holds */
    switch ((a.K + 63u) / 64u) {
        case 1: k_km_assign<1><<<grid, NT, 0, s>>>(a); break;
        case 2: k_km_assign<2><<<grid, NT, 0, s>>>(a); break;
        case 3: k_km_assign<3><<<grid, NT, 0, s>>>(a); break;
        default: k_km_assign<4><<<grid, NT, 0, s>>>(a); break;
    }
    return ok();
}

int launch_km_update(const KmArgs& a, uint32_t split, hipStream_t s) {
    if (!a.K || a.K > KM_MAX_K) return -1;
    if (!a.ndocs || !a.V) return 0;
    if (split < 1u) split = 1u;
    if (split > 1024u) split = 1024u;
    const uint64_t n = (uint64_t)a.V * a.K;
    const unsigned eg = n / NT + 1 < 8192 ? (unsigned)(n / NT + 1) : 8192u;
    k_km_moff<<<1, NT, 0, s>>>(a);
    if (ok()) return -1;
    k_km_members<<<a.K, NT, 0, s>>>(a);
    if (ok()) return -1;
    k_km_clear<<<eg, NT, 0, s>>>(a);
    if (ok()) return -1;
    k_km_accum<<<dim3(a.K, split), NT, 0, s>>>(a);
    if (ok()) return -1;
    k_km_cnorm<<<(a.K + 63u) / 64u, 64, 0, s>>>(a);
    if (ok()) return -1;
    k_km_scale<<<eg, NT, 0, s>>>(a);
    return ok();
}

int launch_km_top(const KmTopArgs& a, hipStream_t s) {
    if (!a.K || a.K > KM_MAX_K || a.T > KM_MAX_TERMS) return -1;
    k_km_top_init<<<grid_for((uint64_t)a.K * (a.T ? a.T : 1u)), NT, 0, s>>>(a);
    if (ok()) return -1;
    for (uint32_t r = 0; r < a.T; ++r) {
        k_km_top_part<<<dim3((a.K + 63u) / 64u, KM_TOP_SLICES), NT, 0, s>>>(a);
        if (ok()) return -1;
        k_km_top_merge<<<grid_for(a.K), NT, 0, s>>>(a, r);
        if (ok()) return -1;
    }
    k_km_wlen<<<grid_for((uint64_t)a.K * a.T + 1), NT, 0, s>>>(a);
    return ok();
}
