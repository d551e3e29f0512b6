/*
 * nb.hip — Naive Bayes classification over the resident result of a run (include/tfidf.h:
 * tfidf_nb_fit, tfidf_nb_predict, tfidf_nb_predict_rows).  The model is two dense matrices in the
 * layout of k-means' centroids, term-major [V][K]: the feature counts FC (u64) and the weights W
 * (f64).  A term's K entries are one contiguous row, so the lanes of a wave read a row with one
 * coalesced load; offsets are 64-bit (t * K + c passes 2^32).
 *
 *   count    document-major: a wave owns a labelled document, its lanes take the pairs and add
 *            x (the count, or 1) into FC[t * K + label] with 64-bit integer atomics.  Integer
 *            sums are exact in any order, so the member-ordered walk that k_km_accum needs for its
 *            floating-point sums (a barrier per member, a workgroup per cluster and term range)
 *            buys nothing here; a term occurs once in a document, so two lanes of a wave never
 *            meet, and contention is between documents of one class on one term only.
 *   sums     a wave per term row: lane l reads the classes l + 64 * i; the row's sum (a wave
 *            reduction) is F[t], and each lane keeps the column sums of its classes over the
 *            wave's rows, added into T[c] once at the end (64-bit integer atomics again).
 *   argmax   the largest log argument and how many lie past the table (integer atomics).
 *   list     those arguments, unordered; the host sorts them, drops the repeats and takes their
 *            logarithms (reweight.hip's table-then-list scheme on 64-bit values).
 *   weights  one thread per entry: the entry's logarithm from the table or by binary search of
 *            the list, and the one rounded subtraction.  No logarithm is taken on the device.
 *   predict  k_km_assign's shape: a wave owns a row; 64 pairs are loaded at once (term, x), then
 *            taken in pair order: term and x are broadcast from the pair's lane, every lane loads
 *            its classes' weights of that row, MU rows in flight, and only then are the products
 *            added, each rounded before its add.  Per (row, class) a fixed sequence of IEEE
 *            operations whatever the grid.  The argmax is a butterfly under (score descending by
 *            value, class ascending): a maximum under a total order (the scores are finite and
 *            never -0.0: a sum that starts at a prior, which is not -0.0, stays so).
 *
 * No product may be fused into an add in this file (similar.hip).  There are no floating-point
 * atomics. */
#include "kernels.h"
#include "dev_common.h"
#include "launch_util.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
typedef unsigned long long ull;

/* ------------------------------------------------------------------- count -- */

/* waves stride over the output positions; a wave owns its document */
__global__ __launch_bounds__(NT) void k_nb_count(const NbFitArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t nwaves = gridDim.x * (NT / 64);
    for (uint32_t j = blockIdx.x * (NT / 64) + wv; j < a.ndocs; j += nwaves) {
        const uint32_t lab = a.lab[j];
        if (lab >= a.K) continue;   /* unlabelled; wave-uniform */
        uint64_t b, e;
        pair_range(a.off, a.npairs, j, b, e);
        for (uint64_t p = b + lane; p < e; p += 64u) {
            const uint32_t t = gload(a.term + p);
            if (t >= a.V) continue;   /* never in a valid result */
            const uint64_t x = a.binary ? 1ull : (uint64_t)gload(a.cnt + p);
            atomicAdd((ull*)(a.FC + (uint64_t)t * a.K + lab), (ull)x);
        }
    }
}

/* -------------------------------------------------------------------- sums -- */

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

/* waves stride over the term rows; lane l owns the classes l + 64 * i */
template <int NA>
__global__ __launch_bounds__(NT) void k_nb_sums(const NbFitArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t nwaves = gridDim.x * (NT / 64);
    uint64_t col[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) col[i] = 0ull;
    for (uint32_t t = blockIdx.x * (NT / 64) + wv; t < a.V; t += nwaves) {
        const uint64_t* row = a.FC + (uint64_t)t * a.K;
        uint64_t mine = 0ull;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const uint32_t c = lane + 64u * i;
            const uint64_t v = c < a.K ? gload(row + c) : 0ull;
            col[i] += v;
            mine += v;
        }
        const uint64_t f = wave_sum_u64(mine);
        if (lane == 0) a.F[t] = f;
    }
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const uint32_t c = lane + 64u * i;
        if (c < a.K && col[i]) atomicAdd((ull*)(a.T + c), (ull)col[i]);
    }
}

/* ------------------------------------------------------- arguments, weights -- */

__device__ __forceinline__ uint64_t nb_arg(const NbFitArgs& a, uint64_t i) {
    const uint64_t fc = gload(a.FC + i);
    return a.complement ? gload(a.F + (uint32_t)(i / a.K)) - fc : fc;
}

__global__ __launch_bounds__(NT) void k_nb_argmax(const NbFitArgs a) {
    const uint64_t n = (uint64_t)a.V * a.K;
    uint64_t mx = 0ull, past = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * NT) {
        const uint64_t m = nb_arg(a, i);
        mx = m > mx ? m : mx;
        past += m >= a.lut_n ? 1ull : 0ull;
    }
    if (mx) atomicMax((ull*)(a.misc + 0), (ull)mx);
    past = wave_sum_u64(past);
    if ((threadIdx.x & 63u) == 0u && past) atomicAdd((ull*)(a.misc + 1), (ull)past);
}

__global__ __launch_bounds__(NT) void k_nb_list(const NbFitArgs a) {
    const uint64_t n = (uint64_t)a.V * a.K;
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * NT) {
        const uint64_t m = nb_arg(a, i);
        if (m >= a.lut_n) {
            const uint64_t at = atomicAdd((ull*)(a.misc + 2), 1ull);
            if (at < a.list_cap) a.list[at] = m;
        }
    }
}

__global__ __launch_bounds__(NT) void k_nb_weights(const NbFitArgs a) {
#pragma clang fp contract(off)
    const uint64_t n = (uint64_t)a.V * a.K;
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * NT) {
        const uint64_t m = nb_arg(a, i);
        double la;
        if (m < a.lut_n) {
            la = gload(a.lut + m);
        } else {
            uint64_t lo = 0, hi = a.list_n;   /* the first key >= m: present by construction */
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (gload(a.list_key + mid) < m) lo = mid + 1; else hi = mid;
            }
            la = lo < a.list_n ? gload(a.list_val + lo) : 0.0;
        }
        const double lc = gload(a.lc + (uint32_t)(i % a.K));
        a.W[i] = a.complement ? lc - la : la - lc;
    }
}

/* ----------------------------------------------------------------- predict -- */

constexpr int MU = 4;   /* rows whose weights are in flight before the first is added */

/* waves stride over the rows; a wave owns its row, lane l the scores of the classes l + 64 * i */
template <int NA>
__global__ __launch_bounds__(NT) void k_nb_predict(const NbPredictArgs a) {
#pragma clang fp contract(off)
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t nwaves = gridDim.x * (NT / 64);
    for (uint32_t r = blockIdx.x * (NT / 64) + wv; r < a.nrows; r += nwaves) {
        const uint32_t j = a.pos ? a.pos[r] : r;
        if (j >= a.ndocs) {   /* not held; wave-uniform */
            if (lane == 0) { a.label[r] = NB_NO_CLASS; a.score[r] = 0.0; }
            if (a.all) {
#pragma unroll
                for (int i = 0; i < NA; ++i) {
                    const uint32_t c = lane + 64u * i;
                    if (c < a.K) a.all[(uint64_t)r * a.K + c] = 0.0;
                }
            }
            continue;
        }
        uint64_t b, e;
        pair_range(a.off, a.npairs, j, b, e);
        if (!a.V) e = b;   /* no matrix: no pairs */
        double acc[NA];
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const uint32_t c = lane + 64u * i;
            acc[i] = c < a.K ? gload(a.prior + c) : 0.0;
        }
        for (uint64_t p = b; p < e; p += 64u) {
            const uint64_t pp = p + lane;
            uint32_t t = pp < e ? gload(a.term + pp) : 0u;
            double x = pp < e ? (a.binary ? 1.0 : (double)gload(a.cnt + pp)) : 0.0;
            if (t >= a.V) { t = 0u; x = 0.0; }   /* never in valid input: adds a zero */
            const int n = e - p < 64u ? (int)(e - p) : 64;
            for (int l0 = 0; l0 < n; l0 += MU) {
                double w[MU][NA], xv[MU];
#pragma unroll
                for (int m = 0; m < MU; ++m) {
                    const int l = l0 + m < n ? l0 + m : n - 1;   /* uniform; the tail's copies are not added */
                    const uint32_t tl = (uint32_t)__builtin_amdgcn_readlane((int)t, l);
                    xv[m] = bcast_f64(x, l);
                    const double* row = a.W + (uint64_t)tl * a.K;
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
                            const double prod = xv[m] * w[m][i];
                            acc[i] = acc[i] + prod;
                        }
                    }
                }
            }
        }
        if (a.all) {
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const uint32_t c = lane + 64u * i;
                if (c < a.K) a.all[(uint64_t)r * a.K + c] = acc[i];
            }
        }
        /* this lane's best: classes ascending, a later one only when strictly larger */
        uint32_t lab = NB_NO_CLASS;
        double best = 0.0;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const uint32_t c = lane + 64u * i;
            if (c < a.K && (lab == NB_NO_CLASS || acc[i] > best)) { best = acc[i]; lab = c; }
        }
        /* the wave's: the largest score by value, the lowest class among equals; a lane past K
         * holds NB_NO_CLASS and loses to every class */
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t bb = (uint64_t)__double_as_longlong(best);
            const uint32_t olo = (uint32_t)__shfl_xor((int)(uint32_t)bb, o, 64);
            const uint32_t ohi = (uint32_t)__shfl_xor((int)(uint32_t)(bb >> 32), o, 64);
            const uint32_t oc = (uint32_t)__shfl_xor((int)lab, o, 64);
            const double ob = __longlong_as_double((long long)(((uint64_t)ohi << 32) | olo));
            const bool take = oc != NB_NO_CLASS && (lab == NB_NO_CLASS || ob > best || (ob == best && oc < lab));
            if (take) { best = ob; lab = oc; }
        }
        if (lane == 0) {
            a.label[r] = lab;
            a.score[r] = best;
        }
    }
}

unsigned wave_grid(uint64_t items, uint32_t ncu) {
    return cu_grid((items + (NT / 64) - 1) / (NT / 64), ncu, NB_WG_PER_CU);
}
unsigned el_grid(uint64_t n, uint32_t ncu) { return cu_grid((n + NT - 1) / NT, ncu, NB_EL_WG_PER_CU); }
bool fit_ok(const NbFitArgs& a) { return a.K && a.K <= NB_MAX_K; }

}  // namespace

int launch_nb_count(const NbFitArgs& a, uint32_t ncu, hipStream_t s) {
    if (!fit_ok(a)) return -1;
    if (a.V && hipMemsetAsync(a.FC, 0, (size_t)a.V * a.K * 8, s) != hipSuccess) return -1;
    if (!a.ndocs || !a.V) return 0;
    k_nb_count<<<wave_grid(a.ndocs, ncu), NT, 0, s>>>(a);
    return ok();
}

int launch_nb_sums(const NbFitArgs& a, uint32_t ncu, hipStream_t s) {
    if (!fit_ok(a)) return -1;
    if (hipMemsetAsync(a.T, 0, (size_t)a.K * 8, s) != hipSuccess) return -1;
    if (!a.V) return 0;
    const unsigned grid = wave_grid(a.V, ncu);
    switch ((a.K + 63u) / 64u) {
        case 1: k_nb_sums<1><<<grid, NT, 0, s>>>(a); break;
        case 2: k_nb_sums<2><<<grid, NT, 0, s>>>(a); break;
        case 3: k_nb_sums<3><<<grid, NT, 0, s>>>(a); break;
        default: k_nb_sums<4><<<grid, NT, 0, s>>>(a); break;
    }
    return ok();
}

int launch_nb_argmax(const NbFitArgs& a, uint32_t ncu, hipStream_t s) {
    if (!fit_ok(a)) return -1;
    if (hipMemsetAsync(a.misc, 0, 3 * 8, s) != hipSuccess) return -1;
    if (!a.V) return 0;
    k_nb_argmax<<<el_grid((uint64_t)a.V * a.K, ncu), NT, 0, s>>>(a);
    return ok();
}

int launch_nb_list(const NbFitArgs& a, uint32_t ncu, hipStream_t s) {
    if (!fit_ok(a)) return -1;
    if (!a.V || !a.list_cap) return 0;
    k_nb_list<<<el_grid((uint64_t)a.V * a.K, ncu), NT, 0, s>>>(a);
    return ok();
}

int launch_nb_weights(const NbFitArgs& a, uint32_t ncu, hipStream_t s) {
    if (!fit_ok(a)) return -1;
    if (!a.V) return 0;
    k_nb_weights<<<el_grid((uint64_t)a.V * a.K, ncu), NT, 0, s>>>(a);
    return ok();
}

int launch_nb_predict(const NbPredictArgs& a, uint32_t ncu, hipStream_t s) {
    if (!a.K || a.K > NB_MAX_K) return -1;
    if (!a.nrows) return 0;
    const unsigned grid = wave_grid(a.nrows, ncu);
    switch ((a.K + 63u) / 64u) {
        case 1: k_nb_predict<1><<<grid, NT, 0, s>>>(a); break;
        case 2: k_nb_predict<2><<<grid, NT, 0, s>>>(a); break;
        case 3: k_nb_predict<3><<<grid, NT, 0, s>>>(a); break;
        default: k_nb_predict<4><<<grid, NT, 0, s>>>(a); break;
    }
    return ok();
}
