/*
 * dedup.hip — near-duplicate detection over the resident result (include/tfidf.h, section "near
 * duplicates"; driver: engine_dedup.cpp).  The reference has no such pass.
 *
 *   k_dd_h0         one lane per term rank: mix64(FNV-1a-64(term bytes)).
 *   k_dd_sig        the hot pass, document-major.  A wave owns a document and its lanes own the
 *                   hash functions (H / 64 of them per lane: the multiplier's two halves, the
 *                   offset and the running minimum in registers).  The document's pairs come 64
 *                   at a time (a coalesced out_term load, an h0 gather); every h0 is broadcast to
 *                   the wave with two v_readlane, so there is no cross-lane reduction and no
 *                   atomic.  (u32)((a * x) >> 32) is one mul_hi and two mul_lo.
 *   k_dd_sig_big    documents over DD_BIG_PAIRS pairs, a workgroup each: the waves take the
 *                   document's 64-pair tiles in turn and combine their minima in LDS.
 *   k_dd_bandkeys   one lane per (band, document with pairs).
 *   k_dd_runflag / k_dd_runwrite, k_dd_uniqflag / k_dd_uniqwrite
 *                   flag -> scan (prims.h) -> write over the sorted band keys and over the sorted
 *                   candidates: the chain candidates, then their set.
 *   k_dd_verify     a wave per candidate: lanes take terms of the shorter list and binary-search
 *                   the longer one; the wave's sum is `shared`; a compare loop over the two
 *                   signatures gives `same`.  k_dd_verify_big: a workgroup per candidate that
 *                   holds a document over DD_BIG_PAIRS pairs.
 * Minima and integer sums are order-free: no result depends on the grid or on which launch takes
 * a document.  The only atomics build the lists of big documents and candidates, whose order
 * shows in no result.
 */
#include "dev_common.h"
#include "kernels.h"
#include "launch_util.h"

namespace {

constexpr int NT = 256;

__device__ __forceinline__ uint64_t fnv_step(uint64_t h, uint32_t c) { return (h ^ (uint64_t)c) * 0x100000001B3ull; }

__global__ void k_dd_h0(const uint4* __restrict__ tkey, const uint32_t* __restrict__ tlen, uint32_t V,
                        const uint8_t* __restrict__ corpus, uint64_t corpus_bytes, uint64_t* __restrict__ h0) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= V) return;
    const uint4 k = tkey[r];
    const uint32_t len = tlen[r];
    uint64_t h = 0xCBF29CE484222325ull;
    if (k.w == 0xFFFFFFFFu) {   /* long term: (length << 40 | corpus offset) in the key's low half (k_term_meta) */
        const uint64_t off = (((uint64_t)k.y << 32) | k.x) & 0xFFFFFFFFFFull;
        const bool in = off + len <= corpus_bytes;
        for (uint32_t x = 0; x < len; ++x) h = fnv_step(h, in ? corpus[off + x] : 0u);
    } else {
        const uint32_t w[4] = {k.x, k.y, k.z, k.w};
        for (uint32_t x = 0; x < len && x < 16u; ++x) h = fnv_step(h, (w[x >> 2] >> (8u * (x & 3u))) & 0xFFu);
    }
    h0[r] = mix64(h);
}

/* a lane's hash functions: i = lane + 64 * k, k < HPL */
template <int HPL> struct Fam {
    uint32_t alo[HPL], ahi[HPL], b[HPL], mn[HPL];
};
template <int HPL>
__device__ __forceinline__ void fam_load(const DdSigArgs& a, uint32_t lane, Fam<HPL>& f) {
#pragma unroll
    for (int k = 0; k < HPL; ++k) {
        const uint32_t i = lane + 64u * k;   /* < DD_MAX_H: the tables are DD_MAX_H long */
        const uint64_t av = a.fam_a[i];
        f.alo[k] = (uint32_t)av;
        f.ahi[k] = (uint32_t)(av >> 32);
        f.b[k] = a.fam_b[i];
        f.mn[k] = 0xFFFFFFFFu;
    }
}
/* one 64-pair tile at p (pairs [p, e) of it): the lanes load, then every pair's h0 visits every lane */
template <int HPL>
__device__ __forceinline__ void sig_tile(const DdSigArgs& a, uint64_t p, uint64_t e, uint32_t lane, Fam<HPL>& f) {
    const uint64_t pp = p + lane;
    uint64_t x = 0;
    bool have = false;
    if (pp < e) {
        const uint32_t t = gload(a.term + pp);
        if (t < a.V) { x = gload(a.h0 + t); have = true; }
    }
    uint64_t m = __ballot(have);
    while (m) {   /* wave-uniform */
        const int l = __builtin_ctzll(m);
        m &= m - 1ull;
        const uint64_t xv = bcast_u64(x, l);
        const uint32_t xlo = (uint32_t)xv, xhi = (uint32_t)(xv >> 32);
#pragma unroll
        for (int k = 0; k < HPL; ++k) {
            const uint32_t g = __umulhi(f.alo[k], xlo) + f.alo[k] * xhi + f.ahi[k] * xlo + f.b[k];
            f.mn[k] = g < f.mn[k] ? g : f.mn[k];
        }
    }
}

/* waves stride over the output positions; a wave owns its document */
template <int HPL>
__global__ __launch_bounds__(NT) void k_dd_sig(const DdSigArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t nwaves = gridDim.x * (NT / 64);
    for (uint32_t j = blockIdx.x * (NT / 64) + wv; j < a.ndocs; j += nwaves) {
        uint64_t b, e;
        pair_range(a.off, a.npairs, j, b, e);
        if (e - b > DD_BIG_PAIRS) {   /* the second launch's: one workgroup per such document */
            if (lane == 0) hand_to_big(a.big_list, a.big_count, a.ndocs, j);
            continue;
        }
        Fam<HPL> f;
        fam_load<HPL>(a, lane, f);
        for (uint64_t p = b; p < e; p += 64u) sig_tile<HPL>(a, p, e, lane, f);
#pragma unroll
        for (int k = 0; k < HPL; ++k) {
            const uint32_t i = lane + 64u * k;
            if (i < a.H) a.sig[(uint64_t)j * a.H + i] = f.mn[k];
        }
    }
}

/* documents over DD_BIG_PAIRS pairs: workgroups stride over the first launch's list */
template <int HPL>
__global__ __launch_bounds__(NT) void k_dd_sig_big(const DdSigArgs a) {
    __shared__ uint32_t mn_s[NT / 64][DD_MAX_H];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t nbig = *a.big_count;
    if (nbig > a.ndocs) nbig = a.ndocs;
    for (uint32_t kb = blockIdx.x; kb < nbig; kb += gridDim.x) {
        const uint32_t j = a.big_list[kb];
        if (j >= a.ndocs) continue;   /* uniform over the workgroup */
        uint64_t b, e;
        pair_range(a.off, a.npairs, j, b, e);
        Fam<HPL> f;
        fam_load<HPL>(a, lane, f);
        for (uint64_t p = b + 64u * wv; p < e; p += 64u * (NT / 64)) sig_tile<HPL>(a, p, e, lane, f);
#pragma unroll
        for (int k = 0; k < HPL; ++k) mn_s[wv][lane + 64u * k] = f.mn[k];
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < a.H; i += NT) {
            uint32_t m = mn_s[0][i];
#pragma unroll
            for (int w = 1; w < NT / 64; ++w) m = mn_s[w][i] < m ? mn_s[w][i] : m;
            a.sig[(uint64_t)j * a.H + i] = m;
        }
        __syncthreads();   /* the buffer is reused by the next document */
    }
}

template <int HPL>
int sig_launch(const DdSigArgs& a, uint32_t ncu, hipStream_t s) {
    const uint32_t need = (a.ndocs + NT / 64 - 1) / (NT / 64);
    k_dd_sig<HPL><<<cu_grid(need, ncu, DD_WG_PER_CU), NT, 0, s>>>(a);
    if (ok()) return -1;
    k_dd_sig_big<HPL><<<cu_grid(a.ndocs, ncu, DD_BIG_WG_PER_CU), NT, 0, s>>>(a);
    return ok();
}

__global__ void k_dd_bandkeys(const uint32_t* __restrict__ sig, const uint32_t* __restrict__ live, uint32_t M, uint32_t H,
                              uint32_t rows, uint64_t n, uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    const uint32_t j = (uint32_t)(x / M), m = (uint32_t)(x - (uint64_t)j * M);
    const uint32_t* sg = sig + (uint64_t)live[m] * H + (uint64_t)j * rows;
    uint64_t k = mix64((uint64_t)j + 1ull);
    for (uint32_t i = 0; i < rows; ++i) k = mix64(k ^ (uint64_t)sg[i]);
    key[x] = k;
    val[x] = (uint32_t)x;
}

__global__ void k_dd_runflag(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val, uint64_t n, uint32_t M,
                             uint32_t* __restrict__ flag) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    flag[x] = (x > 0 && key[x] == key[x - 1] && val[x] / M == val[x - 1] / M) ? 1u : 0u;
}

__global__ void k_dd_runwrite(const uint32_t* __restrict__ val, const uint32_t* __restrict__ at, uint64_t n, uint32_t M,
                              const uint32_t* __restrict__ live, uint64_t* __restrict__ cand) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x == 0 || x >= n) return;
    if (at[x + 1] == at[x]) return;   /* not flagged */
    const uint32_t pa = live[val[x - 1] % M], pb = live[val[x] % M];   /* same band, stable sort: pa < pb */
    cand[at[x]] = ((uint64_t)pa << 32) | pb;
}

__global__ void k_dd_uniqflag(const uint64_t* __restrict__ cand, uint64_t n, uint32_t* __restrict__ flag) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    flag[x] = (x == 0 || cand[x] != cand[x - 1]) ? 1u : 0u;
}

__global__ void k_dd_uniqwrite(const uint64_t* __restrict__ cand, const uint32_t* __restrict__ at, uint64_t n,
                               uint64_t* __restrict__ out) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    if (at[x + 1] != at[x]) out[at[x]] = cand[x];
}

/* is t among the ascending L[0, n)? */
__device__ __forceinline__ bool in_list(const uint32_t* L, uint64_t n, uint32_t t) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (gload(L + mid) < t) lo = mid + 1; else hi = mid;
    }
    return lo < n && gload(L + lo) == t;
}

/* the two pair ranges of candidate c, the shorter one first; false for a candidate outside the positions */
__device__ __forceinline__ bool cand_ranges(const DdVerArgs& a, uint64_t c, uint32_t& pa, uint32_t& pb, uint64_t& sb,
                                            uint64_t& sn, uint64_t& lb, uint64_t& ln) {
    const uint64_t cv = a.cand[c];
    pa = (uint32_t)(cv >> 32);
    pb = (uint32_t)cv;
    if (pa >= a.ndocs || pb >= a.ndocs) return false;
    uint64_t b0, e0, b1, e1;
    pair_range(a.off, a.npairs, pa, b0, e0);
    pair_range(a.off, a.npairs, pb, b1, e1);
    if (e0 - b0 <= e1 - b1) { sb = b0; sn = e0 - b0; lb = b1; ln = e1 - b1; }
    else { sb = b1; sn = e1 - b1; lb = b0; ln = e0 - b0; }
    return true;
}

/* waves stride over the candidates; a wave owns its candidate's output words */
__global__ __launch_bounds__(NT) void k_dd_verify(const DdVerArgs a) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t nwaves = (uint64_t)gridDim.x * (NT / 64);
    for (uint64_t c = (uint64_t)blockIdx.x * (NT / 64) + wv; c < a.ncand; c += nwaves) {
        uint32_t pa, pb;
        uint64_t sb, sn, lb, ln;
        if (!cand_ranges(a, c, pa, pb, sb, sn, lb, ln)) {
            if (lane == 0) { a.shared[c] = 0u; a.same[c] = 0u; }
            continue;
        }
        if (ln > DD_BIG_PAIRS) {   /* the second launch's */
            if (lane == 0) hand_to_big(a.big_list, a.big_count, (uint32_t)a.ncand, (uint32_t)c);
            continue;
        }
        uint32_t sh = 0, sm = 0;
        for (uint64_t i = lane; i < sn; i += 64u) sh += in_list(a.term + lb, ln, gload(a.term + sb + i)) ? 1u : 0u;
        for (uint32_t i = lane; i < a.H; i += 64u)
            sm += gload(a.sig + (uint64_t)pa * a.H + i) == gload(a.sig + (uint64_t)pb * a.H + i) ? 1u : 0u;
        sh = wave_sum(sh);
        sm = wave_sum(sm);
        if (lane == 0) { a.shared[c] = sh; a.same[c] = sm; }
    }
}

/* candidates that hold a document over DD_BIG_PAIRS pairs: workgroups stride over the list */
__global__ __launch_bounds__(NT) void k_dd_verify_big(const DdVerArgs a) {
    __shared__ uint32_t sh_s[NT / 64], sm_s[NT / 64];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint64_t nbig = *a.big_count;
    if (nbig > a.ncand) nbig = a.ncand;
    for (uint64_t kb = blockIdx.x; kb < nbig; kb += gridDim.x) {
        const uint64_t c = a.big_list[kb];
        if (c >= a.ncand) continue;   /* uniform over the workgroup */
        uint32_t pa, pb;
        uint64_t sb, sn, lb, ln;
        if (!cand_ranges(a, c, pa, pb, sb, sn, lb, ln)) continue;
        uint32_t sh = 0, sm = 0;
        for (uint64_t i = threadIdx.x; i < sn; i += NT) sh += in_list(a.term + lb, ln, gload(a.term + sb + i)) ? 1u : 0u;
        for (uint32_t i = threadIdx.x; i < a.H; i += NT)
            sm += gload(a.sig + (uint64_t)pa * a.H + i) == gload(a.sig + (uint64_t)pb * a.H + i) ? 1u : 0u;
        sh = wave_sum(sh);
        sm = wave_sum(sm);
        if (lane == 0) { sh_s[wv] = sh; sm_s[wv] = sm; }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t s0 = 0, s1 = 0;
#pragma unroll
            for (int w = 0; w < NT / 64; ++w) { s0 += sh_s[w]; s1 += sm_s[w]; }
            a.shared[c] = s0;
            a.same[c] = s1;
        }
        __syncthreads();   /* the words are reused by the next candidate */
    }
}

}  // namespace

int launch_dd_h0(const uint4* tkey, const uint32_t* tlen, uint32_t V, const uint8_t* corpus, uint64_t corpus_bytes,
                 uint64_t* h0, hipStream_t s) {
    if (!V) return 0;
    k_dd_h0<<<grid_for(V), NT, 0, s>>>(tkey, tlen, V, corpus, corpus_bytes, h0);
    return ok();
}

int launch_dd_sig(const DdSigArgs& a, uint32_t ncu, hipStream_t s) {
    if (!a.ndocs) return 0;
    if (a.H == 0u || a.H > DD_MAX_H) return -1;
    if (hipMemsetAsync(a.big_count, 0, 4, s) != hipSuccess) return -1;
    switch ((a.H + 63u) / 64u) {
        case 1: return sig_launch<1>(a, ncu, s);
        case 2: return sig_launch<2>(a, ncu, s);
        case 3: return sig_launch<3>(a, ncu, s);
        default: return sig_launch<4>(a, ncu, s);
    }
}

int launch_dd_bandkeys(const uint32_t* sig, const uint32_t* live, uint32_t M, uint32_t H, uint32_t rows, uint64_t* key,
                       uint32_t* val, hipStream_t s) {
    if (!M) return 0;
    if (!rows || H % rows) return -1;
    const uint64_t n = (uint64_t)(H / rows) * M;
    if (n > 0xFFFFFFFFull) return -1;
    k_dd_bandkeys<<<grid_for(n), NT, 0, s>>>(sig, live, M, H, rows, n, key, val);
    return ok();
}

int launch_dd_runflag(const uint64_t* key, const uint32_t* val, uint64_t n, uint32_t M, uint32_t* flag, hipStream_t s) {
    if (!n || !M) return 0;
    k_dd_runflag<<<grid_for(n), NT, 0, s>>>(key, val, n, M, flag);
    return ok();
}

int launch_dd_runwrite(const uint32_t* val, const uint32_t* at, uint64_t n, uint32_t M, const uint32_t* live,
                       uint64_t* cand, hipStream_t s) {
    if (!n || !M) return 0;
    k_dd_runwrite<<<grid_for(n), NT, 0, s>>>(val, at, n, M, live, cand);
    return ok();
}

int launch_dd_uniqflag(const uint64_t* cand, uint64_t n, uint32_t* flag, hipStream_t s) {
    if (!n) return 0;
    k_dd_uniqflag<<<grid_for(n), NT, 0, s>>>(cand, n, flag);
    return ok();
}

int launch_dd_uniqwrite(const uint64_t* cand, const uint32_t* at, uint64_t n, uint64_t* out, hipStream_t s) {
    if (!n) return 0;
    k_dd_uniqwrite<<<grid_for(n), NT, 0, s>>>(cand, at, n, out);
    return ok();
}

int launch_dd_verify(const DdVerArgs& a, uint32_t ncu, hipStream_t s) {
    if (!a.ncand) return 0;
    if (a.ncand > 0xFFFFFFFFull) return -1;
    if (hipMemsetAsync(a.big_count, 0, 4, s) != hipSuccess) return -1;
    const uint64_t need = (a.ncand + NT / 64 - 1) / (NT / 64);
    k_dd_verify<<<cu_grid(need, ncu, DD_WG_PER_CU), NT, 0, s>>>(a);
    if (ok()) return -1;
    k_dd_verify_big<<<cu_grid(a.ncand, ncu, DD_BIG_WG_PER_CU), NT, 0, s>>>(a);
    return ok();
}
