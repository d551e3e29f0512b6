/*
 * terms.hip — per-document top-k keyword extraction over the resident result of a run
 * (include/tfidf.h: tfidf_top_terms).  The reference prints every (document, word) score
 * (TFIDF.c:202,243-245); the k best words of a document are read from the same scores where
 * the run left them in HBM: document-major, terms ascending inside a document.
 *
 *   lookup   one lane per requested id: the id's document-name key (the key of k_doc_keys,
 *            finalize.hip) searched over the output positions, which are sorted by it.
 *   select   one workgroup per document streams the document's scores once.  Keys are (score
 *            bits + 1, pair index inside the document); the order is score descending, then
 *            pair index ascending (= term-table order), total because a term occurs once in
 *            a document.  Documents of up to QS_BIG pairs take a one-wave workgroup.  k <= 64:
 *            the best pairs so far are a sorted list in registers, one entry per lane, and a
 *            pair that beats entry k - 1 is inserted at once (k_terms_select_list).  Larger
 *            k: candidates go to an LDS buffer sized for k (two instances); until it has been
 *            cut once every pair is a candidate, afterwards only a pair that beats the
 *            current k-th key; a full buffer is sorted (bitonic, padded to a power of two),
 *            cut to the best k, and the k-th key becomes the threshold; one last sort orders
 *            the survivors.  Documents over QS_BIG pairs are listed and taken by a second
 *            launch with 256 threads and a buffer of 4096, for every k.
 *   words    the selected terms' lengths are scanned (prims.hip) and their bytes gathered:
 *            short terms from their 16-byte key, long terms from the corpus.
 */
#include "kernels.h"
#include "dev_common.h"
#include "launch_util.h"

namespace {

constexpr int NT = 256;

/* ------------------------------------------------------------------ lookup -- */

/* "docN" as ten base-11 digits, short names padded with the digit 10 (k_doc_keys) */
__device__ __forceinline__ uint64_t doc_name_key(uint32_t id) {
    uint32_t dg[10];
    int k = 0;
    do { dg[k++] = id % 10u; id /= 10u; } while (id);
    uint64_t key = 0;
    for (int p = 0; p < 10; ++p) key = key * 11u + (p < k ? dg[k - 1 - p] : 10u);
    return key;
}

__global__ void k_terms_lookup(const TLookupArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nids) return;
    const uint32_t id = a.ids[i];
    const uint64_t key = doc_name_key(id);
    uint32_t lo = 0, hi = a.ndocs;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (doc_name_key(doc_id_at(a.order, a.doc_ids, mid)) < key) lo = mid + 1;
        else hi = mid;
    }
    a.pos[i] = (lo < a.ndocs && doc_id_at(a.order, a.doc_ids, lo) == id) ? lo : TERMS_NO_POS;
}

/* ------------------------------------------------------------------ select -- */

/* a before b: score descending, then pair index ascending.  Keys are the scores' bit
 * patterns + 1 (scores are >= +0.0 and finite: the patterns order like the values and the
 * increment cannot wrap); 0 pads a sort to a power of two and sorts last (hit_before,
 * query.hip) */
__device__ __forceinline__ bool key_before(uint64_t sa, uint32_t ia, uint64_t sb, uint32_t ib) {
    return sa > sb || (sa == sb && ia < ib);
}

/* TNT threads sort ls / li [0, n) best first and return min(n, kk): the entries kept.  Starts
 * and ends with a barrier. */
template <int TNT>
__device__ __forceinline__ uint32_t sort_cut(uint64_t* ls, uint32_t* li, uint32_t n, uint32_t kk) {
    uint32_t m = 2u;
    while (m < n) m <<= 1;   /* <= the buffer's capacity, a power of two */
    for (uint32_t i = n + threadIdx.x; i < m; i += TNT) { ls[i] = 0ull; li[i] = 0xFFFFFFFFu; }
    __syncthreads();
    for (uint32_t k2 = 2u; k2 <= m; k2 <<= 1) {
        for (uint32_t jj = k2 >> 1; jj > 0u; jj >>= 1) {
            for (uint32_t t = threadIdx.x; t < (m >> 1); t += TNT) {   /* every thread a compare-exchange */
                const uint32_t i = ((t & ~(jj - 1u)) << 1) | (t & (jj - 1u)), x = i | jj;
                const uint64_t si = ls[i], sx = ls[x];
                const uint32_t ii = li[i], ix = li[x];
                const bool up = (i & k2) == 0u;   /* best first in this run */
                if (up ? key_before(sx, ix, si, ii) : key_before(si, ii, sx, ix)) {
                    ls[i] = sx; li[i] = ix;
                    ls[x] = si; li[x] = ii;
                }
            }
            __syncthreads();
        }
    }
    return n < kk ? n : kk;
}

/* One key per lane of a wave: the number of lanes whose key comes before this lane's, which is
 * its place in the sorted order (keys are distinct).  64 broadcasts through scalar registers
 * and no LDS traffic. */
__device__ __forceinline__ uint32_t wave_rank(uint64_t s, uint32_t idx) {
    const int lo = (int)(uint32_t)s, hi = (int)(uint32_t)(s >> 32);
    uint32_t r = 0;
#pragma unroll 8
    for (int l = 0; l < 64; ++l) {
        const uint64_t sl = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(hi, l) << 32) |
                            (uint32_t)__builtin_amdgcn_readlane(lo, l);
        const uint32_t il = (uint32_t)__builtin_amdgcn_readlane((int)idx, l);
        r += key_before(sl, il, s, idx) ? 1u : 0u;
    }
    return r;
}

/* a row's document: its pair range, clamped to the run's pair total, and its global id (no
 * such document: an empty range and id 0) */
__device__ __forceinline__ void row_doc(const TSelArgs& a, uint32_t row, uint64_t& b, uint64_t& e, uint32_t& id) {
    const uint32_t j = a.pos ? a.pos[a.row0 + row] : a.row0 + row;
    b = e = 0;
    id = 0;
    if (j < a.ndocs) {
        pair_range(a.out_off, a.npairs, j, b, e);
        id = doc_id_at(a.order, a.doc_ids, j);
    }
}

/* entry i < k of a row: the pair `pr` with key `key` (score bits + 1), or zeros when !valid */
__device__ __forceinline__ void put_entry(const TSelArgs& a, uint32_t row, uint32_t i, bool valid, uint64_t key, uint64_t pr) {
    const uint64_t o = (uint64_t)row * a.k + i;
    uint64_t sc = 0, wl = 0;
    uint32_t t = 0, cn = 0;
    if (valid) {
        sc = key - 1ull;
        t = gload(a.out_term + pr);
        cn = gload(a.out_cnt + pr);
        wl = t < a.nterms ? a.tlen[t] : 0u;
    } else {
        pr = 0;
    }
    a.score[o] = sc;
    a.pair[o] = pr;
    a.term[o] = t;
    a.cnt[o] = cn;
    a.wlen[o] = wl;
}

/* k <= 64, documents of up to QS_BIG pairs, one wave each: the best 64 pairs so far are a
 * sorted list in registers, entry t in lane t (pads of key 0 behind), and entry k - 1 is the
 * threshold, kept in scalar registers.  The first round is ranked (wave_rank) and permuted
 * through LDS; afterwards a pair that beats the threshold is inserted at once: the lanes whose
 * entry comes before it are a prefix (ballot, popcount = its place), the lanes behind take
 * their left neighbour's entry (DPP).  The threshold is always the true k-th key, so only
 * pairs that enter the current best k cost anything (k ln(pairs / 64) of them on random
 * scores), and the list is the sorted result: no buffer, no sort. */
__global__ __launch_bounds__(64) void k_terms_select_list(const TSelArgs a) {
    __shared__ uint64_t ls[64];
    __shared__ uint32_t li[64];
    constexpr int U = 4;
    const uint32_t lane = threadIdx.x, kk = a.k;
    const int last = (int)kk - 1;
    for (uint32_t row = blockIdx.x; row < a.nrows; row += gridDim.x) {
        uint64_t b, e;
        uint32_t id;
        row_doc(a, row, b, e, id);
        const uint64_t np = e - b;
        if (np > QS_BIG) {   /* the second launch's */
            if (threadIdx.x == 0) hand_to_big(a.big_list, a.big_count, a.nrows, row);
            continue;
        }
        uint64_t ms = 0ull;                    /* this lane's entry: a pad until the first round */
        uint32_t mi = 0xFFFFFFC0u + lane;
        uint64_t ts = 0ull;                    /* entry k - 1 */
        uint32_t ti = 0xFFFFFFFFu;
        for (uint64_t p0 = b; p0 < e; p0 += 64u * U) {
            uint64_t sv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint64_t p = p0 + 64u * u + lane;
                sv[u] = p < e ? (uint64_t)__double_as_longlong(gload(a.out_score + p)) + 1ull : 0ull;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint64_t q0 = p0 + 64u * u;
                if (q0 >= e) break;   /* uniform */
                const uint64_t p = q0 + lane;
                const bool v = p < e;
                const uint64_t s = sv[u];
                const uint32_t idx = v ? (uint32_t)(p - b) : 0xFFFFFFC0u + lane;   /* distinct pads behind every pair */
                if (q0 == b) {   /* the first round becomes the list */
                    const uint32_t r = wave_rank(s, idx);
                    __syncthreads();
                    ls[r] = s;
                    li[r] = idx;
                    __syncthreads();
                    ms = ls[lane];
                    mi = li[lane];
                } else {
                    uint64_t m = __ballot(v && key_before(s, idx, ts, ti));
                    while (m) {   /* in pair order */
                        const int l = __builtin_ctzll(m);
                        m &= m - 1ull;
                        const uint64_t cs = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(s >> 32), l) << 32) |
                                            (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)s, l);
                        const uint32_t ci = (uint32_t)__builtin_amdgcn_readlane((int)idx, l);
                        if (!key_before(cs, ci, ts, ti)) continue;   /* the threshold has moved past it */
                        const uint32_t at = (uint32_t)__popcll(__ballot(key_before(ms, mi, cs, ci)));   /* <= k - 1 */
                        const uint32_t plo = lane_prev((uint32_t)ms), phi = lane_prev((uint32_t)(ms >> 32)), pi = lane_prev(mi);
                        if (lane > at) { ms = ((uint64_t)phi << 32) | plo; mi = pi; }
                        else if (lane == at) { ms = cs; mi = ci; }
                        ts = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(ms >> 32), last) << 32) |
                             (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)ms, last);
                        ti = (uint32_t)__builtin_amdgcn_readlane((int)mi, last);
                    }
                    continue;
                }
                ts = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(ms >> 32), last) << 32) |
                     (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)ms, last);
                ti = (uint32_t)__builtin_amdgcn_readlane((int)mi, last);
            }
        }
        const uint32_t nout = np < kk ? (uint32_t)np : kk;
        if (lane < kk) put_entry(a, row, lane, lane < nout, ms, b + mi);
        if (lane == 0) {
            a.rdoc[row] = id;
            a.rnpairs[row] = np;
            a.rnterms[row] = nout;
        }
    }
}

/* TNT = 64: a workgroup is one wave (the barriers are wave barriers), candidates are appended
 * in pair order behind a ballot; TNT = 256 (BIG): the second launch over the first one's list,
 * appended through an LDS counter in any order (the sort follows).  CAP >= k + TNT. */
template <int TNT, uint32_t CAP, bool BIG>
__global__ __launch_bounds__(TNT) void k_terms_select(const TSelArgs a) {
    __shared__ uint64_t ls[CAP];
    __shared__ uint32_t li[CAP];
    __shared__ uint32_t lcount;
    constexpr int U = 4;   /* rounds of scores in flight */
    const uint32_t kk = a.k;
    uint32_t nwork = a.nrows;
    if (BIG) {
        nwork = *a.big_count;
        if (nwork > a.nrows) nwork = a.nrows;
    }
    for (uint32_t w = blockIdx.x; w < nwork; w += gridDim.x) {
        const uint32_t row = BIG ? a.big_list[w] : w;
        if (row >= a.nrows) continue;
        uint64_t b, e;
        uint32_t id;
        row_doc(a, row, b, e, id);
        const uint64_t np = e - b;
        if (!BIG && np > QS_BIG) {   /* the second launch's */
            if (threadIdx.x == 0) hand_to_big(a.big_list, a.big_count, a.nrows, row);
            continue;
        }
        uint32_t n = 0;          /* candidates in the buffer (uniform) */
        bool have = false;       /* the buffer has been cut: (ts, ti) is the k-th best key so far */
        uint64_t ts = 0;
        uint32_t ti = 0;
        for (uint64_t p0 = b; p0 < e; p0 += (uint64_t)TNT * U) {
            uint64_t sv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint64_t p = p0 + (uint64_t)u * TNT + threadIdx.x;
                sv[u] = p < e ? (uint64_t)__double_as_longlong(gload(a.out_score + p)) + 1ull : 0ull;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint64_t q0 = p0 + (uint64_t)u * TNT;
                if (q0 >= e) break;   /* uniform */
                const uint64_t p = q0 + threadIdx.x;
                const bool v = p < e;
                const uint32_t idx = (uint32_t)(p - b);
                const uint64_t s = sv[u];
                bool pass = v && (!have || key_before(s, idx, ts, ti));
                uint64_t bal = 0;
                uint32_t c;
                if (TNT == 64) { bal = __ballot(pass); c = (uint32_t)__popcll(bal); }
                else c = (uint32_t)__syncthreads_count((int)pass);
                if (c == 0u) continue;
                if (n + c > CAP) {   /* cut to the best k: n <= k afterwards, and k + TNT <= CAP */
                    n = sort_cut<TNT>(ls, li, n, kk);
                    if (n >= kk) { have = true; ts = ls[kk - 1u]; ti = li[kk - 1u]; }
                    pass = v && (!have || key_before(s, idx, ts, ti));
                    if (TNT == 64) { bal = __ballot(pass); c = (uint32_t)__popcll(bal); }
                    else c = (uint32_t)__syncthreads_count((int)pass);
                }
                if (TNT == 64) {
                    if (pass) {
                        const uint32_t at = n + (uint32_t)__popcll(bal & ((1ull << (threadIdx.x & 63u)) - 1ull));
                        ls[at] = s;
                        li[at] = idx;
                    }
                } else {
                    if (threadIdx.x == 0) lcount = n;
                    __syncthreads();
                    if (pass) {
                        const uint32_t at = atomicAdd(&lcount, 1u);
                        ls[at] = s;
                        li[at] = idx;
                    }
                }
                n += c;
            }
        }
        const uint32_t nout = sort_cut<TNT>(ls, li, n, kk);
        for (uint32_t i = threadIdx.x; i < kk; i += TNT) put_entry(a, row, i, i < nout, ls[i], b + li[i]);
        if (threadIdx.x == 0) {
            a.rdoc[row] = id;
            a.rnpairs[row] = np;
            a.rnterms[row] = nout;
        }
        __syncthreads();   /* the buffer is reused by the next document */
    }
}

/* ------------------------------------------------------------------- words -- */

__global__ void k_terms_words(const TWordArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t o = a.woff[i], len = a.woff[i + 1] - o;
    if (!len) return;
    const uint32_t t = a.term[i];
    if (t >= a.nterms) return;
    const uint4 k = a.tkey[t];
    uint8_t* dst = a.bytes + o;
    if (k.w == 0xFFFFFFFFu) {   /* long term: (length << 40 | corpus offset) in the key's low half (k_term_meta) */
        const uint64_t off = (((uint64_t)k.y << 32) | k.x) & 0xFFFFFFFFFFull;
        const bool in = off + len <= a.corpus_bytes;
        for (uint64_t x = 0; x < len; ++x) dst[x] = in ? a.corpus[off + x] : (uint8_t)0;
    } else {
        const uint32_t w[4] = {k.x, k.y, k.z, k.w};
        for (uint32_t x = 0; x < (uint32_t)len && x < 16u; ++x) dst[x] = (uint8_t)(w[x >> 2] >> (8u * (x & 3u)));
    }
}

template <int TNT, uint32_t CAP, bool BIG>
int select_launch(const TSelArgs& a, uint32_t per_cu, uint32_t ncu, hipStream_t s) {
    k_terms_select<TNT, CAP, BIG><<<cu_grid(a.nrows, ncu, per_cu), TNT, 0, s>>>(a);
    return ok();
}

}  // namespace

int launch_terms_lookup(const TLookupArgs& a, hipStream_t s) {
    if (!a.nids) return 0;
    k_terms_lookup<<<grid_for(a.nids), NT, 0, s>>>(a);
    return ok();
}

int launch_terms_select(const TSelArgs& a, uint32_t ncu, hipStream_t s) {
    if (!a.nrows) return 0;
    if (a.k == 0u || a.k > 1024u) return -1;
    if (hipMemsetAsync(a.big_count, 0, 4, s) != hipSuccess) return -1;
    /* by k: the register list, or the wave kernel with 6 or 24 KiB of LDS per one-wave workgroup */
    int rc;
    if (a.k <= 64u) {
        k_terms_select_list<<<cu_grid(a.nrows, ncu, TM_LIST_WG_PER_CU), 64, 0, s>>>(a);
        rc = ok();
    } else if (a.k <= 256u) rc = select_launch<64, 512u, false>(a, TM_W512_WG_PER_CU, ncu, s);
    else rc = select_launch<64, 2048u, false>(a, TM_W2048_WG_PER_CU, ncu, s);
    if (rc) return rc;
    return select_launch<256, 4096u, true>(a, TM_BIG_WG_PER_CU, ncu, s);
}

int launch_terms_words(const TWordArgs& a, hipStream_t s) {
    if (!a.n) return 0;
    k_terms_words<<<grid_for(a.n), NT, 0, s>>>(a);
    return ok();
}
