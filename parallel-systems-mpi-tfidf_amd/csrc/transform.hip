/*
 * transform.hip — scoring unseen documents against the resident model of a run
 * (include/tfidf.h: tfidf_transform).  The reference has one pass over one corpus
 * (TFIDF.c:130-247); here a finished run's vocabulary, global df, N and idf table stay in HBM
 * and a new batch is tokenised, resolved, counted and scored against them, read-only.
 *
 *   bounds   one workgroup per tile of TR_TILE bytes, one 16-byte group per lane: the
 *            whitespace mask (dev_common.h's SWAR form), the document starts from a bitmap, and
 *            from the two a start bit (a token byte whose predecessor is whitespace, a
 *            document's first byte or outside the window) and an end bit (its mirror) per byte.
 *            Counted per tile, scanned, written: the i-th start pairs with the i-th end, so no
 *            lane walks a token to find its end.
 *   resolve  one lane per token: row = upper_bound of the start in doc_off, term = the bytes up
 *            to the first NUL, identity key (dev_common.h), read-only probe of the frozen
 *            table (vocab_find_rank, dev_vocab.h: long terms by their bytes).
 *            key = row << 32 | rank; rank = V marks a term the vocabulary does not hold.
 *   count    the caller sorts (key, token index) with the stable LSD radix sort: a run of
 *            equal keys is a (row, term) pair, its length the count, its first record the
 *            term's first token in the document.  Run heads are flagged and scanned.
 *   pairs    one lane per run head: the run's length by binary search, df by rank, idf from
 *            the run's own table, score = fl(fl(count / docSize) * idf) (TFIDF.c:202,243-244).
 *            docSize is the number of token starts inside the document (every token, also
 *            those outside the vocabulary: TFIDF.c:141-143), row offsets a binary search over
 *            the pairs' rows: integers only, no atomics anywhere.
 */
#include "kernels.h"
#include "dev_common.h"
#include "dev_vocab.h"

namespace {

constexpr int NT = 256;
static_assert(TR_TILE == NT * 16, "one 16-byte group per lane");
inline unsigned grid_for(uint64_t n) { return n ? (unsigned)((n + NT - 1) / NT) : 1u; }
int ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

constexpr uint64_t TERM_MAX = 1ull << 24;   /* a term this long is in no vocabulary (TFIDF_E_CAPACITY of a run) */

/* ------------------------------------------------------------------ bounds -- */

__global__ void k_tr_docstarts(const TrSlice a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t d = (uint64_t)a.d0 + 1u + i;
    if (d >= a.d1) return;
    const uint64_t pos = a.doc_off[d];
    if (pos <= a.b0 || pos >= a.b1) return;   /* the window's own edges are boundaries already */
    const uint64_t bit = (uint64_t)((long long)pos - a.p0);
    atomicOr(&a.dstart[bit >> 5], 1u << (bit & 31u));
}

__device__ __forceinline__ bool tr_token_byte(const TrSlice& a, long long q) {
    return q >= (long long)a.b0 && q < (long long)a.b1 && !is_ws(a.bytes[q]);
}

/* bit j = byte p + j belongs to a token (inside the window and no whitespace) */
__device__ __forceinline__ uint32_t tr_token_mask(const TrSlice& a, long long p) {
    if (p >= (long long)a.b0 && p + 16 <= (long long)a.b1)   /* bytes + p is 16-byte aligned: p0's choice */
        return ~ws_mask16_swar(gload((const uint4*)(a.bytes + p))) & 0xFFFFu;
    uint32_t m = 0;
    for (int j = 0; j < 16; ++j) m |= (tr_token_byte(a, p + j) ? 1u : 0u) << j;
    return m;
}

template <bool WRITE>
__global__ __launch_bounds__(NT) void k_tr_bounds(const TrSlice a) {
    __shared__ uint32_t s_tk[NT + 2], s_ds[NT + 2];
    __shared__ uint32_t wsum_s[NT / 64], wsum_e[NT / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t tile = blockIdx.x;
    const uint64_t g = tile * NT + tid;                      /* this lane's group */
    const long long p = a.p0 + (long long)(g * 16u);
    const uint32_t tk = tr_token_mask(a, p);
    const uint32_t ds = (a.dstart[g >> 1] >> ((g & 1u) * 16u)) & 0xFFFFu;
    s_tk[tid + 1] = tk;
    s_ds[tid + 1] = ds;
    if (tid == 0) s_tk[0] = tr_token_byte(a, p - 1) ? 0x8000u : 0u;
    if (tid == NT - 1) {
        const uint64_t nb = (g + 1u) * 16u;                  /* the next tile's first bit */
        s_tk[NT + 1] = tr_token_byte(a, p + 16) ? 1u : 0u;
        s_ds[NT + 1] = (a.dstart[nb >> 5] >> (nb & 31u)) & 1u;
    }
    __syncthreads();
    const uint32_t prev = s_tk[tid] >> 15, next_tk = s_tk[tid + 2] & 1u, next_ds = s_ds[tid + 2] & 1u;
    const uint32_t st = tk & (~((tk << 1) | prev) | ds) & 0xFFFFu;
    const uint32_t en = tk & (~((tk >> 1) | (next_tk << 15)) | (ds >> 1) | (next_ds << 15)) & 0xFFFFu;
    uint32_t tot_s = 0, tot_e = 0;
    const uint32_t at_s = block_excl_scan<NT>(__popc(st), wsum_s, &tot_s);
    const uint32_t at_e = block_excl_scan<NT>(__popc(en), wsum_e, &tot_e);
    if (!WRITE) {
        if (tid == 0) { a.cnt_s[tile] = tot_s; a.cnt_e[tile] = tot_e; }
        return;
    }
    uint64_t o = a.cnt_s[tile] + at_s;
    for (uint32_t m = st; m; m &= m - 1u, ++o) {
        if (o < a.tok_cap) a.tok_start[o] = (uint64_t)(p + __builtin_ctz(m));
        else atomicOr(a.status, ST_BOUNDS);
    }
    o = a.cnt_e[tile] + at_e;
    for (uint32_t m = en; m; m &= m - 1u, ++o) {
        if (o < a.tok_cap) a.tok_end[o] = (uint64_t)(p + __builtin_ctz(m) + 1);
        else atomicOr(a.status, ST_BOUNDS);
    }
}

/* ----------------------------------------------------------------- resolve -- */

__global__ __launch_bounds__(NT) void k_tr_resolve(const TrResolve a) {
    const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= a.ntok) return;
    const TrSlice& sl = a.sl;
    const uint64_t s = sl.tok_start[i], e = sl.tok_end[i];
    a.val[i] = (uint32_t)i;
    if (!(s >= sl.b0 && s < e && e <= sl.b1 && sl.b1 <= sl.nbytes)) {
        atomicOr(sl.status, ST_BOUNDS);
        a.key[i] = ((uint64_t)sl.d0 << 32) | a.voc.V;
        a.tlen[i] = 0u;
        return;
    }
    /* the last document whose offset is <= s: empty documents share offsets */
    uint64_t lo = sl.d0, hi = sl.d1;   /* doc_off[lo] <= s < doc_off[hi] */
    while (hi - lo > 1u) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (sl.doc_off[mid] > s) hi = mid;
        else lo = mid;
    }
    const uint8_t* p = sl.bytes + s;
    const uint64_t n = e - s, lim = n < TERM_MAX ? n : TERM_MAX;
    uint64_t tl = 0;
    while (tl < lim && p[tl] != 0) ++tl;   /* strcmp semantics: the term ends at the first NUL */
    uint32_t rank = QUERY_NO_TERM;
    if (tl < TERM_MAX) {
        uint64_t klo = 0, khi = 0;
        if (tl < 16u) {
            uint64_t l8 = 0, h8 = 0;
            for (uint32_t b = 0; b < (uint32_t)tl; ++b) {
                const uint64_t c = p[b];
                if (b < 8u) l8 |= c << (8u * b);
                else h8 |= c << (8u * (b - 8u));
            }
            make_short_key(l8, h8, (uint32_t)tl, &klo, &khi);
        } else {
            make_long_key(p, tl, &klo, &khi);
        }
        rank = vocab_find_rank(a.voc, klo, khi, p, tl);
    }
    a.key[i] = (lo << 32) | (rank < a.voc.V ? rank : a.voc.V);
    a.tlen[i] = tl < TERM_MAX ? (uint32_t)tl : (uint32_t)TERM_MAX;
}

/* ------------------------------------------------------------------- pairs -- */

__global__ __launch_bounds__(NT) void k_tr_flags(const TrPairs a) {
    const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= a.ntok) return;
    const uint64_t k = a.key[i];
    a.flag[i] = ((i == 0 || a.key[i - 1] != k) && (uint32_t)k < a.V) ? 1u : 0u;
}

/* first index in [0, n) whose value is >= x */
__device__ __forceinline__ uint64_t lower_bound_u64(const uint64_t* v, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

/* docSize = the token starts inside the document */
__global__ __launch_bounds__(NT) void k_tr_docsize(const TrPairs a) {
    const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= (uint64_t)(a.d1 - a.d0)) return;
    const uint64_t b = a.doc_off[a.d0 + i], e = a.doc_off[a.d0 + i + 1];
    a.doc_size[i] = (uint32_t)(lower_bound_u64(a.tok_start, a.ntok, e) - lower_bound_u64(a.tok_start, a.ntok, b));
}

/* REF: the reference's score, as the run computes it.  !REF (a weighting scheme is active,
 * tfidf_reweight): the integers only; reweight.hip scores the rows afterwards */
template <bool REF>
__global__ __launch_bounds__(NT) void k_tr_pairs(const TrPairs a) {
    const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= a.ntok) return;
    const uint64_t k = a.key[i];
    if (i != 0 && a.key[i - 1] == k) return;   /* run heads only */
    uint64_t lo = i + 1, hi = a.ntok;          /* the run's end: the first key above k */
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a.key[mid] <= k) lo = mid + 1;
        else hi = mid;
    }
    const uint64_t cnt = lo - i;
    const uint32_t row = (uint32_t)(k >> 32), rank = (uint32_t)k;
    if (row < a.d0 || row >= a.d1 || rank > a.V || cnt > 0xFFFFFFFFull) { atomicOr(a.status, ST_BOUNDS); return; }
    if (rank == a.V) {   /* the row's tokens outside the vocabulary: one run per row */
        a.doc_oov[row - a.d0] = (uint32_t)cnt;
        return;
    }
    const uint64_t o = a.pos[i];
    const uint32_t t = a.val[i];   /* the sort is stable: the run's first record is its first token */
    const uint32_t ds = a.doc_size[row - a.d0], df = a.df[rank];
    if (o >= a.ntok || t >= a.ntok || ds == 0u || df == 0u || df > a.Nt) { atomicOr(a.status, ST_BOUNDS); return; }
    a.p_row[o] = row;
    a.p_term[o] = rank;
    a.p_count[o] = (uint32_t)cnt;
    a.p_df[o] = df;
    if (REF) {
        const double idf = a.idf_idx ? a.idf[a.idf_idx[df]] : a.idf[df];
        const double tf = (double)(uint32_t)cnt / (double)ds;   /* TFIDF.c:202 */
        a.p_score[o] = tf * idf;                                /* TFIDF.c:243-244: two roundings */
    }
    a.p_woff[o] = a.tok_start[t];
    a.p_wlen[o] = a.tlen[t];
}

/* row_off[r] = the first pair whose row is >= d0 + r (the pairs are in row order) */
__global__ __launch_bounds__(NT) void k_tr_rowoff(const TrPairs a) {
    const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (i > (uint64_t)(a.d1 - a.d0)) return;
    const uint64_t P = a.pos[a.ntok], want = (uint64_t)a.d0 + i;
    uint64_t lo = 0, hi = P;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)a.p_row[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    a.row_off[i] = lo;
}

}  // namespace

int launch_tr_docstarts(const TrSlice& a, hipStream_t s) {
    if (hipMemsetAsync(a.dstart, 0, (size_t)(a.ntiles * (TR_TILE / 32u) + 1u) * 4u, s) != hipSuccess) return -1;
    if (a.d1 - a.d0 < 2u) return 0;
    k_tr_docstarts<<<grid_for((uint64_t)(a.d1 - a.d0) - 1u), NT, 0, s>>>(a);
    return ok();
}

int launch_tr_count(const TrSlice& a, hipStream_t s) {
    if (!a.ntiles) return 0;
    if (a.ntiles > 0x7FFFFFFFull) return -1;
    k_tr_bounds<false><<<(unsigned)a.ntiles, NT, 0, s>>>(a);
    return ok();
}

int launch_tr_write(const TrSlice& a, hipStream_t s) {
    if (!a.ntiles) return 0;
    if (a.ntiles > 0x7FFFFFFFull) return -1;
    k_tr_bounds<true><<<(unsigned)a.ntiles, NT, 0, s>>>(a);
    return ok();
}

int launch_tr_resolve(const TrResolve& a, hipStream_t s) {
    if (!a.ntok) return 0;
    k_tr_resolve<<<grid_for(a.ntok), NT, 0, s>>>(a);
    return ok();
}

int launch_tr_flags(const TrPairs& a, hipStream_t s) {
    if (!a.ntok) return 0;
    k_tr_flags<<<grid_for(a.ntok), NT, 0, s>>>(a);
    return ok();
}

int launch_tr_pairs(const TrPairs& a, hipStream_t s) {
    const uint64_t nd = (uint64_t)(a.d1 - a.d0);
    if (nd) k_tr_docsize<<<grid_for(nd), NT, 0, s>>>(a);
    if (a.ntok) k_tr_pairs<true><<<grid_for(a.ntok), NT, 0, s>>>(a);
    k_tr_rowoff<<<grid_for(nd + 1u), NT, 0, s>>>(a);
    return ok();
}

int launch_tr_pairs_w(const TrPairs& a, hipStream_t s) {
    const uint64_t nd = (uint64_t)(a.d1 - a.d0);
    if (nd) k_tr_docsize<<<grid_for(nd), NT, 0, s>>>(a);
    if (a.ntok) k_tr_pairs<false><<<grid_for(a.ntok), NT, 0, s>>>(a);
    k_tr_rowoff<<<grid_for(nd + 1u), NT, 0, s>>>(a);
    return ok();
}
