/*
 * match.hip — fuzzy and prefix matching of patterns against the resident term table
 * (include/tfidf.h: tfidf_match_terms).  Integer arithmetic on bytes only.
 *
 *   scan     workgroups of MT_NT lanes stride over tiles of MT_NT terms, one lane per term.  The
 *            patterns of a group (at most MT_GROUP) are staged in LDS once per workgroup.  A lane
 *            loads its term's length first; only when some pattern of the group passes the
 *            length filter (fuzzy: |len(t) - len(p)| <= d, prefix: len(t) >= len(p)) does it load
 *            the term's bytes, at most MT_TERM_MAX of them, into its own LDS row (17 words: an
 *            odd stride, so the lanes' byte reads fall into distinct banks).  From a run a term
 *            under 16 bytes is its 16-byte key, a longer one comes from the corpus; from an
 *            imported model the bytes are m_off / m_blob.  Then, per candidate pattern, the
 *            fixed-prefix compare and the distance.
 *   dist     a banded dynamic program: the cells |i - j| <= 2 of each row, five per row, in
 *            registers; three rows are live under TFIDF_MATCH_TRANSPOSE (the optimal-string-
 *            alignment recurrence reads row i - 2).  Values are capped at MT_NO_MATCH = 3: a cell
 *            of at most 2 is exact, because a path of cost c never leaves the band |i - j| <= c.
 *            A row whose cells all exceed the budget ends the evaluation: the row minimum never
 *            decreases down the rows.
 *   list     a match adds 1 to nmatch[pattern] and appends (pattern, dist, ~df, rank) to the
 *            device list; past the capacity it is counted and not written.  The key holds the
 *            rank, so the order of the appends cannot show in the sorted list.
 *   cut      over the sorted list: the first k records of each pattern's segment, with the
 *            terms' byte lengths for the word gather.
 */
#include "kernels.h"
#include "dev_common.h"
#include "launch_util.h"

namespace {

constexpr uint32_t ROW_WORDS = 17;   /* 68 bytes >= MT_TERM_MAX, an odd word stride */
static_assert(ROW_WORDS * 4 >= MT_TERM_MAX + 2, "a lane's row holds MT_TERM_MAX bytes");
static_assert(MT_TERM_MAX == MT_PAT + 2, "the longest term a fuzzy pattern of MT_PAT bytes can match");

__device__ __forceinline__ uint32_t term_len(const MtSrc& s, uint32_t t) {
    if (s.tkey) return s.tlen[t];
    const uint64_t n = s.moff[t + 1] - s.moff[t];
    return n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n;
}

/* the first min(len, MT_TERM_MAX) bytes of term t into the lane's row; false when they lie
 * outside the corpus or blob (no such table is built: the term then matches nothing) */
__device__ __forceinline__ bool term_load(const MtSrc& s, uint32_t t, uint32_t len, uint32_t* row) {
    const uint32_t nb = len < MT_TERM_MAX ? len : MT_TERM_MAX;
    uint8_t* rb = (uint8_t*)row;
    const uint8_t* from;
    if (s.tkey) {
        const uint4 k = s.tkey[t];
        if (k.w != 0xFFFFFFFFu) {   /* under 16 bytes: the key's own bytes (k_term_meta) */
            row[0] = k.x; row[1] = k.y; row[2] = k.z; row[3] = k.w;
            return len < 16u;
        }
        const uint64_t off = (((uint64_t)k.y << 32) | k.x) & 0xFFFFFFFFFFull;
        if (off + nb > s.corpus_bytes) return false;
        from = s.corpus + off;
    } else {
        const uint64_t off = s.moff[t];
        if (off + nb > s.corpus_bytes) return false;
        from = s.blob + off;
    }
    for (uint32_t x = 0; x < nb; ++x) rb[x] = from[x];
    return true;
}

__device__ __forceinline__ uint32_t min3(uint32_t a) { return a < MT_NO_MATCH ? a : MT_NO_MATCH; }

/* dist(p, t) when it is <= d, else a value > d (at most MT_NO_MATCH); |n - m| <= d <= 2.
 * Cell k of row i is D[i][i + k - 2]: i bytes of the term against j = i + k - 2 of the pattern. */
__device__ uint32_t band_dist(const uint8_t* p, uint32_t m, const uint8_t* t, uint32_t n, uint32_t d, bool osa) {
    uint32_t pp[5], pv[5], cu[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        pp[k] = MT_NO_MATCH;
        pv[k] = (k >= 2 && (uint32_t)(k - 2) <= m) ? (uint32_t)(k - 2) : MT_NO_MATCH;   /* D[0][j] = j */
    }
    for (uint32_t i = 1; i <= n; ++i) {
        const uint32_t tb = t[i - 1], tb2 = i > 1 ? t[i - 2] : 0x100u;
        uint32_t best = MT_NO_MATCH;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int j = (int)i + k - 2;
            uint32_t v = MT_NO_MATCH;
            if (j == 0) v = min3(i);
            else if (j > 0 && (uint32_t)j <= m) {
                const uint32_t pj = p[j - 1];
                v = pv[k] + (tb != pj ? 1u : 0u);                      /* D[i-1][j-1] */
                if (k < 4 && pv[k + 1] + 1u < v) v = pv[k + 1] + 1u;    /* D[i-1][j] */
                if (k > 0 && cu[k - 1] + 1u < v) v = cu[k - 1] + 1u;    /* D[i][j-1] */
                if (osa && j > 1 && tb == (uint32_t)p[j - 2] && tb2 == pj && pp[k] + 1u < v) v = pp[k] + 1u;   /* D[i-2][j-2] */
                v = min3(v);
            }
            cu[k] = v;
            best = v < best ? v : best;
        }
        if (best > d) return MT_NO_MATCH;
#pragma unroll
        for (int k = 0; k < 5; ++k) { pp[k] = pv[k]; pv[k] = cu[k]; }
    }
    const uint32_t kf = m + 2u - n;   /* 0..4 */
    uint32_t r = MT_NO_MATCH;
#pragma unroll
    for (int k = 0; k < 5; ++k)
        if (kf == (uint32_t)k) r = pv[k];
    return r;
}

__global__ __launch_bounds__(MT_NT) void k_mt_scan(const MtScanArgs a) {
    __shared__ uint32_t s_term[MT_NT * ROW_WORDS];
    __shared__ uint32_t s_pat[MT_GROUP * MT_PAT / 4];
    __shared__ uint8_t s_len[MT_GROUP], s_kind[MT_GROUP], s_bud[MT_GROUP];
    const uint32_t tid = threadIdx.x;
    const uint32_t np = a.np < MT_GROUP ? a.np : MT_GROUP;
    {   /* the group's patterns: MT_PAT bytes each, 16-byte aligned slots */
        const uint32_t* src = (const uint32_t*)(a.pat + (uint64_t)a.p0 * MT_PAT);
        for (uint32_t w = tid; w < np * (MT_PAT / 4); w += MT_NT) s_pat[w] = src[w];
        if (tid < np) {
            s_len[tid] = a.plen[a.p0 + tid];
            s_kind[tid] = a.pkind[a.p0 + tid];
            s_bud[tid] = a.pbudget[a.p0 + tid];
        }
    }
    __syncthreads();
    uint32_t* row = s_term + tid * ROW_WORDS;
    const uint8_t* tb = (const uint8_t*)row;
    const uint8_t* pats = (const uint8_t*)s_pat;
    const uint64_t ntiles = ((uint64_t)a.V + MT_NT - 1) / MT_NT;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t t64 = tile * MT_NT + tid;
        if (t64 >= a.V) continue;   /* the row is the lane's own: no barrier inside the loop */
        const uint32_t t = (uint32_t)t64;
        const uint32_t len = term_len(a.src, t);
        bool loaded = false, have = false;
        for (uint32_t i = 0; i < np; ++i) {
            const uint32_t m = s_len[i], prefix = s_kind[i], d = prefix ? 0u : s_bud[i];
            if (prefix ? len < m : (len + d < m || len > m + d)) continue;
            if (!loaded) {
                have = term_load(a.src, t, len, row);
                loaded = true;
            }
            if (!have) break;
            const uint8_t* p = pats + i * MT_PAT;
            const uint32_t fix = prefix ? m : (a.fixed_prefix < m ? a.fixed_prefix : m);
            if (len < fix) continue;
            bool eq = true;
            for (uint32_t x = 0; x < fix && eq; ++x) eq = tb[x] == p[x];
            if (!eq) continue;
            const uint32_t dist = prefix ? 0u : band_dist(p, m, tb, len, d, a.transpose != 0u);
            if (dist > d) continue;
            atomicAdd(&a.nmatch[a.p0 + i], 1ull);
            const unsigned long long at = atomicAdd(a.nrec, 1ull);
            if (at < a.list_cap) {
                a.key[at] = make_uint4(t, ~a.df[t], dist, i);
                a.val[at] = t;
            }
        }
    }
}

__global__ void k_mt_cut(const MtCutArgs a) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n = (uint64_t)a.np * a.k;
    if (e > n) return;
    if (e == n) { a.wlen[e] = 0; return; }
    const uint32_t i = (uint32_t)(e / a.k), j = (uint32_t)(e % a.k);
    const uint32_t lo = a.seg[i], hi = a.seg[i + 1];
    uint32_t term = 0, dist = 0, df = 0;
    uint64_t wl = 0;
    if (j < hi - lo) {
        const uint4 k = a.key[lo + j];
        if (k.x < a.V) {
            term = k.x;
            df = ~k.y;
            dist = k.z;
            wl = term_len(a.src, term);
        }
    }
    a.term[e] = term;
    a.dist[e] = (uint8_t)dist;
    a.df[e] = df;
    a.wlen[e] = wl;
}

__global__ void k_mt_words_model(const uint32_t* __restrict__ term, const uint64_t* __restrict__ woff, uint64_t n,
                                 const MtSrc src, uint32_t V, uint8_t* __restrict__ bytes) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t o = woff[i], len = woff[i + 1] - o;
    const uint32_t t = term[i];
    if (!len || t >= V) return;
    const uint64_t off = src.moff[t];
    const bool in = off + len <= src.corpus_bytes;
    for (uint64_t x = 0; x < len; ++x) bytes[o + x] = in ? src.blob[off + x] : (uint8_t)0;
}

}  // namespace

int launch_match_scan(const MtScanArgs& a, uint32_t ncu, hipStream_t s) {
    if (!a.V || !a.np) return 0;
    if (a.np > MT_GROUP) return -1;
    const uint64_t ntiles = ((uint64_t)a.V + MT_NT - 1) / MT_NT;
    k_mt_scan<<<cu_grid(ntiles, ncu, MT_WG_PER_CU), MT_NT, 0, s>>>(a);
    return ok();
}

int launch_match_cut(const MtCutArgs& a, hipStream_t s) {
    if (!a.np || !a.k) return 0;
    k_mt_cut<<<grid_for((uint64_t)a.np * a.k + 1), 256, 0, s>>>(a);
    return ok();
}

int launch_match_words_model(const uint32_t* term, const uint64_t* woff, uint64_t n, const MtSrc& src, uint32_t V,
                             uint8_t* bytes, hipStream_t s) {
    if (!n) return 0;
    k_mt_words_model<<<grid_for(n), 256, 0, s>>>(term, woff, n, src, V, bytes);
    return ok();
}
