/*
 * snippets.hip — best passage and match marks of (query, document) jobs over the resident corpus
 * (include/tfidf.h: tfidf_snippet).  The run stores no positions; they are found on demand in the
 * documents that were hit.
 *
 *   lookup   one lane per query term: its identity key (dev_common.h) and whether the run's
 *            vocabulary holds it (vocab_find_rank: the probe of k_query_lookup).  The host builds
 *            every query's table of found terms from the keys.
 *   scan     the unit of work is a tile of SN_TILE bytes of a job's document, so one long document
 *            spreads over the whole grid.  A lane loads one 16-byte group, builds its whitespace
 *            mask (SWAR) and its token-start bits; the tile, a halo behind it and the query's keys
 *            lie in LDS.  A lane that owns a token start reads at most lmax + 1 bytes forward
 *            (lmax: the query's longest found term), forms the term's key and probes the table.
 *            The count pass leaves per tile the tokens and the matches; after the scans of both
 *            the write pass does the same work again and writes the match records, in position
 *            order by construction.  No atomics.
 *   select   one lane per candidate start (a match position): it walks the following matches
 *            inside the window, ORing a 256-bit slot mask in registers.  The maximum of the total
 *            key (cover, hits, ~position) is reduced in LDS and across a job's slices by an atomic
 *            maximum, whose result does not depend on the order; the document's slots by an OR.
 *   emit     per job: centring, the recount, the window's byte bounds (the tile by binary search
 *            in the token prefix sums, the byte by a select inside the tile's start bits).
 *   fill     the marks and the window's bytes.
 */
#include "../../include/tfidf.h"
#include "dev_vocab.h"
#include "launch_util.h"

namespace {

constexpr int NT = SN_NT;
constexpr uint32_t GROUPS = SN_TILE / 16u;            /* 256: one per lane */
constexpr uint32_t HALO_GROUPS = SN_HALO / 16u;
constexpr uint32_t ROW = 5u;                          /* u32 words per 16-byte group in LDS: the lanes' byte reads at
                                                         one index of their groups fall into 32 distinct banks */

/* ------------------------------------------------------------------ lookup -- */

__device__ __forceinline__ void term_key(const uint8_t* p, uint64_t n, uint64_t* klo, uint64_t* khi) {
    if (n < 16u) {
        uint64_t lo = 0, hi = 0;
        for (uint32_t b = 0; b < (uint32_t)n; ++b) {
            const uint64_t c = p[b];
            if (b < 8u) lo |= c << (8u * b);
            else hi |= c << (8u * (b - 8u));
        }
        make_short_key(lo, hi, (uint32_t)n, klo, khi);
    } else {
        make_long_key(p, n, klo, khi);
    }
}

__global__ void k_sn_lookup(const SnLookupArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nterms) return;
    const uint64_t t0 = a.toff[i], n = a.toff[i + 1] - t0;
    const uint8_t* p = a.tbytes + t0;
    uint64_t klo = 0, khi = 0;
    term_key(p, n, &klo, &khi);
    a.key[2 * (size_t)i] = klo;
    a.key[2 * (size_t)i + 1] = khi;
    a.found[i] = a.voc.V && vocab_find_rank(a.voc, klo, khi, p, n) != QUERY_NO_TERM ? 1u : 0u;
}

__global__ void k_sn_jobs(const uint32_t* pos, const uint32_t* job_query, uint32_t njobs, const uint32_t* order,
                          const uint64_t* doc_off, SnJob* jobs) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= njobs) return;
    SnJob o{};
    o.query = job_query[j];
    if (pos[j] == TERMS_NO_POS) {
        o.flags = TFIDF_SNIP_NO_DOC;
    } else {
        const uint32_t d = order[pos[j]];
        o.base = doc_off[d];
        o.len = doc_off[d + 1] - o.base;
    }
    jobs[j] = o;
}

/* -------------------------------------------------------------------- scan -- */

/* the last index i in [0, n] with first[i] <= x, first non-decreasing, first[0] <= x */
__device__ __forceinline__ uint32_t owner_of(const uint32_t* first, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (first[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

/* A tile of a document: `doc` its first byte, len its bytes, ts the tile's first position relative
 * to the document (negative in the first tile of a misaligned document, a multiple of 16 away from
 * an aligned address).  Group g of the tile is the positions [ts + 16 g, + 16). */
struct Tile {
    const uint8_t* doc;
    uint64_t len;
    int64_t ts;
};

/* group g's 16 bytes (zero outside the document) and its whitespace mask (set outside the document).
 * A group inside the document is one aligned 16-byte load; one that straddles an edge of the
 * document is read byte by byte, so nothing outside the document is touched. */
__device__ __forceinline__ uint4 load_group(const Tile& t, uint32_t g, uint32_t* ws) {
    const int64_t r = t.ts + 16 * (int64_t)g;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r + 16 <= 0 || r >= (int64_t)t.len) {
        *ws = 0xFFFFu;
        return v;
    }
    if (r >= 0 && r + 16 <= (int64_t)t.len) {
        v = gload(reinterpret_cast<const uint4*>(t.doc + r));
        *ws = ws_mask16_swar(v);
        return v;
    }
    uint32_t w[4] = {0, 0, 0, 0}, m = 0xFFFFu;
    for (int b = 0; b < 16; ++b) {
        const int64_t p = r + b;
        if (p >= 0 && p < (int64_t)t.len) {
            const uint32_t c = t.doc[p];
            w[b >> 2] |= c << (8 * (b & 3));
            if (!is_ws(c)) m &= ~(1u << b);
        }
    }
    *ws = m;
    return make_uint4(w[0], w[1], w[2], w[3]);
}

/* The token-start bits of the lane's group of tile `t`: a byte that is no whitespace behind one that
 * is, or behind the document's edge.  wsm: NT words of LDS.  One barrier. */
__device__ __forceinline__ uint32_t start_bits(const Tile& t, uint32_t ws, uint32_t* wsm) {
    const uint32_t l = threadIdx.x;
    wsm[l] = ws;
    lds_barrier();
    uint32_t prev;
    if (l) {
        prev = wsm[l - 1] >> 15;
    } else {   /* the byte before the tile: the previous tile's last, or the document's edge */
        const int64_t p = t.ts - 1;
        prev = (p < 0 || p >= (int64_t)t.len) ? 1u : (is_ws(t.doc[p]) ? 1u : 0u);
    }
    return ~ws & ((ws << 1) | prev) & 0xFFFFu;
}

/* byte y of the staged tile (y < SN_TILE + SN_HALO) */
__device__ __forceinline__ uint32_t lds_byte(const uint32_t* tile, uint32_t y) {
    return (tile[(y >> 4) * ROW + ((y >> 2) & 3u)] >> (8u * (y & 3u))) & 0xFFu;
}

template <bool WRITE>
__global__ void __launch_bounds__(NT) k_sn_scan(const SnScanArgs a) {
    __shared__ uint32_t s_tile[(GROUPS + HALO_GROUPS) * ROW];
    __shared__ uint32_t s_wsm[NT];
    __shared__ uint64_t s_key[2 * SN_TAB_MAX];
    __shared__ uint32_t s_sum[NT / 64];
    const uint32_t l = threadIdx.x;
    for (uint32_t t = a.t0 + blockIdx.x; t < a.t1; t += gridDim.x) {
        const uint32_t j = owner_of(a.tile_first, a.njobs, t);
        const SnJob job = a.jobs[j];
        const SnQuery q = a.queries[job.query];
        Tile tl;
        tl.doc = a.corpus + job.base;
        tl.len = job.len;
        tl.ts = (int64_t)(t - a.tile_first[j]) * SN_TILE - (int64_t)((uintptr_t)tl.doc & 15u);
        uint32_t ws;
        const uint4 v = load_group(tl, l, &ws);
        s_tile[l * ROW] = v.x;
        s_tile[l * ROW + 1] = v.y;
        s_tile[l * ROW + 2] = v.z;
        s_tile[l * ROW + 3] = v.w;
        if (l < HALO_GROUPS) {
            uint32_t hw;
            const uint4 h = load_group(tl, GROUPS + l, &hw);
            s_tile[(GROUPS + l) * ROW] = h.x;
            s_tile[(GROUPS + l) * ROW + 1] = h.y;
            s_tile[(GROUPS + l) * ROW + 2] = h.z;
            s_tile[(GROUPS + l) * ROW + 3] = h.w;
        }
        for (uint32_t i = l; i < q.tab_size; i += NT) {
            const SnEnt e = a.tab[q.tab_off + i];
            s_key[2 * i] = e.klo;
            s_key[2 * i + 1] = e.khi;
        }
        const uint32_t starts = start_bits(tl, ws, s_wsm);   /* the barrier publishes the tile and the keys too */
        const uint32_t ntok = __popc(starts);

        /* the lane's tokens: which of them match, and what */
        uint32_t mbits = 0, nm = 0;
        uint32_t mrec[8];   /* len << 8 | slot of the lane's matches: a group of 16 bytes holds at most 8 token starts.
                               Indexed by constants after unrolling, so it stays in registers */
        if (q.tab_size) {
            uint32_t k = 0;
            for (uint32_t sb = starts; sb; sb &= sb - 1, ++k) {
                const uint32_t y0 = 16u * l + (uint32_t)__builtin_ctz(sb);
                const uint64_t r0 = (uint64_t)(tl.ts + (int64_t)y0);
                const uint64_t room = tl.len - r0;             /* bytes of the document from the token on */
                const uint64_t lim = room < (uint64_t)q.lmax + 1u ? room : (uint64_t)q.lmax + 1u;
                uint64_t lo = 0, hi = 0;
                uint32_t n = 0;
                for (; n < lim; ++n) {
                    const uint32_t y = y0 + n;
                    const uint32_t c = y < SN_TILE + SN_HALO ? lds_byte(s_tile, y) : (uint32_t)tl.doc[r0 + n];
                    if (c == 0u || is_ws(c)) break;
                    if (n < 8u) lo |= (uint64_t)c << (8u * n);
                    else if (n < 16u) hi |= (uint64_t)c << (8u * (n - 8u));
                }
                if (n > q.lmax) continue;                      /* longer than every found term */
                uint64_t klo, khi;
                if (n < 16u) make_short_key(lo, hi, n, &klo, &khi);
                else make_long_key(tl.doc + r0, n, &klo, &khi);
                const uint32_t mask = q.tab_size - 1u;
                for (uint32_t h = sn_hash(klo, khi) & mask, probe = 0; probe < q.tab_size; h = (h + 1u) & mask, ++probe) {
                    const uint64_t ehi = s_key[2 * h + 1];
                    if (ehi == SN_ENT_EMPTY) break;
                    if (ehi != khi || s_key[2 * h] != klo) continue;
                    const SnEnt e = a.tab[q.tab_off + h];
                    bool same = e.len == n;
                    if (same && n >= 16u)                      /* a 120-bit hash: the bytes decide */
                        for (uint32_t b = 0; same && b < n; ++b) same = a.tbytes[e.boff + b] == tl.doc[r0 + b];
                    if (!same) continue;
                    mbits |= 1u << k;
                    if (WRITE) {
#pragma unroll
                        for (uint32_t x = 0; x < 8; ++x)
                            if (x == nm) mrec[x] = (n << 8) | e.slot;
                    }
                    ++nm;
                    break;
                }
            }
        }
        if (!WRITE) {
            uint32_t tt, tm;
            (void)block_excl_scan<NT, true>(ntok, s_sum, &tt);
            (void)block_excl_scan<NT, true>(nm, s_sum, &tm);
            if (l == 0) {
                a.tile_tok[t] = tt;
                a.tile_match[t] = tm;
            }
        } else {
            uint32_t tt, tm;
            const uint32_t tok0 = block_excl_scan<NT, true>(ntok, s_sum, &tt);
            const uint32_t m0 = block_excl_scan<NT, true>(nm, s_sum, &tm);
            const uint32_t tokbase = a.tile_tok[t] - a.tile_tok[a.tile_first[j]] + tok0;
            uint4* out = a.rec + (a.tile_match[t] - a.rec0) + m0;
            uint32_t k = 0, w = 0;
            for (uint32_t sb = starts; sb; sb &= sb - 1, ++k) {
                if (!(mbits >> k & 1u)) continue;
                const uint64_t r0 = (uint64_t)(tl.ts + (int64_t)(16u * l + (uint32_t)__builtin_ctz(sb)));
                uint32_t ls = 0;
#pragma unroll
                for (uint32_t x = 0; x < 8; ++x)
                    if (x == w) ls = mrec[x];
                out[w] = make_uint4((uint32_t)r0, (uint32_t)(r0 >> 32), tokbase + k, ls);
                ++w;
            }
        }
        lds_barrier();   /* the next trip overwrites the tile */
    }
}

__global__ void k_sn_totals(const uint32_t* tile_first, uint32_t njobs, const uint32_t* tile_tok, const uint32_t* tile_match,
                            uint32_t* tot) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= njobs) return;
    const uint32_t a = tile_first[j], b = tile_first[j + 1];
    tot[2 * (size_t)j] = tile_tok[b] - tile_tok[a];
    tot[2 * (size_t)j + 1] = tile_match[b] - tile_match[a];
}

/* ------------------------------------------------------------------ select -- */

/* job jj's records in the sub-batch's list: [*mb, *mb + *m) */
__device__ __forceinline__ void job_list(const SnSelArgs& a, uint32_t jj, uint32_t* mb, uint32_t* m) {
    const uint32_t ta = a.tile_first[a.j0 + jj], tb = a.tile_first[a.j0 + jj + 1];
    const uint32_t rec0 = a.tile_match[a.tile_first[a.j0]];
    *mb = a.tile_match[ta] - rec0;
    *m = a.tile_match[tb] - a.tile_match[ta];
}

__global__ void __launch_bounds__(NT) k_sn_select(const SnSelArgs a) {
    __shared__ unsigned long long s_best;
    __shared__ unsigned long long s_mask[4];
    const uint32_t nj = a.j1 - a.j0;
    for (uint32_t x = blockIdx.x; x < a.nslices; x += gridDim.x) {
        const uint32_t jj = owner_of(a.slice_first, nj, x);
        uint32_t mb, m;
        job_list(a, jj, &mb, &m);
        const uint4* rec = a.rec + mb;
        if (threadIdx.x == 0) s_best = 0ull;
        if (threadIdx.x < 4) s_mask[threadIdx.x] = 0ull;
        lds_barrier();
        const uint32_t c0 = (x - a.slice_first[jj]) * SN_SLICE;
        unsigned long long best = 0ull, own[4] = {0ull, 0ull, 0ull, 0ull};
        for (uint32_t i = c0 + threadIdx.x; i < c0 + SN_SLICE && i < m; i += NT) {
            const uint4 r = gload(rec + i);
            const uint64_t end = (uint64_t)r.z + a.window;
            unsigned long long mk[4] = {0ull, 0ull, 0ull, 0ull};
            uint32_t hits = 0;
            for (uint32_t ii = i; ii < m; ++ii) {             /* at most `window` steps: positions are distinct */
                const uint4 f = gload(rec + ii);
                if ((uint64_t)f.z >= end) break;
                const uint32_t sl = f.w & 0xFFu;
#pragma unroll
                for (uint32_t w = 0; w < 4; ++w) mk[w] |= (sl >> 6) == w ? 1ull << (sl & 63u) : 0ull;
                ++hits;
            }
            const uint32_t cover = __popcll(mk[0]) + __popcll(mk[1]) + __popcll(mk[2]) + __popcll(mk[3]);
            const unsigned long long key = (unsigned long long)cover << 44 | (unsigned long long)hits << 32 | (0xFFFFFFFFu - r.z);
            best = key > best ? key : best;
            const uint32_t sl = r.w & 0xFFu;
#pragma unroll
            for (uint32_t w = 0; w < 4; ++w) own[w] |= (sl >> 6) == w ? 1ull << (sl & 63u) : 0ull;
        }
        /* the wave's maximum and OR, then one LDS atomic per wave */
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long ob = __shfl_xor(best, o, 64);
            best = ob > best ? ob : best;
#pragma unroll
            for (uint32_t w = 0; w < 4; ++w) own[w] |= __shfl_xor(own[w], o, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMax(&s_best, best);
            for (uint32_t w = 0; w < 4; ++w) atomicOr(&s_mask[w], own[w]);
        }
        lds_barrier();
        if (threadIdx.x == 0 && s_best) atomicMax(a.best + jj, s_best);
        if (threadIdx.x < 4 && s_mask[threadIdx.x]) atomicOr(a.mask + 4 * (size_t)jj + threadIdx.x, s_mask[threadIdx.x]);
        lds_barrier();
    }
}

/* -------------------------------------------------------------------- emit -- */

/* first record of rec[0, m) whose position is >= pos */
__device__ __forceinline__ uint32_t lower_rec(const uint4* rec, uint32_t m, uint64_t pos) {
    uint32_t lo = 0, hi = m;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)gload(rec + mid).z < pos) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

/* The first byte (relative to the document) of the job's token k < T, by the whole workgroup: the
 * tile by binary search in the token prefix sums, the byte by a select inside its start bits.
 * Every thread returns the value.  Starts and ends with a barrier. */
__device__ uint64_t token_byte(const SnSelArgs& a, const SnJob& job, uint32_t ta, uint32_t tb, uint32_t k, uint32_t* s_wsm,
                               uint32_t* s_sum, uint64_t* s_res) {
    /* the last tile of [ta, tb) whose base ordinal is <= k */
    uint32_t lo = ta, hi = tb - 1;
    const uint32_t base = a.tile_tok[ta];
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (a.tile_tok[mid] - base <= k) lo = mid;
        else hi = mid - 1;
    }
    const uint32_t want = k - (a.tile_tok[lo] - base);   /* the want-th start of that tile */
    Tile tl;
    tl.doc = a.corpus + job.base;
    tl.len = job.len;
    tl.ts = (int64_t)(lo - ta) * SN_TILE - (int64_t)((uintptr_t)tl.doc & 15u);
    uint32_t ws;
    (void)load_group(tl, threadIdx.x, &ws);
    const uint32_t starts = start_bits(tl, ws, s_wsm);
    uint32_t total;
    const uint32_t before = block_excl_scan<NT, true>(__popc(starts), s_sum, &total);
    if (want >= before && want < before + __popc(starts)) {
        uint32_t sb = starts;
        for (uint32_t i = before; i < want; ++i) sb &= sb - 1;
        *s_res = (uint64_t)(tl.ts + (int64_t)(16u * threadIdx.x + (uint32_t)__builtin_ctz(sb)));
    }
    lds_barrier();
    const uint64_t r = *s_res;
    lds_barrier();
    return r;
}

__global__ void __launch_bounds__(NT) k_sn_emit(const SnSelArgs a) {
    __shared__ uint32_t s_wsm[NT];
    __shared__ uint32_t s_sum[NT / 64];
    __shared__ uint64_t s_res;
    __shared__ unsigned long long s_mask[4];
    const uint32_t nj = a.j1 - a.j0, W = a.window;
    for (uint32_t jj = blockIdx.x; jj < nj; jj += gridDim.x) {
        const SnJob job = a.jobs[a.j0 + jj];
        const uint32_t ta = a.tile_first[a.j0 + jj], tb = a.tile_first[a.j0 + jj + 1];
        uint32_t mb, m;
        job_list(a, jj, &mb, &m);
        const uint4* rec = a.rec + mb;
        const uint32_t T = a.tile_tok[tb] - a.tile_tok[ta];
        SnOut o{};
        o.flags = job.flags;
        o.ntokens = T;
        o.nmatch = m;
        uint32_t lo = 0, hi = 0;
        if (T) {   /* uniform over the workgroup */
            uint64_t s1 = 0, e1 = W < T ? W : T;
            if (m) {
                const unsigned long long key = a.best[jj];
                const uint64_t s = 0xFFFFFFFFu - (uint32_t)key;
                const uint32_t hits = (uint32_t)(key >> 32) & 0xFFFu;
                const uint32_t i0 = lower_rec(rec, m, s);
                const uint64_t last = gload(rec + i0 + hits - 1).z;
                const uint64_t slack = W - (last - s + 1), back = slack / 2 < s ? slack / 2 : s;
                s1 = s - back;
                e1 = s1 + W < T ? s1 + W : T;
                lo = lower_rec(rec, m, s1);
                hi = lower_rec(rec, m, e1);
            }
            if (threadIdx.x < 4) s_mask[threadIdx.x] = 0ull;
            lds_barrier();
            for (uint32_t i = lo + threadIdx.x; i < hi; i += NT) {   /* at most `window` records */
                const uint32_t sl = gload(rec + i).w & 0xFFu;
                atomicOr(&s_mask[sl >> 6], 1ull << (sl & 63u));
            }
            lds_barrier();
            o.cover = __popcll(s_mask[0]) + __popcll(s_mask[1]) + __popcll(s_mask[2]) + __popcll(s_mask[3]);
            o.hits = hi - lo;
            o.win_tok[0] = (uint32_t)s1;
            o.win_tok[1] = (uint32_t)e1;
            o.win_byte[0] = token_byte(a, job, ta, tb, (uint32_t)s1, s_wsm, s_sum, &s_res);
            o.win_byte[1] = e1 < T ? token_byte(a, job, ta, tb, (uint32_t)e1, s_wsm, s_sum, &s_res) : job.len;
            o.nmarks = o.hits < a.max_marks ? o.hits : a.max_marks;
            o.mlo = (uint64_t)mb + lo;
            o.text_len = a.want_text ? o.win_byte[1] - o.win_byte[0] : 0ull;
            const unsigned long long* dm = a.mask + 4 * (size_t)jj;
            o.nterms_matched = __popcll(dm[0]) + __popcll(dm[1]) + __popcll(dm[2]) + __popcll(dm[3]);
        }
        if (threadIdx.x == 0) a.out[jj] = o;
    }
}

__global__ void __launch_bounds__(NT) k_sn_fill(const SnFillArgs a) {
    const uint32_t nj = a.j1 - a.j0;
    for (uint32_t jj = blockIdx.x; jj < nj; jj += gridDim.x) {
        const SnOut o = a.out[jj];
        const uint64_t m0 = a.mark_off[jj];
        for (uint32_t i = threadIdx.x; i < o.nmarks; i += NT) {
            const uint4 r = gload(a.rec + o.mlo + i);
            a.mark_byte[m0 + i] = (uint64_t)r.y << 32 | r.x;
            a.mark_len[m0 + i] = r.w >> 8;
            a.mark_slot[m0 + i] = r.w & 0xFFu;
        }
        const uint8_t* src = a.corpus + a.jobs[a.j0 + jj].base + o.win_byte[0];
        uint8_t* dst = a.text + a.text_off[jj];
        for (uint64_t i = threadIdx.x; i < o.text_len; i += NT) dst[i] = src[i];
    }
}

}  // namespace

int launch_sn_lookup(const SnLookupArgs& a, hipStream_t s) {
    if (!a.nterms) return 0;
    k_sn_lookup<<<grid_for(a.nterms, 64), 64, 0, s>>>(a);
    return ok();
}

int launch_sn_jobs(const uint32_t* pos, const uint32_t* job_query, uint32_t njobs, const uint32_t* order,
                   const uint64_t* doc_off, SnJob* jobs, hipStream_t s) {
    if (!njobs) return 0;
    k_sn_jobs<<<grid_for(njobs), NT, 0, s>>>(pos, job_query, njobs, order, doc_off, jobs);
    return ok();
}

int launch_sn_scan(const SnScanArgs& a, uint32_t ncu, hipStream_t s) {
    if (a.t1 <= a.t0) return 0;
    const unsigned grid = cu_grid(a.t1 - a.t0, ncu, SN_WG_PER_CU);
    if (a.rec) k_sn_scan<true><<<grid, NT, 0, s>>>(a);
    else k_sn_scan<false><<<grid, NT, 0, s>>>(a);
    return ok();
}

int launch_sn_totals(const uint32_t* tile_first, uint32_t njobs, const uint32_t* tile_tok, const uint32_t* tile_match,
                     uint32_t* tot, hipStream_t s) {
    if (!njobs) return 0;
    k_sn_totals<<<grid_for(njobs), NT, 0, s>>>(tile_first, njobs, tile_tok, tile_match, tot);
    return ok();
}

int launch_sn_select(const SnSelArgs& a, uint32_t ncu, hipStream_t s) {
    if (!a.nslices) return 0;
    k_sn_select<<<cu_grid(a.nslices, ncu, SN_WG_PER_CU), NT, 0, s>>>(a);
    return ok();
}

int launch_sn_emit(const SnSelArgs& a, uint32_t ncu, hipStream_t s) {
    const uint32_t nj = a.j1 - a.j0;
    if (!nj) return 0;
    k_sn_emit<<<cu_grid(nj, ncu, SN_WG_PER_CU), NT, 0, s>>>(a);
    return ok();
}

int launch_sn_fill(const SnFillArgs& a, uint32_t ncu, hipStream_t s) {
    const uint32_t nj = a.j1 - a.j0;
    if (!nj) return 0;
    k_sn_fill<<<cu_grid(nj, ncu, SN_WG_PER_CU), NT, 0, s>>>(a);
    return ok();
}
