/*
 * ngram.hip — word n-grams (shingles) in front of the counter (include/tfidf.h, section
 * "n-grams": tfidf_ngrams).  The first stage whose output has another size than its input.
 *
 *   bounds   transform.hip's boundary kernels, as they are: tok_start / tok_end in order,
 *            document boundaries honoured, windows and unaligned bases handled.
 *   sizes    one lane per token: the lengths of the next max_n - 1 tokens of the same row (no
 *            document starts between two of them: the boundary kernels' bitmap says so).
 *            Segment i = the grams that start at token i; its bytes = the sum over the valid n
 *            of the component lengths plus n (n - 1 joiners and a blank).  The caller scans
 *            them: seg_off[ntok + 1].
 *   offsets  one lane per document: out_off[d] = seg_off[lower_bound(tok_start, doc_off[d])];
 *            one lane per output tile: the segment that holds the tile's first byte.  Binary
 *            searches over integers, no atomics.
 *   write    output-driven: a workgroup per tile of NG_TILE output bytes, one 16-byte group
 *            and one 16-byte store per lane.  The descriptors of the segments that touch the
 *            tile are staged in LDS (offsets relative to the tile, token starts and lengths),
 *            and so are the first NG_SRC_CAP input bytes from the tile's first token on, loaded
 *            as 16-byte groups (a token beyond them is read from device memory); a lane finds
 *            its segment by a binary search there, the gram and the component from the token
 *            lengths, and then steps through its 16 bytes: source byte, joiner
 *            or blank.  No two workgroups write the same byte; the result does not depend on
 *            the grid.  A segment is at least 2 bytes, but a token with fewer than min_n - 1
 *            successors in its row has an empty one, and empty segments are not bounded by the
 *            tile's bytes: a tile that touches more segments than the LDS arrays hold reads
 *            the descriptors from device memory instead, with the same code.
 *
 * -DNG_WRITE_BY_TOKEN (make variant, never the measured library) replaces the write kernel by
 * the A/B baseline: one lane per token walks its segment with byte stores.
 */
#include "kernels.h"
#include "dev_common.h"

namespace {

constexpr int NT = 256;
static_assert(NG_TILE == NT * 16, "one 16-byte group per lane");
inline unsigned grid_for(uint64_t n) { return n ? (unsigned)((n + NT - 1) / NT) : 1u; }
int ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

/* ------------------------------------------------------------------- sizes -- */

/* a document starts in (x, y], x < y both inside the window: from the boundary kernels' bitmap
 * (bit i = a document starts at p0 + i), or for a long stretch by a binary search of doc_off */
__device__ __forceinline__ bool ng_doc_start_in(const NgArgs& a, uint64_t x, uint64_t y) {
    const uint64_t lo = (uint64_t)((long long)x - a.p0) + 1u, hi = (uint64_t)((long long)y - a.p0);   /* bits [lo, hi] */
    if (hi - lo >= 256u) {
        uint64_t b = 0, e = (uint64_t)a.ndocs + 1u;   /* the first offset behind x */
        while (b < e) {
            const uint64_t mid = b + ((e - b) >> 1);
            if (a.doc_off[mid] <= x) b = mid + 1;
            else e = mid;
        }
        return b <= a.ndocs && a.doc_off[b] <= y;
    }
    for (uint64_t w = lo >> 5; w <= hi >> 5; ++w) {
        uint32_t m = a.dstart[w];
        if (w == lo >> 5) m &= ~0u << (lo & 31u);
        if (w == hi >> 5) m &= ~0u >> (31u - (uint32_t)(hi & 31u));
        if (m) return true;
    }
    return false;
}

__global__ __launch_bounds__(NT) void k_ng_sizes(const NgArgs a) {
    __shared__ unsigned long long s_grams;
    if (threadIdx.x == 0) s_grams = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
    uint32_t grams = 0;
    if (i < a.ntok) {
        uint64_t bytes = 0, prefix = 0, prev = 0;
        for (uint32_t k = 0; k < a.max_n; ++k) {
            const uint64_t t = i + k;
            if (t >= a.ntok) break;
            const uint64_t ts = a.tok_start[t];
            if (k && ng_doc_start_in(a, prev, ts)) break;   /* token t belongs to a later row */
            prev = ts;
            prefix += a.tok_end[t] - ts;
            if (k + 1u >= a.min_n) {
                bytes += prefix + (k + 1u);
                ++grams;
            }
        }
        a.seg_off[i] = bytes;
    }
    grams = wave_sum(grams);   /* every lane: one LDS add per wave, one device add per workgroup */
    if ((threadIdx.x & 63u) == 0 && grams) atomicAdd(&s_grams, (unsigned long long)grams);
    __syncthreads();
    if (threadIdx.x == 0 && s_grams) gatomic_add(a.ngrams, s_grams);
}

/* ----------------------------------------------------------------- offsets -- */

__global__ __launch_bounds__(NT) void k_ng_docoff(const NgArgs a) {
    const uint64_t d = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (d > a.ndocs) return;
    const uint64_t x = a.doc_off[d];
    uint64_t lo = 0, hi = a.ntok;   /* the first token that starts at or behind x */
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a.tok_start[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    a.out_off[d] = a.seg_off[lo];
}

__global__ __launch_bounds__(NT) void k_ng_tileseg(const NgArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (t > a.ntiles) return;
    const uint64_t x = t * NG_TILE;
    uint64_t lo = 0, hi = a.ntok;   /* the first segment that starts behind x */
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a.seg_off[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    a.tile_seg[t] = (uint32_t)(lo ? lo - 1u : 0u);   /* seg_off[0] = 0 <= x: lo >= 1 */
}

/* ------------------------------------------------------------------- write -- */

#ifndef NG_WRITE_BY_TOKEN

constexpr uint32_t NG_MAXN = 8;   /* TFIDF_NGRAM_MAX_N */
/* segments of a tile whose descriptors fit in LDS: NG_TILE / 2 + 1 segments of >= 2 bytes can
 * touch a tile, one more may start at its end, the rest is room for a few empty ones */
constexpr uint32_t NG_SEG_CAP = NG_TILE / 2 + 8;
constexpr uint32_t NG_TOK_CAP = NG_SEG_CAP + NG_MAXN - 1;
constexpr uint32_t U32_SAT = 0xFFFFFFFFu;   /* a staged start this large, or a length of U16_SAT, is read from device memory */
constexpr uint32_t U16_SAT = 0xFFFFu;       /* (16-bit words where they do: the kernel's occupancy is bounded by its LDS) */
constexpr uint32_t NG_SRC_CAP = 8192;       /* input bytes a workgroup stages, from its first token on */

/* The descriptors of the segments [seg0, seg0 + nseg] and their tokens as a lane reads them:
 * from LDS (STAGED) or from device memory.  rel(j) = the start of segment seg0 + j relative to
 * the tile, clamped to [0, 2 * NG_TILE] (16 bits); segment seg0 starts at or before the tile, every later
 * one inside it or behind it. */
__device__ __forceinline__ uint32_t ng_rel(uint64_t seg_start, uint64_t tile0) {
    if (seg_start <= tile0) return 0u;
    return seg_start - tile0 < 2u * NG_TILE ? (uint32_t)(seg_start - tile0) : 2u * NG_TILE;
}

template <bool STAGED>
struct NgView {
    const NgArgs& a;
    uint64_t seg0, tile0;
    uint32_t nseg;
    long long src0;              /* the staged source bytes are [src0, src0 + NG_SRC_CAP) of the input */
    const uint16_t* s_rel;
    const uint32_t* s_ts;        /* token starts relative to src0 */
    const uint16_t* s_len;
    const uint8_t* s_src;
    __device__ __forceinline__ uint32_t rel(uint32_t j) const {
        return STAGED ? s_rel[j] : ng_rel(a.seg_off[seg0 + j], tile0);
    }
    __device__ __forceinline__ void tok(uint32_t j, uint64_t* ts, uint64_t* len) const {
        if (STAGED) {
            const uint32_t t = s_ts[j], l = s_len[j];
            *ts = t != U32_SAT ? (uint64_t)(src0 + (long long)t) : a.tok_start[seg0 + j];
            *len = l != U16_SAT ? (uint64_t)l : a.tok_end[seg0 + j] - *ts;
        } else {
            *ts = a.tok_start[seg0 + j];
            *len = a.tok_end[seg0 + j] - *ts;
        }
    }
    /* the input's byte x, x >= src0 */
    __device__ __forceinline__ uint32_t byte(uint64_t x) const {
        if (STAGED) {
            const uint64_t d = (uint64_t)((long long)x - src0);
            if (d < NG_SRC_CAP) return s_src[d];
        }
        return a.bytes[x];
    }
    /* the segment that holds the tile's byte q: the last one that starts at or before q (empty
     * segments share a start with the non-empty one behind them, which is the last) */
    __device__ __forceinline__ uint32_t locate(uint32_t q) const {
        uint32_t lo = 0, hi = nseg;   /* rel(lo) <= q < rel(hi); rel(nseg) is never read */
        while (hi - lo > 1u) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (rel(mid) > q) hi = mid;
            else lo = mid;
        }
        return lo;
    }
};

/* where the staged source bytes begin: the first token's start, moved down to a 16-byte aligned
 * address (it may lie in front of the input) */
__device__ __forceinline__ long long ng_src0(const NgArgs& a, uint64_t seg0) {
    const uint64_t t0 = a.tok_start[seg0];
    return (long long)t0 - (long long)(((uintptr_t)a.bytes + t0) & 15u);
}

/* what a workgroup stages: the nseg + 1 relative starts, the tokens of the segments and of the
 * grams that begin in the last one, and the input's bytes from the first token on: 16-byte
 * groups where a group lies inside the input, single bytes at its edges */
__device__ __forceinline__ void ng_stage(const NgArgs& a, uint64_t seg0, uint64_t tile0, uint32_t nseg, long long src0, uint32_t tid,
                                         uint16_t* s_rel, uint32_t* s_ts, uint16_t* s_len, uint8_t* s_src) {
    for (uint32_t j = tid; j <= nseg; j += NT) s_rel[j] = (uint16_t)ng_rel(a.seg_off[seg0 + j], tile0);
    const uint64_t rest = a.ntok - seg0;
    const uint32_t ntk = (uint64_t)(nseg + NG_MAXN - 1u) < rest ? nseg + NG_MAXN - 1u : (uint32_t)rest;
    for (uint32_t j = tid; j < ntk; j += NT) {
        const uint64_t ts = a.tok_start[seg0 + j], l = a.tok_end[seg0 + j] - ts, t = (uint64_t)((long long)ts - src0);
        s_ts[j] = t < U32_SAT ? (uint32_t)t : U32_SAT;
        s_len[j] = (uint16_t)(l < U16_SAT ? l : U16_SAT);
    }
    const long long src_end = (long long)a.tok_end[seg0 + ntk - 1u];   /* nothing behind the last token is read */
    for (uint32_t g = tid; g < NG_SRC_CAP / 16u; g += NT) {
        const long long x = src0 + (long long)(g * 16u);
        if (x >= src_end) break;
        if (x >= 0 && x + 16 <= (long long)a.nbytes) {
            *(g_u32x4*)(s_src + g * 16u) = *(const GLOBAL_AS g_u32x4*)(a.bytes + x);
        } else {
            for (uint32_t b = 0; b < 16u; ++b)
                if (x + b >= 0 && x + b < (long long)a.nbytes) s_src[g * 16u + b] = a.bytes[x + b];
        }
    }
}

/* the 16 output bytes [tile0 + q, + 16) of one lane as two words, low byte first; bytes at and
 * behind nbytes_out are 0 */
template <bool STAGED>
__device__ __forceinline__ void ng_group(const NgView<STAGED>& v, uint32_t q, uint64_t* w_lo, uint64_t* w_hi) {
    const NgArgs& a = v.a;
    const uint64_t o = v.tile0 + q;
    uint32_t j = v.locate(q);
    uint32_t seg_end = v.rel(j + 1u);   /* relative to the tile like q; clamped far behind it */
    uint64_t r = j ? (uint64_t)(q - v.rel(j)) : o - a.seg_off[v.seg0];   /* the position inside the segment */
    /* the gram: a segment holds the grams n = min_n.. in order, gram n = n components + n bytes */
    uint32_t n = a.min_n, k = 0;
    uint64_t ts = 0, len = 0, prefix = 0;
    for (uint32_t c = 0; c < n; ++c) {
        v.tok(j + c, &ts, &len);
        prefix += len;
    }
    while (n < a.max_n && r >= prefix + n) {   /* r is inside the segment: the next gram exists */
        r -= prefix + n;
        v.tok(j + n, &ts, &len);
        prefix += len;
        ++n;
    }
    /* the component: its bytes and the joiner or blank behind it */
    for (;; ++k) {
        v.tok(j + k, &ts, &len);
        if (r <= len || k + 1u >= n) break;
        r -= len + 1u;
    }
    uint64_t pos = r, lo = 0, hi = 0;
    for (uint32_t i = 0; i < 16u && o + i < a.nbytes_out; ++i) {
        uint64_t c;
        if (pos < len) {
            c = v.byte(ts + pos);
            ++pos;
        } else {
            c = k + 1u < n ? a.joiner : 0x20u;
            pos = 0;
            ++k;
        }
        if (i < 8u) lo |= c << (8u * i);
        else hi |= c << (8u * (i - 8u));
        if (pos != 0 || i == 15u) continue;
        /* behind a joiner or blank: the next component, gram or segment */
        if (q + i + 1u == seg_end) {   /* the next segment that is not empty: it starts here, inside the tile or at its end */
            if (o + i + 1u >= a.nbytes_out) break;
            do {
                ++j;
                seg_end = v.rel(j + 1u);
            } while (seg_end == q + i + 1u && j + 1u < v.nseg);
            n = a.min_n;
            k = 0;
        } else if (k == n) {
            k = 0;
            ++n;
        }
        v.tok(j + k, &ts, &len);
    }
    *w_lo = lo;
    *w_hi = hi;
}

__global__ __launch_bounds__(NT) void k_ng_write(const NgArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_src[NG_SRC_CAP];
    __shared__ uint32_t s_ts[NG_TOK_CAP];
    __shared__ uint16_t s_rel[NG_SEG_CAP + 1];
    __shared__ uint16_t s_len[NG_TOK_CAP];
    const uint32_t tid = threadIdx.x;
    const uint64_t tile0 = (uint64_t)blockIdx.x * NG_TILE;
    const uint64_t seg0 = a.tile_seg[blockIdx.x];
    uint64_t seg1 = a.tile_seg[blockIdx.x + 1u];   /* the last segment that starts at or before the tile's end */
    if (seg1 < seg0) seg1 = seg0;
    const bool staged = seg1 - seg0 < NG_SEG_CAP;
    const uint32_t nseg = (uint32_t)(seg1 - seg0) + 1u;
    const long long src0 = staged ? ng_src0(a, seg0) : 0;
    if (staged) ng_stage(a, seg0, tile0, nseg, src0, tid, s_rel, s_ts, s_len, s_src);
    __syncthreads();
    const uint32_t q = tid * 16u;
    if (tile0 + q >= a.nbytes_out) return;
    uint64_t lo, hi;
    if (staged) ng_group(NgView<true>{a, seg0, tile0, nseg, src0, s_rel, s_ts, s_len, s_src}, q, &lo, &hi);
    else ng_group(NgView<false>{a, seg0, tile0, nseg, 0, nullptr, nullptr, nullptr, nullptr}, q, &lo, &hi);
    g_u32x4 g;
    g.x = (uint32_t)lo; g.y = (uint32_t)(lo >> 32); g.z = (uint32_t)hi; g.w = (uint32_t)(hi >> 32);
    *(GLOBAL_AS g_u32x4*)(a.out + tile0 + q) = g;   /* the slot's buffer is writable up to the next multiple of 16 */
}

#else   /* the A/B baseline: one lane per token, byte stores */

__global__ __launch_bounds__(NT) void k_ng_write_by_token(const NgArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= a.ntok) return;
    uint64_t o = a.seg_off[i];
    const uint64_t end = a.seg_off[i + 1u];
    for (uint32_t n = a.min_n; n <= a.max_n && o < end; ++n) {
        for (uint32_t k = 0; k < n; ++k) {
            const uint64_t ts = a.tok_start[i + k], len = a.tok_end[i + k] - ts;
            for (uint64_t p = 0; p < len; ++p) a.out[o + p] = a.bytes[ts + p];
            a.out[o + len] = (uint8_t)(k + 1u < n ? a.joiner : 0x20u);
            o += len + 1u;
        }
    }
}

#endif

}  // namespace

int launch_ng_sizes(const NgArgs& a, hipStream_t s) {
    if (!a.ntok) return 0;
    k_ng_sizes<<<grid_for(a.ntok), NT, 0, s>>>(a);
    return ok();
}

int launch_ng_offsets(const NgArgs& a, hipStream_t s) {
    if (!a.ntok) return 0;
    k_ng_docoff<<<grid_for((uint64_t)a.ndocs + 1u), NT, 0, s>>>(a);
    if (a.ntiles) k_ng_tileseg<<<grid_for(a.ntiles + 1u), NT, 0, s>>>(a);
    return ok();
}

int launch_ng_write(const NgArgs& a, hipStream_t s) {
    if (!a.ntiles || !a.ntok) return 0;
    if (a.ntiles > 0x7FFFFFFFull) return -1;
#ifndef NG_WRITE_BY_TOKEN
    k_ng_write<<<(unsigned)a.ntiles, NT, 0, s>>>(a);
#else
    k_ng_write_by_token<<<grid_for(a.ntok), NT, 0, s>>>(a);
#endif
    return ok();
}
