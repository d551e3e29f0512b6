/*
 * analyze.hip — the analyzer on the device (include/tfidf.h, section "analyzer"): case folding,
 * punctuation stripping, a minimum token length and a stop-word list, bytes to bytes of the same
 * length, in front of tfidf_run.  The reference has no such stage: it counts what fscanf("%s")
 * returns (TFIDF.c:141-152).
 *
 *   map      the pure byte map (no stop words, min_len <= 1): one 16-byte group per lane, SWAR
 *            range compares on 32-bit words (the form of dev_common.h's ws_mask4), no LDS.
 *   filter   persistent workgroups of 256 lanes, one tile of AN_TILE bytes per step.  The
 *            stop-word table (analyze_tab.h) is copied to LDS once per workgroup.  Per tile:
 *              1. every lane loads its 16 bytes (lanes 0..9 also one group of the AN_HALO bytes
 *                 on either side), maps them and stores them to LDS with two 16-bit masks:
 *                 token bytes, and token bytes that continue a token (no document starts there)
 *              2. a lane that owns a token start (a token byte whose predecessor is none, or a
 *                 document's first byte: transform.hip's scheme) gets the token's length from
 *                 the continuation bits (64 bits, one count-trailing-ones), and for a token of
 *                 at most 64 bytes hashes it four bytes at a time from the aligned LDS words,
 *                 probes the table and marks the token's bytes in a blank bitmap in LDS
 *                 (atomicOr: lanes of one workgroup share the bitmap's words; the held bytes
 *                 themselves are not written in this phase)
 *              3. every lane blanks the marked bytes of its 16 and stores them
 *            With a stemmer (the instantiation k_an_filter<true>; calls without one launch
 *            k_an_filter<false>, the kernel as it was) a token that phase 2 keeps is stemmed by
 *            the same lane (analyze_stem.h: the word's vowel mask and its last 8 letters in
 *            registers).  The tail [S, len) goes into the blank bitmap.  The letters of the
 *            stem's last 8 that differ from the token's go to a byte array of their own in LDS,
 *            s_patch, with their bits in a third bitmap, s_pm; phase 3 merges them.  s_buf is
 *            still not written in phase 2: other lanes read its words, masked, for their own
 *            tokens.  Distinct lanes store distinct bytes of s_patch, and a token has one owner.
 *            A workgroup decides the fate of its own tile's bytes only: a token that began
 *            before the left halo is longer than 64 bytes when it reaches the tile and is never
 *            blanked, and a token that starts in the tile ends inside the right halo or is too
 *            long as well.  So no two workgroups write the same byte and the pass is out of
 *            place.  Tokens blanked are counted where they start: one integer atomic add per
 *            workgroup.
 * With TFIDF_AN_UTF8 (and a map flag: alone it changes nothing and the kernels above run) the
 * instantiations of their own k_an_map_u8 and k_an_filter<STEM, true> run: a group that holds a
 * byte >= 0x80 resolves its UTF-8 sequences (analyze_utf8.h) from its own 16 bytes, the four
 * bytes on either side of them, read from global memory again (its neighbours' loads brought
 * them into the cache), and the document-start bitmap; every other group takes the SWAR path
 * alone.  The tables stay in global memory.  Halo groups are staged the same way, so every byte
 * held in LDS is sequence-mapped whatever its place in the held range.  Sequences changed are
 * counted where they start, by the tile's own groups: one integer atomic add per workgroup.
 * The input may have any alignment: groups are cut at multiples of 16 of the OUTPUT, an
 * unaligned input is read as two aligned 16-byte loads and a byte shift, and byte by byte where
 * that would leave in[0, nbytes).
 */
#include "kernels.h"
#include "dev_common.h"
#include "analyze_tab.h"
#include "analyze_stem.h"
#include "analyze_utf8.h"

namespace {

constexpr int NT = 256;
constexpr uint32_t HG = AN_HALO / 16u;         /* halo groups on each side */
constexpr uint32_t NG = NT + 2u * HG;          /* groups held in LDS */
constexpr uint32_t AN_FLAG_LOWER = 1u, AN_FLAG_PUNCT = 2u;   /* TFIDF_AN_* of include/tfidf.h */
constexpr uint32_t AN_FLAG_UTF8 = 16u;
static_assert(AN_FLAG_LOWER == AN_U8_LOWER && AN_FLAG_PUNCT == AN_U8_PUNCT, "analyze_utf8.h takes the map flags as they are");
constexpr uint32_t AN_MAX_WORD = 64u;
static_assert(AN_TILE == NT * 16u, "one 16-byte group per lane");
static_assert(AN_HALO % 16u == 0 && AN_HALO > AN_MAX_WORD + 1u, "the halo argument");
constexpr uint32_t BM_WORDS = (NG * 16u / 32u + 4u) & ~3u;   /* a bit per held byte, whole 16-byte rows */
constexpr uint32_t AN_STATIC_LDS = NG * 16u + 3u * BM_WORDS * 4u + 16u;
constexpr uint32_t AN_STEM_LDS = NG * 16u + BM_WORDS * 4u;   /* s_patch and s_pm, behind the table */

int ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

/* bit 7 of every byte of lo7 (bytes <= 0x7F) that lies in [a, b], 1 <= a <= b <= 0x7F: both
 * per-byte sums stay inside their byte */
__device__ __forceinline__ uint32_t in_range(uint32_t lo7, uint32_t a, uint32_t b) {
    return (lo7 + (0x80u - a) * 0x01010101u) & ~(lo7 + (0x7Fu - b) * 0x01010101u) & 0x80808080u;
}

/* the byte map on four bytes */
__device__ __forceinline__ uint32_t map_word(uint32_t x, uint32_t flags) {
    const uint32_t ascii = ~x & 0x80808080u, lo7 = x & 0x7F7F7F7Fu;
    const uint32_t upper = in_range(lo7, 0x41u, 0x5Au) & ascii;
    if (flags & AN_FLAG_PUNCT) {
        const uint32_t keep = upper | in_range(lo7, 0x61u, 0x7Au) | in_range(lo7, 0x30u, 0x39u) |
                              in_range(lo7, 0x09u, 0x0Du) | in_range(lo7, 0x20u, 0x20u);
        const uint32_t m = ((ascii & ~keep) >> 7) * 0xFFu;   /* 0xFF in every punctuation byte */
        x = (x & ~m) | (0x20202020u & m);
    }
    if (flags & AN_FLAG_LOWER) x |= upper >> 2;              /* + 0x20: bit 5 of 0x41..0x5A is clear */
    return x;
}

/* 0xFF in byte j for every set bit j of the low four */
__device__ __forceinline__ uint32_t expand4(uint32_t b) { return (((b & 0xFu) * 0x00204081u) & 0x01010101u) * 0xFFu; }

/* the byte map on the bytes of a group whose bit in win is set */
__device__ __forceinline__ uint4 map_group(uint4 v, uint32_t win, uint32_t flags) {
    if (win == 0u || flags == 0u) return v;
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t m = map_word(w[k], flags);
        if (win == 0xFFFFu) w[k] = m;
        else {
            const uint32_t bm = expand4(win >> (4 * k));
            w[k] = (w[k] & ~bm) | (m & bm);
        }
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

/* bit j = byte p + j lies in [lo, hi) */
__device__ __forceinline__ uint32_t range16(long long p, uint64_t lo, uint64_t hi) {
    long long b = (long long)lo - p, e = (long long)hi - p;
    b = b < 0 ? 0 : (b > 16 ? 16 : b);
    e = e < 0 ? 0 : (e > 16 ? 16 : e);
    return e > b ? ((1u << e) - 1u) & ~((1u << b) - 1u) : 0u;
}

/* in[p, p + 16) with 0x20 for the bytes outside in[0, nbytes); phase = the input base's low four
 * address bits (p is a multiple of 16, so it is the group's phase too) */
__device__ __forceinline__ uint4 load16(const AnArgs& a, long long p, uint32_t phase) {
    if (p >= 0 && (uint64_t)p + 16u <= a.nbytes) {
        if (phase == 0u) return gload((const uint4*)(a.in + p));
        if ((uint64_t)p >= phase && (uint64_t)p - phase + 32u <= a.nbytes) {
            const uint4* q = (const uint4*)(a.in + p - phase);
            const uint4 u = gload(q), v = gload(q + 1);
            const uint32_t w[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
            const uint32_t k = phase >> 2, sh = phase & 3u;
            uint32_t r[4] = {0, 0, 0, 0};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                if (k == (uint32_t)kk) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) r[j] = __builtin_amdgcn_alignbyte(w[kk + j + 1], w[kk + j], sh);
                }
            }
            return make_uint4(r[0], r[1], r[2], r[3]);
        }
    }
    uint64_t lo = 0x2020202020202020ull, hi = lo;   /* the edges: a rolled loop, few registers */
#pragma unroll 1
    for (int j = 0; j < 16; ++j) {
        const long long q = p + j;
        if (q >= 0 && (uint64_t)q < a.nbytes) {
            const uint64_t c = (uint64_t)(gload(a.in + q) ^ 0x20u) << (8 * (j & 7));
            if (j < 8) lo ^= c;
            else hi ^= c;
        }
    }
    return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}

/* out[p, p + 16), p a multiple of 16 below nbytes: whole, or byte by byte up to nbytes */
__device__ __forceinline__ void store16(const AnArgs& a, uint64_t p, uint4 v) {
    if (p + 16u <= a.nbytes) {
        g_u32x4 r;
        r.x = v.x; r.y = v.y; r.z = v.z; r.w = v.w;
        *(GLOBAL_AS g_u32x4*)(a.out + p) = r;
        return;
    }
    const uint64_t lo = v.x | ((uint64_t)v.y << 32), hi = v.z | ((uint64_t)v.w << 32);
#pragma unroll 1
    for (int j = 0; j < 16 && p + (uint64_t)j < a.nbytes; ++j)
        gstore(a.out + p + j, (uint8_t)((j < 8 ? lo : hi) >> (8 * (j & 7))));
}

/* the sequence map on the group at byte p: raw are its bytes as loaded, v the byte-mapped ones,
 * which receive the sequences' bytes.  Returns the sequences changed that start in the group.
 * win != 0 puts a byte of the group inside [lo, hi), so 0 <= p < nbytes. */
__device__ __forceinline__ uint32_t u8_patch(const AnArgs& a, long long p, uint4 raw, uint32_t win, uint4& v) {
    uint32_t c[6] = {0u, raw.x, raw.y, raw.z, raw.w, 0u};
    if (win == 0u || !an_u8_any(c + 1)) return 0u;
    c[0] = an_u8_ld4(a.in, a.nbytes, p - 4);
    c[5] = an_u8_ld4(a.in, a.nbytes, p + 16);
    uint32_t g[4] = {v.x, v.y, v.z, v.w};
    const uint32_t n = an_u8_group(c, an_u8_range24(p, a.lo, a.hi), an_u8_cut24(a.dstart, p, a.lo, a.hi),
                                   a.flags & (AN_FLAG_LOWER | AN_FLAG_PUNCT), g);
    v = make_uint4(g[0], g[1], g[2], g[3]);
    return n;
}

/* the workgroup's sum of n, added to *ctr by one lane */
__device__ __forceinline__ void an_count(uint32_t n, uint32_t* s_red, unsigned long long* ctr) {
    const uint32_t tid = threadIdx.x, wsum = wave_sum(n);
    if ((tid & 63u) == 0u) s_red[tid >> 6] = wsum;
    __syncthreads();
    if (tid == 0) {
        uint32_t tot = 0;
        for (int k = 0; k < NT / 64; ++k) tot += s_red[k];
        if (tot) (void)gatomic_add(ctr, (unsigned long long)tot);
    }
}

__global__ __launch_bounds__(NT) void k_an_docstarts(const AnArgs a) {
    const uint64_t d = (uint64_t)blockIdx.x * NT + threadIdx.x + 1u;
    if (d >= a.ndocs) return;
    const uint64_t pos = a.doc_off[d];
    if (pos <= a.lo || pos >= a.hi || pos >= a.nbytes) return;   /* the window's own edges are boundaries already */
    atomicOr(&a.dstart[pos >> 5], 1u << (pos & 31u));
}

__global__ __launch_bounds__(NT) void k_an_map(const AnArgs a, uint64_t ngroups) {
    const uint64_t g = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (g >= ngroups) return;
    const uint32_t phase = (uint32_t)((uintptr_t)a.in & 15u);
    const long long p = (long long)(g * 16u);
    const uint4 v = load16(a, p, phase);
    store16(a, (uint64_t)p, map_group(v, range16(p, a.lo, a.hi), a.flags));
}

/* k_an_map with the sequence map: every lane stays for the count */
__global__ __launch_bounds__(NT) void k_an_map_u8(const AnArgs a, uint64_t ngroups) {
    __shared__ uint32_t s_red[NT / 64];
    const uint64_t g = (uint64_t)blockIdx.x * NT + threadIdx.x;
    uint32_t n = 0u;
    if (g < ngroups) {
        const uint32_t phase = (uint32_t)((uintptr_t)a.in & 15u);
        const long long p = (long long)(g * 16u);
        const uint32_t win = range16(p, a.lo, a.hi);
        const uint4 raw = load16(a, p, phase);
        uint4 v = map_group(raw, win, a.flags);
        n = u8_patch(a, p, raw, win, v);
        store16(a, (uint64_t)p, v);
    }
    an_count(n, s_red, a.blanked + 2);
}

struct Group {
    uint32_t tk, ds;
};

/* loads, maps and publishes group gi of the tile whose first group lies at byte p0; with U8 the
 * sequences too, and nu8 receives the ones changed that start in the group */
template <bool U8>
__device__ __forceinline__ Group an_stage(const AnArgs& a, long long p0, uint32_t gi, uint32_t phase, uint32_t* s_buf,
                                          uint32_t* s_tk, uint32_t* s_cont, uint32_t& nu8) {
    const long long p = p0 + (long long)(gi * 16u);
    const uint32_t win = range16(p, a.lo, a.hi);
    const uint4 raw = load16(a, p, phase);
    uint4 v = map_group(raw, win, a.flags);
    if (U8) nu8 += u8_patch(a, p, raw, win, v);
    Group g;
    g.tk = ~ws_mask16_swar(v) & win;
    g.ds = 0u;
    if (p >= 0 && (uint64_t)p < a.nbytes) g.ds = (gload(a.dstart + ((uint64_t)p >> 5)) >> ((uint32_t)p & 16u)) & 0xFFFFu;
    *(uint4*)(s_buf + gi * 4u) = v;
    ((uint16_t*)s_tk)[gi] = (uint16_t)g.tk;
    ((uint16_t*)s_cont)[gi] = (uint16_t)(g.tk & ~g.ds);
    return g;
}

/* sets bits [b, e) of an LDS bitmap whose words the workgroup's lanes share: at most three words */
__device__ __forceinline__ void an_mark(uint32_t* bm, uint32_t b, uint32_t e) {
    while (b < e) {
        const uint32_t w = b >> 5, n = (e < ((w + 1u) << 5) ? e : ((w + 1u) << 5)) - b;
        atomicOr(&bm[w], (n == 32u ? ~0u : (1u << n) - 1u) << (b & 31u));
        b += n;
    }
}

/* the tokens that start in group gi: their bits set in s_blank when short or a stop word.
 * s_buf, s_cont and s_blank are indexed by the byte's position in the held range: bit b of the
 * bitmaps is byte b of s_buf.  Returns the tokens blanked that start inside the tile.  With STEM
 * a token that is kept is stemmed: its tail into s_blank, the changed letters of its head into
 * s_patch and s_pm, and nstem counts the tokens changed that start inside the tile. */
template <bool STEM>
__device__ __forceinline__ uint32_t an_filter(const AnArgs& a, uint32_t gi, Group g, const uint32_t* s_buf, const uint32_t* s_tk,
                                              const uint32_t* s_cont, uint32_t* s_blank, const uint32_t* slots,
                                              uint32_t nslots, const uint32_t* words, uint8_t* s_patch, uint32_t* s_pm,
                                              uint32_t& nstem) {
    /* group 0's predecessor is not held: a token that runs into the halo from before it is
     * longer than 64 bytes when it reaches the tile, so it need not be seen as one */
    const uint32_t prev = gi ? (uint32_t)((const uint16_t*)s_tk)[gi - 1u] >> 15 : 1u;
    uint32_t nblank = 0;
    for (uint32_t m = g.tk & (~((g.tk << 1) | prev) | g.ds) & 0xFFFFu; m; m &= m - 1u) {
        const uint32_t pos = gi * 16u + (uint32_t)__builtin_ctz(m);
        /* the continuation bits behind the start: di + 2 <= (NG * 16 - 1) / 32 for every start this lane owns */
        const uint32_t q = pos + 1u, di = q >> 5, sh = q & 31u;
        const uint64_t c01 = (uint64_t)s_cont[di] | ((uint64_t)s_cont[di + 1u] << 32);
        const uint64_t x = sh ? (c01 >> sh) | ((uint64_t)s_cont[di + 2u] << (64u - sh)) : c01;
        const uint32_t len = 1u + (x == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~x));
        if (len > AN_MAX_WORD || pos + len <= AN_HALO) continue;   /* never blanked, or it ends before the tile */
        bool blank = len < a.min_len;
        if (!blank && nslots) {
            const uint32_t* aw = s_buf + (pos >> 2);
            blank = an_tab_find(slots, nslots, words, aw, pos & 3u, len, an_hash(aw, pos & 3u, len)) != 0;
        }
        if (blank) {
            an_mark(s_blank, pos, pos + len);
            nblank += pos >= AN_HALO ? 1u : 0u;
        } else if (STEM && len >= 3u) {
            const uint32_t* aw = s_buf + (pos >> 2);
            uint64_t t;
            const uint32_t S = an_stem(aw, pos & 3u, len, &t);
            /* the stem's last 8 letters against the token's: S <= len is all this relies on */
            uint64_t x = (t ^ an_tail8(aw, pos & 3u, S)) & ~an_low(S < 8u ? 64u - 8u * S : 0u);
            if (S < len) an_mark(s_blank, pos + S, pos + len);
            nstem += (pos >= AN_HALO && (S < len || x)) ? 1u : 0u;
            for (; x; x &= ~(0xFFull << (8u * ((uint32_t)__builtin_ctzll(x) >> 3)))) {
                const uint32_t j = (uint32_t)__builtin_ctzll(x) >> 3, p = pos + S - 8u + j;   /* byte j of t is letter S - 8 + j */
                s_patch[p] = (uint8_t)(t >> (8u * j));
                atomicOr(&s_pm[p >> 5], 1u << (p & 31u));
            }
        }
    }
    return nblank;
}

template <bool STEM, bool U8 = false>
__global__ __launch_bounds__(NT, (STEM || U8) ? 4 : 8) void k_an_filter(const AnArgs a, uint64_t ntiles) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_tab[];   /* with STEM: s_patch and s_pm behind the table */
    __shared__ __attribute__((aligned(16))) uint32_t s_buf[NG * 4u];
    __shared__ __attribute__((aligned(16))) uint32_t s_tk[BM_WORDS], s_cont[BM_WORDS], s_blank[BM_WORDS];
    __shared__ uint32_t s_red[NT / 64];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < a.tab_bytes / 16u; i += NT) ((uint4*)s_tab)[i] = gload((const uint4*)a.tab + i);
    if (tid < BM_WORDS) s_blank[tid] = 0u;
    uint8_t* s_patch = (uint8_t*)s_tab + a.tab_bytes;   /* NG * 16 bytes: a byte per held byte */
    uint32_t* s_pm = (uint32_t*)(s_patch + NG * 16u);   /* BM_WORDS: the bytes of s_patch that count */
    if (STEM && tid < BM_WORDS) s_pm[tid] = 0u;
    __syncthreads();
    const uint32_t nslots = s_tab[0];
    const uint32_t* slots = s_tab + AN_HDR_WORDS;
    const uint32_t* words = s_tab + s_tab[2] / 4u;
    const uint32_t phase = (uint32_t)((uintptr_t)a.in & 15u);
    const uint32_t hgi = tid < HG ? tid : HG + NT + (tid - HG);   /* lanes 0..2 HG - 1: a halo group too */
    uint32_t nblank = 0, nstem = 0, nu8 = 0, nu8_halo = 0;   /* a halo group's sequences count in its own tile */
    /* no barrier between steps: after the second barrier a lane reads only its own group of
     * s_buf and its own 16 bits of s_blank (which it clears for the next step; the halo groups'
     * bits are set but never read), and the next step's first phase rewrites both from that
     * lane alone.  The same holds for s_patch and s_pm: after the second barrier a lane reads
     * its own group and its own 16 bits of them and clears the bits, the next step's first phase
     * touches neither, and other lanes write them again only behind the next step's first
     * barrier, which this lane reaches after its reads. */
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long p0 = (long long)(tile * AN_TILE) - (long long)AN_HALO;
        const Group gm = an_stage<U8>(a, p0, HG + tid, phase, s_buf, s_tk, s_cont, nu8);
        Group gh{0u, 0u};
        if (tid < 2u * HG) gh = an_stage<U8>(a, p0, hgi, phase, s_buf, s_tk, s_cont, nu8_halo);
        __syncthreads();
        nblank += an_filter<STEM>(a, HG + tid, gm, s_buf, s_tk, s_cont, s_blank, slots, nslots, words, s_patch, s_pm, nstem);
        if (tid < HG) nblank += an_filter<STEM>(a, tid, gh, s_buf, s_tk, s_cont, s_blank, slots, nslots, words, s_patch, s_pm, nstem);
        __syncthreads();
        uint4 v = *(const uint4*)(s_buf + (HG + tid) * 4u);
        if (STEM) {
            const uint32_t pm = ((uint16_t*)s_pm)[HG + tid];
            if (pm) {
                ((uint16_t*)s_pm)[HG + tid] = 0u;
                const uint4 pv = *(const uint4*)(s_patch + (HG + tid) * 16u);
                uint32_t w[4] = {v.x, v.y, v.z, v.w};
                const uint32_t pw[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t bm = expand4(pm >> (4 * k));
                    w[k] = (w[k] & ~bm) | (pw[k] & bm);
                }
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        const uint32_t bl = ((uint16_t*)s_blank)[HG + tid];
        if (bl) {
            ((uint16_t*)s_blank)[HG + tid] = 0u;
            uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t bm = expand4(bl >> (4 * k));
                w[k] = (w[k] & ~bm) | (0x20202020u & bm);
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        store16(a, tile * AN_TILE + tid * 16u, v);
    }
    const uint32_t wsum = wave_sum(nblank);
    if ((tid & 63u) == 0u) s_red[tid >> 6] = wsum;
    __syncthreads();
    if (tid == 0) {
        uint32_t tot = 0;
        for (int k = 0; k < NT / 64; ++k) tot += s_red[k];
        if (tot) (void)gatomic_add(a.blanked, (unsigned long long)tot);
    }
    if (STEM) {
        __syncthreads();
        const uint32_t ssum = wave_sum(nstem);
        if ((tid & 63u) == 0u) s_red[tid >> 6] = ssum;
        __syncthreads();
        if (tid == 0) {
            uint32_t tot = 0;
            for (int k = 0; k < NT / 64; ++k) tot += s_red[k];
            if (tot) (void)gatomic_add(a.blanked + 1, (unsigned long long)tot);
        }
    }
    if (U8) {
        __syncthreads();
        an_count(nu8, s_red, a.blanked + 2);
    }
}

}  // namespace

int launch_an_docstarts(const AnArgs& a, hipStream_t s) {
    if (hipMemsetAsync(a.dstart, 0, (size_t)(a.nbytes / 32u + 2u) * 4u, s) != hipSuccess) return -1;
    if (a.ndocs < 2u) return 0;
    k_an_docstarts<<<(unsigned)(((uint64_t)a.ndocs - 1u + NT - 1u) / NT), NT, 0, s>>>(a);
    return ok();
}

uint32_t an_lds_bytes(const AnArgs& a, uint32_t nstop) {
    if (a.stemmer) return a.tab_bytes + AN_STATIC_LDS + AN_STEM_LDS;   /* the pure byte map cannot stem */
    return (nstop == 0u && a.min_len <= 1u) ? 0u : a.tab_bytes + AN_STATIC_LDS;
}

int launch_analyze(const AnArgs& a, uint32_t nstop, uint32_t ncu, uint32_t grid_cap, uint32_t* grid, hipStream_t s) {
    *grid = 0u;
    if (!a.nbytes) return 0;
    const uint32_t lds = an_lds_bytes(a, nstop);
    const bool u8 = (a.flags & AN_FLAG_UTF8) != 0u;   /* the caller clears it where it changes nothing */
    if (!lds) {
        const uint64_t ngroups = (a.nbytes + 15u) / 16u, nblocks = (ngroups + NT - 1u) / NT;
        if (nblocks > 0x7FFFFFFFull) return -1;
        if (u8) k_an_map_u8<<<(unsigned)nblocks, NT, 0, s>>>(a, ngroups);
        else k_an_map<<<(unsigned)nblocks, NT, 0, s>>>(a, ngroups);
        return ok();
    }
    const uint64_t ntiles = (a.nbytes + AN_TILE - 1u) / AN_TILE;
    uint32_t per_cu = 163840u / lds;   /* LDS of a CU; 2048 lanes of a CU are eight workgroups */
    /* the stemming instantiation holds 74 VGPRs: six waves per SIMD; the ones with the sequence map 103 and 114: four */
    const uint32_t fit = u8 ? 4u : (a.stemmer ? 6u : 8u);
    per_cu = per_cu > fit ? fit : (per_cu ? per_cu : 1u);
    uint64_t slots = (uint64_t)(ncu ? ncu : 256u) * per_cu;
    if (grid_cap && grid_cap < slots) slots = grid_cap;
    *grid = (uint32_t)(ntiles < slots ? ntiles : slots);
    if (u8) {
        if (a.stemmer) k_an_filter<true, true><<<*grid, NT, a.tab_bytes + AN_STEM_LDS, s>>>(a, ntiles);
        else k_an_filter<false, true><<<*grid, NT, a.tab_bytes, s>>>(a, ntiles);
    } else if (a.stemmer) k_an_filter<true><<<*grid, NT, a.tab_bytes + AN_STEM_LDS, s>>>(a, ntiles);
    else k_an_filter<false><<<*grid, NT, a.tab_bytes, s>>>(a, ntiles);
    return ok();
}
