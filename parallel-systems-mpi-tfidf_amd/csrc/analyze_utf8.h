/*
 * analyze_utf8.h — the analyzer's UTF-8 sequence map (include/tfidf.h, section "analyzer",
 * TFIDF_AN_UTF8) in the form the device kernels run (analyze.hip), one 16-byte group at a time.
 * Plain C as well, so a host program can run the same code against the byte-wise map of
 * analyze_host.c (tests/native/utf8_host_test.c).
 *
 * A group at byte p (a multiple of 16) is resolved from a context of 24 bytes, p - 4 .. p + 19,
 * as six 32-bit words c[0..5]: the group is c[1..4].  A sequence has at most four bytes, so every
 * sequence that holds a byte of the group starts at context byte 1..19 and ends at or before
 * context byte 22.  The owner of a group decodes every sequence that starts there, the ones that
 * start in the three bytes in front of the group too, and writes the bytes that fall inside its
 * own group; the part that falls behind the group is written by the next group's owner, who
 * decodes the same sequence from its own context.  So no group needs another group's result, and
 * a group, a tile or a workgroup edge is no special case.  Bytes outside in[0, nbytes) enter the
 * context as 0x20, which is no part of any sequence: a sequence the buffer's end cuts fails the
 * decode.
 *   lead   bit k = context byte k lies inside the documents' window [lo, hi)
 *   cut    bit k = a document boundary lies directly in front of context byte k (lo and hi
 *          included): a sequence with such a bit behind its first byte is left alone
 * A sequence counts (utf8_changed) where its first byte lies: in the group, context byte 4..19.
 *
 * Tables (analyze_utf8_tab.h, generated): two-byte sequences read one 16-bit entry of AN_U8_T2,
 * longer ones search AN_U8_BLANK and AN_U8_FOLD by bisection.
 */
#ifndef TFIDF_ANALYZE_UTF8_H
#define TFIDF_ANALYZE_UTF8_H

#include <stdint.h>

#ifdef __HIPCC__
#define AN_U8_DATA __device__ static const
#define AN_U8_FN __device__ static inline
#else
#define AN_U8_FN static inline
#endif
#include "analyze_utf8_tab.h"

#define AN_U8_LOWER 1u   /* TFIDF_AN_LOWER */
#define AN_U8_PUNCT 2u   /* TFIDF_AN_PUNCT */

/* the length a lead byte announces; 0: no lead of a well-formed sequence of two or more bytes */
AN_U8_FN uint32_t an_u8_len(uint32_t b0) { return b0 < 0xC2u ? 0u : b0 < 0xE0u ? 2u : b0 < 0xF0u ? 3u : b0 < 0xF5u ? 4u : 0u; }

/* the code point of the len bytes in v (the lead in the low byte), 0 when they are not
 * well-formed: a byte that is no continuation, an overlong form, a surrogate, above U+10FFFF */
AN_U8_FN uint32_t an_u8_decode(uint32_t v, uint32_t len) {
    const uint32_t b0 = v & 0xFFu, b1 = (v >> 8) & 0xFFu, b2 = (v >> 16) & 0xFFu, b3 = v >> 24;
    if ((b1 & 0xC0u) != 0x80u) return 0u;
    if (len == 2u) return ((b0 & 0x1Fu) << 6) | (b1 & 0x3Fu);
    if ((b2 & 0xC0u) != 0x80u) return 0u;
    if (len == 3u) {
        const uint32_t cp = ((b0 & 0x0Fu) << 12) | ((b1 & 0x3Fu) << 6) | (b2 & 0x3Fu);
        return (cp < 0x800u || cp - 0xD800u < 0x800u) ? 0u : cp;
    }
    if ((b3 & 0xC0u) != 0x80u) return 0u;
    const uint32_t cp = ((b0 & 0x07u) << 18) | ((b1 & 0x3Fu) << 12) | ((b2 & 0x3Fu) << 6) | (b3 & 0x3Fu);
    return (cp < 0x10000u || cp > 0x10FFFFu) ? 0u : cp;
}

/* UTF-8 of cp in len bytes, the lead in the low byte */
AN_U8_FN uint32_t an_u8_encode(uint32_t cp, uint32_t len) {
    if (len == 2u) return (0xC0u | (cp >> 6)) | ((0x80u | (cp & 0x3Fu)) << 8);
    if (len == 3u) return (0xE0u | (cp >> 12)) | ((0x80u | ((cp >> 6) & 0x3Fu)) << 8) | ((0x80u | (cp & 0x3Fu)) << 16);
    return (0xF0u | (cp >> 18)) | ((0x80u | ((cp >> 12) & 0x3Fu)) << 8) | ((0x80u | ((cp >> 6) & 0x3Fu)) << 16) |
           ((0x80u | (cp & 0x3Fu)) << 24);
}

/* what becomes of the code point cp >= U+0080 of len bytes: 0 it stays, 0x20 it is blanked, else L(cp) */
AN_U8_FN uint32_t an_u8_map_cp(uint32_t cp, uint32_t len, uint32_t flags) {
    if (len == 2u) {
        const uint32_t e = AN_U8_T2[cp - 0x80u];
        if ((flags & AN_U8_PUNCT) && (e & 0x8000u)) return 0x20u;
        return (flags & AN_U8_LOWER) ? (e & 0x7FFu) : 0u;
    }
    if (flags & AN_U8_PUNCT) {   /* the last run with lo <= cp */
        uint32_t b = 0u, e = AN_U8_NBLANK;
        while (e - b > 1u) {
            const uint32_t m = (b + e) >> 1;
            if (AN_U8_BLANK[m].lo <= cp) b = m;
            else e = m;
        }
        if (AN_U8_BLANK[b].lo <= cp && cp <= AN_U8_BLANK[b].hi) return 0x20u;
    }
    if (flags & AN_U8_LOWER) {
        uint32_t b = 0u, e = AN_U8_NFOLD;
        while (e - b > 1u) {
            const uint32_t m = (b + e) >> 1;
            if (AN_U8_FOLD[m].lo <= cp) b = m;
            else e = m;
        }
        const uint32_t lo = AN_U8_FOLD[b].lo;
        if (lo <= cp && cp <= AN_U8_FOLD[b].hi && ((cp - lo) & (AN_U8_FOLD[b].stride - 1u)) == 0u)   /* the stride is 1 or 2 */
            return (uint32_t)((int32_t)cp + AN_U8_FOLD[b].delta);
    }
    return 0u;
}

/* in[q, q + 4) as a word, 0x20 for the bytes outside in[0, nbytes): one aligned load where the
 * four bytes are inside and aligned, else byte by byte */
AN_U8_FN uint32_t an_u8_ld4(const uint8_t* in, uint64_t nbytes, long long q) {
    if (q >= 0 && (uint64_t)q + 4u <= nbytes && (((uintptr_t)(in + q)) & 3u) == 0u) return *(const uint32_t*)(const void*)(in + q);
    uint32_t w = 0x20202020u;
    for (int j = 0; j < 4; ++j)
        if (q + j >= 0 && (uint64_t)(q + j) < nbytes) w ^= (uint32_t)(in[q + j] ^ 0x20u) << (8 * j);
    return w;
}

/* bit k = byte p - 4 + k lies in [lo, hi), k < 24 */
AN_U8_FN uint32_t an_u8_range24(long long p, uint64_t lo, uint64_t hi) {
    long long b = (long long)lo - (p - 4), e = (long long)hi - (p - 4);
    b = b < 0 ? 0 : (b > 24 ? 24 : b);
    e = e < 0 ? 0 : (e > 24 ? 24 : e);
    return e > b ? ((1u << e) - 1u) & ~((1u << b) - 1u) : 0u;
}

/* bit k = a boundary lies directly in front of byte p - 4 + k, k < 24: a document's start from
 * the bitmap dstart (bit i = a document starts at byte i; nbytes / 32 + 2 words), lo or hi.
 * p is a multiple of 16 below nbytes. */
AN_U8_FN uint32_t an_u8_cut24(const uint32_t* dstart, long long p, uint64_t lo, uint64_t hi) {
    const uint64_t i = (uint64_t)p >> 5;
    uint32_t cut;
    if (p & 16) cut = (dstart[i] >> 12) | (dstart[i + 1u] << 20);
    else cut = (i ? dstart[i - 1u] >> 28 : 0u) | (dstart[i] << 4);
    const long long kl = (long long)lo - (p - 4), kh = (long long)hi - (p - 4);
    if (kl >= 0 && kl < 24) cut |= 1u << kl;
    if (kh >= 0 && kh < 24) cut |= 1u << kh;
    return cut & 0xFFFFFFu;
}

/* bit j = bit 7 of byte j of a word whose other bits are clear */
AN_U8_FN uint32_t an_u8_mask4(uint32_t t) { return (((t >> 7) * 0x00204081u) >> 21) & 0xFu; }

/* 1 when the four words hold a byte >= 0x80 */
AN_U8_FN int an_u8_any(const uint32_t g[4]) { return ((g[0] | g[1] | g[2] | g[3]) & 0x80808080u) != 0u; }

/* Resolves the sequences of the group c[1..4] and writes their mapped bytes into g[0..3], the
 * group's words (the byte map of the ASCII bytes may have been applied to them already: it
 * touches no byte >= 0x80 and a sequence holds no other).  Returns the sequences changed whose
 * first byte lies in the group. */
AN_U8_FN uint32_t an_u8_group(const uint32_t c[6], uint32_t lead, uint32_t cut, uint32_t flags, uint32_t g[4]) {
    uint32_t m = 0u;
    for (int k = 0; k < 5; ++k) m |= an_u8_mask4(c[k] & (c[k] << 1) & 0x80808080u) << (4 * k);   /* bytes >= 0xC0 */
    m &= lead & 0x000FFFFEu;
    if (!m) return 0u;
    const uint64_t x0 = (uint64_t)c[0] | ((uint64_t)c[1] << 32), x1 = (uint64_t)c[2] | ((uint64_t)c[3] << 32),
                   x2 = (uint64_t)c[4] | ((uint64_t)c[5] << 32);
    uint64_t glo = (uint64_t)g[0] | ((uint64_t)g[1] << 32), ghi = (uint64_t)g[2] | ((uint64_t)g[3] << 32);
    uint32_t n = 0u;
    for (; m; m &= m - 1u) {
        const uint32_t k = (uint32_t)__builtin_ctz(m), sh = 8u * (k & 7u);
        const uint64_t a = k < 8u ? x0 : (k < 16u ? x1 : x2), b = k < 8u ? x1 : (k < 16u ? x2 : 0ull);
        const uint32_t v = (uint32_t)(sh ? (a >> sh) | (b << (64u - sh)) : a);   /* context bytes k .. k + 3 */
        const uint32_t len = an_u8_len(v & 0xFFu);
        if (!len || ((cut >> (k + 1u)) & ((1u << (len - 1u)) - 1u))) continue;
        const uint32_t cp = an_u8_decode(v, len);
        if (!cp) continue;
        const uint32_t to = an_u8_map_cp(cp, len, flags);
        if (!to) continue;
        const uint64_t bm = len == 4u ? 0xFFFFFFFFull : (1ull << (8u * len)) - 1ull;
        const uint64_t nv = to == 0x20u ? (0x20202020ull & bm) : (uint64_t)an_u8_encode(to, len);
        if (k < 4u) {                 /* it starts in front of the group: its tail */
            const uint32_t s = 8u * (4u - k);
            glo = (glo & ~(bm >> s)) | (nv >> s);
        } else if (k < 12u) {
            const uint32_t s = 8u * (k - 4u);
            glo = (glo & ~(bm << s)) | (nv << s);
            if (s > 32u) ghi = (ghi & ~(bm >> (64u - s))) | (nv >> (64u - s));
        } else {                      /* what runs past the group is the next group's */
            const uint32_t s = 8u * (k - 12u);
            ghi = (ghi & ~(bm << s)) | (nv << s);
        }
        n += k >= 4u ? 1u : 0u;
    }
    g[0] = (uint32_t)glo;
    g[1] = (uint32_t)(glo >> 32);
    g[2] = (uint32_t)ghi;
    g[3] = (uint32_t)(ghi >> 32);
    return n;
}

#endif
