/*
 * analyze_stem.h — the analyzer's Porter stemmer (include/tfidf.h, section "analyzer", step 3)
 * in the form the device kernel runs (analyze.hip): no byte loops over the word after the first
 * pass.  Plain C as well, so a host program can run the same code against the byte-wise
 * tfidf_stem_porter of analyze_host.c (tests/native/stem_host_test.c).
 *
 * The word is read like a stop-word candidate (analyze_tab.h): from aligned 32-bit words `aw`
 * and a byte shift.  One pass over its chunks checks that every byte is a letter a..z (SWAR range
 * compares, the form of analyze.hip's map_word) and builds
 *   vm    bit i = letter i is a vowel.  Whether a y is one depends on its predecessor only, so a
 *         prefix of the word has the same bits as the word: the conditions on "the stem in front
 *         of the suffix" are tests on the low bits of one mask.
 * Then the state is (t, vm, len):
 *   t     the current word's last 8 letters, the last one in the top byte (zero in front of the
 *         word's first letter)
 *   len   the current word's length
 * A suffix of n <= 7 letters is one compare of t's top n bytes.  m of a prefix of p letters is
 * the number of i < p - 1 with vm bit i set and bit i + 1 clear: one popcount.  *v*, *d and *o
 * are bit tests and compares of t's top bytes.
 * Every rule removes a suffix and appends at most four letters without a y.  Removing k letters
 * shifts t up by k bytes and refills its low k bytes from the ORIGINAL word: a rule changes
 * letters only among the last four of the word it produces and no later rule makes the word
 * longer than that by more than one, so the letters more than 8 in front of the current end are
 * always the original ones.  For the same reason the whole difference between the stem and the
 * word's first S letters lies in the stem's last 8 letters, which is t at the end: the caller
 * writes the bytes of t that differ and blanks [S, len).
 */
#ifndef TFIDF_ANALYZE_STEM_H
#define TFIDF_ANALYZE_STEM_H

#include "analyze_tab.h"

#define AN_VOWELS 0x104111u   /* bit (c - 'a') for a, e, i, o, u */

/* a suffix as t's top bytes hold it: its first letter in the lowest byte */
#define AN_S1(a) ((uint64_t)(uint8_t)(a))
#define AN_S2(a, b) (AN_S1(a) | AN_S1(b) << 8)
#define AN_S3(a, b, c) (AN_S2(a, b) | AN_S1(c) << 16)
#define AN_S4(a, b, c, d) (AN_S3(a, b, c) | AN_S1(d) << 24)
#define AN_S5(a, b, c, d, e) (AN_S4(a, b, c, d) | AN_S1(e) << 32)
#define AN_S6(a, b, c, d, e, f) (AN_S5(a, b, c, d, e) | AN_S1(f) << 40)
#define AN_S7(a, b, c, d, e, f, g) (AN_S6(a, b, c, d, e, f) | AN_S1(g) << 48)

typedef struct an_stem_state {
    uint64_t t, vm;
    uint32_t len;
    const uint32_t* aw;
    uint32_t shift;
} an_stem_state;

/* the low n bits */
AN_FN uint64_t an_low(uint32_t n) { return n >= 64u ? ~0ull : (1ull << n) - 1ull; }

/* bytes [q, q + 8) behind aw */
AN_FN uint64_t an_ld8(const uint32_t* aw, uint32_t q) {
    const uint32_t* w = aw + (q >> 2);
    const uint32_t sh = 8u * (q & 3u);
    const uint64_t lo = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    return sh ? (lo >> sh) | ((uint64_t)w[2] << (64u - sh)) : lo;
}

/* the original word's letters [e - 8, e), letter e - 1 in the top byte, zero in front of letter 0 */
AN_FN uint64_t an_tail8(const uint32_t* aw, uint32_t shift, uint32_t e) {
    if (e >= 8u) return an_ld8(aw, shift + e - 8u);
    return e ? an_ld8(aw, shift) << (8u * (8u - e)) : 0ull;
}

/* the current word ends in the n letters s, 1 <= n <= 7 */
AN_FN int an_ends(const an_stem_state* st, uint64_t s, uint32_t n) { return st->len >= n && (st->t >> (64u - 8u * n)) == s; }

/* m of the current word's first p letters */
AN_FN uint32_t an_m(const an_stem_state* st, uint32_t p) {
    return p ? (uint32_t)__builtin_popcountll(st->vm & ~(st->vm >> 1) & an_low(p - 1u)) : 0u;
}

/* *v* of the first p letters */
AN_FN int an_hasv(const an_stem_state* st, uint32_t p) { return (st->vm & an_low(p)) != 0ull; }

/* *d of the first p letters, whose last two are the top bytes of t */
AN_FN int an_double(const an_stem_state* st, uint64_t t, uint32_t p) {
    return p >= 2u && (t >> 56) == ((t >> 48) & 0xFFu) && !((st->vm >> (p - 1u)) & 1ull);
}

/* *o of the first p letters, whose last is the top byte of t */
AN_FN int an_cvc(const an_stem_state* st, uint64_t t, uint32_t p) {
    if (p < 3u || ((st->vm >> (p - 3u)) & 7ull) != 2ull) return 0;
    const uint32_t c = (uint32_t)(t >> 56);
    return c != 'w' && c != 'x' && c != 'y';
}

/* the vowel bits of the rn letters r (none of them a y) */
AN_FN uint64_t an_vowels_of(uint64_t r, uint32_t rn) {
    uint64_t v = 0;
    for (uint32_t i = 0; i < rn; ++i) v |= (uint64_t)((AN_VOWELS >> ((uint32_t)((r >> (8u * i)) & 0xFFu) - 0x61u)) & 1u) << i;
    return v;
}

/* the current word's last n letters (n <= 7) replaced by the rn <= 4 letters r */
AN_FN void an_rep(an_stem_state* st, uint32_t n, uint64_t r, uint32_t rn) {
    if (n) {
        const uint32_t newlen = st->len - n;
        st->t = (st->t << (8u * n)) | (an_tail8(st->aw, st->shift, newlen) & an_low(8u * n));
        st->len = newlen;
    }
    if (rn) {
        st->t = (st->t >> (8u * rn)) | (r << (64u - 8u * rn));
        st->vm = (st->vm & an_low(st->len)) | (an_vowels_of(r, rn) << st->len);
        st->len += rn;
    }
}

#define AN_RULE(sfx, n, r, rn, min_m)                                 \
    if (an_ends(&st, sfx, n)) {                                       \
        if (an_m(&st, st.len - (n)) > (min_m)) an_rep(&st, n, r, rn); \
        break;                                                        \
    }

/* The stem of the len-byte token that starts `shift` bytes (0..3) into aw[0].  Returns its
 * length S, 1 <= S <= len, and in *tail the stem's letters [S - 8, S), the last one in the top
 * byte (zero in front of letter 0): the token's bytes in front of them are the stem's.  An
 * ineligible token (len outside 3..64, a byte outside a..z) returns len and the token's own
 * last bytes.  Reads the words of aw that hold the token and at most two more. */
AN_FN uint32_t an_stem(const uint32_t* aw, uint32_t shift, uint32_t len, uint64_t* tail) {
    an_stem_state st;
    st.aw = aw;
    st.shift = shift;
    st.len = len;
    st.t = an_tail8(aw, shift, len);
    st.vm = 0ull;
    *tail = st.t;
    if (len < 3u || len > 64u) return len;
    /* four letters at a time: the chunk's missing bytes become 'b' (a consonant, no y; their
     * bits lie at and above len, where every use masks them), all four are letters when bit 7
     * of both per-byte sums says so (the sums stay inside their bytes), and the vowel and y bits
     * are gathered as nibbles of two 32-bit halves */
    uint32_t v_lo = 0u, v_hi = 0u, y_lo = 0u, y_hi = 0u;
    for (uint32_t k = 0; 4u * k < len; ++k) {
        const uint32_t rem = len - 4u * k;
        const uint32_t c4 = an_chunk(aw, shift, k, len) | (rem < 4u ? 0x62626262u << (8u * rem) : 0u);
        const uint32_t lo7 = c4 & 0x7F7F7F7Fu;
        if (((lo7 + 0x1F1F1F1Fu) & ~(lo7 + 0x05050505u) & ~c4 & 0x80808080u) != 0x80808080u) return len;
        uint32_t v4 = 0u, y4 = 0u;
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t d = ((c4 >> (8u * j)) & 0xFFu) - 0x61u;
            v4 |= ((AN_VOWELS >> d) & 1u) << j;
            y4 |= (uint32_t)(d == 24u) << j;
        }
        const uint32_t at = 4u * (k & 7u);
        if (k < 8u) { v_lo |= v4 << at; y_lo |= y4 << at; }
        else { v_hi |= v4 << at; y_hi |= y4 << at; }
    }
    st.vm = (uint64_t)v_lo | ((uint64_t)v_hi << 32);
    uint64_t ys = (uint64_t)y_lo | ((uint64_t)y_hi << 32);
    for (; ys; ys &= ys - 1ull) {   /* in rising order: a y is a vowel behind a consonant */
        const uint32_t i = (uint32_t)__builtin_ctzll(ys);
        if (i && !((st.vm >> (i - 1u)) & 1ull)) st.vm |= 1ull << i;
    }

    /* 1a */
    if (an_ends(&st, AN_S4('s', 's', 'e', 's'), 4u) || an_ends(&st, AN_S3('i', 'e', 's'), 3u)) an_rep(&st, 2u, 0ull, 0u);
    else if (!an_ends(&st, AN_S2('s', 's'), 2u) && an_ends(&st, AN_S1('s'), 1u)) an_rep(&st, 1u, 0ull, 0u);

    /* 1b */
    if (an_ends(&st, AN_S3('e', 'e', 'd'), 3u)) {
        if (an_m(&st, st.len - 3u) > 0u) an_rep(&st, 1u, 0ull, 0u);
    } else {
        const uint32_t n = an_ends(&st, AN_S2('e', 'd'), 2u) ? 2u : (an_ends(&st, AN_S3('i', 'n', 'g'), 3u) ? 3u : 0u);
        if (n && an_hasv(&st, st.len - n)) {
            an_rep(&st, n, 0ull, 0u);
            const uint32_t last = (uint32_t)(st.t >> 56);
            if (an_ends(&st, AN_S2('a', 't'), 2u) || an_ends(&st, AN_S2('b', 'l'), 2u) || an_ends(&st, AN_S2('i', 'z'), 2u))
                an_rep(&st, 0u, AN_S1('e'), 1u);
            else if (an_double(&st, st.t, st.len) && last != 'l' && last != 's' && last != 'z') an_rep(&st, 1u, 0ull, 0u);
            else if (an_m(&st, st.len) == 1u && an_cvc(&st, st.t, st.len)) an_rep(&st, 0u, AN_S1('e'), 1u);
        }
    }

    /* 1c */
    if (an_ends(&st, AN_S1('y'), 1u) && an_hasv(&st, st.len - 1u)) an_rep(&st, 1u, AN_S1('i'), 1u);

    /* 2: by the penultimate letter, the longer suffix first where one ends in another */
    switch ((uint32_t)(st.t >> 48) & 0xFFu) {
        case 'a':
            AN_RULE(AN_S7('a', 't', 'i', 'o', 'n', 'a', 'l'), 7u, AN_S3('a', 't', 'e'), 3u, 0u)
            AN_RULE(AN_S6('t', 'i', 'o', 'n', 'a', 'l'), 6u, AN_S4('t', 'i', 'o', 'n'), 4u, 0u)
            break;
        case 'c':
            AN_RULE(AN_S4('e', 'n', 'c', 'i'), 4u, AN_S4('e', 'n', 'c', 'e'), 4u, 0u)
            AN_RULE(AN_S4('a', 'n', 'c', 'i'), 4u, AN_S4('a', 'n', 'c', 'e'), 4u, 0u)
            break;
        case 'e':
            AN_RULE(AN_S4('i', 'z', 'e', 'r'), 4u, AN_S3('i', 'z', 'e'), 3u, 0u)
            break;
        case 'l':
            AN_RULE(AN_S4('a', 'b', 'l', 'i'), 4u, AN_S4('a', 'b', 'l', 'e'), 4u, 0u)
            AN_RULE(AN_S4('a', 'l', 'l', 'i'), 4u, AN_S2('a', 'l'), 2u, 0u)
            AN_RULE(AN_S5('e', 'n', 't', 'l', 'i'), 5u, AN_S3('e', 'n', 't'), 3u, 0u)
            AN_RULE(AN_S3('e', 'l', 'i'), 3u, AN_S1('e'), 1u, 0u)
            AN_RULE(AN_S5('o', 'u', 's', 'l', 'i'), 5u, AN_S3('o', 'u', 's'), 3u, 0u)
            break;
        case 'o':
            AN_RULE(AN_S7('i', 'z', 'a', 't', 'i', 'o', 'n'), 7u, AN_S3('i', 'z', 'e'), 3u, 0u)
            AN_RULE(AN_S5('a', 't', 'i', 'o', 'n'), 5u, AN_S3('a', 't', 'e'), 3u, 0u)
            AN_RULE(AN_S4('a', 't', 'o', 'r'), 4u, AN_S3('a', 't', 'e'), 3u, 0u)
            break;
        case 's':
            AN_RULE(AN_S5('a', 'l', 'i', 's', 'm'), 5u, AN_S2('a', 'l'), 2u, 0u)
            AN_RULE(AN_S7('i', 'v', 'e', 'n', 'e', 's', 's'), 7u, AN_S3('i', 'v', 'e'), 3u, 0u)
            AN_RULE(AN_S7('f', 'u', 'l', 'n', 'e', 's', 's'), 7u, AN_S3('f', 'u', 'l'), 3u, 0u)
            AN_RULE(AN_S7('o', 'u', 's', 'n', 'e', 's', 's'), 7u, AN_S3('o', 'u', 's'), 3u, 0u)
            break;
        case 't':
            AN_RULE(AN_S5('a', 'l', 'i', 't', 'i'), 5u, AN_S2('a', 'l'), 2u, 0u)
            AN_RULE(AN_S5('i', 'v', 'i', 't', 'i'), 5u, AN_S3('i', 'v', 'e'), 3u, 0u)
            AN_RULE(AN_S6('b', 'i', 'l', 'i', 't', 'i'), 6u, AN_S3('b', 'l', 'e'), 3u, 0u)
            break;
        default: break;
    }

    /* 3: by the last letter */
    switch ((uint32_t)(st.t >> 56)) {
        case 'e':
            AN_RULE(AN_S5('i', 'c', 'a', 't', 'e'), 5u, AN_S2('i', 'c'), 2u, 0u)
            AN_RULE(AN_S5('a', 't', 'i', 'v', 'e'), 5u, 0ull, 0u, 0u)
            AN_RULE(AN_S5('a', 'l', 'i', 'z', 'e'), 5u, AN_S2('a', 'l'), 2u, 0u)
            break;
        case 'i':
            AN_RULE(AN_S5('i', 'c', 'i', 't', 'i'), 5u, AN_S2('i', 'c'), 2u, 0u)
            break;
        case 'l':
            AN_RULE(AN_S4('i', 'c', 'a', 'l'), 4u, AN_S2('i', 'c'), 2u, 0u)
            AN_RULE(AN_S3('f', 'u', 'l'), 3u, 0ull, 0u, 0u)
            break;
        case 's':
            AN_RULE(AN_S4('n', 'e', 's', 's'), 4u, 0ull, 0u, 0u)
            break;
        default: break;
    }

    /* 4: by the penultimate letter */
    switch ((uint32_t)(st.t >> 48) & 0xFFu) {
        case 'a':
            AN_RULE(AN_S2('a', 'l'), 2u, 0ull, 0u, 1u)
            break;
        case 'c':
            AN_RULE(AN_S4('a', 'n', 'c', 'e'), 4u, 0ull, 0u, 1u)
            AN_RULE(AN_S4('e', 'n', 'c', 'e'), 4u, 0ull, 0u, 1u)
            break;
        case 'e':
            AN_RULE(AN_S2('e', 'r'), 2u, 0ull, 0u, 1u)
            break;
        case 'i':
            AN_RULE(AN_S2('i', 'c'), 2u, 0ull, 0u, 1u)
            break;
        case 'l':
            AN_RULE(AN_S4('a', 'b', 'l', 'e'), 4u, 0ull, 0u, 1u)
            AN_RULE(AN_S4('i', 'b', 'l', 'e'), 4u, 0ull, 0u, 1u)
            break;
        case 'n':
            AN_RULE(AN_S3('a', 'n', 't'), 3u, 0ull, 0u, 1u)
            AN_RULE(AN_S5('e', 'm', 'e', 'n', 't'), 5u, 0ull, 0u, 1u)
            AN_RULE(AN_S4('m', 'e', 'n', 't'), 4u, 0ull, 0u, 1u)
            AN_RULE(AN_S3('e', 'n', 't'), 3u, 0ull, 0u, 1u)
            break;
        case 'o':
            if (an_ends(&st, AN_S3('i', 'o', 'n'), 3u)) {
                const uint32_t c = (uint32_t)(st.t >> 32) & 0xFFu;   /* the letter in front of ion */
                if (st.len > 3u && (c == 's' || c == 't') && an_m(&st, st.len - 3u) > 1u) an_rep(&st, 3u, 0ull, 0u);
                break;
            }
            AN_RULE(AN_S2('o', 'u'), 2u, 0ull, 0u, 1u)
            break;
        case 's':
            AN_RULE(AN_S3('i', 's', 'm'), 3u, 0ull, 0u, 1u)
            break;
        case 't':
            AN_RULE(AN_S3('a', 't', 'e'), 3u, 0ull, 0u, 1u)
            AN_RULE(AN_S3('i', 't', 'i'), 3u, 0ull, 0u, 1u)
            break;
        case 'u':
            AN_RULE(AN_S3('o', 'u', 's'), 3u, 0ull, 0u, 1u)
            break;
        case 'v':
            AN_RULE(AN_S3('i', 'v', 'e'), 3u, 0ull, 0u, 1u)
            break;
        case 'z':
            AN_RULE(AN_S3('i', 'z', 'e'), 3u, 0ull, 0u, 1u)
            break;
        default: break;
    }

    /* 5a: *o of the letters in front of the e, whose last is t's second byte from the top */
    if (an_ends(&st, AN_S1('e'), 1u)) {
        const uint32_t m = an_m(&st, st.len - 1u);
        if (m > 1u || (m == 1u && !an_cvc(&st, st.t << 8, st.len - 1u))) an_rep(&st, 1u, 0ull, 0u);
    }
    /* 5b */
    if ((uint32_t)(st.t >> 56) == 'l' && an_double(&st, st.t, st.len) && an_m(&st, st.len) > 1u) an_rep(&st, 1u, 0ull, 0u);

    *tail = st.t;
    return st.len;
}

#undef AN_RULE

#endif
