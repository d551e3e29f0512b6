/*
 * analyze_host_test.c — tfidf_analyze_host and tfidf_analyzer_check (csrc/analyze_host.c) on
 * edge inputs, as a stand-alone program: built with -fsanitize=address,undefined by
 * tests/test_analyze_native.py, so every read and write of the host function, its table build
 * and its probes is checked.  Links only analyze_host.c.  Exit status 0: every case passed.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"

static int g_fail = 0;

static tfidf_analyzer make(uint32_t flags, uint32_t min_len, const char** stop, uint32_t nstop, uint8_t** sb, uint64_t** so) {
    tfidf_analyzer a;
    memset(&a, 0, sizeof(a));
    a.size = sizeof(a);
    a.flags = flags;
    a.min_len = min_len;
    size_t total = 0;
    for (uint32_t i = 0; i < nstop; ++i) total += strlen(stop[i]);
    *sb = (uint8_t*)malloc(total ? total : 1);          /* exact sizes: a read past the list is a report */
    *so = (uint64_t*)malloc(((size_t)nstop + 1) * sizeof(uint64_t));
    (*so)[0] = 0;
    for (uint32_t i = 0; i < nstop; ++i) {
        memcpy(*sb + (*so)[i], stop[i], strlen(stop[i]));
        (*so)[i + 1] = (*so)[i] + strlen(stop[i]);
    }
    a.stop_bytes = nstop ? *sb : NULL;
    a.stop_off = nstop ? *so : NULL;
    a.nstop = nstop;
    return a;
}

/* analyzes `in` (n bytes, documents at off) out of place and in place, both in exact-size heap
 * blocks, twice (idempotence), and compares with `want` */
static void expect(const char* name, uint32_t flags, uint32_t min_len, const char** stop, uint32_t nstop, const char* in,
                   size_t n, const uint64_t* off, uint32_t nd, const char* want) {
    uint8_t *sb, *src = (uint8_t*)malloc(n ? n : 1), *out = (uint8_t*)malloc(n ? n : 1);
    uint64_t* so;
    tfidf_analyzer a = make(flags, min_len, stop, nstop, &sb, &so);
    memcpy(src, in, n);
    int rc = tfidf_analyze_host(&a, src, n, off, nd, out);
    int ok = rc == 0 && memcmp(out, want, n) == 0;
    rc = tfidf_analyze_host(&a, src, n, off, nd, src);              /* in place */
    ok = ok && rc == 0 && memcmp(src, want, n) == 0;
    rc = tfidf_analyze_host(&a, out, n, off, nd, out);              /* a second application */
    ok = ok && rc == 0 && memcmp(out, want, n) == 0;
    if (!ok) { printf("FAIL %s\n", name); ++g_fail; }
    free(sb); free(so); free(src); free(out);
}

static void expect_check(const char* name, const tfidf_analyzer* a, int want) {
    if (tfidf_analyzer_check(a) != want) { printf("FAIL check %s\n", name); ++g_fail; }
}

int main(void) {
    const uint32_t L = TFIDF_AN_LOWER, P = TFIDF_AN_PUNCT;
    {   /* the byte map on every byte value */
        char in[256], want[256];
        for (int c = 0; c < 256; ++c) {
            in[c] = (char)c;
            int m = c;
            const int sep = c == 0x20 || (c >= 0x09 && c <= 0x0D);
            const int alnum = (c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z');
            if (c < 0x80 && !sep && !alnum) m = 0x20;
            if (c >= 'A' && c <= 'Z') m = c + 0x20;
            want[c] = (char)m;
        }
        const uint64_t off[2] = {0, 256};
        expect("byte map", L | P, 0, NULL, 0, in, 256, off, 1, want);
        expect("identity", 0, 1, NULL, 0, in, 256, off, 1, in);
    }
    {   /* a document boundary cuts a token; windows keep their bytes */
        const char* s1[] = {"abcd"};
        const char* s2[] = {"ab"};
        const uint64_t off[3] = {0, 4, 8};
        expect("cut, whole word listed", P, 0, s1, 1, "..abcd..", 8, off, 2, "  abcd  ");
        expect("cut, half listed", P, 0, s2, 1, "..abcd..", 8, off, 2, "    cd  ");
        const uint64_t win[2] = {3, 9};
        expect("window", L | P, 2, s2, 1, "AB,AB ab a,AB", 13, win, 1, "AB,      a,AB");
        const uint64_t none[1] = {5};
        expect("no documents", L | P, 2, s2, 1, "AB ab", 5, none, 0, "AB ab");
        expect("no bytes", L | P, 2, s2, 1, "", 0, none, 0, "");
        const uint64_t empty[4] = {2, 2, 2, 2};
        expect("empty documents", L | P, 2, s2, 1, "AB ab", 5, empty, 3, "AB ab");
    }
    {   /* stop words of 1, 15, 16, 63 and 64 bytes; a 65-byte token with a listed prefix; a NUL */
        static const uint32_t lens[5] = {1, 15, 16, 63, 64};
        for (int t = 0; t < 5; ++t) {
            const uint32_t n = lens[t];
            char w[65], in[200], want[200];
            for (uint32_t i = 0; i < n; ++i) w[i] = (char)('a' + (i * 7) % 26);
            w[n] = 0;
            const char* stop[] = {w, "zz", w};           /* a duplicate */
            size_t len = 0;
            memcpy(in + len, w, n); memset(want + len, 0x20, n); len += n;
            in[len] = ' '; want[len] = ' '; ++len;
            memcpy(in + len, w, n); memcpy(want + len, w, n); len += n;   /* w + "k": not listed */
            in[len] = 'k'; want[len] = 'k'; ++len;
            in[len] = '\n'; want[len] = '\n'; ++len;
            memcpy(in + len, w, n); memset(want + len, 0x20, n); len += n;
            const uint64_t off[2] = {0, len};
            expect("stop word length", 0, 0, stop, 3, in, len, off, 1, want);
        }
        const char* s3[] = {"ab"};
        const uint64_t off[2] = {0, 7};
        expect("a token with a NUL never matches", 0, 0, s3, 1, "ab\0 ab\0", 7, off, 1, "ab\0 ab\0");
        expect("with PUNCT the NUL is a blank", P, 0, s3, 1, "ab\0 ab\0", 7, off, 1, "       ");
        expect("min_len 64", 0, 64, NULL, 0, "ab\0 abc", 7, off, 1, "       ");
    }
    {   /* the maximal list: 4096 words, 32768 bytes */
        uint8_t* sb = (uint8_t*)malloc(TFIDF_AN_MAX_STOP_BYTES);
        uint64_t* so = (uint64_t*)malloc((TFIDF_AN_MAX_STOP + 1) * sizeof(uint64_t));
        for (uint32_t i = 0; i <= TFIDF_AN_MAX_STOP; ++i) so[i] = 8ull * i;
        for (uint32_t i = 0; i < TFIDF_AN_MAX_STOP; ++i) {
            char w[9];
            snprintf(w, sizeof(w), "%08u", i);
            memcpy(sb + 8 * i, w, 8);
        }
        tfidf_analyzer a;
        memset(&a, 0, sizeof(a));
        a.size = sizeof(a);
        a.stop_bytes = sb;
        a.stop_off = so;
        a.nstop = TFIDF_AN_MAX_STOP;
        expect_check("maximal list", &a, TFIDF_OK);
        const char in[] = "00000000 00004095 00004096 0000409";
        const char want[] = "                  00004096 0000409";
        uint8_t* out = (uint8_t*)malloc(sizeof(in) - 1);
        const uint64_t off[2] = {0, sizeof(in) - 1};
        if (tfidf_analyze_host(&a, (const uint8_t*)in, sizeof(in) - 1, off, 1, out) != 0 || memcmp(out, want, sizeof(in) - 1) != 0) {
            printf("FAIL maximal list lookup\n");
            ++g_fail;
        }
        free(out);
        a.nstop = TFIDF_AN_MAX_STOP + 1;
        expect_check("too many words", &a, TFIDF_E_INVAL);
        a.nstop = 2;
        so[1] = 9; so[2] = 8;
        expect_check("non-monotone offsets", &a, TFIDF_E_INVAL);
        so[1] = 0;
        expect_check("an empty word", &a, TFIDF_E_INVAL);
        so[1] = 8; so[2] = 8 + 65;
        expect_check("a word of 65 bytes", &a, TFIDF_E_INVAL);
        so[2] = 16;
        sb[3] = 0;
        expect_check("a NUL", &a, TFIDF_E_INVAL);
        sb[3] = '\t';
        expect_check("a separator", &a, TFIDF_E_INVAL);
        sb[3] = '0';
        a.flags = 4;
        expect_check("an unknown flag", &a, TFIDF_E_INVAL);
        a.flags = 0;
        a.min_len = 65;
        expect_check("min_len 65", &a, TFIDF_E_INVAL);
        a.min_len = 0;
        a.size = sizeof(a) - 1;
        expect_check("a short struct", &a, TFIDF_E_INVAL);
        a.size = sizeof(a);
        a.stop_bytes = NULL;
        expect_check("a NULL list", &a, TFIDF_E_INVAL);
        expect_check("NULL", NULL, TFIDF_E_INVAL);
        free(sb); free(so);
    }
    printf("%s\n", g_fail ? "failed" : "ok");
    return g_fail ? 1 : 0;
}
