/*
 * ngram_host_test.c — tfidf_ngrams_host and tfidf_ngram_check (csrc/ngram_host.c) on edge
 * inputs, as a stand-alone program: built with -fsanitize=address,undefined by
 * tests/test_ngram_native.py, so every read and write of the host function is checked.  Inputs
 * live in exact-size heap blocks: a read past a window is a report.  Links only ngram_host.c
 * (tfidf_free is free).  Exit status 0: every case passed.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"

static int g_fail = 0;

static tfidf_ngram_params make(uint32_t min_n, uint32_t max_n, uint8_t joiner) {
    tfidf_ngram_params p;
    memset(&p, 0, sizeof(p));
    p.size = sizeof(p);
    p.min_n = min_n;
    p.max_n = max_n;
    p.joiner = joiner;
    return p;
}

static void expect(const char* name, uint32_t min_n, uint32_t max_n, uint8_t joiner, const char* in, size_t n, const uint64_t* off,
                   uint32_t nd, const char* want, const uint64_t* want_off) {
    uint8_t* src = (uint8_t*)malloc(n ? n : 1);
    uint64_t* o = (uint64_t*)malloc(((size_t)nd + 1) * sizeof(uint64_t));
    memcpy(src, in, n);
    memcpy(o, off, ((size_t)nd + 1) * sizeof(uint64_t));
    tfidf_ngram_params p = make(min_n, max_n, joiner);
    uint8_t* ob = NULL;
    uint64_t on = 99, *oo = NULL;
    const int rc = tfidf_ngrams_host(&p, n ? src : NULL, n, nd ? o : NULL, nd, &ob, &on, &oo);
    int ok = rc == 0 && ob && oo && on == strlen(want) && memcmp(ob, want, on) == 0;
    for (uint32_t d = 0; ok && d <= nd; ++d) ok = oo[d] == want_off[d];
    if (!ok) { printf("FAIL %s (rc %d, %llu bytes)\n", name, rc, (unsigned long long)on); ++g_fail; }
    free(ob); free(oo); free(src); free(o);
}

static void expect_inval(const char* name, const tfidf_ngram_params* p, const uint8_t* b, uint64_t n, const uint64_t* off, uint32_t nd) {
    uint8_t* ob = (uint8_t*)1;
    uint64_t on = 99, *oo = (uint64_t*)1;
    const int rc = tfidf_ngrams_host(p, b, n, off, nd, &ob, &on, &oo);
    if (rc != TFIDF_E_INVAL || ob || on || oo) { printf("FAIL inval %s\n", name); ++g_fail; }
}

int main(void) {
    {   /* the header's two examples */
        const char in[] = "XXnew  york\ncityrunning onYY";
        const uint64_t off[] = {2, 16, 20, 26}, w12[] = {0, 33, 38, 52}, w23[] = {0, 33, 33, 40};
        expect("literal 1-2", 1, 2, 0, in, sizeof(in) - 1, off, 3, "new new_york york york_city city runn ing ing_on on ", w12);
        expect("literal 2-3", 2, 3, 0, in, sizeof(in) - 1, off, 3, "new_york new_york_city york_city ing_on ", w23);
        expect("joiner", 2, 3, '+', in, sizeof(in) - 1, off, 3, "new+york new+york+city york+city ing+on ", w23);
    }
    {   /* nothing at all, documents without bytes, bytes without documents */
        const uint64_t z[] = {0, 0, 0, 0}, w[] = {0, 0, 0, 0}, o3[] = {3}, o33[] = {3, 3};
        expect("no bytes, no documents", 1, 2, 0, "", 0, z, 0, "", w);
        expect("no bytes, three documents", 1, 2, 0, "", 0, z, 3, "", w);
        expect("bytes, no documents", 1, 2, 0, "a b c", 5, o3, 0, "", w);
        expect("an empty window", 1, 2, 0, "a b c", 5, o33, 1, "", w);
    }
    {   /* tokens that touch the window's and the buffer's edges; separators only; every separator */
        const uint64_t o[] = {0, 5}, w1[] = {0, 6}, w0[] = {0, 0}, o2[] = {1, 4}, w2[] = {0, 4};
        expect("whole buffer one token", 1, 8, 0, "abcde", 5, o, 1, "abcde ", w1);
        expect("fewer tokens than min_n", 2, 8, 0, "abcde", 5, o, 1, "", w0);
        expect("window inside a token", 1, 1, 0, "abcde", 5, o2, 1, "bcd ", w2);
        expect("separators only", 1, 3, 0, " \t\n\v\f\r", 6, (const uint64_t[]){0, 6}, 1, "", w0);
        expect("every separator", 2, 2, 0, "a\tb\nc\vd\fe\rf g", 13, (const uint64_t[]){0, 13}, 1, "a_b b_c c_d d_e e_f f_g ", (const uint64_t[]){0, 24});
        expect("leading and trailing blanks", 1, 2, 0, "  a  b  ", 8, (const uint64_t[]){0, 8}, 1, "a a_b b ", (const uint64_t[]){0, 8});
        expect("one-byte documents", 1, 2, 0, "ab c", 4, (const uint64_t[]){0, 1, 2, 3, 4}, 4, "a b c ", (const uint64_t[]){0, 2, 4, 4, 6});
        expect("max_n = 8 on 9 tokens", 8, 8, 0, "1 2 3 4 5 6 7 8 9", 17, (const uint64_t[]){0, 17}, 1, "1_2_3_4_5_6_7_8 2_3_4_5_6_7_8_9 ",
               (const uint64_t[]){0, 32});
        expect("7-8 on 8 tokens", 7, 8, 0, "1 2 3 4 5 6 7 8", 15, (const uint64_t[]){0, 15}, 1, "1_2_3_4_5_6_7 1_2_3_4_5_6_7_8 2_3_4_5_6_7_8 ",
               (const uint64_t[]){0, 44});
    }
    {   /* NUL and high bytes are copied verbatim */
        const char in[] = {'a', 0, 'b', ' ', (char)0xC3, (char)0xA9, ' ', 'c'};
        const char want[] = {'a', 0, 'b', '_', (char)0xC3, (char)0xA9, ' ', (char)0xC3, (char)0xA9, '_', 'c', ' ', 0};
        uint8_t* src = (uint8_t*)malloc(sizeof(in));
        memcpy(src, in, sizeof(in));
        const uint64_t off[] = {0, sizeof(in)};
        tfidf_ngram_params p = make(2, 2, 0);
        uint8_t* ob = NULL;
        uint64_t on = 0, *oo = NULL;
        const int rc = tfidf_ngrams_host(&p, src, sizeof(in), off, 1, &ob, &on, &oo);
        if (rc || on != 12 || memcmp(ob, want, 12) || oo[1] != 12) { printf("FAIL NUL and high bytes\n"); ++g_fail; }
        free(ob); free(oo); free(src);
    }
    {   /* a long document: the ring of token bounds wraps many times */
        const size_t ntok = 5000;
        uint8_t* src = (uint8_t*)malloc(ntok * 2);
        for (size_t i = 0; i < ntok; ++i) { src[2 * i] = (uint8_t)('a' + i % 26); src[2 * i + 1] = ' '; }
        const uint64_t off[] = {0, ntok * 2 - 1};   /* the last blank is outside */
        for (uint32_t lo = 1; lo <= 8; ++lo)
            for (uint32_t hi = lo; hi <= 8; ++hi) {
                tfidf_ngram_params p = make(lo, hi, 0);
                uint8_t* ob = NULL;
                uint64_t on = 0, *oo = NULL, want = 0;
                for (uint32_t n = lo; n <= hi; ++n) want += (ntok - n + 1) * 2 * n;
                const int rc = tfidf_ngrams_host(&p, src, ntok * 2 - 1, off, 1, &ob, &on, &oo);
                int ok = rc == 0 && on == want && oo[0] == 0 && oo[1] == want;
                /* the first position's grams: a b .. */
                uint64_t at = 0;
                for (uint32_t n = lo; ok && n <= hi; ++n)
                    for (uint32_t k = 0; ok && k < n; ++k, at += 2)
                        ok = ob[at] == 'a' + k && ob[at + 1] == (k + 1 < n ? '_' : ' ');
                if (!ok) { printf("FAIL long document %u-%u\n", lo, hi); ++g_fail; }
                free(ob); free(oo);
            }
        free(src);
    }
    {   /* the check and the error rules */
        tfidf_ngram_params p = make(1, 2, 0);
        const uint8_t b[] = "a b c";
        const uint64_t off[] = {0, 5}, down[] = {0, 4, 3}, past[] = {0, 6};
        if (tfidf_ngram_check(&p) != TFIDF_OK) { printf("FAIL check ok\n"); ++g_fail; }
        if (tfidf_ngram_check(NULL) != TFIDF_E_INVAL) { printf("FAIL check NULL\n"); ++g_fail; }
        tfidf_ngram_params q = p;
        q.size = sizeof(q) - 1;
        expect_inval("short size", &q, b, 5, off, 1);
        q = make(0, 2, 0); expect_inval("min_n 0", &q, b, 5, off, 1);
        q = make(3, 2, 0); expect_inval("max_n < min_n", &q, b, 5, off, 1);
        q = make(1, TFIDF_NGRAM_MAX_N + 1, 0); expect_inval("max_n 9", &q, b, 5, off, 1);
        const uint8_t seps[] = {0x20, 0x09, 0x0A, 0x0B, 0x0C, 0x0D};
        for (int i = 0; i < 6; ++i) { q = make(1, 2, seps[i]); expect_inval("separator joiner", &q, b, 5, off, 1); }
        for (int i = 0; i < 7; ++i) { q = make(1, 2, 0); q.reserved[i] = 1; expect_inval("reserved", &q, b, 5, off, 1); }
        expect_inval("NULL params", NULL, b, 5, off, 1);
        expect_inval("NULL bytes", &p, NULL, 5, off, 1);
        expect_inval("NULL off", &p, b, 5, NULL, 1);
        expect_inval("non-monotone off", &p, b, 5, down, 2);
        expect_inval("off past nbytes", &p, b, 5, past, 1);
        uint8_t* ob = NULL;
        uint64_t on = 0, *oo = NULL;
        if (tfidf_ngrams_host(&p, b, 5, off, 1, NULL, &on, &oo) != TFIDF_E_INVAL || tfidf_ngrams_host(&p, b, 5, off, 1, &ob, NULL, &oo) != TFIDF_E_INVAL ||
            tfidf_ngrams_host(&p, b, 5, off, 1, &ob, &on, NULL) != TFIDF_E_INVAL) {
            printf("FAIL NULL outputs\n");
            ++g_fail;
        }
    }
    if (g_fail) { printf("%d failed\n", g_fail); return 1; }
    printf("ok\n");
    return 0;
}
