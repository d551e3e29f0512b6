/*
 * weight_host_test.c — tfidf_weighting_check and tfidf_result_reweight (csrc/weight_host.c) on
 * edge inputs, as a stand-alone program: built with -fsanitize=address,undefined by
 * tests/test_weight_native.py, so every read and write of the host functions is checked.  The
 * results live in exact-size heap blocks: a read past an array is a report.  The expected values
 * are computed here by the definition of include/tfidf.h, one operation per statement.  Exit
 * status 0: every case passed.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"

static int g_fail = 0;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
            ++g_fail;                                                       \
        }                                                                   \
    } while (0)

static tfidf_weighting make(uint32_t tf, uint32_t idf, uint32_t norm) {
    tfidf_weighting w;
    memset(&w, 0, sizeof(w));
    w.size = sizeof(w);
    w.tf = tf;
    w.idf = idf;
    w.norm = norm;
    return w;
}

static uint64_t bits(double x) {
    uint64_t u;
    memcpy(&u, &x, 8);
    return u;
}

/* a result of n pairs in exact-size blocks */
static tfidf_result build(uint64_t n, uint64_t N, const uint32_t* doc, const uint32_t* cnt, const uint32_t* ds,
                          const uint32_t* df) {
    tfidf_result r;
    memset(&r, 0, sizeof(r));
    r.npairs = n;
    r.ndocs_total = N;
    if (!n) return r;
    r.pair_doc = (uint32_t*)malloc((size_t)n * 4);
    r.pair_count = (uint32_t*)malloc((size_t)n * 4);
    r.pair_docsize = (uint32_t*)malloc((size_t)n * 4);
    r.pair_df = (uint32_t*)malloc((size_t)n * 4);
    r.pair_score = (double*)malloc((size_t)n * 8);
    memcpy(r.pair_doc, doc, (size_t)n * 4);
    memcpy(r.pair_count, cnt, (size_t)n * 4);
    memcpy(r.pair_docsize, ds, (size_t)n * 4);
    memcpy(r.pair_df, df, (size_t)n * 4);
    for (uint64_t i = 0; i < n; ++i) r.pair_score[i] = -1.0;
    return r;
}

static void drop(tfidf_result* r) {
    free(r->pair_doc);
    free(r->pair_count);
    free(r->pair_docsize);
    free(r->pair_df);
    free(r->pair_score);
    memset(r, 0, sizeof(*r));
}

static double want_tf(uint32_t mode, uint32_t c, uint32_t ds) {
    if (mode == TFIDF_TF_RATIO) return (double)c / (double)ds;
    if (mode == TFIDF_TF_RAW) return (double)c;
    if (mode == TFIDF_TF_LOG) {
        volatile double l = log((double)c);
        return 1.0 + l;
    }
    return 1.0;
}

static double want_idf(uint32_t mode, uint64_t N, uint32_t df) {
    if (mode == TFIDF_IDF_REF) return log(1.0 * (double)N / (double)df);
    if (mode == TFIDF_IDF_SMOOTH) {
        volatile double a = (double)N + 1.0, b = (double)df + 1.0;
        volatile double q = a / b;
        volatile double l = log(q);
        return l + 1.0;
    }
    if (mode == TFIDF_IDF_PLUS1) {
        volatile double l = log(1.0 * (double)N / (double)df);
        return l + 1.0;
    }
    return 1.0;
}

/* every valid scheme on r against the definition; the integers must stay */
static void check_all(const tfidf_result* src, const char* what) {
    const uint64_t n = src->npairs;
    for (uint32_t tf = 0; tf < 4; ++tf)
        for (uint32_t idf = 0; idf < 4; ++idf)
            for (uint32_t norm = 0; norm < 3; ++norm) {
                tfidf_weighting w = make(tf, idf, norm);
                tfidf_result r = build(n, src->ndocs_total, src->pair_doc, src->pair_count, src->pair_docsize, src->pair_df);
                const int rc = tfidf_result_reweight(&r, &w);
                const int refused = (tf == TFIDF_TF_RAW && norm == TFIDF_NORM_NONE) ||
                                    (tf == TFIDF_TF_LOG && norm == TFIDF_NORM_NONE && src->ndocs_total >= (1ull << 48));
                if (refused) {
                    CHECK(rc == TFIDF_E_INVAL);
                    for (uint64_t i = 0; i < n; ++i) CHECK(r.pair_score[i] == -1.0);
                    drop(&r);
                    continue;
                }
                if (rc != TFIDF_OK) {
                    printf("FAIL %s: scheme %u %u %u returned %d\n", what, tf, idf, norm, rc);
                    ++g_fail;
                    drop(&r);
                    continue;
                }
                for (uint64_t b = 0; b < n;) {
                    uint64_t e = b + 1;
                    while (e < n && src->pair_doc[e] == src->pair_doc[b]) ++e;
                    volatile double sum = 0.0;
                    for (uint64_t i = b; i < e; ++i) {
                        volatile double x = want_tf(tf, src->pair_count[i], src->pair_docsize[i]) *
                                            want_idf(idf, src->ndocs_total, src->pair_df[i]);
                        volatile double t = norm == TFIDF_NORM_L2 ? x * x : x;
                        sum = sum + t;
                    }
                    const double d = norm == TFIDF_NORM_L2 ? sqrt(sum) : sum;
                    for (uint64_t i = b; i < e; ++i) {
                        volatile double x = want_tf(tf, src->pair_count[i], src->pair_docsize[i]) *
                                            want_idf(idf, src->ndocs_total, src->pair_df[i]);
                        const double s = (norm == TFIDF_NORM_NONE || d == 0.0) ? x : x / d;
                        if (bits(r.pair_score[i]) != bits(s)) {
                            printf("FAIL %s: scheme %u %u %u pair %llu: %.17g, expected %.17g\n", what, tf, idf, norm,
                                   (unsigned long long)i, r.pair_score[i], s);
                            ++g_fail;
                        }
                        CHECK(r.pair_score[i] >= 0.0 && r.pair_score[i] < 922.0);
                    }
                    b = e;
                }
                if (n) {
                    CHECK(memcmp(r.pair_count, src->pair_count, (size_t)n * 4) == 0);
                    CHECK(memcmp(r.pair_df, src->pair_df, (size_t)n * 4) == 0);
                }
                drop(&r);
            }
}

int main(void) {
    /* tfidf_weighting_check */
    {
        tfidf_weighting w = make(TFIDF_TF_LOG, TFIDF_IDF_SMOOTH, TFIDF_NORM_L2);
        CHECK(tfidf_weighting_check(&w) == TFIDF_OK);
        CHECK(tfidf_weighting_check(NULL) == TFIDF_E_INVAL);
        w.size = sizeof(w) - 1;
        CHECK(tfidf_weighting_check(&w) == TFIDF_E_INVAL);
        w = make(4, 0, 0);
        CHECK(tfidf_weighting_check(&w) == TFIDF_E_INVAL);
        w = make(0, 4, 0);
        CHECK(tfidf_weighting_check(&w) == TFIDF_E_INVAL);
        w = make(0, 0, 3);
        CHECK(tfidf_weighting_check(&w) == TFIDF_E_INVAL);
        w = make(0, 0, 0);
        w.reserved = 1;
        CHECK(tfidf_weighting_check(&w) == TFIDF_E_INVAL);
        w = make(TFIDF_TF_RAW, TFIDF_IDF_NONE, TFIDF_NORM_NONE);
        CHECK(tfidf_weighting_check(&w) == TFIDF_E_INVAL);
        w = make(TFIDF_TF_RAW, TFIDF_IDF_NONE, TFIDF_NORM_L1);
        CHECK(tfidf_weighting_check(&w) == TFIDF_OK);
        w = make(TFIDF_TF_LOG, TFIDF_IDF_REF, TFIDF_NORM_NONE);   /* the limit that needs N is not this function's */
        CHECK(tfidf_weighting_check(&w) == TFIDF_OK);
    }
    /* NULL arguments; an empty result with no arrays */
    {
        tfidf_weighting w = make(TFIDF_TF_LOG, TFIDF_IDF_SMOOTH, TFIDF_NORM_L2);
        tfidf_result r = build(0, 5, NULL, NULL, NULL, NULL);
        CHECK(tfidf_result_reweight(NULL, &w) == TFIDF_E_INVAL);
        CHECK(tfidf_result_reweight(&r, NULL) == TFIDF_E_INVAL);
        CHECK(tfidf_result_reweight(&r, &w) == TFIDF_OK);
        check_all(&r, "empty");
    }
    /* one pair; N = 1 (df = N: every reference idf is +0.0) */
    {
        const uint32_t doc[] = {1}, cnt[] = {3}, ds[] = {3}, df[] = {1};
        tfidf_result r = build(1, 1, doc, cnt, ds, df);
        check_all(&r, "one pair, N = 1");
        tfidf_weighting w = make(TFIDF_TF_RATIO, TFIDF_IDF_REF, TFIDF_NORM_L2);
        CHECK(tfidf_result_reweight(&r, &w) == TFIDF_OK);
        CHECK(bits(r.pair_score[0]) == bits(0.0));   /* a zero norm: the score stays w = +0.0 */
        drop(&r);
    }
    /* a document of only df = N pairs between two ordinary ones, under each norm */
    {
        const uint32_t doc[] = {1, 1, 2, 2, 2, 3}, cnt[] = {1, 2, 1, 1, 5, 7}, ds[] = {3, 3, 7, 7, 7, 7};
        const uint32_t df[] = {1, 3, 3, 3, 3, 2};
        tfidf_result r = build(6, 3, doc, cnt, ds, df);
        check_all(&r, "df = N document");
        for (uint32_t norm = 1; norm < 3; ++norm) {
            tfidf_weighting w = make(TFIDF_TF_RATIO, TFIDF_IDF_REF, norm);
            CHECK(tfidf_result_reweight(&r, &w) == TFIDF_OK);
            for (int i = 2; i < 5; ++i) CHECK(bits(r.pair_score[i]) == bits(0.0));
            CHECK(r.pair_score[0] > 0.0 && r.pair_score[5] == 1.0);
        }
        drop(&r);
    }
    /* counts of 1 and 2^32 - 1 */
    {
        const uint32_t doc[] = {9, 9}, cnt[] = {1, 0xFFFFFFFFu}, ds[] = {0xFFFFFFFFu, 0xFFFFFFFFu}, df[] = {1, 2};
        tfidf_result r = build(2, 0xFFFFFFFFull, doc, cnt, ds, df);
        check_all(&r, "count limits");
        drop(&r);
    }
    /* N = 2^48: sublinear tf without a norm is refused, everything else is computed */
    {
        const uint32_t doc[] = {1, 2}, cnt[] = {0xFFFFFFFFu, 2}, ds[] = {0xFFFFFFFFu, 2}, df[] = {1, 0xFFFFFFFFu};
        tfidf_result r = build(2, 1ull << 48, doc, cnt, ds, df);
        check_all(&r, "N = 2^48");
        r.ndocs_total = (1ull << 48) - 1;
        tfidf_weighting w = make(TFIDF_TF_LOG, TFIDF_IDF_PLUS1, TFIDF_NORM_NONE);
        CHECK(tfidf_result_reweight(&r, &w) == TFIDF_OK);
        CHECK(r.pair_score[0] > 700.0 && r.pair_score[0] < 922.0);
        drop(&r);
    }
    /* invalid integers leave the scores */
    {
        const uint32_t doc[] = {1, 1}, cnt[] = {1, 0}, ds[] = {2, 2}, df[] = {1, 1};
        tfidf_result r = build(2, 2, doc, cnt, ds, df);
        tfidf_weighting w = make(TFIDF_TF_RATIO, TFIDF_IDF_REF, TFIDF_NORM_NONE);
        CHECK(tfidf_result_reweight(&r, &w) == TFIDF_E_INVAL);
        CHECK(r.pair_score[0] == -1.0 && r.pair_score[1] == -1.0);
        r.pair_count[1] = 1;
        r.pair_df[0] = 3;   /* df > N */
        CHECK(tfidf_result_reweight(&r, &w) == TFIDF_E_INVAL);
        drop(&r);
    }
    if (g_fail) {
        printf("%d failures\n", g_fail);
        return 1;
    }
    printf("ok\n");
    return 0;
}
