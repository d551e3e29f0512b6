/*
 * weight_host.c — host-side pieces of the weighting schemes (include/tfidf.h, section
 * "weighting"): the parameter check every reweight call starts with, the scheme's tf and idf as
 * the tables of the device path tabulate them, the row norm, and the whole definition applied to
 * a fetched result.  Plain C, no device calls.  It serves a caller that already holds a fetched
 * result, is the second opinion on the device's pair pass (reweight.hip), and normalises the
 * merged rows of tfidf_group_transform.  The reference has the one formula of TFIDF.c:202,243-244.
 *
 * Every operation rounds on its own: no product may be fused into an add in this file.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

int tfidf_weighting_check(const tfidf_weighting* w) {
    if (!w || w->size < sizeof(tfidf_weighting)) return TFIDF_E_INVAL;
    if (w->tf > TFIDF_TF_BINARY || w->idf > TFIDF_IDF_NONE || w->norm > TFIDF_NORM_L1) return TFIDF_E_INVAL;
    if (w->reserved != 0u) return TFIDF_E_INVAL;
    if (w->tf == TFIDF_TF_RAW && w->norm == TFIDF_NORM_NONE) return TFIDF_E_INVAL;
    return TFIDF_OK;
}

/* the limit that needs N: sublinear tf without a norm stays inside the formatter's range only
 * below 2^48 documents */
int tfidf_weighting_check_n(const tfidf_weighting* w, uint64_t ndocs_total) {
    const int rc = tfidf_weighting_check(w);
    if (rc) return rc;
    if (w->tf == TFIDF_TF_LOG && w->norm == TFIDF_NORM_NONE && ndocs_total >= (1ull << 48)) return TFIDF_E_INVAL;
    return TFIDF_OK;
}

/* fl(1.0 + log((double)c)): the entry of the sublinear tf table for count c */
double tfidf_weight_tf_log(uint32_t c) {
    const double l = log((double)c);
    return 1.0 + l;
}

/* the scheme's idf for a term of `df` documents out of N (TFIDF_IDF_REF: TFIDF.c:243) */
double tfidf_weight_idf(uint32_t mode, uint64_t N, uint32_t df) {
    switch (mode) {
    case TFIDF_IDF_REF:
        return log(1.0 * (double)N / (double)df);
    case TFIDF_IDF_SMOOTH: {
        const double n1 = (double)N + 1.0, d1 = (double)df + 1.0;
        const double q = n1 / d1;
        const double l = log(q);
        return l + 1.0;
    }
    case TFIDF_IDF_PLUS1: {
        const double l = log(1.0 * (double)N / (double)df);
        return l + 1.0;
    }
    default:
        return 1.0;
    }
}

static double weight_tf(uint32_t mode, uint32_t c, uint32_t ds) {
    switch (mode) {
    case TFIDF_TF_RATIO: return (double)c / (double)ds;
    case TFIDF_TF_RAW: return (double)c;
    case TFIDF_TF_LOG: return tfidf_weight_tf_log(c);
    default: return 1.0;
    }
}

/* one row's norm in place: w[0..n) in pair order; returns 1 when the norm is 0 (the row stays) */
int tfidf_weight_normalize(double* w, uint64_t n, uint32_t norm) {
    if (norm == TFIDF_NORM_NONE) return 0;
    double sum = 0.0;
    for (uint64_t i = 0; i < n; ++i) {
        const double x = norm == TFIDF_NORM_L2 ? w[i] * w[i] : w[i];
        sum = sum + x;
    }
    const double d = norm == TFIDF_NORM_L2 ? sqrt(sum) : sum;
    if (d == 0.0) return 1;
    for (uint64_t i = 0; i < n; ++i) w[i] = w[i] / d;
    return 0;
}

int tfidf_result_reweight(tfidf_result* r, const tfidf_weighting* w) {
    if (!r || !w) return TFIDF_E_INVAL;
    if (tfidf_weighting_check_n(w, r->ndocs_total) != TFIDF_OK) return TFIDF_E_INVAL;
    const uint64_t P = r->npairs, N = r->ndocs_total;
    if (P == 0) return TFIDF_OK;
    if (!r->pair_doc || !r->pair_count || !r->pair_docsize || !r->pair_df || !r->pair_score) return TFIDF_E_INVAL;
    for (uint64_t p = 0; p < P; ++p)
        if (r->pair_count[p] == 0u || r->pair_docsize[p] == 0u || r->pair_df[p] == 0u || r->pair_df[p] > N)
            return TFIDF_E_INVAL;
    for (uint64_t p = 0; p < P; ++p) {
        const double tf = weight_tf(w->tf, r->pair_count[p], r->pair_docsize[p]);
        const double idf = tfidf_weight_idf(w->idf, N, r->pair_df[p]);
        r->pair_score[p] = tf * idf;
    }
    if (w->norm != TFIDF_NORM_NONE)
        for (uint64_t b = 0; b < P;) {
            uint64_t e = b + 1;
            while (e < P && r->pair_doc[e] == r->pair_doc[b]) ++e;
            (void)tfidf_weight_normalize(r->pair_score + b, e - b, w->norm);
            b = e;
        }
    return TFIDF_OK;
}
