/*
 * prune_host.c — host-side pieces of vocabulary pruning (include/tfidf.h, section "prune"): the
 * parameter check every prune call starts with, and the definition applied to a model struct,
 * for which the df and the term order are all it needs.  Plain C, no device calls.  It prunes a
 * saved model with no GPU and is the second opinion on the device's term selection
 * (prune.hip).  The reference keeps every word (TFIDF.c:152-188).
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"

int tfidf_prune_check(const tfidf_prune_params* p) {
    if (!p || p->size < sizeof(tfidf_prune_params)) return TFIDF_E_INVAL;
    if (p->reserved != 0u) return TFIDF_E_INVAL;
    if (p->max_df != 0u && p->min_df > p->max_df) return TFIDF_E_INVAL;
    return TFIDF_OK;
}

/* df descending, then term rank ascending: a total order, so qsort's instability does not show */
typedef struct { uint32_t df, rank; } cand;
static int cand_cmp(const void* a, const void* b) {
    const cand* x = (const cand*)a;
    const cand* y = (const cand*)b;
    if (x->df != y->df) return x->df > y->df ? -1 : 1;
    return x->rank < y->rank ? -1 : (x->rank > y->rank ? 1 : 0);
}

int tfidf_model_prune(const tfidf_model* in, const tfidf_prune_params* p, tfidf_model* out) {
    if (!out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!in || tfidf_prune_check(p) != TFIDF_OK || tfidf_model_check(in) != TFIDF_OK) return TFIDF_E_INVAL;
    const uint64_t V = in->nterms;
    uint8_t* keep = (uint8_t*)calloc((size_t)V + 1, 1);
    if (!keep) return TFIDF_E_NOMEM;
    uint64_t S = 0;
    for (uint64_t t = 0; t < V; ++t) {
        const uint32_t df = in->term_df[t];
        keep[t] = (p->min_df <= 1u || df >= p->min_df) && (p->max_df == 0u || df <= p->max_df);
        S += keep[t];
    }
    if (p->max_features != 0u && S > p->max_features) {
        cand* c = (cand*)malloc((size_t)S * sizeof(cand));
        if (!c) { free(keep); return TFIDF_E_NOMEM; }
        uint64_t n = 0;
        for (uint64_t t = 0; t < V; ++t)
            if (keep[t]) { c[n].df = in->term_df[t]; c[n].rank = (uint32_t)t; ++n; }
        qsort(c, (size_t)S, sizeof(cand), cand_cmp);
        for (uint64_t i = p->max_features; i < S; ++i) keep[c[i].rank] = 0;
        free(c);
        S = p->max_features;
    }
    uint64_t nbytes = 0;
    for (uint64_t t = 0; t < V; ++t)
        if (keep[t]) nbytes += in->term_off[t + 1] - in->term_off[t];
    out->size = sizeof(tfidf_model);
    out->ndocs_total = in->ndocs_total;
    out->nterms = (uint32_t)S;
    out->term_off = (uint64_t*)malloc((size_t)(S + 1) * 8);
    out->term_df = (uint32_t*)malloc((size_t)S * 4 + 4);
    out->term_bytes = (uint8_t*)malloc((size_t)nbytes + 1);
    if (!out->term_off || !out->term_df || !out->term_bytes) {
        free(keep);
        tfidf_model_free(out);
        return TFIDF_E_NOMEM;
    }
    uint64_t k = 0, at = 0;
    for (uint64_t t = 0; t < V; ++t) {
        if (!keep[t]) continue;
        const uint64_t len = in->term_off[t + 1] - in->term_off[t];
        out->term_off[k] = at;
        out->term_df[k] = in->term_df[t];
        if (len) memcpy(out->term_bytes + at, in->term_bytes + in->term_off[t], (size_t)len);
        at += len;
        ++k;
    }
    out->term_off[k] = at;
    free(keep);
    return TFIDF_OK;
}
