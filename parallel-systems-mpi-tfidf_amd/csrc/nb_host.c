/*
 * nb_host.c — host-side pieces of Naive Bayes classification (include/tfidf.h, section
 * "classify"): the parameter check every call starts with, the fit on a fetched result and the
 * prediction of rows against a model on the host.  Plain C, no device calls: the second opinion
 * on nb.hip, and the helpers engine_nb.cpp shares (nb_alpha, nb_prior, the frees).  Every formula
 * is evaluated one operation at a time (built with -ffp-contract=off).  The reference has no
 * such pass.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"

static int nb_u32_cmp(const void* a, const void* b) {
    const uint32_t x = *(const uint32_t*)a, y = *(const uint32_t*)b;
    return x < y ? -1 : (x > y ? 1 : 0);
}

int tfidf_nb_check(const tfidf_nb_params* p) {
    if (!p || p->size < sizeof(tfidf_nb_params)) return TFIDF_E_INVAL;
    if (p->nclasses == 0u || p->nclasses > TFIDF_NB_MAX_CLASSES) return TFIDF_E_INVAL;
    if (p->variant > TFIDF_NB_COMPLEMENT || p->feature > TFIDF_NB_BINARY) return TFIDF_E_INVAL;
    if (!(p->alpha >= 0.0 && p->alpha <= TFIDF_NB_MAX_ALPHA)) return TFIDF_E_INVAL;   /* NaN fails both */
    if (p->nlabelled > 0xFFFFFFFFull) return TFIDF_E_INVAL;
    if (p->nlabelled && (!p->doc || !p->label)) return TFIDF_E_INVAL;
    uint8_t has[TFIDF_NB_MAX_CLASSES] = {0};
    for (uint64_t i = 0; i < p->nlabelled; ++i) {
        if (p->label[i] >= p->nclasses) return TFIDF_E_INVAL;
        has[p->label[i]] = 1;
    }
    for (uint32_t c = 0; c < p->nclasses; ++c)
        if (!has[c]) return TFIDF_E_INVAL;
    uint32_t* ids = (uint32_t*)malloc((size_t)p->nlabelled * 4);
    if (!ids) return TFIDF_E_NOMEM;
    memcpy(ids, p->doc, (size_t)p->nlabelled * 4);
    qsort(ids, (size_t)p->nlabelled, 4, nb_u32_cmp);
    int rc = TFIDF_OK;
    for (uint64_t i = 1; i < p->nlabelled; ++i)
        if (ids[i] == ids[i - 1]) { rc = TFIDF_E_INVAL; break; }
    free(ids);
    return rc;
}

void tfidf_nb_model_free(tfidf_nb_model* m) {
    if (!m) return;
    free(m->class_docs); free(m->class_total); free(m->feature_count); free(m->prior); free(m->weight);
    memset(m, 0, sizeof(*m));
}

void tfidf_nb_labels_free(tfidf_nb_labels* l) {
    if (!l) return;
    free(l->doc); free(l->pos); free(l->label); free(l->score); free(l->scores);
    memset(l, 0, sizeof(*l));
}

/* ---- the fit on a fetched result ---- */

typedef struct { uint32_t id, label; } nb_idlab;
static int nb_idlab_cmp(const void* a, const void* b) {
    const nb_idlab* x = (const nb_idlab*)a;
    const nb_idlab* y = (const nb_idlab*)b;
    return x->id < y->id ? -1 : (x->id > y->id ? 1 : 0);
}
static const nb_idlab* nb_find(const nb_idlab* v, uint64_t n, uint32_t id) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (v[mid].id < id) lo = mid + 1; else hi = mid;
    }
    return lo < n && v[lo].id == id ? v + lo : NULL;
}

int tfidf_result_nb_fit(const tfidf_result* r, const tfidf_nb_params* p, tfidf_nb_model* out) {
    if (!out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!r) return TFIDF_E_INVAL;
    int rc = tfidf_nb_check(p);
    if (rc) return rc;
    const uint32_t K = p->nclasses, V = r->nterms, N = r->ndocs;
    const uint64_t P = r->npairs, n = p->nlabelled;
    const size_t KV = (size_t)K * V;
    const double alpha = p->alpha == 0.0 ? 1.0 : p->alpha;
    const int comp = p->variant == TFIDF_NB_COMPLEMENT, bin = p->feature == TFIDF_NB_BINARY;
    if (N && !r->doc_id) return TFIDF_E_INVAL;
    if (P && (!r->pair_doc || !r->pair_term || !r->pair_count || !N)) return TFIDF_E_INVAL;
    nb_idlab* lab = (nb_idlab*)malloc(((size_t)n + 1) * sizeof(nb_idlab));
    uint32_t* ids = (uint32_t*)malloc(((size_t)N + 1) * 4);
    uint64_t* F = (uint64_t*)calloc((size_t)V + 1, 8);
    out->class_docs = (uint64_t*)calloc((size_t)K + 1, 8);
    out->class_total = (uint64_t*)calloc((size_t)K + 1, 8);
    out->feature_count = (uint64_t*)calloc(KV + 1, 8);
    out->prior = (double*)calloc((size_t)K + 1, 8);
    out->weight = (double*)calloc(KV + 1, 8);
    if (!lab || !ids || !F || !out->class_docs || !out->class_total || !out->feature_count || !out->prior || !out->weight) {
        rc = TFIDF_E_NOMEM;
        goto done;
    }
    memcpy(ids, r->doc_id, (size_t)N * 4);
    qsort(ids, N, 4, nb_u32_cmp);
    for (uint64_t i = 0; i < n; ++i) {
        lab[i].id = p->doc[i];
        lab[i].label = p->label[i];
        if (!bsearch(&p->doc[i], ids, N, 4, nb_u32_cmp)) { rc = TFIDF_E_INVAL; goto done; }
        out->class_docs[p->label[i]] += 1u;
    }
    qsort(lab, (size_t)n, sizeof(nb_idlab), nb_idlab_cmp);
    for (uint64_t q = 0; q < P;) {   /* a document: a maximal run of equal pair_doc */
        const uint32_t id = r->pair_doc[q];
        if (!bsearch(&id, ids, N, 4, nb_u32_cmp)) { rc = TFIDF_E_INVAL; goto done; }
        const nb_idlab* l = nb_find(lab, n, id);
        for (; q < P && r->pair_doc[q] == id; ++q) {
            const uint32_t t = r->pair_term[q];
            if (t >= V) { rc = TFIDF_E_INVAL; goto done; }
            if (l) out->feature_count[(size_t)t * K + l->label] += bin ? 1u : r->pair_count[q];
        }
    }
    uint64_t Ttot = 0;
    for (uint32_t t = 0; t < V; ++t)
        for (uint32_t c = 0; c < K; ++c) {
            const uint64_t fc = out->feature_count[(size_t)t * K + c];
            out->class_total[c] += fc;
            F[t] += fc;
        }
    for (uint32_t c = 0; c < K; ++c) Ttot += out->class_total[c];
    {
        const double aV = alpha * (double)V;
        for (uint32_t c = 0; c < K; ++c) {
            double lc;   /* the class's own logarithm */
            if (comp) {
                const double a = (double)(Ttot - out->class_total[c]) + aV;
                lc = log(a);
                out->prior[c] = 0.0;
            } else {
                const double a = (double)out->class_total[c] + aV;
                lc = log(a);
                if (p->uniform_prior) {
                    out->prior[c] = 0.0;
                } else {
                    const double ln_c = log((double)out->class_docs[c]), ln_n = log((double)n);
                    out->prior[c] = ln_c - ln_n;
                }
            }
            for (uint32_t t = 0; t < V; ++t) {
                const uint64_t fc = out->feature_count[(size_t)t * K + c];
                const double a = (double)(comp ? F[t] - fc : fc) + alpha;
                const double la = log(a);
                out->weight[(size_t)t * K + c] = comp ? lc - la : la - lc;
            }
        }
    }
    out->size = sizeof(*out);
    out->nclasses = K;
    out->nterms = V;
    out->variant = p->variant;
    out->feature = p->feature;
    out->uniform_prior = p->uniform_prior ? 1u : 0u;
    out->alpha = alpha;
    out->nlabelled = n;
done:
    free(lab); free(ids); free(F);
    if (rc) tfidf_nb_model_free(out);
    return rc;
}

/* ---- rows against a model ---- */

int tfidf_nb_model_predict(const tfidf_nb_model* m, uint32_t nrows, const uint64_t* row_off, const uint32_t* term,
                           const uint32_t* count, uint32_t flags, tfidf_nb_labels* out) {
    if (!out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!m || m->size < sizeof(tfidf_nb_model) || (flags & ~TFIDF_NB_ALL_SCORES)) return TFIDF_E_INVAL;
    const uint32_t K = m->nclasses, V = m->nterms;
    if (K == 0u || K > TFIDF_NB_MAX_CLASSES || !m->prior || (V && !m->weight)) return TFIDF_E_INVAL;
    if (nrows && !row_off) return TFIDF_E_INVAL;
    for (uint32_t r = 0; r < nrows; ++r)
        if (row_off[r + 1] < row_off[r]) return TFIDF_E_INVAL;
    const uint64_t P = nrows ? row_off[nrows] : 0u, P0 = nrows ? row_off[0] : 0u;
    if (P > P0 && (!term || !count)) return TFIDF_E_INVAL;
    for (uint64_t q = P0; q < P; ++q)
        if (term[q] >= V) return TFIDF_E_INVAL;
    const int bin = m->feature == TFIDF_NB_BINARY, all = (flags & TFIDF_NB_ALL_SCORES) != 0;
    out->ndocs = nrows;
    out->nclasses = K;
    out->doc = (uint32_t*)calloc((size_t)nrows + 1, 4);
    out->pos = (uint32_t*)calloc((size_t)nrows + 1, 4);
    out->label = (uint32_t*)calloc((size_t)nrows + 1, 4);
    out->score = (double*)calloc((size_t)nrows + 1, 8);
    if (all) out->scores = (double*)calloc((size_t)nrows * K + 1, 8);
    if (!out->doc || !out->pos || !out->label || !out->score || (all && !out->scores)) {
        tfidf_nb_labels_free(out);
        return TFIDF_E_NOMEM;
    }
    for (uint32_t r = 0; r < nrows; ++r) {
        uint32_t best_c = 0;
        double best = 0.0;
        for (uint32_t c = 0; c < K; ++c) {
            double s = m->prior[c];
            for (uint64_t q = row_off[r]; q < row_off[r + 1]; ++q) {
                const double x = bin ? 1.0 : (double)count[q];
                const double prod = x * m->weight[(size_t)term[q] * K + c];
                s = s + prod;
            }
            if (all) out->scores[(size_t)r * K + c] = s;
            if (c == 0u || s > best) { best = s; best_c = c; }   /* a later class only when strictly larger */
        }
        out->doc[r] = r;
        out->pos[r] = r;
        out->label[r] = best_c;
        out->score[r] = best;
    }
    return TFIDF_OK;
}
