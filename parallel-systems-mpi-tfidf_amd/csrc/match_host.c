/*
 * match_host.c — the host half of term matching (include/tfidf.h, "term matching"): the
 * parameter check every entry point shares, and tfidf_model_match_terms, the definition in plain
 * C over a model struct.  No GPU, no floating point.  The device scan is match.hip; the two
 * share nothing but the header.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"

int tfidf_match_check(const tfidf_patterns* ps, const tfidf_match_params* pr) {
    if (!ps || !pr) return TFIDF_E_INVAL;
    if (pr->size < sizeof(tfidf_match_params)) return TFIDF_E_INVAL;
    if (pr->max_expansions == 0 || pr->max_expansions > TFIDF_MATCH_MAX_EXPANSIONS) return TFIDF_E_INVAL;
    if (pr->flags & ~TFIDF_MATCH_TRANSPOSE) return TFIDF_E_INVAL;
    if (pr->fixed_prefix > TFIDF_MATCH_MAX_PATTERN) return TFIDF_E_INVAL;
    if (pr->list_records != 0 && pr->list_records < 1024) return TFIDF_E_INVAL;
    if (ps->npatterns > TFIDF_MATCH_MAX_PATTERNS) return TFIDF_E_INVAL;
    if (ps->npatterns == 0) return TFIDF_OK;
    if (!ps->p_off || !ps->kind || !ps->max_edits || !ps->bytes) return TFIDF_E_INVAL;
    if (ps->p_off[ps->npatterns] > ps->nbytes) return TFIDF_E_INVAL;
    for (uint32_t p = 0; p < ps->npatterns; ++p) {
        if (ps->p_off[p + 1] < ps->p_off[p]) return TFIDF_E_INVAL;
        const uint64_t len = ps->p_off[p + 1] - ps->p_off[p];
        if (len == 0 || len > TFIDF_MATCH_MAX_PATTERN) return TFIDF_E_INVAL;
        if (ps->kind[p] != TFIDF_MATCH_FUZZY && ps->kind[p] != TFIDF_MATCH_PREFIX) return TFIDF_E_INVAL;
        if (ps->kind[p] == TFIDF_MATCH_FUZZY && ps->max_edits[p] > TFIDF_MATCH_MAX_EDITS) return TFIDF_E_INVAL;
    }
    return TFIDF_OK;
}

void tfidf_term_matches_free(tfidf_term_matches* m) {
    if (!m) return;
    free(m->nmatch); free(m->nterms); free(m->term); free(m->dist); free(m->df); free(m->word_off);
    free(m->word_bytes);
    memset(m, 0, sizeof(*m));
}

/* dist(p, t) when it is <= d, else d + 1: two (three with the transposition) full rows of the
 * matrix over the pattern, the term's bytes down the rows.  |len(t) - len(p)| > d is decided by
 * the caller. */
static uint32_t bounded_dist(const uint8_t* p, uint32_t m, const uint8_t* t, uint32_t n, uint32_t d, int osa) {
    uint32_t row[3][TFIDF_MATCH_MAX_PATTERN + 1];
    uint32_t *prev2 = row[0], *prev = row[1], *cur = row[2];
    for (uint32_t j = 0; j <= m; ++j) prev[j] = j;
    for (uint32_t i = 1; i <= n; ++i) {
        uint32_t best = cur[0] = i;
        for (uint32_t j = 1; j <= m; ++j) {
            uint32_t v = prev[j - 1] + (t[i - 1] != p[j - 1]);
            if (prev[j] + 1 < v) v = prev[j] + 1;
            if (cur[j - 1] + 1 < v) v = cur[j - 1] + 1;
            if (osa && i > 1 && j > 1 && t[i - 1] == p[j - 2] && t[i - 2] == p[j - 1] && prev2[j - 2] + 1 < v)
                v = prev2[j - 2] + 1;
            cur[j] = v;
            if (v < best) best = v;
        }
        if (best > d) return d + 1;   /* a row's minimum never decreases down the rows */
        uint32_t* x = prev2;
        prev2 = prev;
        prev = cur;
        cur = x;
    }
    return prev[m] <= d ? prev[m] : d + 1;
}

typedef struct {
    uint32_t dist, df, term;
} match_rec;

static int rec_cmp(const void* a, const void* b) {
    const match_rec *x = (const match_rec*)a, *y = (const match_rec*)b;
    if (x->dist != y->dist) return x->dist < y->dist ? -1 : 1;
    if (x->df != y->df) return x->df > y->df ? -1 : 1;
    return x->term < y->term ? -1 : (x->term > y->term ? 1 : 0);
}

int tfidf_model_match_terms(const tfidf_model* m, const tfidf_patterns* ps, const tfidf_match_params* pr,
                            tfidf_term_matches* out) {
    if (!out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!m || tfidf_match_check(ps, pr) != TFIDF_OK || tfidf_model_check(m) != TFIDF_OK) return TFIDF_E_INVAL;
    const uint32_t P = ps->npatterns, E = pr->max_expansions, V = m->nterms;
    const int osa = (pr->flags & TFIDF_MATCH_TRANSPOSE) != 0;
    const size_t PE = (size_t)P * E;
    out->npatterns = P;
    out->k = E;
    out->nmatch = (uint64_t*)calloc((size_t)P + 1, 8);
    out->nterms = (uint32_t*)calloc((size_t)P + 1, 4);
    out->term = (uint32_t*)calloc(PE + 1, 4);
    out->dist = (uint8_t*)calloc(PE + 1, 1);
    out->df = (uint32_t*)calloc(PE + 1, 4);
    out->word_off = (uint64_t*)calloc(PE + 1, 8);
    out->word_bytes = (uint8_t*)calloc(1, 1);
    match_rec* rec = (match_rec*)malloc(((size_t)V + 1) * sizeof(match_rec));
    if (!out->nmatch || !out->nterms || !out->term || !out->dist || !out->df || !out->word_off || !out->word_bytes ||
        !rec) {
        free(rec);
        tfidf_term_matches_free(out);
        return TFIDF_E_NOMEM;
    }
    uint64_t wbase = 0;
    for (uint32_t p = 0; p < P; ++p) {
        const uint8_t* pb = ps->bytes + ps->p_off[p];
        const uint32_t plen = (uint32_t)(ps->p_off[p + 1] - ps->p_off[p]);
        const int prefix = ps->kind[p] == TFIDF_MATCH_PREFIX;
        const uint32_t d = prefix ? 0 : ps->max_edits[p];
        const uint32_t fix = prefix ? plen : (pr->fixed_prefix < plen ? pr->fixed_prefix : plen);
        size_t n = 0;
        for (uint32_t t = 0; t < V; ++t) {
            const uint8_t* tb = m->term_bytes + m->term_off[t];
            const uint64_t tlen = m->term_off[t + 1] - m->term_off[t];
            if (tlen < fix || (fix && memcmp(tb, pb, fix) != 0)) continue;
            uint32_t dist = 0;
            if (!prefix) {
                if (tlen > (uint64_t)plen + d || tlen + d < plen) continue;
                dist = bounded_dist(pb, plen, tb, (uint32_t)tlen, d, osa);
                if (dist > d) continue;
            }
            rec[n].dist = dist;
            rec[n].df = m->term_df[t];
            rec[n].term = t;
            ++n;
        }
        qsort(rec, n, sizeof(match_rec), rec_cmp);
        const uint32_t keep = n < E ? (uint32_t)n : E;
        out->nmatch[p] = n;
        out->nterms[p] = keep;
        uint64_t wb = 0;
        for (uint32_t j = 0; j < keep; ++j) wb += m->term_off[rec[j].term + 1] - m->term_off[rec[j].term];
        uint8_t* grown = (uint8_t*)realloc(out->word_bytes, (size_t)(wbase + wb) + 1);
        if (!grown) {
            free(rec);
            tfidf_term_matches_free(out);
            return TFIDF_E_NOMEM;
        }
        out->word_bytes = grown;
        for (uint32_t j = 0; j < E; ++j) {
            const size_t e = (size_t)p * E + j;
            out->word_off[e] = wbase;
            if (j >= keep) continue;
            const uint32_t t = rec[j].term;
            const uint64_t tlen = m->term_off[t + 1] - m->term_off[t];
            out->term[e] = t;
            out->dist[e] = (uint8_t)rec[j].dist;
            out->df[e] = rec[j].df;
            if (tlen) memcpy(out->word_bytes + wbase, m->term_bytes + m->term_off[t], (size_t)tlen);
            wbase += tlen;
        }
    }
    out->word_off[PE] = wbase;
    free(rec);
    return TFIDF_OK;
}
