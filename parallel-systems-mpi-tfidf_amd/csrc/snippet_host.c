/*
 * snippet_host.c — the host half of snippets (include/tfidf.h, "snippets"): the parameter check
 * every entry point shares, tfidf_snippets_free, and tfidf_result_snippet, the definition in plain
 * C over a fetched result and the host corpus.  No GPU, no floating point.  The device path is
 * snippets.hip / engine_snippets.cpp; the two share nothing but the header.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"

int tfidf_snippets_check(const tfidf_snippet_params* pr) {
    if (!pr) return TFIDF_E_INVAL;
    if (pr->size < sizeof(tfidf_snippet_params)) return TFIDF_E_INVAL;
    if (pr->window == 0 || pr->window > TFIDF_SNIP_MAX_WINDOW) return TFIDF_E_INVAL;
    if (pr->max_marks > TFIDF_SNIP_MAX_MARKS) return TFIDF_E_INVAL;
    if (pr->flags & ~TFIDF_SNIP_TEXT) return TFIDF_E_INVAL;
    if (pr->scratch_bytes != 0 && pr->scratch_bytes < TFIDF_SNIP_MIN_SCRATCH) return TFIDF_E_INVAL;
    return TFIDF_OK;
}

void tfidf_snippets_free(tfidf_snippets* s) {
    if (!s) return;
    free(s->flags); free(s->ntokens); free(s->nmatch); free(s->nterms_matched); free(s->win_tok); free(s->win_byte);
    free(s->cover); free(s->hits); free(s->mark_off); free(s->mark_byte); free(s->mark_len); free(s->mark_slot);
    free(s->text_off); free(s->text); free(s->qterm_off); free(s->qterm_pos); free(s->qterm_len); free(s->qterm_found);
    memset(s, 0, sizeof(*s));
}

static int is_ws(uint8_t c) { return c == 0x20u || (c >= 0x09u && c <= 0x0Du); }

/* a byte string's length up to its first NUL */
static uint64_t term_len(const uint8_t* p, uint64_t n) {
    const uint8_t* z = n ? (const uint8_t*)memchr(p, 0, (size_t)n) : NULL;
    return z ? (uint64_t)(z - p) : n;
}

/* the order of the result's term table: strcmp of "word\t" (a term holds no TAB) */
static int cmp_tab(const uint8_t* a, uint64_t la, const uint8_t* b, uint64_t lb) {
    for (uint64_t i = 0;; ++i) {
        if (i == la && i == lb) return 0;
        const uint8_t ca = i < la ? a[i] : 0x09u, cb = i < lb ? b[i] : 0x09u;
        if (ca != cb) return ca < cb ? -1 : 1;
        if (i == la || i == lb) return i == la ? -1 : 1;   /* unreachable for terms without a TAB */
    }
}

static int vocab_has(const tfidf_result* r, const uint8_t* t, uint64_t n) {
    uint64_t lo = 0, hi = r->nterms;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const int c = cmp_tab(r->term_bytes + r->term_off[mid], r->term_off[mid + 1] - r->term_off[mid], t, n);
        if (c == 0) return 1;
        if (c < 0) lo = mid + 1;
        else hi = mid;
    }
    return 0;
}

typedef struct {
    uint32_t id, idx;
} id_idx;
static int cmp_id(const void* a, const void* b) {
    const id_idx *x = (const id_idx*)a, *y = (const id_idx*)b;
    if (x->id != y->id) return x->id < y->id ? -1 : 1;
    return x->idx < y->idx ? -1 : (x->idx > y->idx);
}

/* a growable array of `el`-byte elements */
typedef struct {
    uint8_t* p;
    uint64_t n, cap;
} vec;
static void* vec_push(vec* v, uint64_t count, size_t el) {
    if (v->n + count > v->cap || !v->p) {   /* never NULL, also for no elements */
        uint64_t cap = v->cap ? v->cap * 2 : 256;
        while (cap < v->n + count) cap *= 2;
        uint8_t* q = (uint8_t*)realloc(v->p, (size_t)cap * el);
        if (!q) return NULL;
        v->p = q;
        v->cap = cap;
    }
    void* at = v->p + (size_t)v->n * el;
    v->n += count;
    return at;
}

typedef struct {
    uint64_t byte;
    uint32_t pos, len, slot;
} match_rec;

/* first index in m[0, n) whose position is >= pos */
static uint64_t lower_pos(const match_rec* m, uint64_t n, uint64_t pos) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (m[mid].pos < pos) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

int tfidf_result_snippet(const tfidf_result* r, const tfidf_corpus* hc, const tfidf_queries* qs, const uint32_t* job_query,
                         const uint32_t* job_doc, uint32_t njobs, const tfidf_snippet_params* pr, tfidf_snippets* out) {
    if (!out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!r || !hc || !qs || tfidf_snippets_check(pr) != TFIDF_OK) return TFIDF_E_INVAL;
    if (njobs > TFIDF_SNIP_MAX_JOBS || (njobs && (!job_query || !job_doc))) return TFIDF_E_INVAL;
    const uint32_t nq = qs->nqueries;
    if (nq > TFIDF_QUERY_MAX_QUERIES || !qs->q_off || (qs->nbytes && !qs->bytes)) return TFIDF_E_INVAL;
    for (uint32_t q = 0; q < nq; ++q)
        if (qs->q_off[q + 1] < qs->q_off[q]) return TFIDF_E_INVAL;
    if (qs->q_off[nq] > qs->nbytes) return TFIDF_E_INVAL;
    for (uint32_t j = 0; j < njobs; ++j)
        if (job_query[j] >= nq) return TFIDF_E_INVAL;
    if (hc->flags & TFIDF_CORPUS_DEVICE) return TFIDF_E_INVAL;
    if (hc->ndocs && !hc->doc_off) return TFIDF_E_INVAL;
    for (uint32_t d = 0; d < hc->ndocs; ++d)
        if (hc->doc_off[d + 1] < hc->doc_off[d]) return TFIDF_E_INVAL;
    if (hc->ndocs && hc->doc_off[hc->ndocs] > hc->nbytes) return TFIDF_E_INVAL;
    if (hc->nbytes && !hc->bytes) return TFIDF_E_INVAL;
    const uint32_t W = pr->window, M = pr->max_marks;
    const int want_text = (pr->flags & TFIDF_SNIP_TEXT) != 0;

    int rc = TFIDF_E_NOMEM;
    id_idx* ids = NULL;
    uint8_t* truncated = NULL;
    vec qpos = {0, 0, 0}, qlen = {0, 0, 0}, qfound = {0, 0, 0}, matches = {0, 0, 0};
    vec mbyte = {0, 0, 0}, mlen = {0, 0, 0}, mslot = {0, 0, 0}, text = {0, 0, 0};
    out->njobs = njobs;
    out->nqueries = nq;
    out->flags = (uint32_t*)calloc((size_t)njobs + 1, 4);
    out->ntokens = (uint32_t*)calloc((size_t)njobs + 1, 4);
    out->nmatch = (uint32_t*)calloc((size_t)njobs + 1, 4);
    out->nterms_matched = (uint32_t*)calloc((size_t)njobs + 1, 4);
    out->win_tok = (uint32_t*)calloc(2 * (size_t)njobs + 1, 4);
    out->win_byte = (uint64_t*)calloc(2 * (size_t)njobs + 1, 8);
    out->cover = (uint32_t*)calloc((size_t)njobs + 1, 4);
    out->hits = (uint32_t*)calloc((size_t)njobs + 1, 4);
    out->mark_off = (uint64_t*)calloc((size_t)njobs + 1, 8);
    out->text_off = (uint64_t*)calloc((size_t)njobs + 1, 8);
    out->qterm_off = (uint64_t*)calloc((size_t)nq + 1, 8);
    truncated = (uint8_t*)calloc((size_t)nq + 1, 1);
    ids = (id_idx*)malloc(((size_t)hc->ndocs + 1) * sizeof(id_idx));
    if (!out->flags || !out->ntokens || !out->nmatch || !out->nterms_matched || !out->win_tok || !out->win_byte ||
        !out->cover || !out->hits || !out->mark_off || !out->text_off || !out->qterm_off || !truncated || !ids)
        goto done;

    /* ---- U(q): the distinct terms in order of first occurrence, cut at TFIDF_SNIP_MAX_TERMS ---- */
    for (uint32_t q = 0; q < nq; ++q) {
        const uint8_t* qb = qs->bytes + qs->q_off[q];
        const uint64_t qn = qs->q_off[q + 1] - qs->q_off[q], first = qpos.n;
        for (uint64_t i = 0; i < qn;) {
            if (is_ws(qb[i])) { ++i; continue; }
            uint64_t e = i;
            while (e < qn && !is_ws(qb[e])) ++e;
            const uint64_t tl = term_len(qb + i, e - i);
            int seen = 0;
            for (uint64_t u = first; u < qpos.n && !seen; ++u)
                seen = ((uint32_t*)qlen.p)[u] == tl && memcmp(qb + ((uint64_t*)qpos.p)[u], qb + i, (size_t)tl) == 0;
            if (!seen) {
                if (qpos.n - first == TFIDF_SNIP_MAX_TERMS) {
                    truncated[q] = 1;
                } else {
                    uint64_t* a = (uint64_t*)vec_push(&qpos, 1, 8);
                    uint32_t* b = (uint32_t*)vec_push(&qlen, 1, 4);
                    uint8_t* c = (uint8_t*)vec_push(&qfound, 1, 1);
                    if (!a || !b || !c) goto done;
                    *a = i;
                    *b = (uint32_t)tl;
                    *c = (uint8_t)vocab_has(r, qb + i, tl);
                }
            }
            i = e;
        }
        out->qterm_off[q + 1] = qpos.n;
    }

    /* ---- global document id -> local index (the first of equal ids) ---- */
    for (uint32_t d = 0; d < hc->ndocs; ++d) {
        ids[d].id = hc->doc_ids ? hc->doc_ids[d] : d + 1;
        ids[d].idx = d;
    }
    qsort(ids, hc->ndocs, sizeof(id_idx), cmp_id);

    for (uint32_t j = 0; j < njobs; ++j) {
        const uint32_t q = job_query[j];
        out->mark_off[j] = mbyte.n;
        out->text_off[j] = text.n;
        uint32_t lo = 0, hi = hc->ndocs;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (ids[mid].id < job_doc[j]) lo = mid + 1;
            else hi = mid;
        }
        if (lo == hc->ndocs || ids[lo].id != job_doc[j]) {
            out->flags[j] = TFIDF_SNIP_NO_DOC;
            continue;
        }
        if (truncated[q]) out->flags[j] |= TFIDF_SNIP_TRUNCATED;
        const uint32_t d = ids[lo].idx;
        const uint8_t* doc = hc->bytes + hc->doc_off[d];
        const uint64_t dn = hc->doc_off[d + 1] - hc->doc_off[d];
        const uint8_t* qb = qs->bytes + qs->q_off[q];
        const uint64_t u0 = out->qterm_off[q], nu = out->qterm_off[q + 1] - u0;
        const uint64_t* up = (const uint64_t*)qpos.p + u0;
        const uint32_t* ul = (const uint32_t*)qlen.p + u0;
        const uint8_t* uf = qfound.p + u0;
        uint64_t lmax = 0;
        int any = 0;
        for (uint64_t u = 0; u < nu; ++u)
            if (uf[u]) { any = 1; if (ul[u] > lmax) lmax = ul[u]; }

        /* ---- the document's tokens and matches ---- */
        matches.n = 0;
        uint64_t T = 0;
        for (uint64_t i = 0; i < dn;) {
            if (is_ws(doc[i])) { ++i; continue; }
            uint64_t e = i;
            while (e < dn && !is_ws(doc[e])) ++e;
            if (any) {
                const uint64_t tl = term_len(doc + i, e - i);
                if (tl <= lmax)
                    for (uint64_t u = 0; u < nu; ++u)
                        if (uf[u] && ul[u] == tl && memcmp(qb + up[u], doc + i, (size_t)tl) == 0) {
                            match_rec* m = (match_rec*)vec_push(&matches, 1, sizeof(match_rec));
                            if (!m) goto done;
                            m->byte = i;
                            m->pos = (uint32_t)T;
                            m->len = (uint32_t)tl;
                            m->slot = (uint32_t)u;
                            break;
                        }
            }
            ++T;
            i = e;
        }
        const match_rec* m = (const match_rec*)matches.p;
        const uint64_t nm = matches.n;
        out->ntokens[j] = (uint32_t)T;
        out->nmatch[j] = (uint32_t)nm;
        uint32_t cnt[TFIDF_SNIP_MAX_TERMS];
        memset(cnt, 0, sizeof(cnt));
        uint32_t distinct = 0;
        for (uint64_t i = 0; i < nm; ++i) distinct += cnt[m[i].slot]++ == 0;
        out->nterms_matched[j] = distinct;
        if (T == 0) continue;

        /* ---- the best window among the match positions: two pointers over the list ---- */
        uint64_t s1 = 0, e1 = W < T ? W : T;
        if (nm) {
            memset(cnt, 0, sizeof(cnt));
            uint32_t cover = 0, best_cover = 0;
            uint64_t best_hits = 0, best_i = 0, best_end = 0, jx = 0;
            for (uint64_t i = 0; i < nm; ++i) {
                while (jx < nm && (uint64_t)m[jx].pos < (uint64_t)m[i].pos + W) cover += cnt[m[jx++].slot]++ == 0;
                const uint64_t hits = jx - i;
                if (cover > best_cover || (cover == best_cover && hits > best_hits)) {
                    best_cover = cover;
                    best_hits = hits;
                    best_i = i;
                    best_end = jx;
                }
                cover -= --cnt[m[i].slot] == 0;
            }
            const uint64_t s = m[best_i].pos, last = m[best_end - 1].pos;
            const uint64_t slack = W - (last - s + 1), back = slack / 2 < s ? slack / 2 : s;
            s1 = s - back;
            e1 = s1 + W < T ? s1 + W : T;
        }
        const uint64_t mlo = lower_pos(m, nm, s1), mhi = lower_pos(m, nm, e1);
        memset(cnt, 0, sizeof(cnt));
        uint32_t cover = 0;
        for (uint64_t i = mlo; i < mhi; ++i) cover += cnt[m[i].slot]++ == 0;
        out->win_tok[2 * (size_t)j] = (uint32_t)s1;
        out->win_tok[2 * (size_t)j + 1] = (uint32_t)e1;
        out->cover[j] = cover;
        out->hits[j] = (uint32_t)(mhi - mlo);

        /* ---- the bytes of tokens s' and e' ---- */
        uint64_t b0 = dn, b1 = dn, k = 0;
        for (uint64_t i = 0; i < dn && k <= e1;) {
            if (is_ws(doc[i])) { ++i; continue; }
            if (k == s1) b0 = i;
            if (k == e1) b1 = i;
            ++k;
            while (i < dn && !is_ws(doc[i])) ++i;
        }
        out->win_byte[2 * (size_t)j] = b0;
        out->win_byte[2 * (size_t)j + 1] = b1;

        const uint64_t nmarks = mhi - mlo < M ? mhi - mlo : M;
        uint64_t* mb = (uint64_t*)vec_push(&mbyte, nmarks, 8);
        uint32_t* ml = (uint32_t*)vec_push(&mlen, nmarks, 4);
        uint32_t* ms = (uint32_t*)vec_push(&mslot, nmarks, 4);
        if (!mb || !ml || !ms) goto done;
        for (uint64_t i = 0; i < nmarks; ++i) {
            mb[i] = m[mlo + i].byte;
            ml[i] = m[mlo + i].len;
            ms[i] = m[mlo + i].slot;
        }
        if (want_text) {
            uint8_t* t = (uint8_t*)vec_push(&text, b1 - b0, 1);
            if (!t) goto done;
            if (b1 > b0) memcpy(t, doc + b0, (size_t)(b1 - b0));
        }
    }
    out->mark_off[njobs] = mbyte.n;
    out->text_off[njobs] = text.n;
    /* the arrays are never NULL in a returned result, also when they are empty */
    if (!vec_push(&qpos, 1, 8) || !vec_push(&qlen, 1, 4) || !vec_push(&qfound, 1, 1) || !vec_push(&mbyte, 1, 8) ||
        !vec_push(&mlen, 1, 4) || !vec_push(&mslot, 1, 4) || !vec_push(&text, 1, 1))
        goto done;
    out->qterm_pos = (uint64_t*)qpos.p;
    out->qterm_len = (uint32_t*)qlen.p;
    out->qterm_found = qfound.p;
    out->mark_byte = (uint64_t*)mbyte.p;
    out->mark_len = (uint32_t*)mlen.p;
    out->mark_slot = (uint32_t*)mslot.p;
    out->text = text.p;
    qpos.p = qlen.p = qfound.p = mbyte.p = mlen.p = mslot.p = text.p = NULL;
    rc = TFIDF_OK;
done:
    free(ids);
    free(truncated);
    free(matches.p);
    free(qpos.p); free(qlen.p); free(qfound.p); free(mbyte.p); free(mlen.p); free(mslot.p); free(text.p);
    if (rc != TFIDF_OK) tfidf_snippets_free(out);
    return rc;
}
