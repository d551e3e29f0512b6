/*
 * query_expand.h — term expansion for `tfidf --query FILE --fuzzy D|auto [--prefix-ops]` and
 * `--suggest FILE`: the tokens of the query lines become the patterns of one tfidf_match_terms call
 * (include/tfidf.h, "term matching"), and every line is rewritten as the words its tokens matched.
 *
 * Tokens are the maximal runs of bytes outside {0x20, 0x09..0x0D}, as everywhere else.
 *
 *   split    with prefix operators, before the analyzer (as query_ops.h reads '+' and '-'): a
 *            token of >= 2 bytes that ends in '*' goes to the prefix text without the '*', every
 *            other token to the plain text; each text is its tokens in their order, joined by one
 *            blank.  Both texts then pass through the analyzer and the n-grams as ordinary
 *            batches.  Only the last byte is an operator: "a**" is the prefix "a*"; in "Conn*,"
 *            nothing is (the ',' ends it), and --strip-punct makes the plain token "Conn" of it.
 *   plan     the tokens of the two processed texts, as the lookup would see them (a term is its
 *            token up to the first NUL).  A term of 1..TFIDF_MATCH_MAX_PATTERN bytes of the prefix
 *            text is a prefix pattern; one of the plain text is a fuzzy pattern when a budget is
 *            given (0..2, or QEXP_AUTO: by the term's length, <= 2 bytes -> 0, 3..5 -> 1, longer
 *            -> 2); every other token stays as it is.  Equal patterns (kind, budget, bytes) are
 *            one pattern of the call.
 *   rewrite  a line becomes the blank-joined words of its tokens' matches, the plain text's tokens
 *            first, then the prefix text's, each in its order and once per occurrence; a token
 *            that stays as it is is copied; a pattern without a match contributes nothing.
 *   suggest  per line, per distinct pattern in that order, per match:
 *            q<line>\t<token>\t<word>\t<dist>\t<df>, a prefix token with its '*'.
 */
#ifndef TFIDF_QUERY_EXPAND_H
#define TFIDF_QUERY_EXPAND_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"

enum { QEXP_PLAIN = 0, QEXP_PREFIX = 1 };
#define QEXP_OFF  (-1)           /* no fuzzy budget: plain tokens stay as they are */
#define QEXP_AUTO 3              /* the budget goes by the term's length */
#define QEXP_NO_PATTERN 0xFFFFFFFFu
#define QEXP_E_NOMEM (-1)
#define QEXP_E_PATTERNS (-2)     /* more than TFIDF_MATCH_MAX_PATTERNS distinct patterns */

static inline int qexp_is_ws(uint8_t c) { return c == 0x20u || (c >= 0x09u && c <= 0x0Du); }

static inline uint32_t qexp_auto_budget(size_t len) { return len <= 2 ? 0u : len <= 5 ? 1u : 2u; }

/* A batch of nq lines (line q = bytes[off[q], off[q + 1])) into the plain and the prefix text over
 * the same lines.  The arrays come from malloc: bytes_out[c] (never NULL on success),
 * nbytes_out[c], off_out[c] with nq + 1 entries.  Returns 0 or QEXP_E_NOMEM (nothing is kept). */
static inline int qexp_split_batch(const uint8_t* bytes, const uint64_t* off, uint32_t nq, uint8_t* bytes_out[2],
                                   uint64_t nbytes_out[2], uint64_t* off_out[2]) {
    const uint64_t total = nq ? off[nq] - off[0] : 0;
    for (int c = 0; c < 2; ++c) {
        bytes_out[c] = (uint8_t*)malloc((size_t)total + 1);
        off_out[c] = (uint64_t*)malloc(((size_t)nq + 1) * sizeof(uint64_t));
    }
    if (!bytes_out[0] || !bytes_out[1] || !off_out[0] || !off_out[1]) {
        for (int c = 0; c < 2; ++c) { free(bytes_out[c]); free(off_out[c]); bytes_out[c] = NULL; off_out[c] = NULL; }
        return QEXP_E_NOMEM;
    }
    uint64_t at[2] = {0, 0};
    for (uint32_t q = 0; q < nq; ++q) {
        const uint8_t* line = bytes + off[q];
        const size_t len = (size_t)(off[q + 1] - off[q]);
        const uint64_t start[2] = {at[0], at[1]};
        for (size_t i = 0; i < len;) {
            while (i < len && qexp_is_ws(line[i])) ++i;
            if (i >= len) break;
            const size_t t0 = i;
            while (i < len && !qexp_is_ws(line[i])) ++i;
            const int c = (i - t0 >= 2 && line[i - 1] == '*') ? QEXP_PREFIX : QEXP_PLAIN;
            const size_t n = i - t0 - (c == QEXP_PREFIX ? 1 : 0);
            if (at[c] > start[c]) bytes_out[c][at[c]++] = ' ';
            memcpy(bytes_out[c] + at[c], line + t0, n);
            at[c] += n;
        }
        off_out[0][q] = start[0];
        off_out[1][q] = start[1];
    }
    for (int c = 0; c < 2; ++c) { off_out[c][nq] = at[c]; nbytes_out[c] = at[c]; }
    return 0;
}

typedef struct {
    uint32_t line;
    uint32_t pat;                /* the token's pattern in the call, or QEXP_NO_PATTERN: it stays as it is */
    uint64_t at;                 /* the token's bytes in its text */
    uint32_t len;
    uint32_t which;              /* QEXP_PLAIN / QEXP_PREFIX */
} qexp_token;

typedef struct {
    qexp_token* tok;             /* the plain text's tokens line by line, then the prefix text's */
    size_t ntok;
    size_t first[2];             /* tok[first[c]] is text c's first token; its tokens end at first[c + 1] or ntok */
    uint8_t* pbytes;             /* the distinct patterns, as tfidf_patterns wants them */
    uint64_t* p_off;
    uint8_t* kind;
    uint8_t* edits;
    uint32_t npat;
    tfidf_patterns patterns;     /* over the arrays above */
} qexp_plan;

static inline void qexp_plan_free(qexp_plan* p) {
    if (!p) return;
    free(p->tok); free(p->pbytes); free(p->p_off); free(p->kind); free(p->edits);
    memset(p, 0, sizeof(*p));
}

static inline uint64_t qexp_hash(const uint8_t* b, size_t n, uint32_t salt) {
    uint64_t h = 0xcbf29ce484222325ull ^ salt;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

/* The tokens and the distinct patterns of the processed texts.  text[c] / off[c] (nq + 1 offsets)
 * may be NULL for a text that does not exist (no prefix operators).  fuzzy: QEXP_OFF, 0..2 or
 * QEXP_AUTO.  Returns 0, QEXP_E_NOMEM or QEXP_E_PATTERNS; *out is zeroed on an error. */
static inline int qexp_plan_build(const uint8_t* const text[2], const uint64_t* const off[2], uint32_t nq, int fuzzy,
                                  qexp_plan* out) {
    memset(out, 0, sizeof(*out));
    size_t ntok = 0;
    uint64_t pbytes = 0;
    for (int c = 0; c < 2; ++c) {
        if (!text[c] || !off[c]) continue;
        for (uint32_t q = 0; q < nq; ++q)   /* line by line: a line's end ends a token */
            for (uint64_t i = off[c][q]; i < off[c][q + 1];) {
                while (i < off[c][q + 1] && qexp_is_ws(text[c][i])) ++i;
                if (i >= off[c][q + 1]) break;
                const uint64_t t0 = i;
                while (i < off[c][q + 1] && !qexp_is_ws(text[c][i])) ++i;
                ++ntok;
                pbytes += i - t0;
            }
    }
    size_t tcap = 16;
    while (tcap < 2 * ntok) tcap *= 2;
    uint32_t* tab = (uint32_t*)calloc(tcap, sizeof(uint32_t));   /* pattern id + 1 by hash */
    out->tok = (qexp_token*)malloc((ntok + 1) * sizeof(qexp_token));
    out->pbytes = (uint8_t*)malloc((size_t)pbytes + 1);
    out->p_off = (uint64_t*)malloc((ntok + 1) * sizeof(uint64_t));
    out->kind = (uint8_t*)malloc(ntok + 1);
    out->edits = (uint8_t*)malloc(ntok + 1);
    if (!tab || !out->tok || !out->pbytes || !out->p_off || !out->kind || !out->edits) {
        free(tab);
        qexp_plan_free(out);
        return QEXP_E_NOMEM;
    }
    out->p_off[0] = 0;
    size_t nt = 0;
    for (int c = 0; c < 2; ++c) {
        out->first[c] = nt;
        if (!text[c] || !off[c]) continue;
        for (uint32_t q = 0; q < nq; ++q) {
            for (uint64_t i = off[c][q]; i < off[c][q + 1];) {
                while (i < off[c][q + 1] && qexp_is_ws(text[c][i])) ++i;
                if (i >= off[c][q + 1]) break;
                const uint64_t t0 = i;
                while (i < off[c][q + 1] && !qexp_is_ws(text[c][i])) ++i;
                qexp_token* t = &out->tok[nt++];
                t->line = q;
                t->at = t0;
                t->len = (uint32_t)(i - t0);
                t->which = (uint32_t)c;
                t->pat = QEXP_NO_PATTERN;
                const uint8_t* b = text[c] + t0;
                const uint8_t* nul = (const uint8_t*)memchr(b, 0, (size_t)(i - t0));
                const size_t term = nul ? (size_t)(nul - b) : (size_t)(i - t0);   /* as the lookup sees it */
                if (term < 1 || term > TFIDF_MATCH_MAX_PATTERN) continue;
                if (c == QEXP_PLAIN && fuzzy == QEXP_OFF) continue;
                const uint8_t kind = c == QEXP_PREFIX ? TFIDF_MATCH_PREFIX : TFIDF_MATCH_FUZZY;
                const uint8_t bud = c == QEXP_PREFIX ? 0 : (uint8_t)(fuzzy == QEXP_AUTO ? qexp_auto_budget(term) : (uint32_t)fuzzy);
                size_t h = (size_t)qexp_hash(b, term, (uint32_t)kind * 4u + bud) & (tcap - 1);
                for (;; h = (h + 1) & (tcap - 1)) {
                    if (!tab[h]) {
                        if (out->npat >= TFIDF_MATCH_MAX_PATTERNS) {
                            free(tab);
                            qexp_plan_free(out);
                            return QEXP_E_PATTERNS;
                        }
                        const uint32_t id = out->npat++;
                        memcpy(out->pbytes + out->p_off[id], b, term);
                        out->p_off[id + 1] = out->p_off[id] + term;
                        out->kind[id] = kind;
                        out->edits[id] = bud;
                        tab[h] = id + 1;
                        t->pat = id;
                        break;
                    }
                    const uint32_t id = tab[h] - 1;
                    if (out->kind[id] == kind && out->edits[id] == bud && out->p_off[id + 1] - out->p_off[id] == term &&
                        memcmp(out->pbytes + out->p_off[id], b, term) == 0) {
                        t->pat = id;
                        break;
                    }
                }
            }
        }
    }
    free(tab);
    out->ntok = nt;
    out->patterns.bytes = out->pbytes;
    out->patterns.nbytes = out->p_off[out->npat];
    out->patterns.p_off = out->p_off;
    out->patterns.npatterns = out->npat;
    out->patterns.kind = out->kind;
    out->patterns.max_edits = out->edits;
    return 0;
}

/* The rewritten batch: nq lines (malloc'd bytes, never NULL on success, and nq + 1 offsets).
 * m: the answer to plan->patterns.  Returns 0 or QEXP_E_NOMEM. */
static inline int qexp_rewrite(const qexp_plan* plan, const uint8_t* const text[2], uint32_t nq,
                               const tfidf_term_matches* m, uint8_t** bytes, uint64_t* nbytes, uint64_t** off) {
    uint64_t total = 0;
    for (size_t i = 0; i < plan->ntok; ++i) {
        const qexp_token* t = &plan->tok[i];
        if (t->pat == QEXP_NO_PATTERN) total += t->len + 1u;
        else {
            const size_t e = (size_t)t->pat * m->k;
            total += m->word_off[e + m->nterms[t->pat]] - m->word_off[e] + m->nterms[t->pat];
        }
    }
    uint8_t* b = (uint8_t*)malloc((size_t)total + 1);
    uint64_t* o = (uint64_t*)malloc(((size_t)nq + 1) * sizeof(uint64_t));
    if (!b || !o) { free(b); free(o); return QEXP_E_NOMEM; }
    uint64_t at = 0;
    size_t cur[2] = {plan->first[0], plan->first[1]};
    const size_t end[2] = {plan->first[1], plan->ntok};
    for (uint32_t q = 0; q < nq; ++q) {
        o[q] = at;
        for (int c = 0; c < 2; ++c)
            for (; cur[c] < end[c] && plan->tok[cur[c]].line == q; ++cur[c]) {
                const qexp_token* t = &plan->tok[cur[c]];
                if (t->pat == QEXP_NO_PATTERN) {
                    if (at > o[q]) b[at++] = ' ';
                    memcpy(b + at, text[c] + t->at, t->len);
                    at += t->len;
                    continue;
                }
                for (uint32_t j = 0; j < m->nterms[t->pat]; ++j) {
                    const size_t e = (size_t)t->pat * m->k + j;
                    const uint64_t wl = m->word_off[e + 1] - m->word_off[e];
                    if (at > o[q]) b[at++] = ' ';
                    memcpy(b + at, m->word_bytes + m->word_off[e], (size_t)wl);
                    at += wl;
                }
            }
    }
    o[nq] = at;
    *bytes = b;
    *nbytes = at;
    *off = o;
    return 0;
}

/* The suggestion lines of every line to f. */
static inline void qexp_suggest(const qexp_plan* plan, uint32_t nq, const tfidf_term_matches* m, FILE* f) {
    size_t cur[2] = {plan->first[0], plan->first[1]};
    const size_t end[2] = {plan->first[1], plan->ntok};
    for (uint32_t q = 0; q < nq; ++q)
        for (int c = 0; c < 2; ++c) {
            const size_t line0 = cur[c];
            for (; cur[c] < end[c] && plan->tok[cur[c]].line == q; ++cur[c]) {
                const uint32_t p = plan->tok[cur[c]].pat;
                if (p == QEXP_NO_PATTERN) continue;
                int seen = 0;
                for (size_t i = line0; i < cur[c] && !seen; ++i) seen = plan->tok[i].pat == p;
                if (seen) continue;
                for (uint32_t j = 0; j < m->nterms[p]; ++j) {
                    const size_t e = (size_t)p * m->k + j;
                    fprintf(f, "q%u\t", q + 1);
                    fwrite(plan->pbytes + plan->p_off[p], 1, (size_t)(plan->p_off[p + 1] - plan->p_off[p]), f);
                    if (plan->kind[p] == TFIDF_MATCH_PREFIX) fputc('*', f);
                    fputc('\t', f);
                    fwrite(m->word_bytes + m->word_off[e], 1, (size_t)(m->word_off[e + 1] - m->word_off[e]), f);
                    fprintf(f, "\t%u\t%u\n", (unsigned)m->dist[e], m->df[e]);
                }
            }
        }
}

#endif
