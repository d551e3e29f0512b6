/*
 * match_host_test — the host half of term matching on edge inputs: csrc/match_host.c (the check,
 * tfidf_model_match_terms) and host/query_expand.h (split, plan, rewrite, suggest).  A stand-alone
 * program that tests/test_match_native.py builds with AddressSanitizer and
 * UndefinedBehaviorSanitizer; no GPU.  Prints "ok" and returns 0, or names the first failure.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"
#include "../../parallel-systems-mpi-tfidf_amd/host/query_expand.h"

#define CHECK(x)                                                 \
    do {                                                         \
        if (!(x)) {                                              \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                            \
        }                                                        \
    } while (0)

/* a model over exactly sized heap arrays, so that a read past an end is seen */
static int make_model(tfidf_model* m, const char* const* words, const uint32_t* df, uint32_t n, uint64_t N) {
    memset(m, 0, sizeof(*m));
    m->size = sizeof(*m);
    m->ndocs_total = N;
    m->nterms = n;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) total += strlen(words[i]);
    m->term_off = (uint64_t*)malloc(((size_t)n + 1) * 8);
    m->term_bytes = (uint8_t*)malloc((size_t)total ? (size_t)total : 1);
    m->term_df = (uint32_t*)malloc(((size_t)n ? n : 1) * 4);
    if (!m->term_off || !m->term_bytes || !m->term_df) return 1;
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        m->term_off[i] = at;
        memcpy(m->term_bytes + at, words[i], strlen(words[i]));
        at += strlen(words[i]);
        m->term_df[i] = df[i];
    }
    m->term_off[n] = at;
    return 0;
}
static void free_model(tfidf_model* m) { free(m->term_off); free(m->term_bytes); free(m->term_df); }

typedef struct {
    uint8_t* bytes;
    uint64_t* off;
    uint8_t *kind, *edits;
    tfidf_patterns p;
} pats;
static int make_pats(pats* ps, const char* const* w, const uint8_t* kind, const uint8_t* edits, uint32_t n) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) total += strlen(w[i]);
    ps->bytes = (uint8_t*)malloc((size_t)total ? (size_t)total : 1);
    ps->off = (uint64_t*)malloc(((size_t)n + 1) * 8);
    ps->kind = (uint8_t*)malloc(n ? n : 1);
    ps->edits = (uint8_t*)malloc(n ? n : 1);
    if (!ps->bytes || !ps->off || !ps->kind || !ps->edits) return 1;
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        ps->off[i] = at;
        memcpy(ps->bytes + at, w[i], strlen(w[i]));
        at += strlen(w[i]);
        ps->kind[i] = kind[i];
        ps->edits[i] = edits[i];
    }
    ps->off[n] = at;
    ps->p.bytes = ps->bytes;
    ps->p.nbytes = at;
    ps->p.p_off = ps->off;
    ps->p.npatterns = n;
    ps->p.kind = ps->kind;
    ps->p.max_edits = ps->edits;
    return 0;
}
static void free_pats(pats* ps) { free(ps->bytes); free(ps->off); free(ps->kind); free(ps->edits); }

static int word_is(const tfidf_term_matches* m, size_t e, const char* w) {
    const uint64_t n = m->word_off[e + 1] - m->word_off[e];
    return n == strlen(w) && memcmp(m->word_bytes + m->word_off[e], w, (size_t)n) == 0;
}

static int test_model_match(void) {
    /* in strcmp("word\t") order; the empty term first */
    static const char* const words[] = {"", "a", "ab", "abc", "abd", "ba", "bcd", "ca", "receive", "recieve"};
    static const uint32_t df[] = {1, 5, 3, 3, 7, 2, 1, 4, 9, 2};
    tfidf_model m;
    CHECK(!make_model(&m, words, df, 10, 10));
    CHECK(tfidf_model_check(&m) == TFIDF_OK);
    tfidf_match_params pr;
    memset(&pr, 0, sizeof(pr));
    pr.size = sizeof(pr);
    pr.max_expansions = 3;
    pr.flags = TFIDF_MATCH_TRANSPOSE;
    static const char* const pw[] = {"ab", "ca", "a", "recieve", "x", "zzzz", "ab"};
    static const uint8_t kind[] = {0, 0, 1, 0, 0, 0, 1};
    static const uint8_t edits[] = {1, 2, 9, 1, 1, 2, 0};   /* 9: ignored for a prefix pattern */
    pats ps;
    CHECK(!make_pats(&ps, pw, kind, edits, 7));
    tfidf_term_matches t;
    CHECK(tfidf_model_match_terms(&m, &ps.p, &pr, &t) == TFIDF_OK);
    CHECK(t.npatterns == 7 && t.k == 3);
    /* "ab" d=1 with the transposition: ab 0; then a(5) abd(7) abc(3) ba(2, transposed) at 1: by df */
    CHECK(t.nmatch[0] == 5 && t.nterms[0] == 3);
    CHECK(word_is(&t, 0, "ab") && t.dist[0] == 0 && t.df[0] == 3 && t.term[0] == 2);
    CHECK(word_is(&t, 1, "abd") && t.dist[1] == 1 && t.df[1] == 7);
    CHECK(word_is(&t, 2, "a") && t.dist[2] == 1 && t.df[2] == 5);
    /* "ca" d=2 does not reach "abc" (3 under the optimal string alignment) */
    for (uint32_t j = 0; j < t.nterms[1]; ++j) CHECK(!word_is(&t, 3 + j, "abc"));
    CHECK(word_is(&t, 3, "ca") && t.dist[3] == 0);
    /* prefix "a": a, ab, abc, abd by df: abd 7, a 5, then ab before abc (rank) */
    CHECK(t.nmatch[2] == 4 && word_is(&t, 6, "abd") && word_is(&t, 7, "a") && word_is(&t, 8, "ab"));
    CHECK(t.dist[6] == 0 && t.dist[8] == 0);
    /* "recieve" d=1: itself, then receive by the transposition */
    CHECK(t.nmatch[3] == 2 && word_is(&t, 9, "recieve") && word_is(&t, 10, "receive") && t.dist[10] == 1);
    CHECK(t.word_off[12] == t.word_off[11]);                       /* an unused entry is empty */
    /* "x" d=1: the empty term (1 insertion), a (substitution) */
    CHECK(t.nmatch[4] == 2 && word_is(&t, 12, "a") && word_is(&t, 13, "") && t.term[13] == 0);
    CHECK(t.nmatch[5] == 0 && t.nterms[5] == 0);
    CHECK(t.nmatch[6] == 3);
    tfidf_term_matches_free(&t);
    /* without the flag the transposition is two edits */
    pr.flags = 0;
    CHECK(tfidf_model_match_terms(&m, &ps.p, &pr, &t) == TFIDF_OK);
    CHECK(t.nmatch[0] == 4 && t.nmatch[3] == 1);
    tfidf_term_matches_free(&t);
    /* a fixed prefix longer than the pattern is the whole pattern */
    pr.flags = TFIDF_MATCH_TRANSPOSE;
    pr.fixed_prefix = 64;
    CHECK(tfidf_model_match_terms(&m, &ps.p, &pr, &t) == TFIDF_OK);
    CHECK(t.nmatch[0] == 3 && t.nmatch[4] == 0);                   /* ab, abc, abd; nothing starts with x */
    tfidf_term_matches_free(&t);
    /* refused, and the answer zeroed */
    pr.max_expansions = 0;
    memset(&t, 0xAB, sizeof(t));
    CHECK(tfidf_model_match_terms(&m, &ps.p, &pr, &t) == TFIDF_E_INVAL && t.nmatch == NULL && t.npatterns == 0);
    pr.max_expansions = 1024;
    ps.edits[0] = 3;
    CHECK(tfidf_match_check(&ps.p, &pr) == TFIDF_E_INVAL);
    ps.edits[0] = 1;
    CHECK(tfidf_match_check(&ps.p, &pr) == TFIDF_OK);
    /* a 64-byte pattern against 62..66-byte terms, at the arrays' ends */
    char w62[80], w64[80], w66[80];
    memset(w62, 'q', 62); w62[62] = 0;
    memset(w64, 'q', 64); w64[64] = 0;
    memset(w66, 'q', 66); w66[66] = 0;
    const char* const lw[] = {w62, w64, w66};
    static const uint32_t ldf[] = {1, 1, 1};
    tfidf_model lm;
    CHECK(!make_model(&lm, lw, ldf, 3, 3));
    CHECK(tfidf_model_check(&lm) == TFIDF_OK);
    const char* const lp[] = {w64};
    static const uint8_t lk[] = {0}, le[] = {2};
    pats lps;
    CHECK(!make_pats(&lps, lp, lk, le, 1));
    pr.fixed_prefix = 0;
    CHECK(tfidf_model_match_terms(&lm, &lps.p, &pr, &t) == TFIDF_OK);
    CHECK(t.nmatch[0] == 3 && t.dist[0] == 0 && t.dist[1] == 2 && t.dist[2] == 2);
    tfidf_term_matches_free(&t);
    tfidf_term_matches_free(&t);                                   /* a zeroed struct: no-op */
    tfidf_term_matches_free(NULL);
    free_pats(&lps);
    free_model(&lm);
    free_pats(&ps);
    free_model(&m);
    return 0;
}

/* a heap copy of exactly n bytes */
static uint8_t* dup_bytes(const char* s, size_t n) {
    uint8_t* b = (uint8_t*)malloc(n ? n : 1);
    if (b && n) memcpy(b, s, n);
    return b;
}

static int test_expand(void) {
    /* three lines; the last has no newline; a NUL inside a token; a lone '*'; "a**" */
    static const char lines[] = "recieve Conn* x\n* a** Conn*, ab\0cd*\nfoo";
    const size_t n = sizeof(lines) - 1;
    uint8_t* b = dup_bytes(lines, n);
    CHECK(b);
    uint64_t off[4] = {0, 16, 0, n};
    off[2] = (uint64_t)((const char*)memchr(lines + 16, '\n', n - 16) - lines) + 1;
    uint8_t* tb[2];
    uint64_t tn[2], *to[2];
    CHECK(qexp_split_batch(b, off, 3, tb, tn, to) == 0);
    CHECK(tn[0] == strlen("recieve x") + strlen("* Conn*,") + strlen("foo"));
    CHECK(memcmp(tb[0], "recieve x* Conn*,foo", (size_t)tn[0]) == 0);
    CHECK(to[0][1] == 9 && to[0][2] == 17 && to[0][3] == 20);
    CHECK(tn[1] == strlen("Conn") + strlen("a* ab") + 3 && memcmp(tb[1], "Conna* ab\0cd", (size_t)tn[1]) == 0);
    CHECK(to[1][0] == 0 && to[1][1] == 4 && to[1][2] == 12 && to[1][3] == 12);
    const uint8_t* const text[2] = {tb[0], tb[1]};
    const uint64_t* const offs[2] = {to[0], to[1]};
    qexp_plan plan;
    CHECK(qexp_plan_build(text, offs, 3, QEXP_AUTO, &plan) == 0);
    /* plain: recieve(2) x(0) *(0) Conn*,(2) foo(1); prefix: Conn a* ab */
    CHECK(plan.ntok == 8 && plan.npat == 8 && plan.first[0] == 0 && plan.first[1] == 5);
    CHECK(plan.edits[plan.tok[0].pat] == 2 && plan.edits[plan.tok[1].pat] == 0 && plan.edits[plan.tok[4].pat] == 1);
    CHECK(plan.kind[plan.tok[5].pat] == TFIDF_MATCH_PREFIX && plan.kind[plan.tok[0].pat] == TFIDF_MATCH_FUZZY);
    const uint32_t pab = plan.tok[7].pat;
    CHECK(plan.tok[7].len == 5 && plan.p_off[pab + 1] - plan.p_off[pab] == 2);   /* "ab\0cd": the term is "ab" */
    tfidf_match_params pr;
    memset(&pr, 0, sizeof(pr));
    pr.size = sizeof(pr);
    pr.max_expansions = 2;
    CHECK(tfidf_match_check(&plan.patterns, &pr) == TFIDF_OK);       /* the plan's patterns are a legal call */
    /* an answer by hand: pattern i matched i % 3 words "w<i>_<j>" */
    tfidf_term_matches m;
    memset(&m, 0, sizeof(m));
    m.npatterns = plan.npat;
    m.k = 2;
    m.nmatch = (uint64_t*)calloc(plan.npat, 8);
    m.nterms = (uint32_t*)calloc(plan.npat, 4);
    m.term = (uint32_t*)calloc((size_t)plan.npat * 2, 4);
    m.dist = (uint8_t*)calloc((size_t)plan.npat * 2, 1);
    m.df = (uint32_t*)calloc((size_t)plan.npat * 2, 4);
    m.word_off = (uint64_t*)calloc((size_t)plan.npat * 2 + 1, 8);
    m.word_bytes = (uint8_t*)malloc(plan.npat * 2 * 4);
    CHECK(m.nmatch && m.nterms && m.term && m.dist && m.df && m.word_off && m.word_bytes);
    uint64_t at = 0;
    for (uint32_t p = 0; p < plan.npat; ++p) {
        m.nterms[p] = p % 3;
        m.nmatch[p] = p % 3;
        for (uint32_t j = 0; j < 2; ++j) {
            m.word_off[(size_t)p * 2 + j] = at;
            if (j >= m.nterms[p]) continue;
            const char w[5] = {'w', (char)('0' + p), '_', (char)('0' + j), 0};
            memcpy(m.word_bytes + at, w, 4);
            at += 4;
            m.dist[(size_t)p * 2 + j] = (uint8_t)j;
            m.df[(size_t)p * 2 + j] = 10 * p + j;
        }
    }
    m.word_off[(size_t)plan.npat * 2] = at;
    uint8_t* rb = NULL;
    uint64_t rn = 0, *ro = NULL;
    CHECK(qexp_rewrite(&plan, text, 3, &m, &rb, &rn, &ro) == 0);
    /* line 1: recieve = pattern 0 (no word), x = 1 (w1_0), then the prefix Conn = 5 (w5_0 w5_1) */
    CHECK(ro[0] == 0 && ro[1] == strlen("w1_0 w5_0 w5_1") && memcmp(rb, "w1_0 w5_0 w5_1", (size_t)ro[1]) == 0);
    CHECK(ro[3] == rn);
    free(rb);
    free(ro);
    FILE* f = tmpfile();
    CHECK(f);
    qexp_suggest(&plan, 3, &m, f);
    const long flen = ftell(f);
    rewind(f);
    char* sug = (char*)malloc((size_t)flen + 1);
    CHECK(sug && fread(sug, 1, (size_t)flen, f) == (size_t)flen);
    sug[flen] = 0;
    fclose(f);
    static const char first_lines[] = "q1\tx\tw1_0\t0\t10\nq1\tConn*\tw5_0\t0\t50\nq1\tConn*\tw5_1\t1\t51\nq2\t";
    CHECK(strncmp(sug, first_lines, sizeof(first_lines) - 1) == 0);
    free(sug);
    free(m.nmatch); free(m.nterms); free(m.term); free(m.dist); free(m.df); free(m.word_off); free(m.word_bytes);
    qexp_plan_free(&plan);
    /* without a budget the plain tokens stay as they are and are copied; a repeated token is one pattern */
    CHECK(qexp_plan_build(text, offs, 3, QEXP_OFF, &plan) == 0);
    CHECK(plan.npat == 3 && plan.tok[0].pat == QEXP_NO_PATTERN);
    qexp_plan_free(&plan);
    static const char rep[] = "abc abc abcd abc";
    uint8_t* r2 = dup_bytes(rep, sizeof(rep) - 1);
    CHECK(r2);
    const uint64_t roff[2] = {0, sizeof(rep) - 1};
    const uint8_t* const t2[2] = {r2, NULL};
    const uint64_t* const o2[2] = {roff, NULL};
    CHECK(qexp_plan_build(t2, o2, 1, 2, &plan) == 0);
    CHECK(plan.ntok == 4 && plan.npat == 2 && plan.tok[0].pat == plan.tok[1].pat && plan.tok[3].pat == plan.tok[0].pat);
    qexp_plan_free(&plan);
    /* a token of 65 bytes is no pattern; one of 64 is */
    char longline[140];
    memset(longline, 'k', 65);
    longline[65] = ' ';
    memset(longline + 66, 'k', 64);
    uint8_t* r3 = dup_bytes(longline, 130);
    CHECK(r3);
    const uint64_t loff[2] = {0, 130};
    const uint8_t* const t3[2] = {r3, NULL};
    const uint64_t* const o3[2] = {loff, NULL};
    CHECK(qexp_plan_build(t3, o3, 1, QEXP_AUTO, &plan) == 0);
    CHECK(plan.ntok == 2 && plan.npat == 1 && plan.tok[0].pat == QEXP_NO_PATTERN && plan.tok[1].pat == 0);
    CHECK(plan.p_off[1] == 64 && plan.edits[0] == 2);
    qexp_plan_free(&plan);
    /* nothing at all */
    const uint64_t zoff[1] = {0};
    const uint64_t* const o4[2] = {zoff, NULL};
    CHECK(qexp_plan_build(t3, o4, 0, 1, &plan) == 0 && plan.ntok == 0 && plan.npat == 0);
    qexp_plan_free(&plan);
    CHECK(qexp_auto_budget(1) == 0 && qexp_auto_budget(2) == 0 && qexp_auto_budget(3) == 1 && qexp_auto_budget(5) == 1 &&
          qexp_auto_budget(6) == 2);
    free(r3);
    free(r2);
    for (int c = 0; c < 2; ++c) { free(tb[c]); free(to[c]); }
    free(b);
    return 0;
}

int main(void) {
    if (test_model_match()) return 1;
    if (test_expand()) return 1;
    printf("ok\n");
    return 0;
}
