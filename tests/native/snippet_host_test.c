/*
 * snippet_host_test — the host half of snippets on edge inputs: csrc/snippet_host.c (the check,
 * tfidf_result_snippet).  A stand-alone program that tests/test_snippet_native.py builds with
 * AddressSanitizer and UndefinedBehaviorSanitizer; no GPU.  Every array is an exactly sized heap
 * block, so a read past an end is seen.  Prints "ok" and returns 0, or names the first failure.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"

#define CHECK(x)                                                 \
    do {                                                         \
        if (!(x)) {                                              \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                            \
        }                                                        \
    } while (0)

/* an exactly sized heap copy of n bytes (n == 0: a one-byte block that is never to be read) */
static void* heap(const void* p, size_t n) {
    void* q = malloc(n ? n : 1);
    if (q && n) memcpy(q, p, n);
    return q;
}

typedef struct {
    tfidf_result r;
    tfidf_corpus c;
    tfidf_queries q;
} fixture;

/* terms: sorted by "word\t"; docs and queries concatenated with their offsets */
static int make(fixture* f, const char* const* terms, uint32_t nterms, const char* docs, const uint64_t* doc_off,
                uint32_t ndocs, const char* queries, const uint64_t* q_off, uint32_t nq) {
    memset(f, 0, sizeof(*f));
    uint64_t at = 0, toff[16];
    char tb[256];
    for (uint32_t i = 0; i < nterms; ++i) {
        toff[i] = at;
        memcpy(tb + at, terms[i], strlen(terms[i]));
        at += strlen(terms[i]);
    }
    toff[nterms] = at;
    f->r.nterms = nterms;
    f->r.term_off = (uint64_t*)heap(toff, ((size_t)nterms + 1) * 8);
    f->r.term_bytes = (uint8_t*)heap(tb, (size_t)at);
    f->c.nbytes = ndocs ? doc_off[ndocs] : 0;
    f->c.bytes = (const uint8_t*)heap(docs, (size_t)f->c.nbytes);
    f->c.doc_off = (const uint64_t*)heap(doc_off, ((size_t)ndocs + 1) * 8);
    f->c.ndocs = ndocs;
    f->q.nbytes = q_off[nq];
    f->q.bytes = (const uint8_t*)heap(queries, (size_t)f->q.nbytes);
    f->q.q_off = (const uint64_t*)heap(q_off, ((size_t)nq + 1) * 8);
    f->q.nqueries = nq;
    return !(f->r.term_off && f->r.term_bytes && f->c.bytes && f->c.doc_off && f->q.bytes && f->q.q_off);
}
static void unmake(fixture* f) {
    free(f->r.term_off); free(f->r.term_bytes); free((void*)f->c.bytes); free((void*)f->c.doc_off);
    free((void*)f->q.bytes); free((void*)f->q.q_off);
}

int main(void) {
    tfidf_snippet_params pr;
    memset(&pr, 0, sizeof(pr));
    pr.size = sizeof(pr);
    pr.window = 4;
    pr.max_marks = 8;
    pr.flags = TFIDF_SNIP_TEXT;
    CHECK(tfidf_snippets_check(&pr) == TFIDF_OK && tfidf_snippets_check(NULL) == TFIDF_E_INVAL);
    tfidf_snippets s;
    fixture f;

    /* ---- a corpus whose last document ends with the buffer, its last token unterminated ---- */
    {
        const char* terms[] = {"a", "fox", "the", "wolf"};
        const char docs[] = "the fox" "" "a wolf the fox";
        const uint64_t doc_off[] = {0, 7, 7, 21};
        const char queries[] = "fox wolf" "nothere" "";
        const uint64_t q_off[] = {0, 8, 15, 15};
        CHECK(make(&f, terms, 4, docs, doc_off, 3, queries, q_off, 3) == 0);
        const uint32_t jq[] = {0, 0, 0, 1, 2, 0, 0}, jd[] = {3, 1, 2, 3, 3, 4, 0};
        uint32_t* hq = (uint32_t*)heap(jq, sizeof(jq));
        uint32_t* hd = (uint32_t*)heap(jd, sizeof(jd));
        CHECK(hq && hd);
        CHECK(tfidf_result_snippet(&f.r, &f.c, &f.q, hq, hd, 7, &pr, &s) == TFIDF_OK);
        CHECK(s.njobs == 7 && s.nqueries == 3);
        CHECK(s.ntokens[0] == 4 && s.nmatch[0] == 2 && s.cover[0] == 2 && s.hits[0] == 2);
        CHECK(s.win_tok[0] == 1 && s.win_tok[1] == 4 && s.win_byte[0] == 2 && s.win_byte[1] == 14);   /* e' = T: the length */
        CHECK(s.mark_off[1] - s.mark_off[0] == 2 && s.mark_byte[1] == 11 && s.mark_len[1] == 3 && s.mark_slot[1] == 0);
        CHECK(s.text_off[1] - s.text_off[0] == 12 && memcmp(s.text, "wolf the fox", 12) == 0);
        CHECK(s.ntokens[1] == 2 && s.nmatch[1] == 1 && s.win_byte[3] == 7);
        CHECK(s.flags[2] == 0 && s.ntokens[2] == 0 && s.win_tok[5] == 0 && s.win_byte[5] == 0);      /* the empty document */
        CHECK(s.nmatch[3] == 0 && s.cover[3] == 0 && s.win_tok[7] == 4 && s.nmatch[4] == 0);           /* no found term, no term */
        CHECK(s.flags[5] == TFIDF_SNIP_NO_DOC && s.flags[6] == TFIDF_SNIP_NO_DOC && s.ntokens[5] == 0);
        CHECK(s.qterm_off[1] == 2 && s.qterm_off[2] == 3 && s.qterm_off[3] == 3);
        CHECK(s.qterm_found[0] == 1 && s.qterm_found[1] == 1 && s.qterm_found[2] == 0);
        tfidf_snippets_free(&s);
        /* zero jobs, with and without arrays */
        CHECK(tfidf_result_snippet(&f.r, &f.c, &f.q, NULL, NULL, 0, &pr, &s) == TFIDF_OK && s.njobs == 0 && s.mark_off[0] == 0);
        tfidf_snippets_free(&s);
        CHECK(tfidf_result_snippet(&f.r, &f.c, &f.q, hq, hd, 0, &pr, &s) == TFIDF_OK);
        tfidf_snippets_free(&s);
        /* a query index out of range, arrays missing, bad parameters: *out zeroed */
        hq[3] = 3;
        CHECK(tfidf_result_snippet(&f.r, &f.c, &f.q, hq, hd, 7, &pr, &s) == TFIDF_E_INVAL && s.flags == NULL);
        CHECK(tfidf_result_snippet(&f.r, &f.c, &f.q, hq, hd, 3, &pr, &s) == TFIDF_OK);
        tfidf_snippets_free(&s);
        CHECK(tfidf_result_snippet(&f.r, &f.c, &f.q, NULL, hd, 3, &pr, &s) == TFIDF_E_INVAL);
        CHECK(tfidf_result_snippet(&f.r, &f.c, &f.q, hq, hd, TFIDF_SNIP_MAX_JOBS + 1, &pr, &s) == TFIDF_E_INVAL);
        pr.window = 0;
        CHECK(tfidf_result_snippet(&f.r, &f.c, &f.q, hq, hd, 3, &pr, &s) == TFIDF_E_INVAL);
        pr.window = 1;
        pr.max_marks = 0;
        pr.flags = 0;
        CHECK(tfidf_result_snippet(&f.r, &f.c, &f.q, hq, hd, 3, &pr, &s) == TFIDF_OK);
        CHECK(s.mark_off[3] == 0 && s.text_off[3] == 0 && s.hits[0] == 1 && s.win_tok[0] == 1 && s.win_tok[1] == 2);
        tfidf_snippets_free(&s);
        tfidf_snippets_free(&s);   /* twice is harmless */
        pr.window = 4;
        pr.max_marks = 8;
        pr.flags = TFIDF_SNIP_TEXT;
        free(hq);
        free(hd);
        unmake(&f);
    }

    /* ---- an empty corpus and an empty vocabulary ---- */
    {
        const uint64_t doc_off[] = {0}, q_off[] = {0, 3};
        CHECK(make(&f, NULL, 0, "", doc_off, 0, "fox", q_off, 1) == 0);
        const uint32_t jq[] = {0}, jd[] = {1};
        CHECK(tfidf_result_snippet(&f.r, &f.c, &f.q, jq, jd, 1, &pr, &s) == TFIDF_OK);
        CHECK(s.flags[0] == TFIDF_SNIP_NO_DOC && s.qterm_found[0] == 0 && s.qterm_len[0] == 3);
        tfidf_snippets_free(&s);
        unmake(&f);
    }

    /* ---- NUL: a token's term ends at its first NUL; a token beginning with NUL has the empty term ---- */
    {
        const char* terms[] = {"", "fox"};
        const char docs[] = "fox\0abc \0x fox";
        const uint64_t doc_off[] = {0, 14};
        const char queries[] = "\0 fox\0z";
        const uint64_t q_off[] = {0, 7};
        CHECK(make(&f, terms, 2, docs, doc_off, 1, queries, q_off, 1) == 0);
        const uint32_t jq[] = {0}, jd[] = {1};
        CHECK(tfidf_result_snippet(&f.r, &f.c, &f.q, jq, jd, 1, &pr, &s) == TFIDF_OK);
        CHECK(s.ntokens[0] == 3 && s.nmatch[0] == 3 && s.nterms_matched[0] == 2 && s.qterm_len[0] == 0 && s.qterm_len[1] == 3);
        CHECK(s.mark_len[0] == 3 && s.mark_slot[0] == 1 && s.mark_len[1] == 0 && s.mark_slot[1] == 0 && s.mark_byte[1] == 8);
        tfidf_snippets_free(&s);
        unmake(&f);
    }
    printf("ok\n");
    return 0;
}
