/*
 * prune_host_test.c — tfidf_prune_check and tfidf_model_prune (csrc/prune_host.c) on edge
 * inputs, as a stand-alone program: built with -fsanitize=address,undefined by
 * tests/test_prune_native.py, so every read and write of the host functions is checked.  The
 * models live in exact-size heap blocks: a read past an array is a report.  Links prune_host.c
 * and model_io.c (tfidf_model_check, tfidf_model_free).  Exit status 0: every case passed.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"

static int g_fail = 0;

static tfidf_prune_params make(uint32_t min_df, uint32_t max_df, uint32_t max_features) {
    tfidf_prune_params p;
    memset(&p, 0, sizeof(p));
    p.size = sizeof(p);
    p.min_df = min_df;
    p.max_df = max_df;
    p.max_features = max_features;
    return p;
}

/* a model over `n` words in exact-size blocks; term_off starts at `base` to show that the
 * function does not assume 0 (the bytes in front are never a term's) */
static tfidf_model build(const char* const* words, const uint32_t* df, uint32_t n, uint64_t N, uint64_t base) {
    tfidf_model m;
    memset(&m, 0, sizeof(m));
    m.size = sizeof(m);
    m.ndocs_total = N;
    m.nterms = n;
    size_t total = (size_t)base;
    for (uint32_t i = 0; i < n; ++i) total += strlen(words[i]);
    m.term_off = (uint64_t*)malloc(((size_t)n + 1) * 8);
    m.term_df = (uint32_t*)malloc(n ? (size_t)n * 4 : 1);
    m.term_bytes = (uint8_t*)malloc(total ? total : 1);
    memset(m.term_bytes, 'X', (size_t)base);
    size_t at = (size_t)base;
    for (uint32_t i = 0; i < n; ++i) {
        m.term_off[i] = at;
        memcpy(m.term_bytes + at, words[i], strlen(words[i]));
        at += strlen(words[i]);
        m.term_df[i] = df[i];
    }
    m.term_off[n] = at;
    return m;
}

static void expect(const char* name, const tfidf_model* in, tfidf_prune_params p, const char* want /* kept words joined by ',' */) {
    tfidf_model out;
    memset(&out, 0x5A, sizeof(out));
    const int rc = tfidf_model_prune(in, &p, &out);
    char got[4096];
    size_t g = 0;
    int ok = rc == 0 && tfidf_model_check(&out) == 0 && out.ndocs_total == in->ndocs_total;
    for (uint32_t t = 0; ok && t < out.nterms; ++t) {
        const uint64_t a = out.term_off[t], b = out.term_off[t + 1];
        if (t) got[g++] = ',';
        memcpy(got + g, out.term_bytes + a, (size_t)(b - a));
        g += (size_t)(b - a);
    }
    got[g] = 0;
    ok = ok && strcmp(got, want) == 0 && (out.nterms == 0 || out.term_off[0] == 0);
    /* the kept df are the input's */
    for (uint32_t t = 0, s = 0; ok && t < out.nterms; ++t) {
        const uint64_t len = out.term_off[t + 1] - out.term_off[t];
        while (s < in->nterms && !(in->term_off[s + 1] - in->term_off[s] == len &&
                                   memcmp(in->term_bytes + in->term_off[s], out.term_bytes + out.term_off[t], (size_t)len) == 0))
            ++s;
        ok = s < in->nterms && in->term_df[s] == out.term_df[t];
    }
    if (!ok) { printf("FAIL %s (rc %d, got \"%s\", want \"%s\")\n", name, rc, rc == 0 ? got : "", want); ++g_fail; }
    tfidf_model_free(&out);
}

static void expect_rc(const char* name, int rc, int want) {
    if (rc != want) { printf("FAIL %s (rc %d, want %d)\n", name, rc, want); ++g_fail; }
}

int main(void) {
    /* ---- tfidf_prune_check: every rejecting case ---- */
    tfidf_prune_params p = make(2, 0, 0);
    expect_rc("check ok", tfidf_prune_check(&p), TFIDF_OK);
    expect_rc("check NULL", tfidf_prune_check(NULL), TFIDF_E_INVAL);
    p.size = sizeof(p) - 1;
    expect_rc("check short size", tfidf_prune_check(&p), TFIDF_E_INVAL);
    p = make(2, 0, 0);
    p.reserved = 7;
    expect_rc("check reserved", tfidf_prune_check(&p), TFIDF_E_INVAL);
    p = make(3, 2, 0);
    expect_rc("check min > max", tfidf_prune_check(&p), TFIDF_E_INVAL);
    p = make(3, 3, 0);
    expect_rc("check min == max", tfidf_prune_check(&p), TFIDF_OK);
    p = make(9, 0, 0);
    expect_rc("check max 0 is no bound", tfidf_prune_check(&p), TFIDF_OK);

    /* ---- tfidf_model_prune ---- */
    /* strcmp("word\t") order: "" < "ab\x01" < "ab" < "b" < "b!" ... kept simple: ascending bytes, no prefix pairs but one */
    const char* words[] = {"", "ab\x01", "ab", "c", "d", "e", "\x80\xff", "\xc3\xa9"};
    const uint32_t df[] = {1, 2, 5, 5, 5, 1, 3, 5};
    tfidf_model m = build(words, df, 8, 6, 0);
    expect_rc("fixture is a model", tfidf_model_check(&m), TFIDF_OK);
    expect("identity", &m, make(0, 0, 0), ",ab\x01,ab,c,d,e,\x80\xff,\xc3\xa9");
    expect("min_df 1 is no bound", &m, make(1, 0, 0), ",ab\x01,ab,c,d,e,\x80\xff,\xc3\xa9");
    expect("min_df 2", &m, make(2, 0, 0), "ab\x01,ab,c,d,\x80\xff,\xc3\xa9");
    expect("max_df 3", &m, make(0, 3, 0), ",ab\x01,e,\x80\xff");
    expect("range 2..3", &m, make(2, 3, 0), "ab\x01,\x80\xff");
    expect("nothing left", &m, make(6, 0, 0), "");
    /* ties at the cut: four terms of df 5, the lowest ranks win; the output keeps term order */
    expect("M 1", &m, make(0, 0, 1), "ab");
    expect("M 3", &m, make(0, 0, 3), "ab,c,d");
    expect("M 4", &m, make(0, 0, 4), "ab,c,d,\xc3\xa9");
    expect("M 5", &m, make(0, 0, 5), "ab,c,d,\x80\xff,\xc3\xa9");
    expect("M V-1", &m, make(0, 0, 7), ",ab\x01,ab,c,d,\x80\xff,\xc3\xa9");   /* df 1: "" before "e" by rank, so "e" goes */
    expect("M V", &m, make(0, 0, 8), ",ab\x01,ab,c,d,e,\x80\xff,\xc3\xa9");
    expect("M V+1", &m, make(0, 0, 9), ",ab\x01,ab,c,d,e,\x80\xff,\xc3\xa9");
    expect("range then cut", &m, make(0, 3, 2), "ab\x01,\x80\xff");
    {   /* errors zero *out */
        tfidf_model out;
        memset(&out, 0x5A, sizeof(out));
        tfidf_prune_params bad = make(3, 2, 0);
        expect_rc("bad params", tfidf_model_prune(&m, &bad, &out), TFIDF_E_INVAL);
        if (out.term_off || out.term_bytes || out.term_df || out.nterms) { printf("FAIL out not zeroed\n"); ++g_fail; }
        tfidf_prune_params okp = make(2, 0, 0);
        expect_rc("NULL model", tfidf_model_prune(NULL, &okp, &out), TFIDF_E_INVAL);
        expect_rc("NULL params", tfidf_model_prune(&m, NULL, &out), TFIDF_E_INVAL);
        expect_rc("NULL out", tfidf_model_prune(&m, &okp, NULL), TFIDF_E_INVAL);
    }
    tfidf_model_free(&m);
    {   /* offsets that do not start at 0, and the empty model */
        const char* w2[] = {"aa", "bb", "cc"};
        const uint32_t d2[] = {2, 1, 2};
        tfidf_model m2 = build(w2, d2, 3, 2, 5);
        expect("based offsets", &m2, make(2, 0, 0), "aa,cc");
        expect("based offsets cut", &m2, make(0, 0, 1), "aa");
        tfidf_model_free(&m2);
        tfidf_model m0 = build(w2, d2, 0, 3, 0);
        expect("empty model", &m0, make(2, 0, 1), "");
        tfidf_model_free(&m0);
    }
    {   /* many equal df: M in the middle of one long tie */
        enum { NW = 300 };
        char* store = (char*)malloc(NW * 6);
        const char* w3[NW];
        uint32_t d3[NW];
        for (int i = 0; i < NW; ++i) {
            snprintf(store + i * 6, 6, "t%03d", i);
            w3[i] = store + i * 6;
            d3[i] = 4;
        }
        tfidf_model m3 = build(w3, d3, NW, 9, 0);
        tfidf_model out;
        tfidf_prune_params c = make(0, 0, 123);
        int rc = tfidf_model_prune(&m3, &c, &out);
        int ok = rc == 0 && out.nterms == 123;
        for (uint32_t t = 0; ok && t < out.nterms; ++t)
            ok = out.term_off[t + 1] - out.term_off[t] == 4 && memcmp(out.term_bytes + out.term_off[t], w3[t], 4) == 0;
        if (!ok) { printf("FAIL long tie (rc %d)\n", rc); ++g_fail; }
        tfidf_model_free(&out);
        tfidf_model_free(&m3);
        free(store);
    }
    if (g_fail) { printf("%d case(s) failed\n", g_fail); return 1; }
    printf("ok\n");
    return 0;
}
