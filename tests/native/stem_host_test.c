/*
 * stem_host_test.c — the host stemmer tfidf_stem_porter and tfidf_analyze_host with a stemmer
 * (csrc/analyze_host.c) on edge inputs, and the kernel's bit-mask form of the stemmer
 * (csrc/analyze_stem.h, plain C as well) against the byte-wise one, as a stand-alone program:
 * built with -fsanitize=address,undefined by tests/test_stem_native.py.  Links only
 * analyze_host.c.  Exit status 0: every case passed.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"
#include "../../parallel-systems-mpi-tfidf_amd/csrc/analyze_stem.h"

static int g_fail = 0;
static unsigned long g_words = 0;

static void fail(const char* what, const char* w) {
    if (g_fail < 20) printf("FAIL %s: %s\n", what, w);
    ++g_fail;
}

/* the host stemmer on an exact-size heap copy (a write past the word is a report) */
static uint32_t host_stem(const char* w, uint32_t n, char* out) {
    uint8_t* b = (uint8_t*)malloc(n ? n : 1);
    memcpy(b, w, n);
    const int s = tfidf_stem_porter(b, n);
    if (s < 1 || (uint32_t)s > n) { fail("stem length", w); free(b); return 0; }
    if (memcmp(b + s, w + s, n - (uint32_t)s) != 0) fail("bytes behind the stem written", w);
    memcpy(out, b, (size_t)s);
    out[s] = 0;
    free(b);
    return (uint32_t)s;
}

static void expect_stem(const char* w, const char* want) {
    char got[80];
    host_stem(w, (uint32_t)strlen(w), got);
    if (strcmp(got, want) != 0) { printf("FAIL %s -> %s, want %s\n", w, got, want); ++g_fail; }
}

/* the mask form on the word at every byte shift, between letters that are not its own, against
 * the host stemmer: the same length, and the same bytes once the tail is applied */
static void cross(const char* w, uint32_t n) {
    char want[80];
    const uint32_t s = host_stem(w, n, want);
    ++g_words;
    for (uint32_t shift = 0; shift < 4u; ++shift) {
        uint32_t aw[24];
        uint8_t* b = (uint8_t*)aw;
        memset(b, 's', sizeof(aw));   /* neighbours that would extend a suffix */
        memcpy(b + 8 + shift, w, n);
        uint64_t tail = 0;
        const uint32_t got = an_stem(aw + 2, shift, n, &tail);
        if (got != s) { fail("mask form: length", w); return; }
        char r[80];
        memcpy(r, w, n);
        for (uint32_t j = 0; j < 8u && j < got; ++j) r[got - 1u - j] = (char)(tail >> (56u - 8u * j));
        if (memcmp(r, want, s) != 0) { fail("mask form: bytes", w); return; }
    }
}

static const char* STEMS[] = {"a",   "b",    "tr",   "y",    "ay",   "by",    "oat", "be",  "ee",   "hop",  "fil", "fail", "fizz",
                              "hiss", "fall", "contr", "abl", "siz",  "yy",   "eye", "troubl", "conflat", "agr", "sens", "ration", "gener"};
static const char* SUFFIXES[] = {"sses", "ies", "ss", "s", "eed", "ed", "ing", "at", "bl", "iz", "ational", "tional", "enci", "anci",
                                 "izer", "abli", "alli", "entli", "eli", "ousli", "ization", "ation", "ator", "alism", "iveness",
                                 "fulness", "ousness", "aliti", "iviti", "biliti", "icate", "ative", "alize", "iciti", "ical", "ful",
                                 "ness", "al", "ance", "ence", "er", "ic", "able", "ible", "ant", "ement", "ment", "ent", "ion", "ou",
                                 "ism", "ate", "iti", "ous", "ive", "ize", "e", "ll", "y", "es", "ying", "pping", "ated", "bled", "ized",
                                 "sion", "tion", "l", "i"};
#define COUNT(a) (sizeof(a) / sizeof((a)[0]))

static tfidf_analyzer make(uint32_t flags, uint32_t min_len, const char* stop, uint32_t stemmer, uint64_t so[2]) {
    tfidf_analyzer a;
    memset(&a, 0, sizeof(a));
    a.size = sizeof(a);
    a.flags = flags;
    a.min_len = min_len;
    a.stemmer = stemmer;
    if (stop) {
        so[0] = 0;
        so[1] = strlen(stop);
        a.stop_bytes = (const uint8_t*)stop;
        a.stop_off = so;
        a.nstop = 1;
    }
    return a;
}

/* out of place and in place, both in exact-size heap blocks */
static void expect(const char* name, uint32_t flags, uint32_t min_len, const char* stop, const char* in, size_t n,
                   const uint64_t* off, uint32_t nd, const char* want) {
    uint64_t so[2];
    const tfidf_analyzer a = make(flags, min_len, stop, TFIDF_STEM_PORTER, so);
    uint8_t *src = (uint8_t*)malloc(n ? n : 1), *out = (uint8_t*)malloc(n ? n : 1);
    memcpy(src, in, n);
    int rc = tfidf_analyze_host(&a, src, n, off, nd, out);
    int ok = rc == 0 && memcmp(out, want, n) == 0;
    rc = tfidf_analyze_host(&a, src, n, off, nd, src);
    ok = ok && rc == 0 && memcmp(src, want, n) == 0;
    if (!ok) { printf("FAIL %s\n", name); ++g_fail; }
    free(src); free(out);
}

int main(void) {
    /* whole words */
    static const char* pairs[][2] = {
        {"generalizations", "gener"}, {"oscillators", "oscil"}, {"relational", "relat"}, {"running", "run"}, {"agreed", "agre"},
        {"conflated", "conflat"}, {"controlling", "control"}, {"rolling", "roll"}, {"abilities", "abil"},
        {"sensibilities", "sensibl"}, {"internationalization", "internation"}, {"connection", "connect"},
        {"connections", "connect"}, {"connected", "connect"}, {"connecting", "connect"}, {"connective", "connect"},
        {"was", "wa"}, {"this", "thi"}, {"say", "sai"}, {"yes", "ye"}, {"yyy", "yyi"}, {"ies", "i"}, {"sses", "ss"},
        {"ing", "ing"}, {"eed", "eed"}, {"as", "as"}, {"is", "is"}, {"feed", "feed"}, {"happy", "happi"}, {"sky", "sky"},
        {"hopping", "hop"}, {"filing", "file"}, {"cement", "cement"}, {"adoption", "adopt"}, {"onion", "onion"},
        {"Running", "Running"}, {"runn1ng", "runn1ng"}, {"caf\xc3\xa9s", "caf\xc3\xa9s"}};
    for (size_t i = 0; i < COUNT(pairs); ++i) expect_stem(pairs[i][0], pairs[i][1]);
    {   /* ineligible lengths, NULL */
        char w[66];
        memset(w, 'a', 65);
        memcpy(w + 62, "ing", 3);
        uint8_t* b = (uint8_t*)malloc(65);
        memcpy(b, w, 65);
        if (tfidf_stem_porter(b, 65) != 65 || memcmp(b, w, 65) != 0) fail("65 bytes", "unchanged");
        memcpy(b + 61, "ing", 3);
        if (tfidf_stem_porter(b, 64) != 61) fail("64 bytes", "aaa...ing");
        free(b);
        if (tfidf_stem_porter(NULL, 3) != TFIDF_E_INVAL || tfidf_stem_porter(NULL, 0) != 0) fail("NULL", "");
        uint8_t two[2] = {'e', 'd'};
        if (tfidf_stem_porter(two, 2) != 2 || tfidf_stem_porter(two, 1) != 1 || tfidf_stem_porter(two, 0) != 0) fail("short", "ed");
    }
    /* the mask form against the byte-wise one: every word of 3..6 letters over 8 letters, and
     * stems x suffixes x suffixes */
    {
        static const char alpha[8] = {'a', 'e', 'y', 's', 'l', 't', 'i', 'd'};
        char w[8];
        for (uint32_t n = 3; n <= 6; ++n) {
            uint32_t total = 1;
            for (uint32_t k = 0; k < n; ++k) total *= 8u;
            for (uint32_t x = 0; x < total; ++x) {
                for (uint32_t k = 0, v = x; k < n; ++k, v >>= 3) w[k] = alpha[v & 7u];
                w[n] = 0;
                cross(w, n);
            }
        }
        char buf[80];
        for (size_t a = 0; a < COUNT(STEMS); ++a)
            for (size_t b = 0; b < COUNT(SUFFIXES); ++b) {
                snprintf(buf, sizeof(buf), "%s%s", STEMS[a], SUFFIXES[b]);
                cross(buf, (uint32_t)strlen(buf));
                for (size_t c = 0; c < COUNT(SUFFIXES); ++c) {
                    snprintf(buf, sizeof(buf), "%s%s%s", STEMS[a], SUFFIXES[b], SUFFIXES[c]);
                    cross(buf, (uint32_t)strlen(buf));
                }
            }
        /* long words: the tail's refill from the original letters, up to 64 bytes */
        for (uint32_t n = 40; n <= 64; ++n)
            for (size_t b = 0; b < COUNT(SUFFIXES); ++b)
                for (size_t c = 0; c < COUNT(SUFFIXES); ++c) {
                    const uint32_t sl = (uint32_t)(strlen(SUFFIXES[b]) + strlen(SUFFIXES[c]));
                    for (uint32_t k = 0; k + sl < n; ++k) buf[k] = "abetyoil"[(k * 5u + n) & 7u];
                    snprintf(buf + n - sl, sizeof(buf) - (n - sl), "%s%s", SUFFIXES[b], SUFFIXES[c]);
                    cross(buf, n);
                }
    }
    /* tfidf_analyze_host with a stemmer */
    {
        const uint32_t L = TFIDF_AN_LOWER, P = TFIDF_AN_PUNCT;
        const uint64_t o1[2] = {0, 32};
        expect("words", 0, 0, NULL, "running as is ing relational sky", 32, o1, 1, "run     as is ing relat      sky");
        const uint64_t o2[2] = {0, 28};
        expect("ineligible", 0, 0, NULL, "Running runn1ng caf\xc3\xa9s b\0ing", 28, o2, 1, "Running runn1ng caf\xc3\xa9s b\0ing");
        expect("lower first", L | P, 0, NULL, "Running runn1ng caf\xc3\xa9s b\0ing", 28, o2, 1, "run     runn1ng caf\xc3\xa9s b ing");
        const uint64_t o3[2] = {0, 11};
        expect("running listed", 0, 0, "running", "running run", 11, o3, 1, "        run");
        expect("run listed", 0, 0, "run", "running run", 11, o3, 1, "run        ");
        expect("min_len sees the word", 0, 4, NULL, "running run", 11, o3, 1, "run        ");
        const uint64_t o4[3] = {0, 4, 7};
        expect("a boundary inside", 0, 0, NULL, "running", 7, o4, 2, "running");
        const uint64_t o5[2] = {3, 10};
        expect("window", 0, 0, NULL, "ed running ed", 13, o5, 1, "ed run     ed");
        char in[200], want[200];
        for (uint32_t n = 64; n <= 65; ++n) {   /* 64 letters are stemmed, 65 are not */
            memset(in, 'a', n);
            in[0] = 'b';
            memcpy(in + n - 3, "ing", 3);
            memcpy(want, in, n);
            if (n == 64) memset(want + n - 3, ' ', 3);
            const uint64_t o[2] = {0, n};
            expect("64 and 65", 0, 0, NULL, in, n, o, 1, want);
        }
        uint64_t so[2];
        tfidf_analyzer a = make(0, 0, NULL, 2u, so);
        if (tfidf_analyzer_check(&a) != TFIDF_E_INVAL) fail("check", "stemmer 2");
        a.stemmer = TFIDF_STEM_PORTER;
        if (tfidf_analyzer_check(&a) != TFIDF_OK) fail("check", "stemmer 1");
    }
    printf("%lu words crossed\n%s\n", g_words, g_fail ? "failed" : "ok");
    return g_fail ? 1 : 0;
}
