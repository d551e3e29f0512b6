/*
 * nb_host_test — the labels-file parser of the CLI (host/labels_file.h) and the host Naive Bayes
 * functions (csrc/nb_host.c) on edge inputs, as a stand-alone program for the sanitizers
 * (tests/test_nb_native.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer).
 * No GPU.  Prints "ok" and exits 0, or names the first failed check.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"
#include "../../parallel-systems-mpi-tfidf_amd/host/labels_file.h"

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

static int parse(const char* s, size_t n, labels_file* l, size_t* bad) { return labels_parse((const uint8_t*)s, n, l, bad); }
#define PARSE(s, l, bad) parse(s, sizeof(s) - 1, l, bad)

static int labels_tests(void) {
    labels_file l;
    size_t bad = 99;
    /* names to classes in byte order: upper case before lower, a prefix before the longer name */
    CHECK(PARSE("doc3\tsport\ndoc1\tarts\ndoc12\tSport\ndoc7\tart\ndoc4294967295\tsport", &l, &bad) == 0);
    CHECK(bad == 0 && l.n == 5 && l.k == 4);
    CHECK(!strcmp(l.name[0], "Sport") && !strcmp(l.name[1], "art") && !strcmp(l.name[2], "arts") && !strcmp(l.name[3], "sport"));
    CHECK(l.doc[0] == 3 && l.doc[1] == 1 && l.doc[2] == 12 && l.doc[3] == 7 && l.doc[4] == 4294967295u);
    CHECK(l.label[0] == 3 && l.label[1] == 2 && l.label[2] == 0 && l.label[3] == 1 && l.label[4] == 3);
    labels_free(&l);
    CHECK(l.n == 0 && l.name == NULL);
    labels_free(&l);   /* twice, and a zeroed struct */
    /* a name may hold spaces and bytes above 0x7F; they sort as unsigned bytes */
    CHECK(PARSE("doc1\t\xC3\xA9t\xC3\xA9\ndoc2\tz z\n", &l, &bad) == 0);
    CHECK(l.k == 2 && !strcmp(l.name[0], "z z") && l.label[0] == 1 && l.label[1] == 0);
    labels_free(&l);
    /* bad lines, each refused with its number */
    static const struct { const char* s; size_t n, line; } BAD[] = {
        {"doc1 arts\n", 10, 1},                 /* no tab */
        {"doc1\tarts\ndoc2\t\n", 16, 2},        /* an empty name */
        {"doc0\tarts\n", 10, 1},                /* ids start at 1 */
        {"doc01\tarts\n", 11, 1},               /* a leading zero */
        {"doc4294967296\tarts\n", 19, 1},       /* past 32 bits */
        {"doc99999999999999999999\ta\n", 26, 1},
        {"dox1\tarts\n", 10, 1},
        {"1\tarts\n", 7, 1},
        {"doc+1\tarts\n", 11, 1},
        {"doc1\tarts\n\ndoc2\tb\n", 18, 2},     /* an empty line */
        {"doc1\tarts\n\n", 11, 2},
        {"doc1\ta\tb\n", 9, 1},                 /* a tab in the name */
        {"doc1\ta\0b\n", 9, 1},                 /* a NUL in the name */
        {"doc1\t", 5, 1},
        {"doc", 3, 1},
        {"doc1\tok\ndoc2", 12, 2},
    };
    for (size_t i = 0; i < sizeof(BAD) / sizeof(BAD[0]); ++i) {
        bad = 0;
        if (parse(BAD[i].s, BAD[i].n, &l, &bad) == 0 || bad != BAD[i].line || l.doc || l.name) {
            printf("FAILED bad labels case %zu: line %zu\n", i, bad);
            return 1;
        }
    }
    CHECK(parse("", 0, &l, &bad) != 0 && bad == 0);   /* no line */
    /* 256 classes are taken, 257 are not */
    char* big = (char*)malloc(257 * 16);
    size_t n = 0;
    for (int i = 0; i < 257; ++i) {
        if (i == 256) {
            CHECK(parse(big, n, &l, &bad) == 0 && l.k == 256 && l.n == 256);
            CHECK(!strcmp(l.name[0], "c000") && !strcmp(l.name[255], "c255") && l.label[255] == 255);
            labels_free(&l);
        }
        n += (size_t)sprintf(big + n, "doc%d\tc%03d\n", i + 1, i);
    }
    CHECK(parse(big, n, &l, &bad) != 0 && bad == 0 && !l.doc);
    free(big);
    return 0;
}

static int nb_tests(void) {
    /* "a a b" in class 0, "b c" in class 1, "a c c" and an empty document unlabelled */
    uint32_t pair_doc[] = {1, 1, 2, 2, 3, 3}, pair_term[] = {0, 1, 1, 2, 0, 2}, pair_count[] = {2, 1, 1, 1, 1, 2};
    uint32_t doc_id[] = {1, 2, 3, 4};
    tfidf_result r;
    memset(&r, 0, sizeof(r));
    r.npairs = 6; r.ndocs = 4; r.nterms = 3;
    r.pair_doc = pair_doc; r.pair_term = pair_term; r.pair_count = pair_count; r.doc_id = doc_id;
    uint32_t docs[] = {1, 2}, labels[] = {0, 1};
    tfidf_nb_params p;
    memset(&p, 0, sizeof(p));
    p.size = sizeof(p);
    p.nclasses = 2; p.nlabelled = 2; p.doc = docs; p.label = labels;
    CHECK(tfidf_nb_check(&p) == TFIDF_OK);
    tfidf_nb_model m;
    CHECK(tfidf_result_nb_fit(&r, &p, &m) == TFIDF_OK);
    CHECK(m.nclasses == 2 && m.nterms == 3 && m.nlabelled == 2 && m.alpha == 1.0);
    CHECK(m.feature_count[0] == 2 && m.feature_count[1] == 0 && m.feature_count[5] == 1);
    CHECK(m.class_total[0] == 3 && m.class_total[1] == 2 && m.class_docs[0] == 1);
    const double w00 = log(3.0) - log(6.0);
    CHECK(m.weight[0] == w00 && m.prior[0] == log(1.0) - log(2.0));
    /* rows: the two unlabelled documents, an offset table that starts past 0 */
    uint64_t row_off[] = {4, 6, 6};
    tfidf_nb_labels out;
    CHECK(tfidf_nb_model_predict(&m, 2, row_off, pair_term, pair_count, TFIDF_NB_ALL_SCORES, &out) == TFIDF_OK);
    CHECK(out.ndocs == 2 && out.nclasses == 2 && out.label[0] == 1 && out.scores && out.score[0] == out.scores[1]);
    CHECK(out.label[1] == 0 && out.score[1] == m.prior[0] && out.scores[2] == m.prior[0] && out.scores[3] == m.prior[1]);
    tfidf_nb_labels_free(&out);
    CHECK(tfidf_nb_model_predict(&m, 0, NULL, NULL, NULL, 0, &out) == TFIDF_OK && out.ndocs == 0 && !out.scores);
    tfidf_nb_labels_free(&out);
    tfidf_nb_labels_free(&out);
    CHECK(tfidf_nb_model_predict(&m, 2, row_off, pair_term, pair_count, 2u, &out) == TFIDF_E_INVAL);   /* an unknown flag */
    uint64_t back[] = {2, 1};
    CHECK(tfidf_nb_model_predict(&m, 1, back, pair_term, pair_count, 0, &out) == TFIDF_E_INVAL && !out.label);
    uint32_t far_term[] = {3};
    uint64_t one[] = {0, 1};
    CHECK(tfidf_nb_model_predict(&m, 1, one, far_term, pair_count, 0, &out) == TFIDF_E_INVAL);
    CHECK(tfidf_nb_model_predict(NULL, 1, one, pair_term, pair_count, 0, &out) == TFIDF_E_INVAL);
    tfidf_nb_model_free(&m);
    CHECK(!m.weight && m.nclasses == 0);
    tfidf_nb_model_free(&m);
    tfidf_nb_model_free(NULL);
    tfidf_nb_labels_free(NULL);
    /* the largest and smallest alpha, the complement with one class, binary features */
    p.variant = TFIDF_NB_COMPLEMENT; p.alpha = 0x1p+900; p.feature = TFIDF_NB_BINARY;
    uint32_t one_class[] = {0, 0};
    p.nclasses = 1; p.label = one_class;
    CHECK(tfidf_result_nb_fit(&r, &p, &m) == TFIDF_OK);
    for (int i = 0; i < 3; ++i) CHECK(isfinite(m.weight[i]));
    CHECK(m.prior[0] == 0.0 && m.feature_count[0] == 1);
    tfidf_nb_model_free(&m);
    p.alpha = 0x1p-1074; p.variant = TFIDF_NB_MULTINOMIAL;
    CHECK(tfidf_result_nb_fit(&r, &p, &m) == TFIDF_OK);
    for (int i = 0; i < 3; ++i) CHECK(isfinite(m.weight[i]));
    tfidf_nb_model_free(&m);
    /* refusals: *out zeroed */
    p.nclasses = 2; p.label = labels; p.alpha = 0;
    uint32_t far_doc[] = {1, 9};
    p.doc = far_doc;
    memset(&m, 0xAB, sizeof(m));
    CHECK(tfidf_result_nb_fit(&r, &p, &m) == TFIDF_E_INVAL && !m.weight && !m.size);
    p.doc = docs;
    pair_term[5] = 3;   /* a term outside the table */
    CHECK(tfidf_result_nb_fit(&r, &p, &m) == TFIDF_E_INVAL && !m.weight);
    pair_term[5] = 2;
    pair_doc[5] = 8;    /* a pair of a document that is not among doc_id */
    CHECK(tfidf_result_nb_fit(&r, &p, &m) == TFIDF_E_INVAL);
    pair_doc[5] = 3;
    CHECK(tfidf_result_nb_fit(NULL, &p, &m) == TFIDF_E_INVAL && tfidf_result_nb_fit(&r, NULL, &m) == TFIDF_E_INVAL);
    CHECK(tfidf_result_nb_fit(&r, &p, NULL) == TFIDF_E_INVAL);
    p.alpha = NAN;
    CHECK(tfidf_nb_check(&p) == TFIDF_E_INVAL);
    p.alpha = -0x1p-1074;
    CHECK(tfidf_nb_check(&p) == TFIDF_E_INVAL);
    p.alpha = 0;
    p.nlabelled = 0;
    CHECK(tfidf_nb_check(&p) == TFIDF_E_INVAL);   /* no class has a document */
    /* no pairs and no terms at all */
    memset(&r, 0, sizeof(r));
    r.ndocs = 2; r.doc_id = doc_id;
    p.nlabelled = 2;
    CHECK(tfidf_result_nb_fit(&r, &p, &m) == TFIDF_OK && m.nterms == 0);
    uint64_t empty_rows[] = {0, 0};
    CHECK(tfidf_nb_model_predict(&m, 1, empty_rows, NULL, NULL, TFIDF_NB_ALL_SCORES, &out) == TFIDF_OK);
    CHECK(out.label[0] == 0 && out.score[0] == m.prior[0]);
    tfidf_nb_labels_free(&out);
    tfidf_nb_model_free(&m);
    return 0;
}

int main(void) {
    if (labels_tests() || nb_tests()) return 1;
    printf("ok\n");
    return 0;
}
