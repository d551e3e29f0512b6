/* dedup_host.c on edge inputs, stand-alone (tests/test_dedup_native.py builds it with
 * AddressSanitizer and UndefinedBehaviorSanitizer): no documents, one document, all documents
 * empty, H = 1, H = 256, r = H, the parameter errors, the union-find.  Prints "ok". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

static tfidf_dedup_params params(uint32_t H, uint32_t r, uint64_t seed, double thr) {
    tfidf_dedup_params p;
    memset(&p, 0, sizeof p);
    p.size = sizeof p;
    p.nhashes = H;
    p.rows = r;
    p.seed = seed;
    p.threshold = thr;
    return p;
}

/* a result of ndocs documents (ids 1..ndocs) whose sets are rows of `sets` (term ranks ascending,
 * -1 ends a row) over a term table of single letters "a", "b", ... */
#define MAXT 8
typedef struct {
    tfidf_result r;
    uint32_t doc[64], term[64], ids[16];
    uint64_t toff[MAXT + 1];
    uint8_t tbytes[MAXT];
} fixture;

static void build(fixture* f, uint32_t ndocs, const int sets[][MAXT + 1]) {
    memset(f, 0, sizeof *f);
    uint64_t P = 0;
    /* output order is the "docN@" string order; with ids 1..9 it is the numeric order */
    for (uint32_t d = 0; d < ndocs; ++d) {
        f->ids[d] = d + 1;
        for (int k = 0; sets[d][k] >= 0; ++k) {
            f->doc[P] = d + 1;
            f->term[P] = (uint32_t)sets[d][k];
            ++P;
        }
    }
    for (uint32_t t = 0; t < MAXT; ++t) {
        f->toff[t] = t;
        f->tbytes[t] = (uint8_t)('a' + t);
    }
    f->toff[MAXT] = MAXT;
    f->r.npairs = P;
    f->r.ndocs = ndocs;
    f->r.nterms = MAXT;
    f->r.pair_doc = f->doc;
    f->r.pair_term = f->term;
    f->r.doc_id = f->ids;
    f->r.term_off = f->toff;
    f->r.term_bytes = f->tbytes;
}

int main(void) {
    tfidf_dups d;
    tfidf_signatures s;
    tfidf_dedup_params p = params(128, 4, 1, 0.5);
    fixture f;

    /* ---- parameter errors ---- */
    CHECK(tfidf_dedup_check(NULL) == TFIDF_E_INVAL);
    CHECK(tfidf_dedup_check(&p) == TFIDF_OK);
    { tfidf_dedup_params q = p; q.size = sizeof q - 1; CHECK(tfidf_dedup_check(&q) == TFIDF_E_INVAL); }
    { tfidf_dedup_params q = params(257, 1, 1, 0.5); CHECK(tfidf_dedup_check(&q) == TFIDF_E_INVAL); }
    { tfidf_dedup_params q = params(128, 0, 1, 0.5); CHECK(tfidf_dedup_check(&q) == TFIDF_E_INVAL); }
    { tfidf_dedup_params q = params(128, 5, 1, 0.5); CHECK(tfidf_dedup_check(&q) == TFIDF_E_INVAL); }
    { tfidf_dedup_params q = params(128, 4, 1, 1.5); CHECK(tfidf_dedup_check(&q) == TFIDF_E_INVAL); }
    { tfidf_dedup_params q = params(128, 4, 1, -0.5); CHECK(tfidf_dedup_check(&q) == TFIDF_E_INVAL); }
    { tfidf_dedup_params q = params(128, 4, 1, strtod("nan", NULL)); CHECK(tfidf_dedup_check(&q) == TFIDF_E_INVAL); }
    { tfidf_dedup_params q = params(0, 0, 0, 1.0); CHECK(tfidf_dedup_check(&q) == TFIDF_OK); }
    d.ndocs = 9;
    CHECK(tfidf_result_near_dups(NULL, &p, &d) == TFIDF_E_INVAL && d.ndocs == 0 && d.doc == NULL);
    CHECK(tfidf_result_near_dups(NULL, &p, NULL) == TFIDF_E_INVAL);
    CHECK(tfidf_result_minhash(NULL, &p, NULL) == TFIDF_E_INVAL);

    /* ---- no documents ---- */
    {
        static const int none[1][MAXT + 1] = {{-1}};
        build(&f, 0, none);
        f.r.doc_id = NULL;
        f.r.pair_doc = NULL;
        f.r.pair_term = NULL;
        CHECK(tfidf_result_near_dups(&f.r, &p, &d) == TFIDF_OK);
        CHECK(d.ndocs == 0 && d.ncand == 0 && d.nedges == 0 && d.ngroups == 0);
        tfidf_dups_free(&d);
        CHECK(tfidf_result_minhash(&f.r, &p, &s) == TFIDF_OK && s.ndocs == 0 && s.nhashes == 128);
        tfidf_signatures_free(&s);
        tfidf_result zero;
        memset(&zero, 0, sizeof zero);
        CHECK(tfidf_result_near_dups(&zero, &p, &d) == TFIDF_OK && d.ndocs == 0);
        tfidf_dups_free(&d);
    }
    /* ---- one document ---- */
    {
        static const int one[1][MAXT + 1] = {{0, 2, 5, -1}};
        build(&f, 1, one);
        CHECK(tfidf_result_near_dups(&f.r, &p, &d) == TFIDF_OK);
        CHECK(d.ndocs == 1 && d.ncand == 0 && d.nedges == 0 && d.ngroups == 0 && d.group[0] == 0 && d.doc[0] == 1);
        tfidf_dups_free(&d);
    }
    /* ---- all documents empty ---- */
    {
        static const int empty[3][MAXT + 1] = {{-1}, {-1}, {-1}};
        build(&f, 3, empty);
        CHECK(tfidf_result_near_dups(&f.r, &p, &d) == TFIDF_OK);
        CHECK(d.ndocs == 3 && d.ncand == 0 && d.ngroups == 0 && d.group[0] == 0 && d.group[1] == 1 && d.group[2] == 2);
        tfidf_dups_free(&d);
        CHECK(tfidf_result_minhash(&f.r, &p, &s) == TFIDF_OK);
        for (uint32_t i = 0; i < 3u * 128u; ++i) CHECK(s.sig[i] == 0xFFFFFFFFu);
        CHECK(s.npairs[0] == 0 && s.npairs[2] == 0);
        tfidf_signatures_free(&s);
    }
    /* ---- H = 1, H = 256, r = H on two equal documents, a different one and an empty one ---- */
    {
        static const int sets[4][MAXT + 1] = {{0, 1, 2, -1}, {-1}, {0, 1, 2, -1}, {5, 6, 7, -1}};
        static const uint32_t shapes[4][2] = {{1, 1}, {256, 1}, {256, 256}, {96, 96}};
        build(&f, 4, sets);
        for (int k = 0; k < 4; ++k) {
            tfidf_dedup_params q = params(shapes[k][0], shapes[k][1], 42, 1.0);
            CHECK(tfidf_result_near_dups(&f.r, &q, &d) == TFIDF_OK);
            CHECK(d.ndocs == 4 && d.nedges == 1 && d.ngroups == 1);
            CHECK(d.a_pos[0] == 0 && d.b_pos[0] == 2 && d.a_doc[0] == 1 && d.b_doc[0] == 3);
            CHECK(d.shared[0] == 3 && d.uni[0] == 3 && d.same[0] == shapes[k][0] && d.jaccard[0] == 1.0);
            CHECK(d.group[0] == 0 && d.group[1] == 1 && d.group[2] == 0 && d.group[3] == 3);
            tfidf_dups_free(&d);
            CHECK(tfidf_result_minhash(&f.r, &q, &s) == TFIDF_OK && s.nhashes == shapes[k][0]);
            CHECK(memcmp(s.sig, s.sig + 2u * s.nhashes, 4u * s.nhashes) == 0);
            CHECK(s.sig[s.nhashes] == 0xFFFFFFFFu && s.npairs[0] == 3 && s.npairs[1] == 0);
            tfidf_signatures_free(&s);
        }
    }
    /* ---- invalid results ---- */
    {
        static const int sets[2][MAXT + 1] = {{0, 1, -1}, {1, 2, -1}};
        build(&f, 2, sets);
        f.term[1] = MAXT;   /* outside the term table */
        CHECK(tfidf_result_near_dups(&f.r, &p, &d) == TFIDF_E_INVAL && d.doc == NULL);
        build(&f, 2, sets);
        f.doc[3] = 7;       /* not among doc_id */
        CHECK(tfidf_result_near_dups(&f.r, &p, &d) == TFIDF_E_INVAL && d.doc == NULL);
        build(&f, 2, sets);
        f.term[0] = 1;      /* not ascending */
        CHECK(tfidf_result_minhash(&f.r, &p, &s) == TFIDF_E_INVAL && s.sig == NULL);
    }
    /* ---- union-find ---- */
    {
        const uint32_t a[3] = {4, 2, 0}, b[3] = {5, 4, 0};
        uint32_t g[6], ng = 9;
        CHECK(tfidf_dedup_groups(6, a, b, 3, g, &ng) == TFIDF_OK && ng == 1);
        CHECK(g[0] == 0 && g[1] == 1 && g[2] == 2 && g[3] == 3 && g[4] == 2 && g[5] == 2);
        CHECK(tfidf_dedup_groups(0, NULL, NULL, 0, NULL, &ng) == TFIDF_OK && ng == 0);
        CHECK(tfidf_dedup_groups(6, a, b, 3, NULL, &ng) == TFIDF_E_INVAL);
        const uint32_t out_of_range[1] = {6};
        CHECK(tfidf_dedup_groups(6, out_of_range, a, 1, g, &ng) == TFIDF_E_INVAL);
    }
    printf("ok\n");
    return 0;
}
