/*
 * labels_file.h — the labels file of `tfidf --labels FILE` (host/tfidf_main.c): lines
 * "doc<N>\t<name>".  Plain C, no library calls, so tests/native/nb_host_test.c can include it.
 *
 *   line     "doc", the decimal id 1..4294967295 without a sign or leading zero, one tab, the
 *            name: one byte or more up to the line's end, no tab and no NUL in it.  The last line
 *            may lack its newline; there are no empty lines
 *   classes  the distinct names in byte order (memcmp, a prefix before the longer name): class c
 *            is name[c].  At most LABELS_MAX_CLASSES of them
 * A repeated id is not this parser's business: tfidf_nb_check refuses it.
 */
#ifndef TFIDF_LABELS_FILE_H
#define TFIDF_LABELS_FILE_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define LABELS_MAX_CLASSES 256u   /* TFIDF_NB_MAX_CLASSES */

typedef struct labels_file {
    uint32_t n, k;          /* labelled documents, classes */
    uint32_t* doc;          /* n ids, in file order */
    uint32_t* label;        /* n classes */
    char** name;            /* k names, NUL-terminated copies, in byte order */
} labels_file;

static void labels_free(labels_file* l) {
    if (!l) return;
    for (uint32_t c = 0; l->name && c < l->k; ++c) free(l->name[c]);
    free(l->name); free(l->doc); free(l->label);
    memset(l, 0, sizeof(*l));
}

typedef struct { const uint8_t* p; size_t n; } labels_span;
static int labels_span_cmp(const void* a, const void* b) {
    const labels_span* x = (const labels_span*)a;
    const labels_span* y = (const labels_span*)b;
    const size_t m = x->n < y->n ? x->n : y->n;
    const int c = memcmp(x->p, y->p, m);
    if (c) return c;
    return x->n < y->n ? -1 : (x->n > y->n ? 1 : 0);
}

/* 0, or -1 with *bad_line = the 1-based line that is refused (0: no lines, too many classes or
 * no memory) and *out zeroed */
static int labels_parse(const uint8_t* b, size_t n, labels_file* out, size_t* bad_line) {
    memset(out, 0, sizeof(*out));
    *bad_line = 0;
    size_t lines = 0;
    for (size_t i = 0; i < n; ++i) lines += b[i] == '\n';
    if (n && b[n - 1] != '\n') ++lines;
    if (!lines || lines > 0xFFFFFFFFull) return -1;
    labels_span* nm = (labels_span*)malloc(lines * sizeof(labels_span));
    labels_span* uniq = (labels_span*)malloc(lines * sizeof(labels_span));
    out->doc = (uint32_t*)malloc(lines * sizeof(uint32_t));
    out->label = (uint32_t*)malloc(lines * sizeof(uint32_t));
    int rc = -1;
    size_t at = 0, k = 0;
    if (!nm || !uniq || !out->doc || !out->label) goto done;
    for (size_t ln = 0; ln < lines; ++ln) {
        size_t e = at;
        while (e < n && b[e] != '\n') ++e;
        *bad_line = ln + 1;
        if (e - at < 6 || memcmp(b + at, "doc", 3) != 0) goto done;
        size_t i = at + 3;
        uint64_t id = 0;
        if (b[i] < '1' || b[i] > '9') goto done;   /* no sign, no leading zero, not empty */
        for (; i < e && b[i] >= '0' && b[i] <= '9'; ++i) {
            id = id * 10 + (uint64_t)(b[i] - '0');
            if (id > 0xFFFFFFFFull) goto done;
        }
        if (i >= e || b[i] != '\t') goto done;
        ++i;
        if (i >= e) goto done;   /* an empty name */
        for (size_t j = i; j < e; ++j)
            if (b[j] == '\t' || b[j] == 0) goto done;
        out->doc[ln] = (uint32_t)id;
        nm[ln].p = b + i;
        nm[ln].n = e - i;
        at = e + 1;
    }
    *bad_line = 0;
    memcpy(uniq, nm, lines * sizeof(labels_span));
    qsort(uniq, lines, sizeof(labels_span), labels_span_cmp);
    for (size_t i = 0; i < lines; ++i)
        if (!i || labels_span_cmp(&uniq[i], &uniq[k - 1]) != 0) uniq[k++] = uniq[i];
    if (k > LABELS_MAX_CLASSES) goto done;
    out->name = (char**)calloc(k, sizeof(char*));
    if (!out->name) goto done;
    out->k = (uint32_t)k;
    for (size_t c = 0; c < k; ++c) {
        out->name[c] = (char*)malloc(uniq[c].n + 1);
        if (!out->name[c]) goto done;
        memcpy(out->name[c], uniq[c].p, uniq[c].n);
        out->name[c][uniq[c].n] = 0;
    }
    for (size_t ln = 0; ln < lines; ++ln) {
        size_t lo = 0, hi = k;   /* the name's class: present by construction */
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (labels_span_cmp(&uniq[mid], &nm[ln]) < 0) lo = mid + 1; else hi = mid;
        }
        out->label[ln] = (uint32_t)lo;
    }
    out->n = (uint32_t)lines;
    rc = 0;
done:
    free(nm); free(uniq);
    if (rc) labels_free(out);
    return rc;
}

#endif
