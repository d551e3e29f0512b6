/*
 * model_io.c — host-side pieces of the portable model (include/tfidf.h, section "model"):
 * the validity check every other model call starts with, and the file format.  Plain C, no
 * device calls.  The reference keeps nothing past its one pass (TFIDF.c:130-247); the order
 * checked here is the strcmp order of its "docN@word\t..." lines for a fixed document
 * (TFIDF.c:245,273).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"

#define MODEL_TERM_MAX (1ull << 24)   /* a term this long is in no vocabulary (TFIDF_E_CAPACITY of a run) */
#define MODEL_HEADER 40u
#define MODEL_VERSION 1u
static const char kMagic[8] = {'T', 'F', 'I', 'D', 'F', 'M', 'D', 'L'};

static int is_sep(uint8_t c) { return c == 0x20u || (c >= 0x09u && c <= 0x0Du); }

/* a + "\t" < b + "\t" under strcmp on unsigned bytes; neither holds a NUL or a TAB */
static int term_less(const uint8_t* a, uint64_t la, const uint8_t* b, uint64_t lb) {
    const uint64_t n = la < lb ? la : lb;
    const int c = n ? memcmp(a, b, (size_t)n) : 0;
    if (c) return c < 0;
    if (la == lb) return 0;
    return la < lb ? 0x09u < b[la] : a[lb] < 0x09u;
}

int tfidf_model_check(const tfidf_model* m) {
    if (!m || m->size < sizeof(tfidf_model)) return TFIDF_E_INVAL;
    const uint64_t V = m->nterms;
    if (V >= 0xFFFFFFFFull) return TFIDF_E_INVAL;
    if (V == 0) return TFIDF_OK;
    if (!m->term_off || !m->term_df) return TFIDF_E_INVAL;
    for (uint64_t t = 0; t < V; ++t) {
        const uint64_t o = m->term_off[t], e = m->term_off[t + 1];
        if (e < o || e - o >= MODEL_TERM_MAX) return TFIDF_E_INVAL;
        if (e > o && !m->term_bytes) return TFIDF_E_INVAL;
        if (m->term_df[t] < 1u || m->term_df[t] > m->ndocs_total) return TFIDF_E_INVAL;
    }
    for (uint64_t i = m->term_off[0]; i < m->term_off[V]; ++i)
        if (m->term_bytes[i] == 0u || is_sep(m->term_bytes[i])) return TFIDF_E_INVAL;
    for (uint64_t t = 1; t < V; ++t) {
        const uint64_t a = m->term_off[t - 1], b = m->term_off[t], e = m->term_off[t + 1];
        if (!term_less(m->term_bytes + a, b - a, m->term_bytes + b, e - b)) return TFIDF_E_INVAL;
    }
    return TFIDF_OK;
}

void tfidf_model_free(tfidf_model* m) {
    if (!m) return;
    free(m->term_off);
    free(m->term_bytes);
    free(m->term_df);
    memset(m, 0, sizeof(*m));
}

static void put_le(uint8_t* p, uint64_t v, int n) {
    for (int i = 0; i < n; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
static uint64_t get_le(const uint8_t* p, int n) {
    uint64_t v = 0;
    for (int i = 0; i < n; ++i) v |= (uint64_t)p[i] << (8 * i);
    return v;
}
static uint64_t fnv1a(uint64_t h, const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

int tfidf_model_save(const tfidf_model* m, const char* path) {
    if (!path) return TFIDF_E_INVAL;
    const int chk = tfidf_model_check(m);
    if (chk) return chk;
    const uint64_t V = m->nterms;
    const uint64_t base = V ? m->term_off[0] : 0, nbytes = V ? m->term_off[V] - base : 0;
    const size_t payload = (size_t)(8 * (V + 1) + 4 * V + nbytes);
    uint8_t* buf = (uint8_t*)malloc(MODEL_HEADER + payload);
    if (!buf) return TFIDF_E_NOMEM;
    uint8_t* p = buf + MODEL_HEADER;
    for (uint64_t t = 0; t <= V; ++t, p += 8) put_le(p, V ? m->term_off[t] - base : 0, 8);
    for (uint64_t t = 0; t < V; ++t, p += 4) put_le(p, m->term_df[t], 4);
    if (nbytes) memcpy(p, m->term_bytes + base, (size_t)nbytes);
    memcpy(buf, kMagic, 8);
    put_le(buf + 8, MODEL_VERSION, 4);
    put_le(buf + 12, V, 4);
    put_le(buf + 16, m->ndocs_total, 8);
    put_le(buf + 24, nbytes, 8);
    put_le(buf + 32, fnv1a(0xcbf29ce484222325ull, buf + MODEL_HEADER, payload), 8);
    FILE* fp = fopen(path, "wb");
    if (!fp) { free(buf); return TFIDF_E_OUTPUT; }
    const size_t total = MODEL_HEADER + payload;
    const int bad = fwrite(buf, 1, total, fp) != total;
    free(buf);
    if (fclose(fp) != 0 || bad) return TFIDF_E_OUTPUT;
    return TFIDF_OK;
}

int tfidf_model_load(const char* path, tfidf_model* out) {
    if (!out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!path) return TFIDF_E_INVAL;
    FILE* fp = fopen(path, "rb");
    if (!fp) return TFIDF_E_MODEL;
    int rc = TFIDF_E_MODEL;
    uint8_t h[MODEL_HEADER];
    uint8_t* raw = NULL;
    if (fread(h, 1, MODEL_HEADER, fp) != MODEL_HEADER) goto done;
    if (memcmp(h, kMagic, 8) != 0 || get_le(h + 8, 4) != MODEL_VERSION) goto done;
    {
        const uint64_t V = get_le(h + 12, 4), nbytes = get_le(h + 24, 8);
        if (V >= 0xFFFFFFFFull || nbytes > V * (MODEL_TERM_MAX - 1)) goto done;
        const uint64_t payload = 8 * (V + 1) + 4 * V + nbytes;
        /* the file's length decides before anything of that size is allocated */
        if (fseek(fp, 0, SEEK_END) != 0) goto done;
        const long end = ftell(fp);
        if (end < 0 || (uint64_t)end != MODEL_HEADER + payload) goto done;
        if (fseek(fp, MODEL_HEADER, SEEK_SET) != 0) goto done;
        raw = (uint8_t*)malloc((size_t)payload);
        if (!raw) { rc = TFIDF_E_NOMEM; goto done; }
        if (fread(raw, 1, (size_t)payload, fp) != payload) goto done;
        if (fnv1a(0xcbf29ce484222325ull, raw, (size_t)payload) != get_le(h + 32, 8)) goto done;
        out->size = sizeof(tfidf_model);
        out->ndocs_total = get_le(h + 16, 8);
        out->nterms = (uint32_t)V;
        out->term_off = (uint64_t*)malloc((size_t)(V + 1) * 8);
        out->term_df = (uint32_t*)malloc((size_t)V * 4 + 4);
        out->term_bytes = (uint8_t*)malloc((size_t)nbytes + 1);
        if (!out->term_off || !out->term_df || !out->term_bytes) { rc = TFIDF_E_NOMEM; goto done; }
        const uint8_t* p = raw;
        for (uint64_t t = 0; t <= V; ++t, p += 8) out->term_off[t] = get_le(p, 8);
        for (uint64_t t = 0; t < V; ++t, p += 4) out->term_df[t] = (uint32_t)get_le(p, 4);
        if (nbytes) memcpy(out->term_bytes, p, (size_t)nbytes);
        /* the offsets index the bytes just read: they start at 0, end at nbytes and never go back */
        if (out->term_off[0] != 0 || out->term_off[V] != nbytes) goto done;
        for (uint64_t t = 0; t < V; ++t)
            if (out->term_off[t] > out->term_off[t + 1]) goto done;
        if (tfidf_model_check(out) != TFIDF_OK) goto done;
        rc = TFIDF_OK;
    }
done:
    fclose(fp);
    free(raw);
    if (rc != TFIDF_OK) tfidf_model_free(out);
    return rc;
}
