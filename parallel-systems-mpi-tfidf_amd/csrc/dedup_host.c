/*
 * dedup_host.c — host-side pieces of near-duplicate detection (include/tfidf.h, section "near
 * duplicates"): the parameter check every call starts with, the definition applied to a fetched
 * result (MinHash signatures, LSH band chains, exact Jaccard), and the union-find that builds
 * `group`, which the device path (engine_dedup.cpp) calls for its last step.  Plain C, no device
 * calls: the second opinion on dedup.hip.  The reference has no such pass.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"

static uint64_t dd_mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t dd_fnv1a(const uint8_t* p, uint64_t n) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (uint64_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001B3ull;
    return h;
}

int tfidf_dedup_check(const tfidf_dedup_params* p) {
    if (!p || p->size < sizeof(tfidf_dedup_params)) return TFIDF_E_INVAL;
    if (p->nhashes > TFIDF_MINHASH_MAX_H) return TFIDF_E_INVAL;
    if (p->nhashes != 0u && (p->rows == 0u || p->nhashes % p->rows != 0u)) return TFIDF_E_INVAL;
    if (!(p->threshold >= 0.0 && p->threshold <= 1.0)) return TFIDF_E_INVAL;   /* NaN fails both */
    return TFIDF_OK;
}

static void dd_resolve(const tfidf_dedup_params* p, uint32_t* H, uint32_t* r, uint64_t* seed) {
    if (p->nhashes == 0u) {
        *H = TFIDF_DEDUP_DEFAULT_H; *r = TFIDF_DEDUP_DEFAULT_ROWS; *seed = TFIDF_DEDUP_DEFAULT_SEED;
    } else {
        *H = p->nhashes; *r = p->rows; *seed = p->seed;
    }
}

static void dd_family(uint64_t seed, uint32_t H, uint64_t* a, uint32_t* b) {
    uint64_t s = seed;
    for (uint32_t i = 0; i < H; ++i) {
        s += 0x9E3779B97F4A7C15ull;
        a[i] = dd_mix64(s) | 1ull;
        s += 0x9E3779B97F4A7C15ull;
        b[i] = (uint32_t)(dd_mix64(s) >> 32);
    }
}

void tfidf_signatures_free(tfidf_signatures* s) {
    if (!s) return;
    free(s->doc); free(s->npairs); free(s->sig);
    memset(s, 0, sizeof(*s));
}

void tfidf_dups_free(tfidf_dups* d) {
    if (!d) return;
    free(d->doc); free(d->group); free(d->a_pos); free(d->b_pos); free(d->a_doc); free(d->b_doc);
    free(d->shared); free(d->uni); free(d->same); free(d->jaccard);
    memset(d, 0, sizeof(*d));
}

/* ---- groups: union-find whose root is always the lowest position of its set ---- */

static uint32_t uf_find(uint32_t* parent, uint32_t x) {
    uint32_t root = x;
    while (parent[root] != root) root = parent[root];
    while (parent[x] != root) {
        const uint32_t nx = parent[x];
        parent[x] = root;
        x = nx;
    }
    return root;
}

int tfidf_dedup_groups(uint32_t ndocs, const uint32_t* a_pos, const uint32_t* b_pos, uint64_t n, uint32_t* group,
                       uint32_t* ngroups) {
    if (ngroups) *ngroups = 0;
    if ((ndocs && !group) || (n && (!a_pos || !b_pos))) return TFIDF_E_INVAL;
    for (uint32_t i = 0; i < ndocs; ++i) group[i] = i;
    for (uint64_t e = 0; e < n; ++e) {
        if (a_pos[e] >= ndocs || b_pos[e] >= ndocs) return TFIDF_E_INVAL;
        const uint32_t x = uf_find(group, a_pos[e]), y = uf_find(group, b_pos[e]);
        if (x < y) group[y] = x;
        else if (y < x) group[x] = y;
    }
    uint32_t g = 0;
    for (uint32_t i = 0; i < ndocs; ++i) group[i] = uf_find(group, i);
    /* a component of two or more has a member that is not its own root; count each root once:
     * the first such member in position order marks it (roots are the lowest position, so a
     * root's first follower is met after the root) */
    if (ndocs) {
        uint8_t* seen = (uint8_t*)calloc(ndocs, 1);
        if (!seen) return TFIDF_E_NOMEM;
        for (uint32_t i = 0; i < ndocs; ++i)
            if (group[i] != i && !seen[group[i]]) { seen[group[i]] = 1; ++g; }
        free(seen);
    }
    if (ngroups) *ngroups = g;
    return TFIDF_OK;
}

/* ---- the definition on a fetched result ---- */

typedef struct { char name[16]; uint32_t id, idx; } dd_doc;
static int dd_doc_cmp(const void* a, const void* b) {   /* the "docN@" strcmp order; ties by input index */
    const dd_doc* x = (const dd_doc*)a;
    const dd_doc* y = (const dd_doc*)b;
    const int c = strcmp(x->name, y->name);
    if (c) return c;
    return x->idx < y->idx ? -1 : (x->idx > y->idx ? 1 : 0);
}
typedef struct { uint32_t id, pos; } dd_idpos;
static int dd_idpos_cmp(const void* a, const void* b) {
    const dd_idpos* x = (const dd_idpos*)a;
    const dd_idpos* y = (const dd_idpos*)b;
    if (x->id != y->id) return x->id < y->id ? -1 : 1;
    return x->pos < y->pos ? -1 : (x->pos > y->pos ? 1 : 0);
}
typedef struct { uint64_t key; uint32_t pos; } dd_band;
static int dd_band_cmp(const void* a, const void* b) {
    const dd_band* x = (const dd_band*)a;
    const dd_band* y = (const dd_band*)b;
    if (x->key != y->key) return x->key < y->key ? -1 : 1;
    return x->pos < y->pos ? -1 : (x->pos > y->pos ? 1 : 0);
}
static int dd_u64_cmp(const void* a, const void* b) {
    const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
    return x < y ? -1 : (x > y ? 1 : 0);
}

/* what both host calls need of the result: documents by position, their pair ranges, signatures */
typedef struct {
    uint32_t N, H;
    uint32_t* doc;       /* id by position */
    uint64_t* start;     /* first pair by position */
    uint32_t* n;         /* n(d) by position */
    uint32_t* sig;       /* N * H */
} dd_state;

static void dd_state_free(dd_state* s) {
    free(s->doc); free(s->start); free(s->n); free(s->sig);
    memset(s, 0, sizeof(*s));
}

static int dd_build(const tfidf_result* r, uint32_t H, uint64_t seed, dd_state* s) {
    memset(s, 0, sizeof(*s));
    const uint32_t N = r->ndocs, V = r->nterms;
    const uint64_t P = r->npairs;
    if (N && !r->doc_id) return TFIDF_E_INVAL;
    if (P && (!r->pair_doc || !r->pair_term || !N)) return TFIDF_E_INVAL;
    if (V && (!r->term_off || (r->term_off[V] && !r->term_bytes))) return TFIDF_E_INVAL;
    s->N = N;
    s->H = H;
    s->doc = (uint32_t*)calloc((size_t)N + 1, 4);
    s->start = (uint64_t*)calloc((size_t)N + 1, 8);
    s->n = (uint32_t*)calloc((size_t)N + 1, 4);
    s->sig = (uint32_t*)malloc(((size_t)N * H + 1) * 4);
    dd_doc* docs = (dd_doc*)malloc(((size_t)N + 1) * sizeof(dd_doc));
    dd_idpos* ip = (dd_idpos*)malloc(((size_t)N + 1) * sizeof(dd_idpos));
    uint64_t* h0 = (uint64_t*)malloc(((size_t)V + 1) * 8);
    int rc = TFIDF_OK;
    if (!s->doc || !s->start || !s->n || !s->sig || !docs || !ip || !h0) { rc = TFIDF_E_NOMEM; goto done; }
    for (uint32_t i = 0; i < N; ++i) {
        docs[i].id = r->doc_id[i];
        docs[i].idx = i;
        snprintf(docs[i].name, sizeof(docs[i].name), "doc%u@", r->doc_id[i]);
    }
    qsort(docs, N, sizeof(dd_doc), dd_doc_cmp);
    for (uint32_t j = 0; j < N; ++j) {
        s->doc[j] = docs[j].id;
        ip[j].id = docs[j].id;
        ip[j].pos = j;
    }
    qsort(ip, N, sizeof(dd_idpos), dd_idpos_cmp);
    for (uint64_t p = 0; p < P;) {
        const uint32_t id = r->pair_doc[p];
        uint64_t e = p + 1;
        while (e < P && r->pair_doc[e] == id) ++e;
        uint32_t lo = 0, hi = N;   /* the first entry with this id */
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (ip[mid].id < id) lo = mid + 1; else hi = mid;
        }
        if (lo >= N || ip[lo].id != id || s->n[ip[lo].pos] != 0u || e - p > 0xFFFFFFFFull) { rc = TFIDF_E_INVAL; goto done; }
        const uint32_t j = ip[lo].pos;
        s->start[j] = p;
        s->n[j] = (uint32_t)(e - p);
        for (uint64_t q = p; q < e; ++q)   /* a set by term rank: in range and strictly ascending */
            if (r->pair_term[q] >= V || (q > p && r->pair_term[q] <= r->pair_term[q - 1])) { rc = TFIDF_E_INVAL; goto done; }
        p = e;
    }
    for (uint32_t t = 0; t < V; ++t) {
        if (r->term_off[t + 1] < r->term_off[t]) { rc = TFIDF_E_INVAL; goto done; }
        h0[t] = dd_mix64(dd_fnv1a(r->term_bytes + r->term_off[t], r->term_off[t + 1] - r->term_off[t]));
    }
    {
        uint64_t fa[TFIDF_MINHASH_MAX_H];
        uint32_t fb[TFIDF_MINHASH_MAX_H];
        dd_family(seed, H, fa, fb);
        for (uint32_t j = 0; j < N; ++j) {
            uint32_t* sg = s->sig + (size_t)j * H;
            for (uint32_t i = 0; i < H; ++i) sg[i] = 0xFFFFFFFFu;
            for (uint64_t q = s->start[j]; q < s->start[j] + s->n[j]; ++q) {
                const uint64_t x = h0[r->pair_term[q]];
                for (uint32_t i = 0; i < H; ++i) {
                    const uint32_t g = (uint32_t)((fa[i] * x) >> 32) + fb[i];
                    if (g < sg[i]) sg[i] = g;
                }
            }
        }
    }
done:
    free(docs); free(ip); free(h0);
    if (rc) dd_state_free(s);
    return rc;
}

int tfidf_result_minhash(const tfidf_result* r, const tfidf_dedup_params* params, tfidf_signatures* out) {
    if (!out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!r || tfidf_dedup_check(params) != TFIDF_OK) return TFIDF_E_INVAL;
    uint32_t H, rows;
    uint64_t seed;
    dd_resolve(params, &H, &rows, &seed);
    dd_state s;
    const int rc = dd_build(r, H, seed, &s);
    if (rc) return rc;
    out->ndocs = s.N;
    out->nhashes = H;
    out->doc = s.doc;
    out->npairs = s.n;
    out->sig = s.sig;
    free(s.start);
    return TFIDF_OK;
}

int tfidf_result_near_dups(const tfidf_result* r, const tfidf_dedup_params* params, tfidf_dups* out) {
    if (!out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!r || tfidf_dedup_check(params) != TFIDF_OK) return TFIDF_E_INVAL;
    uint32_t H, rows;
    uint64_t seed;
    dd_resolve(params, &H, &rows, &seed);
    dd_state s;
    int rc = dd_build(r, H, seed, &s);
    if (rc) return rc;
    const uint32_t N = s.N, nb = H / rows;
    uint32_t M = 0;
    for (uint32_t j = 0; j < N; ++j) M += s.n[j] != 0u;
    const uint64_t cmax = M ? (uint64_t)nb * (M - 1u) : 0u;
    dd_band* band = (dd_band*)malloc(((size_t)M + 1) * sizeof(dd_band));
    uint64_t* cand = (uint64_t*)malloc(((size_t)cmax + 1) * 8);
    uint64_t nc = 0, ne = 0;
    if (!band || !cand) { rc = TFIDF_E_NOMEM; goto done; }
    for (uint32_t jb = 0; jb < nb; ++jb) {
        uint32_t m = 0;
        for (uint32_t j = 0; j < N; ++j) {
            if (!s.n[j]) continue;
            uint64_t k = dd_mix64((uint64_t)jb + 1u);
            for (uint32_t i = jb * rows; i < jb * rows + rows; ++i) k = dd_mix64(k ^ s.sig[(size_t)j * H + i]);
            band[m].key = k;
            band[m].pos = j;
            ++m;
        }
        qsort(band, m, sizeof(dd_band), dd_band_cmp);
        for (uint32_t i = 1; i < m; ++i)
            if (band[i].key == band[i - 1].key) cand[nc++] = ((uint64_t)band[i - 1].pos << 32) | band[i].pos;
    }
    qsort(cand, (size_t)nc, 8, dd_u64_cmp);
    {
        uint64_t u = 0;
        for (uint64_t i = 0; i < nc; ++i)
            if (i == 0 || cand[i] != cand[i - 1]) cand[u++] = cand[i];
        nc = u;
    }
    out->ndocs = N;
    out->ncand = nc;
    out->doc = s.doc;
    s.doc = NULL;
    out->group = (uint32_t*)calloc((size_t)N + 1, 4);
    out->a_pos = (uint32_t*)calloc((size_t)nc + 1, 4);
    out->b_pos = (uint32_t*)calloc((size_t)nc + 1, 4);
    out->a_doc = (uint32_t*)calloc((size_t)nc + 1, 4);
    out->b_doc = (uint32_t*)calloc((size_t)nc + 1, 4);
    out->shared = (uint32_t*)calloc((size_t)nc + 1, 4);
    out->uni = (uint32_t*)calloc((size_t)nc + 1, 4);
    out->same = (uint32_t*)calloc((size_t)nc + 1, 4);
    out->jaccard = (double*)calloc((size_t)nc + 1, 8);
    if (!out->group || !out->a_pos || !out->b_pos || !out->a_doc || !out->b_doc || !out->shared || !out->uni ||
        !out->same || !out->jaccard) { rc = TFIDF_E_NOMEM; goto done; }
    for (uint64_t c = 0; c < nc; ++c) {
        const uint32_t a = (uint32_t)(cand[c] >> 32), b = (uint32_t)cand[c];
        const uint32_t* ta = r->pair_term + s.start[a];
        const uint32_t* tb = r->pair_term + s.start[b];
        const uint32_t na = s.n[a], nbp = s.n[b];
        uint32_t i = 0, j = 0, shared = 0, same = 0;
        while (i < na && j < nbp) {
            if (ta[i] == tb[j]) { ++shared; ++i; ++j; }
            else if (ta[i] < tb[j]) ++i;
            else ++j;
        }
        for (uint32_t h = 0; h < H; ++h) same += s.sig[(size_t)a * H + h] == s.sig[(size_t)b * H + h];
        const uint32_t uni = na + nbp - shared;
        const double jac = (double)shared / (double)uni;
        if (!(jac >= params->threshold)) continue;
        out->a_pos[ne] = a;
        out->b_pos[ne] = b;
        out->a_doc[ne] = out->doc[a];
        out->b_doc[ne] = out->doc[b];
        out->shared[ne] = shared;
        out->uni[ne] = uni;
        out->same[ne] = same;
        out->jaccard[ne] = jac;
        ++ne;
    }
    out->nedges = ne;
    rc = tfidf_dedup_groups(N, out->a_pos, out->b_pos, ne, out->group, &out->ngroups);
done:
    free(band); free(cand);
    dd_state_free(&s);
    if (rc) tfidf_dups_free(out);
    return rc;
}
