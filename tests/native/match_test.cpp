/*
 * match_test — the scan, cut and word-gather kernels of csrc/match.hip on crafted term tables
 * against plain host loops: no engine, no corpus (tests/test_gpu_match_native.py runs it; links
 * match.o and prims.o alone).
 *
 *   dist     every string over {a, b, c} of length 1..5 as a table, in both source forms (the
 *            run's keys and corpus, a model's offsets and blob), against every such string as a
 *            pattern, for both flag settings and d = 0..2; terms of 62..67 bytes against 63- and
 *            64-byte patterns; the distance of every reported match and the absence of every
 *            other pair against a full host matrix
 *   scan     tables of V = tile * grid * 3 + 1 terms and that +- 1 with the grid of one CU: every
 *            workgroup makes three and more trips and the last tile is partial
 *   select   a list capacity below the matches: the counts stay exact, nothing is written past
 *            the capacity; then the sort (both forms), the cut and the words of duplicate
 *            patterns, of patterns that match nothing and of one pattern that matches everything
 *
 * Every comparison is exact.  Prints one "ok  " line per case and "ALL OK"; ends at the first HIP
 * error or mismatch with a non-zero status.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/tfidf.h"
#include "kernels.h"

#define CK(call)                                                                                  \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            printf("HIP error %s at %s:%d: %s\n", hipGetErrorString(e_), __FILE__, __LINE__, #call); \
            exit(2);                                                                              \
        }                                                                                         \
    } while (0)

static hipStream_t g_s;
static uint32_t g_ncu;
typedef std::string Str;   /* bytes; chars are compared as unsigned below */

template <typename T> static T* up(const std::vector<T>& h, size_t extra = 0) {
    T* d = nullptr;
    CK(hipMalloc((void**)&d, (h.size() + extra + 16) * sizeof(T)));
    CK(hipMemset(d, 0, (h.size() + extra + 16) * sizeof(T)));
    if (!h.empty()) CK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
template <typename T> static std::vector<T> down(const T* d, size_t n) {
    std::vector<T> h(n);
    if (n) CK(hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
    return h;
}
static void fail(const char* what, const char* field, uint64_t idx) {
    printf("MISMATCH %s: %s at index %llu\n", what, field, (unsigned long long)idx);
    exit(1);
}

/* ---- the host definition: a full matrix ---- */
static uint32_t host_dist(const Str& p, const Str& t, bool osa) {
    const size_t m = p.size(), n = t.size();
    std::vector<std::vector<uint32_t>> D(m + 1, std::vector<uint32_t>(n + 1, 0));
    for (size_t i = 0; i <= m; ++i) D[i][0] = (uint32_t)i;
    for (size_t j = 0; j <= n; ++j) D[0][j] = (uint32_t)j;
    for (size_t i = 1; i <= m; ++i)
        for (size_t j = 1; j <= n; ++j) {
            uint32_t v = std::min(std::min(D[i - 1][j] + 1, D[i][j - 1] + 1), D[i - 1][j - 1] + (p[i - 1] != t[j - 1]));
            if (osa && i > 1 && j > 1 && p[i - 1] == t[j - 2] && p[i - 2] == t[j - 1]) v = std::min(v, D[i - 2][j - 2] + 1);
            D[i][j] = v;
        }
    return D[m][n];
}
static bool tab_less(const Str& a, const Str& b) {   /* strcmp of word + "\t" on unsigned bytes */
    const Str x = a + "\t", y = b + "\t";
    return std::lexicographical_compare(x.begin(), x.end(), y.begin(), y.end(),
                                        [](char c, char d) { return (unsigned char)c < (unsigned char)d; });
}

struct Pat {
    Str bytes;
    uint8_t kind, budget;
};
struct Rec {
    uint32_t pat, dist, df, rank;
    bool operator<(const Rec& o) const {
        if (pat != o.pat) return pat < o.pat;
        if (dist != o.dist) return dist < o.dist;
        if (df != o.df) return df > o.df;
        return rank < o.rank;
    }
    bool operator==(const Rec& o) const { return pat == o.pat && dist == o.dist && df == o.df && rank == o.rank; }
};
static std::vector<Rec> host_matches(const std::vector<Str>& terms, const std::vector<uint32_t>& df,
                                     const std::vector<Pat>& pats, uint32_t fixed, bool osa) {
    std::vector<Rec> out;
    for (uint32_t i = 0; i < pats.size(); ++i) {
        const Str& p = pats[i].bytes;
        for (uint32_t r = 0; r < terms.size(); ++r) {
            const Str& t = terms[r];
            if (pats[i].kind == TFIDF_MATCH_PREFIX) {
                if (t.size() >= p.size() && t.compare(0, p.size(), p) == 0) out.push_back({i, 0, df[r], r});
                continue;
            }
            const size_t fx = std::min<size_t>(fixed, p.size());
            if (t.size() < fx || t.compare(0, fx, p, 0, fx) != 0) continue;
            const uint32_t d = host_dist(p, t, osa);
            if (d <= pats[i].budget) out.push_back({i, d, df[r], r});
        }
    }
    std::sort(out.begin(), out.end());
    return out;
}

/* ---- a table on the device, in one of the two source forms ---- */
struct Table {
    MtSrc src{};
    uint32_t V = 0;
    uint32_t* df = nullptr;
    std::vector<void*> own;
    ~Table() { for (void* p : own) (void)hipFree(p); }
};
static void make_table(Table& tb, const std::vector<Str>& terms, const std::vector<uint32_t>& df, bool model) {
    const uint32_t V = (uint32_t)terms.size();
    for (uint32_t r = 1; r < V; ++r)
        if (!tab_less(terms[r - 1], terms[r])) fail("table", "term order", r);
    std::vector<uint64_t> off(V + 1, 0);
    std::vector<uint8_t> blob;
    for (uint32_t r = 0; r < V; ++r) {
        off[r] = blob.size();
        blob.insert(blob.end(), terms[r].begin(), terms[r].end());
    }
    off[V] = blob.size();
    tb.V = V;
    tb.df = up(df);
    tb.own.push_back(tb.df);
    uint8_t* d_blob = up(blob, 64);
    tb.own.push_back(d_blob);
    if (model) {
        uint64_t* d_off = up(off);
        tb.own.push_back(d_off);
        tb.src = MtSrc{nullptr, nullptr, nullptr, blob.size(), d_off, d_blob};
        return;
    }
    std::vector<uint4> key(V);
    std::vector<uint32_t> len(V);
    for (uint32_t r = 0; r < V; ++r) {
        const Str& t = terms[r];
        len[r] = (uint32_t)t.size();
        if (t.size() < 16) {   /* the bytes, the TAB terminator, zeros (k_term_meta) */
            uint8_t b[16] = {0};
            memcpy(b, t.data(), t.size());
            b[t.size()] = 0x09;
            memcpy(&key[r], b, 16);
        } else {
            const uint64_t rep = ((uint64_t)t.size() << 40) | off[r];
            key[r] = make_uint4((uint32_t)rep, (uint32_t)(rep >> 32), 0u, 0xFFFFFFFFu);
        }
    }
    uint4* d_key = up(key);
    uint32_t* d_len = up(len);
    tb.own.push_back(d_key);
    tb.own.push_back(d_len);
    tb.src = MtSrc{d_key, d_len, d_blob, blob.size(), nullptr, nullptr};
}

/* ---- one scan of the patterns [p0, p0 + np) on the device: counts, cursor, the written records ---- */
struct ScanOut {
    std::vector<uint64_t> nmatch;
    uint64_t nrec = 0;
    std::vector<uint4> key;   /* the written records, unsorted */
};
struct PatBlock {
    uint8_t* d = nullptr;
    uint32_t P = 0;
    ~PatBlock() { (void)hipFree(d); }
};
static void make_patterns(PatBlock& pb, const std::vector<Pat>& pats) {
    const uint32_t P = (uint32_t)pats.size();
    std::vector<uint8_t> blk((size_t)P * (MT_PAT + 3), 0);
    for (uint32_t p = 0; p < P; ++p) {
        memcpy(blk.data() + (size_t)p * MT_PAT, pats[p].bytes.data(), pats[p].bytes.size());
        blk[(size_t)P * MT_PAT + p] = (uint8_t)pats[p].bytes.size();
        blk[(size_t)P * (MT_PAT + 1) + p] = pats[p].kind;
        blk[(size_t)P * (MT_PAT + 2) + p] = pats[p].kind ? 0 : pats[p].budget;
    }
    pb.d = up(blk);
    pb.P = P;
}
static ScanOut device_scan(const Table& tb, const PatBlock& pb, uint32_t p0, uint32_t np, uint32_t fixed, bool osa,
                           uint64_t cap, uint64_t alloc, uint4* d_key, uint32_t* d_val) {
    const uint32_t P = pb.P;
    unsigned long long* d_cnt = nullptr;
    CK(hipMalloc((void**)&d_cnt, ((size_t)P + 1) * 8));
    CK(hipMemset(d_cnt, 0, ((size_t)P + 1) * 8));
    CK(hipMemset(d_key, 0xEE, alloc * 16));   /* a record never holds this pattern: what was not written shows */
    MtScanArgs a{};
    a.src = tb.src;
    a.df = tb.df;
    a.V = tb.V;
    a.pat = pb.d;
    a.plen = pb.d + (size_t)P * MT_PAT;
    a.pkind = a.plen + P;
    a.pbudget = a.pkind + P;
    a.p0 = p0;
    a.np = np;
    a.fixed_prefix = fixed;
    a.transpose = osa ? 1u : 0u;
    a.nmatch = d_cnt;
    a.nrec = d_cnt + P;
    a.key = d_key;
    a.val = d_val;
    a.list_cap = cap;
    if (launch_match_scan(a, g_ncu, g_s)) { printf("launch_match_scan failed\n"); exit(2); }
    CK(hipStreamSynchronize(g_s));
    ScanOut o;
    std::vector<unsigned long long> c = down(d_cnt, (size_t)P + 1);
    o.nmatch.assign(c.begin(), c.begin() + P);
    o.nrec = c[P];
    o.key = down(d_key, alloc);
    CK(hipFree(d_cnt));
    return o;
}

/* every pattern in groups of MT_GROUP with a list that holds every match: the records, sorted on
 * the host, are the host's */
static uint64_t check_all(const char* what, const Table& tb, const std::vector<Str>& terms, const std::vector<uint32_t>& df,
                          const std::vector<Pat>& pats, uint32_t fixed, bool osa) {
    const std::vector<Rec> want = host_matches(terms, df, pats, fixed, osa);
    PatBlock pb;
    make_patterns(pb, pats);
    const uint64_t cap = (uint64_t)tb.V * MT_GROUP + 1;
    uint4* d_key = nullptr;
    uint32_t* d_val = nullptr;
    CK(hipMalloc((void**)&d_key, cap * 16));
    CK(hipMalloc((void**)&d_val, cap * 4));
    std::vector<Rec> got;
    std::vector<uint64_t> nm(pats.size(), 0);
    for (uint32_t p0 = 0; p0 < pats.size(); p0 += MT_GROUP) {
        const uint32_t np = std::min<uint32_t>(MT_GROUP, (uint32_t)pats.size() - p0);
        const ScanOut o = device_scan(tb, pb, p0, np, fixed, osa, cap, std::min<uint64_t>(cap, (uint64_t)tb.V * np + 1), d_key, d_val);
        if (o.nrec > cap) fail(what, "cursor", p0);
        for (uint64_t i = 0; i < o.nrec; ++i) got.push_back({o.key[i].w + p0, o.key[i].z, ~o.key[i].y, o.key[i].x});
        for (uint32_t i = 0; i < np; ++i) nm[p0 + i] = o.nmatch[p0 + i];
    }
    std::sort(got.begin(), got.end());
    if (got.size() != want.size()) fail(what, "matches in all", got.size());
    for (size_t i = 0; i < want.size(); ++i)
        if (!(got[i] == want[i])) fail(what, "record", i);
    std::vector<uint64_t> cnt(pats.size(), 0);
    for (const Rec& r : want) ++cnt[r.pat];
    for (size_t p = 0; p < pats.size(); ++p)
        if (cnt[p] != nm[p]) fail(what, "nmatch", p);
    CK(hipFree(d_key));
    CK(hipFree(d_val));
    return want.size();
}

static std::vector<Str> abc_strings() {
    std::vector<Str> out;
    for (int n = 1; n <= 5; ++n) {
        int total = 1;
        for (int i = 0; i < n; ++i) total *= 3;
        for (int x = 0; x < total; ++x) {
            Str s(n, 'a');
            int y = x;
            for (int i = n - 1; i >= 0; --i) { s[i] = (char)('a' + y % 3); y /= 3; }
            out.push_back(s);
        }
    }
    return out;
}
static std::vector<uint32_t> some_df(size_t n, uint32_t classes) {
    std::vector<uint32_t> df(n);
    for (size_t i = 0; i < n; ++i) df[i] = 1 + (uint32_t)((i * 7) % classes);
    return df;
}

/* -------------------------------------------------------------------- dist -- */
static void dist_group() {
    std::vector<Str> terms = abc_strings();
    std::sort(terms.begin(), terms.end(), tab_less);
    const std::vector<uint32_t> df = some_df(terms.size(), 5);
    for (int model = 0; model < 2; ++model) {
        Table tb;
        make_table(tb, terms, df, model != 0);
        for (int osa = 0; osa < 2; ++osa)
            for (uint8_t d = 0; d <= 2; ++d) {
                std::vector<Pat> pats;
                for (const Str& s : abc_strings()) pats.push_back({s, TFIDF_MATCH_FUZZY, d});
                char what[96];
                snprintf(what, sizeof what, "abc5 %s osa=%d d=%u", model ? "model" : "run", osa, d);
                const uint64_t n = check_all(what, tb, terms, df, pats, 0, osa != 0);
                printf("ok  %s: %llu matches of %zu pairs\n", what, (unsigned long long)n, terms.size() * pats.size());
            }
    }
    /* 62..67-byte terms 0..3 edits apart, 63- and 64-byte patterns */
    const Str al = "abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghij";
    std::vector<Str> lt;
    for (size_t n = 62; n <= 67; ++n) {
        Str s = al.substr(0, n);
        lt.push_back(s);
        Str a = s; a[0] = '#'; lt.push_back(a);
        Str b = s; b[n - 1] = '#'; lt.push_back(b);
        Str c = s; c[n / 2] = '#'; c[0] = '%'; lt.push_back(c);
        Str e = s; std::swap(e[n / 2], e[n / 2 + 1]); lt.push_back(e);
        Str f = s; std::swap(f[n - 2], f[n - 1]); lt.push_back(f);
        Str g = s; g[1] = '#'; g[n / 2] = '#'; g[n - 2] = '#'; lt.push_back(g);
    }
    std::sort(lt.begin(), lt.end(), tab_less);
    lt.erase(std::unique(lt.begin(), lt.end()), lt.end());
    const std::vector<uint32_t> ldf = some_df(lt.size(), 3);
    for (int model = 0; model < 2; ++model) {
        Table tb;
        make_table(tb, lt, ldf, model != 0);
        for (int osa = 0; osa < 2; ++osa) {
            std::vector<Pat> pats;
            for (size_t n = 63; n <= 64; ++n)
                for (uint8_t d = 0; d <= 2; ++d) {
                    Str s = al.substr(0, n);
                    pats.push_back({s, TFIDF_MATCH_FUZZY, d});
                    Str a = s; a[n - 1] = '!'; pats.push_back({a, TFIDF_MATCH_FUZZY, d});
                    Str b = s; std::swap(b[0], b[1]); pats.push_back({b, TFIDF_MATCH_FUZZY, d});
                    pats.push_back({s.substr(1), TFIDF_MATCH_FUZZY, d});
                    pats.push_back({s, TFIDF_MATCH_PREFIX, 0});
                }
            char what[96];
            snprintf(what, sizeof what, "long terms %s osa=%d", model ? "model" : "run", osa);
            const uint64_t n = check_all(what, tb, lt, ldf, pats, osa ? 0u : 3u, osa != 0);
            if (n < 20) fail(what, "too few matches to mean anything", n);
            printf("ok  %s: %llu matches\n", what, (unsigned long long)n);
        }
    }
}

/* a table of V distinct terms: "t" + five base-7 digits over {a..g}, every 11th padded to 15, 16, 17
 * and 40 bytes in turn */
static std::vector<Str> stride_terms(uint32_t V) {
    std::vector<Str> t;
    for (uint32_t i = 0; i < V; ++i) {
        Str s = "t";
        uint32_t y = i;
        for (int k = 0; k < 5; ++k) { s.insert(s.begin() + 1, (char)('a' + y % 7)); y /= 7; }
        if (i % 11 == 3) { static const size_t pad[4] = {15, 16, 17, 40}; s += Str(pad[(i / 11) % 4] - s.size(), 'x'); }
        t.push_back(s);
    }
    std::sort(t.begin(), t.end(), tab_less);
    return t;
}
static std::vector<Pat> stride_patterns() {
    std::vector<Pat> p = {{"tabcde", 0, 2}, {"tgggggg", 0, 2}, {"tgfgfg", 0, 1}, {"t", 1, 0}, {"tg", 1, 0}, {"tabc", 1, 0},
                          {"tabcdexxxxxxxxx", 0, 2}, {"tabcdexxxxxxxxxx", 0, 2}, {"taaadexxxxxxxxxxx", 0, 2},
                          {"nothing", 0, 2}, {"taaaad", 0, 0}, {"atbcde", 0, 1}};
    return p;
}

/* -------------------------------------------------------------------- scan -- */
static void scan_group() {
    g_ncu = 1;   /* the grid of one CU */
    const uint32_t base = MT_NT * MT_WG_PER_CU * 3u + 1u;
    for (uint32_t V : {base - 1, base, base + 1})
        for (int model = 0; model < 2; ++model) {
            const std::vector<Str> terms = stride_terms(V);
            const std::vector<uint32_t> df = some_df(V, 9);
            Table tb;
            make_table(tb, terms, df, model != 0);
            char what[96];
            snprintf(what, sizeof what, "V=%u %s", V, model ? "model" : "run");
            const uint64_t n = check_all(what, tb, terms, df, stride_patterns(), 0, true);
            if (n < V) fail(what, "the prefix t matches every term", n);
            printf("ok  %s: %llu matches, %u tiles over %u workgroups\n", what, (unsigned long long)n,
                   (V + MT_NT - 1) / MT_NT, MT_WG_PER_CU);
        }
}

/* ------------------------------------------------------------------ select -- */
static void select_group() {
    const uint32_t V = 3000;
    const std::vector<Str> terms = stride_terms(V);
    const std::vector<uint32_t> df = some_df(V, 9);
    std::vector<Pat> pats = stride_patterns();
    pats.push_back(pats[0]);                       /* duplicates */
    pats.push_back(pats[3]);
    const std::vector<Rec> want = host_matches(terms, df, pats, 0, true);
    const uint32_t P = (uint32_t)pats.size();
    std::vector<uint32_t> seg(P + 1, 0);
    for (const Rec& r : want) ++seg[r.pat + 1];
    for (uint32_t p = 0; p < P; ++p) seg[p + 1] += seg[p];
    for (int model = 0; model < 2; ++model) {
        Table tb;
        make_table(tb, terms, df, model != 0);
        PatBlock pb;
        make_patterns(pb, pats);
        const uint64_t full = (uint64_t)V * P + 1;
        uint4 *k0 = nullptr, *k1 = nullptr;
        uint32_t *v0 = nullptr, *v1 = nullptr;
        CK(hipMalloc((void**)&k0, full * 16));
        CK(hipMalloc((void**)&k1, full * 16));
        CK(hipMalloc((void**)&v0, full * 4));
        CK(hipMalloc((void**)&v1, full * 4));
        char what[96];
        {   /* a capacity below the matches */
            snprintf(what, sizeof what, "capacity 1024 %s", model ? "model" : "run");
            const ScanOut o = device_scan(tb, pb, 0, P, 0, true, 1024, 2048, k0, v0);
            if (o.nrec != want.size() || o.nrec <= 1024) fail(what, "cursor", o.nrec);
            for (uint32_t p = 0; p < P; ++p)
                if (o.nmatch[p] != seg[p + 1] - seg[p]) fail(what, "nmatch", p);
            for (uint64_t i = 0; i < 2048; ++i)
                if ((o.key[i].w == 0xEEEEEEEEu) != (i >= 1024)) fail(what, "written records", i);
            printf("ok  %s: %llu matches counted, 1024 written\n", what, (unsigned long long)o.nrec);
        }
        Arena ar;
        CK(hipMalloc((void**)&ar.base, 64u << 20));
        ar.cap = 64u << 20;
        for (int radix = 0; radix < 2; ++radix)
            for (uint32_t E : {1u, 50u, 1024u}) {
                snprintf(what, sizeof what, "%s sort, cut at %u, %s", radix ? "radix" : "tile", E, model ? "model" : "run");
                const ScanOut o = device_scan(tb, pb, 0, P, 0, true, full, full, k0, v0);
                if (o.nrec != want.size()) fail(what, "cursor", o.nrec);
                ar.used = 0;
                const int where = radix ? radix_sort_u128(k0, v0, k1, v1, o.nrec, 0x11FFu, ar, g_s)
                                        : tile_sort_u128(k0, v0, k1, v1, o.nrec, ar, g_s);
                if (where < 0) { printf("sort failed %d\n", where); exit(2); }
                uint32_t* d_seg = up(seg);
                const size_t PE = (size_t)P * E;
                uint32_t *d_term = nullptr, *d_df = nullptr;
                uint8_t* d_dist = nullptr;
                uint64_t* d_wlen = nullptr;
                CK(hipMalloc((void**)&d_term, PE * 4 + 4));
                CK(hipMalloc((void**)&d_df, PE * 4 + 4));
                CK(hipMalloc((void**)&d_dist, PE + 4));
                CK(hipMalloc((void**)&d_wlen, (PE + 1) * 8));
                MtCutArgs ca{where ? k1 : k0, d_seg, P, E, tb.src, V, d_term, d_dist, d_df, d_wlen};
                if (launch_match_cut(ca, g_s)) { printf("launch_match_cut failed\n"); exit(2); }
                ar.used = 0;
                if (scan_excl_u64(d_wlen, d_wlen, PE, ar, g_s)) { printf("scan failed\n"); exit(2); }
                CK(hipStreamSynchronize(g_s));
                const std::vector<uint32_t> term = down(d_term, PE), gdf = down(d_df, PE);
                const std::vector<uint8_t> dist = down(d_dist, PE);
                const std::vector<uint64_t> woff = down(d_wlen, PE + 1);
                uint8_t* d_words = nullptr;
                CK(hipMalloc((void**)&d_words, woff[PE] + 16));
                if (model) {
                    if (launch_match_words_model(d_term, d_wlen, PE, tb.src, V, d_words, g_s)) { printf("words failed\n"); exit(2); }
                    CK(hipStreamSynchronize(g_s));
                }
                const std::vector<uint8_t> words = model ? down(d_words, woff[PE]) : std::vector<uint8_t>();
                for (uint32_t p = 0; p < P; ++p) {
                    const uint32_t n = seg[p + 1] - seg[p], keep = n < E ? n : E;
                    for (uint32_t j = 0; j < E; ++j) {
                        const size_t e = (size_t)p * E + j;
                        if (j >= keep) {
                            if (woff[e + 1] != woff[e]) fail(what, "an unused entry has bytes", e);
                            continue;
                        }
                        const Rec& r = want[seg[p] + j];
                        if (term[e] != r.rank) fail(what, "term", e);
                        if (dist[e] != r.dist) fail(what, "dist", e);
                        if (gdf[e] != r.df) fail(what, "df", e);
                        const Str& w = terms[r.rank];
                        if (woff[e + 1] - woff[e] != w.size()) fail(what, "word length", e);
                        if (model && memcmp(words.data() + woff[e], w.data(), w.size()) != 0) fail(what, "word bytes", e);
                    }
                }
                CK(hipFree(d_seg)); CK(hipFree(d_term)); CK(hipFree(d_df)); CK(hipFree(d_dist)); CK(hipFree(d_wlen));
                CK(hipFree(d_words));
                printf("ok  %s: %zu records\n", what, want.size());
            }
        CK(hipFree(ar.base));
        CK(hipFree(k0)); CK(hipFree(k1)); CK(hipFree(v0)); CK(hipFree(v1));
    }
}

int main(int argc, char** argv) {
    const char* group = argc > 1 ? argv[1] : "all";
    CK(hipSetDevice(0));
    CK(hipStreamCreate(&g_s));
    int ncu = 0;
    CK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0));
    g_ncu = (uint32_t)ncu;
    if (!strcmp(group, "dist") || !strcmp(group, "all")) dist_group();
    if (!strcmp(group, "select") || !strcmp(group, "all")) select_group();
    if (!strcmp(group, "scan") || !strcmp(group, "all")) scan_group();
    CK(hipStreamDestroy(g_s));
    printf("ALL OK\n");
    return 0;
}
