/* GPU test of the packed-record path of csrc/finalize.hip: the packed DF pass (launch_df_hist
 * with pack_sbits: count << sbits | slot in, rank << cb | count out, cb = 32 - rank_bits), the
 * packed score kernels (launch_score_order with K5Args.rec_pack) and k_rec_unpack, on crafted
 * records against host loops and a host sort.  Links only build/finalize.o and build/prims.o.
 *
 *   recpack_test chain | score | guard | unpack
 *
 *   chain   V with rank_bits 1, 9, 11 and 16: K1-style packed records through the packed DF pass
 *           (narrow form, rank16 map and rank_of_slot map; wide form at 16 bits) and then through
 *           the packed score kernels
 *   score   rank_bits 21 and 22 (V over the LDS histogram's limit: records crafted as the DF
 *           pass would leave them) through the packed score kernels
 *   guard   a slot at or past the capacity sets ST_BOUNDS in the packed DF pass
 *   unpack  launch_rec_unpack against the same kind of records
 *
 * Document sizes 1, 63, 64, 65, 128, 129, 512, 513, 1023, 1024, 1025, 2048, 2049 and 4096 pairs
 * (those that V distinct ranks allow), counts 1 and the count field's maximum among random ones,
 * a document with a bucket over K5_GROUP_MAX (the wave kernel's radix path) and one over
 * K5L_GROUP_MAX (k_score_large's), and presorted two-word documents (ranks in rec_slot, full
 * 32-bit counts in rec_cnt, behind the packed records) mixed with the packed ones in one call.
 * rec_cnt's main region holds poison: a kernel that read a packed document's count there would
 * emit it.  One "ok  " line per case, "ALL OK" at the end; a HIP error or a negative launcher
 * return ends the program at once (exit 2), a mismatch too (exit 1).  Integers are compared
 * exactly, scores as bit patterns (compiled without floating-point contraction).  Every stage
 * must leave the status word zero, the arena empty and the 1024 elements behind every buffer
 * untouched; outputs are prefilled with all-ones words. */
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#define CK(call)                                                                                  \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            printf("HIP error %s at %s:%d: %s\n", hipGetErrorString(e_), __FILE__, __LINE__, #call); \
            fflush(stdout);                                                                       \
            exit(2);                                                                              \
        }                                                                                         \
    } while (0)

static hipStream_t g_s, g_s2;
static hipEvent_t g_ev0, g_ev1;
static Arena g_ar;
static size_t g_ar_bytes;
static uint32_t* g_status;
typedef std::mt19937_64 Rng;

static std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
static std::string fmt(const char* f, ...) {
    char b[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(b, sizeof b, f, ap);
    va_end(ap);
    return b;
}
[[noreturn]] static void fail(const std::string& what, const std::string& sizes, uint64_t idx, const char* field) {
    printf("MISMATCH %s (%s) first differing index %llu (%s)\n", what.c_str(), sizes.c_str(), (unsigned long long)idx, field);
    fflush(stdout);
    exit(1);
}
[[noreturn]] static void harness_bug(const char* why) {
    printf("harness bug: %s\n", why);
    fflush(stdout);
    exit(1);
}

constexpr uint64_t GUARD = 1024;
constexpr int GUARD_BYTE = 0xA7;
constexpr uint32_t POISON = 0xDEADBEEFu;     /* rec_cnt under the packed records */
struct GuardRef { const char* name; const uint8_t* p; size_t bytes; };
static std::vector<GuardRef> g_guards;

template <typename T>
struct DBuf {
    T* p = nullptr;
    uint64_t n;
    DBuf(const char* name, uint64_t count) : n(count) {
        CK(hipMalloc((void**)&p, (count + GUARD) * sizeof(T)));
        CK(hipMemsetAsync((void*)(p + count), GUARD_BYTE, GUARD * sizeof(T), g_s));
        g_guards.push_back(GuardRef{name, (const uint8_t*)(p + count), GUARD * sizeof(T)});
    }
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    ~DBuf() {
        for (size_t i = 0; i < g_guards.size(); ++i)
            if (g_guards[i].p == (const uint8_t*)(p + n)) { g_guards.erase(g_guards.begin() + (long)i); break; }
        CK(hipFree(p));
    }
    void fill(int byte) { if (n) CK(hipMemsetAsync((void*)p, byte, n * sizeof(T), g_s)); }
    void up(const std::vector<T>& h) {
        if (h.size() > n) harness_bug("upload past a buffer");
        if (!h.empty()) CK(hipMemcpyAsync((void*)p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, g_s));
    }
    std::vector<T> down() const {
        std::vector<T> h(n);
        CK(hipStreamSynchronize(g_s));
        if (n) CK(hipMemcpy(h.data(), (const void*)p, n * sizeof(T), hipMemcpyDeviceToHost));
        return h;
    }
};
static uint32_t word_at(const uint32_t* dev) {
    uint32_t v = 0;
    CK(hipMemcpy(&v, dev, 4, hipMemcpyDeviceToHost));
    return v;
}
static void begin_case() {
    g_ar.cap = g_ar_bytes;
    g_ar.used = 0;
    CK(hipMemsetAsync(g_status, 0, 4, g_s));
}
/* a stage returned: its return value, the stream, the status word (want_status), the arena, the guards */
static void end_stage(const std::string& what, int rc, uint32_t want_status = 0) {
    if (rc < 0) {
        printf("%s returned %d\n", what.c_str(), rc);
        fflush(stdout);
        exit(2);
    }
    CK(hipStreamSynchronize(g_s));
    CK(hipGetLastError());
    if (g_ar.used != 0) { printf("MISMATCH %s left %zu arena bytes in use\n", what.c_str(), g_ar.used); exit(1); }
    const uint32_t st = word_at(g_status);
    if (st != want_status) { printf("MISMATCH %s: status word 0x%x, expected 0x%x\n", what.c_str(), st, want_status); exit(1); }
    std::vector<uint8_t> g;
    for (const GuardRef& r : g_guards) {
        g.assign(r.bytes, 0);
        CK(hipMemcpy(g.data(), r.p, r.bytes, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < r.bytes; ++i)
            if (g[i] != (uint8_t)GUARD_BYTE) fail(what, fmt("guard behind %s", r.name), i, "guard byte overwritten");
    }
}

/* ------------------------------------------------------------------ the corpus ---- */
/* Documents as K1 and the merge leave them: the packed ones first (records [0, R_main): rank and
 * count of every pair, packed by the case as the stage under test reads them), then the
 * presorted two-word ones (ascending ranks in rec_slot, full counts in rec_cnt). */
struct Doc {
    std::vector<uint32_t> rank, cnt;
    bool presorted;
};
struct Corpus {
    uint32_t V = 0, cmax = 0;   /* cmax: a packed record's largest count */
    std::vector<Doc> docs;
};
static uint32_t rank_bits_of(uint32_t V) { return V > 1 ? 32u - (uint32_t)__builtin_clz(V - 1) : 1u; }

/* n distinct ranks below V, one per stratum, the ends in; shuffled */
static std::vector<uint32_t> some_ranks(uint32_t n, uint32_t V, Rng& g) {
    if (n > V) harness_bug("more distinct ranks than V");
    std::vector<uint32_t> r(n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t lo = (uint64_t)i * V / n, hi = (uint64_t)(i + 1) * V / n;
        r[i] = (uint32_t)(lo + g() % (hi - lo));
    }
    if (n) r[0] = 0;
    if (n > 1) r[n - 1] = V - 1;
    std::shuffle(r.begin(), r.end(), g);
    return r;
}
/* n distinct ranks of which `target` consecutive ones share a bucket of `width` ranks */
static std::vector<uint32_t> skewed_ranks(uint32_t n, uint32_t V, uint32_t width, uint32_t target, Rng& g) {
    if (target > width || target > n || V / width < 4) harness_bug("skewed_ranks");
    const uint32_t b0 = (V / width / 2) * width;
    std::vector<uint32_t> r;
    for (uint32_t i = 0; i < target; ++i) r.push_back(b0 + i);
    /* the rest: strata outside the hot bucket */
    const uint32_t rest = n - target;
    for (uint32_t i = 0; i < rest; ++i) {
        const uint64_t lo = (uint64_t)i * V / rest;
        uint32_t x = (uint32_t)lo;
        if (x >= b0 && x < b0 + width) x = b0 + width + (x - b0);
        r.push_back(x);
    }
    std::sort(r.begin(), r.end());
    if (std::adjacent_find(r.begin(), r.end()) != r.end() || r.back() >= V) harness_bug("skewed_ranks collide");
    std::shuffle(r.begin(), r.end(), g);
    return r;
}
static void add_doc(Corpus& c, std::vector<uint32_t> ranks, bool presorted, Rng& g) {
    Doc d;
    d.presorted = presorted;
    if (presorted) std::sort(ranks.begin(), ranks.end());
    d.rank = ranks;
    d.cnt.resize(ranks.size());
    for (size_t j = 0; j < ranks.size(); ++j) {
        const uint32_t k = (uint32_t)(g() % 8);
        /* presorted documents hold full counts (wider than any field) */
        d.cnt[j] = presorted ? (k == 0 ? 0xFFFFFFF0u : 1u + (uint32_t)(g() % 3000000))
                             : (k == 0 ? 1u : k == 1 ? c.cmax : 1u + (uint32_t)(g() % c.cmax));
    }
    if (!presorted && !ranks.empty()) { d.cnt[0] = c.cmax; d.cnt[ranks.size() - 1] = 1u; }
    c.docs.push_back(d);
}
static const uint32_t kSizes[] = {1, 63, 64, 65, 128, 129, 512, 513, 1023, 1024, 1025, 2048, 2049, 4096};

static Corpus make_corpus(uint32_t V, uint32_t cmax, uint64_t min_main, Rng& g) {
    Corpus c;
    c.V = V;
    c.cmax = cmax;
    const uint32_t rb = rank_bits_of(V);
    for (uint32_t n : kSizes) {
        if (n > V) continue;
        add_doc(c, some_ranks(n, V, g), false, g);
        if (n == 65 || n == 513 || n == 2049 || n == 1) add_doc(c, some_ranks(n, V, g), true, g);
    }
    add_doc(c, {}, false, g);   /* a document without pairs */
    if (rb >= K5_NB_BITS + 7) {   /* a wave-kernel bucket (the rank's top K5_NB_BITS bits) over K5_GROUP_MAX */
        add_doc(c, skewed_ranks(700, V, 1u << (rb - K5_NB_BITS), K5_GROUP_MAX + 9, g), false, g);
        add_doc(c, skewed_ranks(129, V, 1u << (rb - K5_NB_BITS), K5_GROUP_MAX + 1, g), false, g);
    }
    if (rb >= 10 + 6)             /* a k_score_large bucket (10 bucket bits up to K5_MAX_PAIRS / 2 pairs) over K5L_GROUP_MAX */
        add_doc(c, skewed_ranks(1500, V, 1u << (rb - 10), K5L_GROUP_MAX + 5, g), false, g);
    if (rb >= 11 + 6)             /* ... and 11 bucket bits above */
        add_doc(c, skewed_ranks(3000, V, 1u << (rb - 11), K5L_GROUP_MAX + 1, g), false, g);
    uint64_t have = 0;
    for (const Doc& d : c.docs) if (!d.presorted) have += d.rank.size();
    while (have < min_main) {   /* fillers (the wide DF form needs more than DFH_RECS records per workgroup) */
        const uint32_t n = 1u + (uint32_t)(g() % std::min<uint32_t>(V, 1500u));
        add_doc(c, some_ranks(n, V, g), false, g);
        have += n;
    }
    std::shuffle(c.docs.begin(), c.docs.end(), g);
    return c;
}

/* the record arrays of a corpus: packed documents' (rank, count) in [0, R_main), the presorted
 * ones' behind them; doc_recoff / doc_npairs / doc_flags / doc_size */
struct Layout {
    uint64_t R_main = 0, R_total = 0;
    std::vector<uint32_t> mrank, mcnt;         /* main records */
    std::vector<uint32_t> prank, pcnt;         /* presorted records */
    std::vector<uint32_t> np, dsize;
    std::vector<uint64_t> recoff;
    std::vector<uint8_t> flags;
};
static Layout lay_out(const Corpus& c, Rng& g) {
    Layout L;
    for (const Doc& d : c.docs) if (!d.presorted) L.R_main += d.rank.size();
    uint64_t pm = 0, pp = L.R_main;
    for (const Doc& d : c.docs) {
        const uint64_t n = d.rank.size();
        L.np.push_back((uint32_t)n);
        L.flags.push_back(d.presorted ? (uint8_t)(DF_PARTIAL | DF_PRESORTED) : (uint8_t)0);
        L.dsize.push_back(g() % 8 == 0 ? 0xFFFFFFFFu : 1u + (uint32_t)(g() % 1000000));
        if (d.presorted) {
            L.recoff.push_back(n ? pp : 0);
            pp += n;
            L.prank.insert(L.prank.end(), d.rank.begin(), d.rank.end());
            L.pcnt.insert(L.pcnt.end(), d.cnt.begin(), d.cnt.end());
        } else {
            L.recoff.push_back(n ? pm : 0);
            pm += n;
            L.mrank.insert(L.mrank.end(), d.rank.begin(), d.rank.end());
            L.mcnt.insert(L.mcnt.end(), d.cnt.begin(), d.cnt.end());
        }
    }
    L.R_total = pp;
    return L;
}

/* ------------------------------------------------------------------- the stages ---- */
/* slot of rank r: a bijection of the ranks into [0, cap) */
struct SlotMap {
    uint64_t cap, mul, add;
    uint32_t of(uint32_t r) const { return (uint32_t)((r * mul + add) & (cap - 1)); }
};

/* the packed DF pass over `rec` (device: K1's packed words, then the presorted ranks); checks df
 * and every record word */
static void run_df_packed(const std::string& what, const Layout& L, uint32_t V, uint32_t sbits, const SlotMap& sm,
                          bool use16, int force_wgs, bool want_wide, DBuf<uint32_t>& drec) {
    const uint64_t cap = 1ull << sbits;
    const uint32_t cb = 32u - rank_bits_of(V);
    const std::string sz = fmt("V=%u sbits=%u cb=%u main=%llu merged=%llu %s%s", V, sbits, cb, (unsigned long long)L.R_main,
                               (unsigned long long)(L.R_total - L.R_main), use16 ? "rank16" : "rank_of_slot",
                               want_wide ? " wide" : "");
    if (!df_keeps_packed(V, sbits)) harness_bug("the case does not keep packed records");
    if (force_wgs) setenv("TFIDF_DF_WGS", std::to_string(force_wgs).c_str(), 1);
    {   /* the form the case was built for, from the plan df_hist_scratch reports */
        const size_t scratch = df_hist_scratch(L.R_total, V);
        const uint64_t nparts = (scratch - 256) / ((uint64_t)((V + 1) / 2) * 4);
        const uint64_t per = nparts ? (L.R_total + nparts - 1) / nparts : 0;
        if (want_wide != (per > DFH_RECS)) harness_bug("not the DF form the case was built for");
    }
    std::vector<uint32_t> ros(cap, 0xFFFFFFFFu);
    std::vector<uint16_t> r16(use16 ? cap : 1, (uint16_t)0xFFFF);
    for (uint32_t r = 0; r < V; ++r) {
        const uint32_t s = sm.of(r);
        if (ros[s] != 0xFFFFFFFFu) harness_bug("two ranks share a slot");
        ros[s] = r;
        if (use16) r16[s] = (uint16_t)r;
    }
    DBuf<uint32_t> dros("rank_of_slot", cap), ddf("df", V), dex("nrec_extra", 1);
    DBuf<uint16_t> d16("rank16", use16 ? cap : 1);
    dros.up(ros);
    d16.up(r16);
    dex.up(std::vector<uint32_t>(1, (uint32_t)(L.R_total - L.R_main)));
    std::vector<uint32_t> in(L.R_total), want(L.R_total), xdf(V, 0);
    for (uint64_t i = 0; i < L.R_main; ++i) {
        if (L.mcnt[i] >> (32 - sbits)) harness_bug("a count does not fit K1's field");
        in[i] = (L.mcnt[i] << sbits) | sm.of(L.mrank[i]);
        want[i] = (L.mrank[i] << cb) | L.mcnt[i];
        ++xdf[L.mrank[i]];
    }
    for (uint64_t i = L.R_main; i < L.R_total; ++i) {
        in[i] = want[i] = L.prank[i - L.R_main];
        ++xdf[L.prank[i - L.R_main]];
    }
    drec.up(in);
    ddf.fill(0xCD);
    begin_case();
    end_stage(what + " launch_df_hist (packed)",
              launch_df_hist(drec.p, L.R_main, dex.p, L.R_total, dros.p, use16 ? d16.p : nullptr, V, cap, g_status, ddf.p, g_ar,
                             g_s, false, sbits));
    if (force_wgs) unsetenv("TFIDF_DF_WGS");
    const std::vector<uint32_t> gd = ddf.down(), gr = drec.down();
    for (uint32_t r = 0; r < V; ++r) if (gd[r] != xdf[r]) fail(what, sz, r, "df");
    for (uint64_t i = 0; i < L.R_total; ++i)
        if (gr[i] != want[i]) fail(what, sz, i, i < L.R_main ? "packed record rewritten as rank << cb | count" : "merged record");
    printf("ok  %s DF (%s)\n", what.c_str(), sz.c_str());
}

/* the packed score kernels over drec (packed words rank << cb | count, then the presorted
 * ranks) and drcnt (poison, then the presorted counts) against a host sort */
static void run_score_packed(const std::string& what, const Corpus& c, const Layout& L, DBuf<uint32_t>& drec,
                             DBuf<uint32_t>& drcnt, Rng& g) {
    const uint32_t N = (uint32_t)c.docs.size(), V = c.V, rank_bits = rank_bits_of(V), cb = 32u - rank_bits;
    const std::string sz = fmt("ndocs=%u V=%u rank_bits=%u records=%llu of them packed %llu", N, V, rank_bits,
                               (unsigned long long)L.R_total, (unsigned long long)L.R_main);
    const uint32_t Ntot = 1000003;
    std::vector<uint32_t> dfv(V);
    for (auto& d : dfv) d = 1 + (uint32_t)(g() % Ntot);
    std::vector<double> idf((size_t)Ntot + 1);
    idf[0] = 0.0;
    for (uint32_t k = 1; k <= Ntot; ++k) idf[k] = log(1.0 * (double)Ntot / (double)k);
    std::vector<uint32_t> order(N);
    for (uint32_t i = 0; i < N; ++i) order[i] = i;
    std::shuffle(order.begin(), order.end(), g);
    std::vector<uint64_t> xoff(N + 1, 0);
    uint32_t xsmall = 0, xwave = 0, xlarge = 0;
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t n = L.np[order[i]];
        xoff[i + 1] = xoff[i] + n;
        if (n == 0) continue;
        if (n <= K5_SMALL_DOC) ++xsmall;
        else if (n <= K5_WAVE) ++xwave;
        else ++xlarge;   /* no presorted document over K5_PS_SPLIT pairs here */
    }
    const uint64_t P = xoff[N], Pmax = L.R_total;
    if (P != Pmax) harness_bug("pairs and records differ");
    std::vector<uint32_t> xterm(Pmax), xcnt(Pmax);
    std::vector<uint64_t> xscore(Pmax);
    std::vector<std::pair<uint32_t, uint32_t>> rc;
    for (uint32_t i = 0; i < N; ++i) {
        const Doc& d = c.docs[order[i]];
        const uint32_t n = (uint32_t)d.rank.size();
        rc.resize(n);
        for (uint32_t j = 0; j < n; ++j) rc[j] = {d.rank[j], d.cnt[j]};
        if (!d.presorted) std::sort(rc.begin(), rc.end());
        const double ds = (double)L.dsize[order[i]];
        for (uint32_t j = 0; j < n; ++j) {
            const double score = ((double)rc[j].second / ds) * idf[dfv[rc[j].first]];
            xterm[xoff[i] + j] = rc[j].first;
            xcnt[xoff[i] + j] = rc[j].second;
            memcpy(&xscore[xoff[i] + j], &score, 8);
        }
    }
    DBuf<uint32_t> dorder("order", N), lists("large_list + cls_list", 2ull * N + 4), clsoff("cls_off", 3ull * ((N + 255) / 256) + 8),
        oterm("out_term", Pmax + 1), ocnt("out_cnt", Pmax + 1), ros("rank_of_slot", 16), dnp("doc_npairs", N), dds("doc_size", N),
        ddf("df_of_rank", V);
    const uint64_t cap_t = 2 * L.R_total / 4096 + 64;
    DBuf<uint2> split("split_tasks", cap_t + 1);
    DBuf<uint64_t> npo("npairs_ord", (uint64_t)N + 1), ooff("out_off", (uint64_t)N + 1), dro("doc_recoff", N);
    DBuf<uint4> meta("doc_meta", (uint64_t)N + 1);
    DBuf<uint8_t> dfl("doc_flags", N);
    DBuf<double> oscore("out_score", Pmax + 1), idfr("idf_rank", (uint64_t)V + 1), didf("idf", idf.size());
    dorder.up(order); dnp.up(L.np); dds.up(L.dsize); dro.up(L.recoff); dfl.up(L.flags); ddf.up(dfv); didf.up(idf);
    lists.fill(0xCD); clsoff.fill(0xCD); split.fill(0xCD); npo.fill(0xCD); ooff.fill(0xCD); meta.fill(0xCD); idfr.fill(0xCD);
    ros.fill(0xFF); oterm.fill(0xFF); ocnt.fill(0xFF); oscore.fill(0xFF);
    begin_case();
    end_stage(what + " launch_gather_meta", launch_gather_meta(dorder.p, dnp.p, dro.p, dds.p, dfl.p, N, npo.p, meta.p, g_s));
    end_stage(what + " scan_excl_u64", scan_excl_u64(npo.p, ooff.p, N, g_ar, g_s));
    K5Args a{};
    a.order = dorder.p;
    a.meta = meta.p;
    a.out_off = ooff.p;
    a.doc_recoff = dro.p;
    a.doc_npairs = dnp.p;
    a.doc_size = dds.p;
    a.doc_flags = dfl.p;
    a.rec_slot = drec.p;
    a.rec_cnt = drcnt.p;
    a.rank_of_slot = ros.p;
    a.df_of_rank = ddf.p;
    a.idf_idx = nullptr;
    a.idf = didf.p;
    a.idf_rank = idfr.p;
    a.idf_by_df = 0;
    a.large_list = lists.p + 1;
    a.large_count = lists.p;
    a.cls_nblk = (N + 255) / 256;
    a.cls_list = lists.p + N + 2;
    a.cls_off = clsoff.p;
    a.split_count = (uint32_t*)split.p;
    a.split_tasks = split.p + 1;
    a.split_cap = (uint32_t)cap_t;
    a.ndocs = N;
    a.nterms = V;
    a.rank_bits = rank_bits;
    a.rec_total = L.R_total;
    a.slot_cap = 16;
    a.status = g_status;
    a.out_term = oterm.p;
    a.out_cnt = ocnt.p;
    a.out_score = oscore.p;
    a.rec_pack = 1;
    a.pack_cb = cb;
    end_stage(what + " launch_score_order (packed)", launch_score_order(a, g_ar, g_s, g_s2, g_ev0, g_ev1));
    const uint32_t nb = a.cls_nblk;
    const uint32_t c1 = word_at(clsoff.p + nb), c2 = word_at(clsoff.p + 2 * nb), c3 = word_at(clsoff.p + 3 * nb);
    if (c1 != xsmall || c2 - c1 != xwave || c3 - c2 != xlarge || word_at(lists.p) != 0u || word_at((const uint32_t*)split.p) != 0u) {
        printf("MISMATCH %s (%s): classes small/wave/large %u/%u/%u, expected %u/%u/%u, no hand-off, no chunk task\n", what.c_str(),
               sz.c_str(), c1, c2 - c1, c3 - c2, xsmall, xwave, xlarge);
        exit(1);
    }
    const std::vector<uint64_t> goff = ooff.down();
    for (uint32_t i = 0; i <= N; ++i) if (goff[i] != xoff[i]) fail(what, sz, i, "out_off");
    const std::vector<uint32_t> gt = oterm.down(), gc = ocnt.down();
    const std::vector<double> gsd = oscore.down();
    for (uint64_t o = 0; o < Pmax; ++o) {
        uint64_t sb;
        memcpy(&sb, &gsd[o], 8);
        if (gt[o] != xterm[o]) fail(what, sz, o, "out_term");
        if (gc[o] != xcnt[o]) fail(what, sz, o, gc[o] == POISON ? "out_cnt: the poisoned rec_cnt was read" : "out_cnt");
        if (sb != xscore[o]) fail(what, sz, o, "out_score bits");
    }
    if (gt[Pmax] != 0xFFFFFFFFu || gc[Pmax] != 0xFFFFFFFFu) fail(what, sz, Pmax, "output behind the pairs");
    printf("ok  %s score (%s; small/wave/large %u/%u/%u)\n", what.c_str(), sz.c_str(), xsmall, xwave, xlarge);
}

/* rec_cnt as the run leaves it: poison under the packed records, the presorted counts behind */
static void upload_counts(const Layout& L, DBuf<uint32_t>& drcnt) {
    std::vector<uint32_t> h(L.R_total, POISON);
    for (uint64_t i = L.R_main; i < L.R_total; ++i) h[i] = L.pcnt[i - L.R_main];
    drcnt.up(h);
}

static void chain_group() {
    Rng g(20260417);
    struct { uint32_t V, sbits; uint64_t min_main; } cases[] = {
        {2, 20, 0}, {512, 20, 0}, {300, 10, 0}, {2048, 22, 0}, {1025, 11, 0}, {65536, 20, 0}, {40000, 16, 70000}};
    for (auto& k : cases) {
        const uint32_t rb = rank_bits_of(k.V);
        /* the count field after K1 (32 - sbits bits) is the narrower one: rank_bits <= sbits */
        const uint32_t cmax = (1u << (32 - k.sbits)) - 1u;
        const Corpus c = make_corpus(k.V, cmax, k.min_main, g);
        const Layout L = lay_out(c, g);
        const SlotMap sm{1ull << k.sbits, g() | 1, g()};
        const std::string name = fmt("chain V=%u rank_bits=%u sbits=%u", k.V, rb, k.sbits);
        DBuf<uint32_t> drec("rec_slot", L.R_total), drcnt("rec_cnt", L.R_total);
        upload_counts(L, drcnt);
        if (k.min_main) {   /* the wide form: one workgroup over all records */
            run_df_packed(name + " one workgroup", L, k.V, k.sbits, sm, true, 1, true, drec);
            run_score_packed(name + " one workgroup", c, L, drec, drcnt, g);
        }
        run_df_packed(name + " rank_of_slot", L, k.V, k.sbits, sm, false, 0, false, drec);
        run_df_packed(name, L, k.V, k.sbits, sm, true, 0, false, drec);
        run_score_packed(name, c, L, drec, drcnt, g);
        const std::vector<uint32_t> gc = drcnt.down();
        for (uint64_t i = 0; i < L.R_main; ++i) if (gc[i] != POISON) fail(name, "rec_cnt", i, "rec_cnt under the packed records written");
    }
}

/* rank_bits past the LDS histogram's V: the words as a packed DF pass would leave them */
static void score_group() {
    Rng g(20260418);
    const uint32_t Vs[] = {(1u << 21) - 5u, (1u << 22) - 3u, 65536u};
    for (uint32_t V : Vs) {
        const uint32_t rb = rank_bits_of(V), cb = 32u - rb;
        const Corpus c = make_corpus(V, (1u << cb) - 1u, 0, g);   /* counts up to the whole field */
        const Layout L = lay_out(c, g);
        std::vector<uint32_t> h(L.R_total);
        for (uint64_t i = 0; i < L.R_main; ++i) h[i] = (L.mrank[i] << cb) | L.mcnt[i];
        for (uint64_t i = L.R_main; i < L.R_total; ++i) h[i] = L.prank[i - L.R_main];
        DBuf<uint32_t> drec("rec_slot", L.R_total), drcnt("rec_cnt", L.R_total);
        drec.up(h);
        upload_counts(L, drcnt);
        run_score_packed(fmt("score V=%u rank_bits=%u", V, rb), c, L, drec, drcnt, g);
    }
}

/* a slot at or past the capacity: ST_BOUNDS, the other records counted */
static void guard_group() {
    const uint32_t V = 100, sbits = 12;
    const uint64_t cap = 3000;   /* below 1 << sbits: slots 3000..4095 are representable and invalid */
    std::vector<uint32_t> ros(cap, 0xFFFFFFFFu);
    std::vector<uint16_t> r16(cap, (uint16_t)0xFFFF);
    for (uint32_t r = 0; r < V; ++r) { ros[7 * r] = r; r16[7 * r] = (uint16_t)r; }
    std::vector<uint32_t> in(500);
    for (uint32_t i = 0; i < 500; ++i) in[i] = ((1u + i) << sbits) | (7u * (i % V));
    in[123] = (5u << sbits) | 3000u;
    in[499] = (9u << sbits) | 4095u;
    DBuf<uint32_t> drec("rec_slot", 500), dros("rank_of_slot", cap), ddf("df", V);
    DBuf<uint16_t> d16("rank16", cap);
    drec.up(in); dros.up(ros); d16.up(r16);
    begin_case();
    end_stage("guard launch_df_hist (packed)",
              launch_df_hist(drec.p, 500, nullptr, 500, dros.p, d16.p, V, cap, g_status, ddf.p, g_ar, g_s, false, sbits), ST_BOUNDS);
    const std::vector<uint32_t> gd = ddf.down();
    uint64_t tot = 0;
    for (uint32_t r = 0; r < V; ++r) tot += gd[r];
    if (tot != 498) fail("guard", "V=100 nrec=500", tot, "df total with two records dropped");
    printf("ok  guard: a slot past the capacity sets ST_BOUNDS\n");
}

static void unpack_group() {
    Rng g(20260419);
    const uint64_t ns[] = {1, 3, 4, 5, 1023, 1024, 4099, 100001};
    for (uint64_t n : ns) {
        for (uint32_t sbits : {10u, 20u, 22u}) {
            std::vector<uint32_t> in(n + 7), xs(n + 7), xc(n + 7);
            for (uint64_t i = 0; i < n + 7; ++i) {
                in[i] = (uint32_t)g();
                if (i % 5 == 0) in[i] |= 0xFFFFFFFFu << sbits;         /* the field's maximum */
                if (i % 7 == 0) in[i] = (1u << sbits) | (in[i] & ((1u << sbits) - 1u));   /* count 1 */
                xs[i] = i < n ? in[i] & ((1u << sbits) - 1u) : in[i];
                xc[i] = i < n ? in[i] >> sbits : POISON;
            }
            DBuf<uint32_t> ds("rec_slot", n + 7), dc("rec_cnt", n + 7);
            ds.up(in);
            dc.up(std::vector<uint32_t>(n + 7, POISON));
            begin_case();
            end_stage("unpack launch_rec_unpack", launch_rec_unpack(ds.p, dc.p, n, sbits, g_s));
            const std::vector<uint32_t> gs = ds.down(), gc = dc.down();
            const std::string sz = fmt("n=%llu sbits=%u", (unsigned long long)n, sbits);
            for (uint64_t i = 0; i < n + 7; ++i) {
                if (gs[i] != xs[i]) fail("unpack", sz, i, i < n ? "slot" : "rec_slot behind the records");
                if (gc[i] != xc[i]) fail("unpack", sz, i, i < n ? "count" : "rec_cnt behind the records");
            }
        }
        printf("ok  unpack n=%llu\n", (unsigned long long)n);
    }
}

int main(int argc, char** argv) {
    const std::string grp = argc > 1 ? argv[1] : "";
    if (grp != "chain" && grp != "score" && grp != "guard" && grp != "unpack") {
        fprintf(stderr, "usage: %s chain|score|guard|unpack\n", argv[0]);
        return 2;
    }
    CK(hipSetDevice(0));
    CK(hipStreamCreate(&g_s));
    CK(hipStreamCreate(&g_s2));
    CK(hipEventCreateWithFlags(&g_ev0, hipEventDisableTiming));
    CK(hipEventCreateWithFlags(&g_ev1, hipEventDisableTiming));
    g_ar_bytes = 64ull << 20;
    CK(hipMalloc((void**)&g_ar.base, g_ar_bytes));
    CK(hipMalloc((void**)&g_status, 4));
    if (grp == "chain") chain_group();
    if (grp == "score") score_group();
    if (grp == "guard") guard_group();
    if (grp == "unpack") unpack_group();
    CK(hipStreamSynchronize(g_s));
    CK(hipFree(g_status));
    CK(hipFree(g_ar.base));
    CK(hipEventDestroy(g_ev0));
    CK(hipEventDestroy(g_ev1));
    CK(hipStreamDestroy(g_s2));
    CK(hipStreamDestroy(g_s));
    printf("ALL OK\n");
    return 0;
}
