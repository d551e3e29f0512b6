/* GPU test of the stages of csrc/finalize.hip behind the tokenize-and-count kernel, each on
 * records crafted for it and compared with a plain host loop: the partial-record merge
 * (launch_part_heads, scan_excl_u32, launch_part_merge), the document-frequency histogram in
 * its four forms (launch_df_hist: LDS narrow, LDS wide, sliced, device atomics) and the
 * score-and-order stage (launch_gather_meta, scan_excl_u64, launch_score_order).  Links only
 * build/finalize.o and build/prims.o: no engine, no corpus.
 *
 *   finalize_test merge | df | score | chain
 *
 * One "ok  " line per case; "ALL OK" at the end.  Any HIP error or negative launcher return
 * ends the program at once (exit 2) without another launch; a mismatch prints the case, its
 * sizes, the first differing index and the field and ends it too (exit 1).  Integers are
 * compared exactly and scores as bit patterns: the kernels do one division and one
 * multiplication in binary64, each rounded, and so does the reference (this file is compiled
 * without floating-point contraction).  Every case also requires a zero status word, an
 * empty arena afterwards, that every output position was written (the outputs are prefilled
 * with all-ones words, a NaN as a score) and that the 1024 elements behind every buffer still
 * hold their fill.  The thresholds the cases are built around come from kernels.h.
 *
 * The score cases prove the path they were built for: the class totals k_k5_classify leaves
 * in cls_off, the documents the wide wave kernel hands to k_score_large (*large_count) and
 * the chunk tasks of k_emit_split (*split_count) must equal what the host derives from the
 * same thresholds.
 *
 * Not reachable through launch_score_order, so not covered here: k5_class sends every
 * document of at most K5_SMALL_DOC (128) pairs to k_score_small, and launch_score_order
 * refuses a null cls_list, so k_score_wave only ever sees documents of 129..K5_WAVE pairs.
 * Its bitonic branch (n <= 64) and its counting branch (n <= K5_CNT = 128) are dead code as
 * the launcher stands.  Only inputs the stages accept are fed (slots below slot_cap, ranks
 * below V, records inside rec_total, no unsorted document over K5_MAX_PAIRS): the ST_BOUNDS
 * guards are not under test. */
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <unordered_map>
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
static size_t g_ar_bytes;        /* the arena's allocation; g_ar.cap is what a case grants */
static uint32_t* g_status;       /* the device status word */
static uint32_t g_ncu;

typedef std::mt19937_64 Rng;

[[noreturn]] static void fail(const std::string& what, const std::string& sizes, uint64_t idx, const char* field) {
    printf("MISMATCH %s (%s) first differing index %llu (%s)\n", what.c_str(), sizes.c_str(), (unsigned long long)idx, field);
    fflush(stdout);
    exit(1);
}
[[noreturn]] static void bad_case(const std::string& what, const char* why) {
    printf("MISMATCH %s: the case does not take the path it was built for: %s\n", what.c_str(), why);
    fflush(stdout);
    exit(1);
}
static std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
static std::string fmt(const char* f, ...) {
    char b[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(b, sizeof b, f, ap);
    va_end(ap);
    return b;
}

/* ------------------------------------------------------- guarded buffers ---- */
constexpr uint64_t GUARD = 1024;       /* elements behind every buffer */
constexpr int GUARD_BYTE = 0xA7;
constexpr uint32_t GUARD_WORD = 0xA7A7A7A7u;
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
    void up(const std::vector<T>& h, uint64_t at = 0) {
        if (at + h.size() > n) { printf("harness bug: upload past a buffer\n"); exit(1); }
        if (!h.empty()) CK(hipMemcpyAsync((void*)(p + at), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, g_s));
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

static void begin_case(size_t arena_bytes) {
    if (arena_bytes > g_ar_bytes) { printf("harness bug: a case needs %zu arena bytes\n", arena_bytes); exit(1); }
    g_ar.cap = arena_bytes;
    g_ar.used = 0;
    CK(hipMemsetAsync(g_status, 0, 4, g_s));
}
/* a stage returned: its return value, the stream, the status word, the arena, the guards */
static void end_stage(const std::string& what, int rc) {
    if (rc < 0) {
        printf("%s returned %d\n", what.c_str(), rc);
        fflush(stdout);
        exit(2);
    }
    CK(hipStreamSynchronize(g_s));
    CK(hipGetLastError());
    if (g_ar.used != 0) { printf("MISMATCH %s left %zu arena bytes in use\n", what.c_str(), g_ar.used); exit(1); }
    const uint32_t st = word_at(g_status);
    if (st != 0) { printf("MISMATCH %s: status word 0x%x, expected 0\n", what.c_str(), st); exit(1); }
    std::vector<uint8_t> g;
    for (const GuardRef& r : g_guards) {
        g.assign(r.bytes, 0);
        CK(hipMemcpy(g.data(), r.p, r.bytes, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < r.bytes; ++i)
            if (g[i] != (uint8_t)GUARD_BYTE) fail(what, fmt("guard behind %s", r.name), i, "guard byte overwritten");
    }
}

/* the harness's own device code: a table entry per used slot, so that the host never holds a
 * table of 2^28 entries */
__global__ void k_scatter_u32(const uint32_t* idx, const uint32_t* val, uint32_t n, uint32_t* dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[idx[i]] = val[i];
}
__global__ void k_scatter_u16(const uint32_t* idx, const uint32_t* val, uint32_t n, uint16_t* dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[idx[i]] = (uint16_t)val[i];
}
/* dst[idx[i]] = val[i]; every idx[i] < dst_n is checked here */
template <typename T>
static void scatter(const std::vector<uint32_t>& idx, const std::vector<uint32_t>& val, T* dst, uint64_t dst_n) {
    const uint32_t n = (uint32_t)idx.size();
    if (!n) return;
    for (uint32_t i : idx)
        if (i >= dst_n) { printf("harness bug: scatter index past the table\n"); exit(1); }
    DBuf<uint32_t> di("scatter idx", n), dv("scatter val", n);
    di.up(idx);
    dv.up(val);
    if constexpr (sizeof(T) == 4) k_scatter_u32<<<(n + 255) / 256, 256, 0, g_s>>>(di.p, dv.p, n, (uint32_t*)dst);
    else k_scatter_u16<<<(n + 255) / 256, 256, 0, g_s>>>(di.p, dv.p, n, (uint16_t*)dst);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(g_s));
}

/* ======================================================================= merge ==== */
struct PRec { uint32_t doc, rank, cnt; };
constexpr uint64_t RECOFF_FILL = 0xA5A5A5A5A5A5A5A5ull;
constexpr uint32_t NPAIRS_FILL = 0x5A5A5A5Au;
constexpr uint8_t FLAGS_FILL = 0x40;
constexpr uint32_t REC_FILL = 0xEEEEEEEEu;

/* recs sorted by (doc, rank), equal keys adjacent: what the sort before the merge leaves */
static void run_merge(const std::string& what, const std::vector<PRec>& recs, uint32_t ndocs, uint64_t rec_base, Rng& rng) {
    const uint64_t n = recs.size();
    const std::string sz = fmt("n=%llu ndocs=%u rec_base=%llu", (unsigned long long)n, ndocs, (unsigned long long)rec_base);
    std::vector<uint64_t> keys(n);
    std::vector<uint32_t> seq(n), pcnt(n);
    for (uint64_t i = 0; i < n; ++i) {
        keys[i] = ((uint64_t)recs[i].doc << 32) | recs[i].rank;
        seq[i] = (uint32_t)i;
        if (i && keys[i] < keys[i - 1]) { printf("harness bug: unsorted keys\n"); exit(1); }
        if (recs[i].doc >= ndocs) { printf("harness bug: document past ndocs\n"); exit(1); }
    }
    std::shuffle(seq.begin(), seq.end(), rng);
    for (uint64_t i = 0; i < n; ++i) pcnt[seq[i]] = recs[i].cnt;
    /* reference: a stable group-by on (doc, rank) with u32 sums */
    std::vector<uint32_t> xslot(rec_base + n, REC_FILL), xcnt(rec_base + n, REC_FILL), xnp(ndocs, NPAIRS_FILL);
    std::vector<uint64_t> xoff(ndocs, RECOFF_FILL);
    std::vector<uint8_t> xfl(ndocs, FLAGS_FILL);
    for (uint64_t i = 0; i < n; ++i) xcnt[rec_base + i] = 0;
    uint64_t U = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const bool head = i == 0 || keys[i] != keys[i - 1];
        if (head) {
            const uint32_t d = recs[i].doc;
            if (i == 0 || recs[i - 1].doc != d) { xoff[d] = rec_base + U; xnp[d] = 0; xfl[d] = DF_PARTIAL | DF_PRESORTED; }
            xslot[rec_base + U] = recs[i].rank;
            ++xnp[d];
            ++U;
        }
        xcnt[rec_base + U - 1] += recs[i].cnt;
    }
    DBuf<uint64_t> dkeys("keys", n), doff("doc_recoff", ndocs);
    DBuf<uint32_t> dseq("seq", n), dpcnt("part_cnt", n), dhead("head", n + 1), dslot("rec_slot", rec_base + n),
        dcnt("rec_cnt", rec_base + n), dnp("doc_npairs", ndocs), dsor("slot_of_rank", 1);
    DBuf<uint8_t> dfl("doc_flags", ndocs);
    dkeys.up(keys); dseq.up(seq); dpcnt.up(pcnt);
    dhead.fill(0xCD);
    dslot.up(std::vector<uint32_t>(rec_base + n, REC_FILL));
    dcnt.up(std::vector<uint32_t>(rec_base + n, REC_FILL));
    doff.up(std::vector<uint64_t>(ndocs, RECOFF_FILL));
    dnp.up(std::vector<uint32_t>(ndocs, NPAIRS_FILL));
    dfl.up(std::vector<uint8_t>(ndocs, FLAGS_FILL));
    begin_case(g_ar_bytes);
    end_stage(what + " launch_part_heads", launch_part_heads(dkeys.p, n, dhead.p, g_s));
    end_stage(what + " scan_excl_u32", scan_excl_u32(dhead.p, dhead.p, n, g_ar, g_s));
    end_stage(what + " launch_part_merge",
              launch_part_merge(dkeys.p, dseq.p, dpcnt.p, dhead.p, n, dsor.p, rec_base, dslot.p, dcnt.p, doff.p, dnp.p,
                                dfl.p, g_s));
    const std::vector<uint32_t> gh = dhead.down(), gs = dslot.down(), gc = dcnt.down(), gn = dnp.down();
    const std::vector<uint64_t> go = doff.down();
    const std::vector<uint8_t> gf = dfl.down();
    if (gh[n] != (uint32_t)U) fail(what, sz, n, "merged record count (scan total)");
    for (uint64_t i = 0; i < rec_base + U; ++i)
        if (gs[i] != xslot[i]) fail(what, sz, i, i < rec_base ? "rec_slot below rec_base" : "rec_slot (rank)");
    for (uint64_t i = 0; i < rec_base + n; ++i)
        if (gc[i] != xcnt[i])
            fail(what, sz, i, i < rec_base ? "rec_cnt below rec_base" : i < rec_base + U ? "rec_cnt (sum)" : "rec_cnt behind the merged records");
    for (uint32_t d = 0; d < ndocs; ++d) {
        if (go[d] != xoff[d]) fail(what, sz, d, "doc_recoff");
        if (gn[d] != xnp[d]) fail(what, sz, d, "doc_npairs");
        if (gf[d] != xfl[d]) fail(what, sz, d, "doc_flags");
    }
}

/* appends runs to recs with ascending keys; documents change every few runs and skip ids */
struct KeyWalk {
    uint32_t doc = 3, rank = 0, left = 4;
    void next(Rng& g) {
        if (--left == 0) { doc += 1 + (uint32_t)(g() % 3); rank = (uint32_t)(g() % 5); left = 3 + (uint32_t)(g() % 7); }
        else rank += 1 + (uint32_t)(g() % 3);
    }
};
static void add_run(std::vector<PRec>& r, KeyWalk& k, uint64_t len, Rng& g) {
    for (uint64_t i = 0; i < len; ++i) r.push_back(PRec{k.doc, k.rank, 1 + (uint32_t)(g() % 1000)});
    k.next(g);
}

static void merge_group() {
    Rng g(20240607);
    const uint64_t bases[2] = {0, 12345};
    /* a run of each length behind 0..63 single-record runs, each block from a multiple of 64
     * on: the run starts at every lane of a wave, and the long ones cross wave and workgroup
     * boundaries at every alignment */
    for (uint64_t len : {1ull, 2ull, 63ull, 64ull, 65ull, 255ull, 256ull, 257ull, 6000ull}) {
        std::vector<PRec> r;
        KeyWalk k;
        for (uint32_t p = 0; p < 64; ++p) {
            while (r.size() % 64) add_run(r, k, 1, g);
            for (uint32_t q = 0; q < p; ++q) add_run(r, k, 1, g);
            add_run(r, k, len, g);
        }
        for (uint64_t b : bases) run_merge(fmt("merge run length %llu", (unsigned long long)len), r, k.doc + 10, b, g);
        printf("ok  merge run length %llu at every lane n=%zu\n", (unsigned long long)len, r.size());
    }
    {   /* a run whose counts sum to exactly 2^32 - 1, between short runs */
        std::vector<PRec> r;
        KeyWalk k;
        for (int q = 0; q < 37; ++q) add_run(r, k, 1 + g() % 3, g);
        uint64_t sum = 0;
        for (int q = 0; q < 299; ++q) {
            const uint32_t c = 1 + (uint32_t)(g() % 14000000);
            r.push_back(PRec{k.doc, k.rank, c});
            sum += c;
        }
        r.push_back(PRec{k.doc, k.rank, (uint32_t)(0xFFFFFFFFull - sum)});
        k.next(g);
        for (int q = 0; q < 20; ++q) add_run(r, k, 1 + g() % 3, g);
        for (uint64_t b : bases) run_merge("merge run summing to 2^32-1", r, k.doc + 1, b, g);
        printf("ok  merge run summing to 2^32-1 n=%zu\n", r.size());
    }
    {   /* five documents among 1000 own partial records: the others stay untouched */
        std::vector<PRec> r;
        for (uint32_t d : {0u, 7u, 500u, 998u, 999u}) {
            uint32_t rank = (uint32_t)(g() % 9);
            const uint32_t runs = 1 + (uint32_t)(g() % 40);
            for (uint32_t q = 0; q < runs; ++q) {
                const uint32_t len = 1 + (uint32_t)(g() % 4);
                for (uint32_t e = 0; e < len; ++e) r.push_back(PRec{d, rank, 1 + (uint32_t)(g() % 1000)});
                rank += 1 + (uint32_t)(g() % 100);
            }
        }
        for (uint64_t b : bases) run_merge("merge 5 documents among 1000", r, 1000, b, g);
        printf("ok  merge 5 documents among 1000 n=%zu\n", r.size());
    }
    for (uint64_t n : {1ull, 257ull, 300000ull}) {
        std::vector<PRec> r;
        KeyWalk k;
        while (r.size() < n) {
            const uint64_t x = g() % 100;
            uint64_t len = x < 70 ? 1 : x < 90 ? 2 + g() % 4 : x < 99 ? 6 + g() % 195 : 200 + g() % 2800;
            if (len > n - r.size()) len = n - r.size();
            add_run(r, k, len, g);
        }
        for (uint64_t b : bases) run_merge(fmt("merge random runs n=%llu", (unsigned long long)n), r, k.doc + 2, b, g);
        printf("ok  merge random runs n=%llu\n", (unsigned long long)n);
    }
}

/* ========================================================================== DF ==== */
/* dfh_cslot of finalize.hip: the entry of the LDS slot -> rank cache a slot maps to.  Only
 * used to make a few slots share an entry on purpose where V is too small for chance. */
static uint32_t cache_entry(uint32_t slot) { return (slot * 0x9E3779B1u) >> 20; }

/* A sparse slot table over slot_cap = 2^k entries: the slot of rank r is a bijection of r,
 * so used slots are scattered and distinct.  The device tables hold INVALID_SLOT elsewhere. */
struct SlotTable {
    uint64_t cap, mul, add;
    std::unordered_map<uint32_t, uint32_t> special;   /* ranks whose slots collide in the LDS cache */
    uint32_t of(uint32_t r) const {
        auto it = special.find(r);
        return it != special.end() ? it->second : (uint32_t)((r * mul + add) & (cap - 1));
    }
    SlotTable(uint64_t cap_, uint32_t V, bool collide, Rng& g) : cap(cap_), mul(g() | 1), add(g()) {
        if (!collide) return;
        /* the images of indices >= V are no rank's slot: the first few ranks take those that
         * share the cache entry of the first one found */
        const uint32_t want = V < 8 ? V : 8;
        uint32_t e0 = 0;
        for (uint64_t t = V; t < cap && special.size() < want; ++t) {
            const uint32_t s = (uint32_t)((t * mul + add) & (cap - 1));
            if (special.empty()) e0 = cache_entry(s);
            if (cache_entry(s) == e0) { const uint32_t r = (uint32_t)special.size(); special[r] = s; }
        }
    }
};

enum DfForm { DF_LDS_NARROW, DF_LDS_WIDE, DF_SLICED, DF_ATOMIC };
struct DfCase {
    std::string name;
    uint32_t V = 0;
    std::vector<uint32_t> main_ranks;     /* the ranks of the slot records [0, nrec) */
    std::vector<uint32_t> merged_ranks;   /* the merged records behind them */
    uint64_t nrec_max = 0;
    bool extra_null = false;              /* nrec_extra == nullptr (no merged records then) */
    bool use16 = false;
    int force_wgs = 0;                    /* TFIDF_DF_WGS */
    DfForm form = DF_LDS_NARROW;
};
static uint32_t df_pattern(uint32_t r) { return ((r * 2654435761u) >> 9) + 1u; }

static void run_df(const DfCase& c, Rng& g) {
    const uint32_t V = c.V;
    const uint64_t nrec = c.main_ranks.size(), nm = c.merged_ranks.size();
    if (c.extra_null && nm) { printf("harness bug: merged records without nrec_extra\n"); exit(1); }
    if (nrec + nm > c.nrec_max || c.nrec_max == 0) { printf("harness bug: nrec_max\n"); exit(1); }
    const bool giant = V > (1u << 20);
    const uint64_t slot_cap = giant ? 1ull << 28 : [&] { uint64_t p = 65536; while (p < 8ull * V) p <<= 1; return p; }();
    const std::string sz = fmt("V=%u nrec=%llu merged=%llu nrec_max=%llu slot_cap=%llu %s%s", V, (unsigned long long)nrec,
                               (unsigned long long)nm, (unsigned long long)c.nrec_max, (unsigned long long)slot_cap,
                               c.use16 ? "rank16" : "rank_of_slot", c.extra_null ? " nrec_extra=null" : "");
    for (uint32_t r : c.main_ranks) if (r >= V) { printf("harness bug: rank past V\n"); exit(1); }
    for (uint32_t r : c.merged_ranks) if (r >= V) { printf("harness bug: rank past V\n"); exit(1); }
    /* the form this case was built for, from the thresholds of kernels.h and the plan that
     * df_hist_scratch reports */
    if (c.force_wgs) setenv("TFIDF_DF_WGS", std::to_string(c.force_wgs).c_str(), 1);
    const size_t scratch = df_hist_scratch(c.nrec_max, V);
    const uint64_t nsl = ((uint64_t)V + DFS_SLICE - 1) / DFS_SLICE;
    if (V <= DFH_MAXV) {
        const uint64_t nparts = (scratch - 256) / ((uint64_t)((V + 1) / 2) * 4);
        const uint64_t per = nparts ? (c.nrec_max + nparts - 1) / nparts : 0;
        if (c.form == DF_LDS_NARROW && !(nparts >= 1 && per <= DFH_RECS)) bad_case(c.name, "not the narrow LDS form");
        if (c.form == DF_LDS_WIDE && !(nparts == (uint64_t)c.force_wgs && per > DFH_RECS)) bad_case(c.name, "not the wide LDS form");
        if (c.form != DF_LDS_NARROW && c.form != DF_LDS_WIDE) bad_case(c.name, "V takes an LDS form");
    } else if (nsl <= DFS_MAXSL) {
        if (c.form != DF_SLICED) bad_case(c.name, "V takes the sliced form");
    } else if (c.form != DF_ATOMIC) bad_case(c.name, "V takes the atomic fallback");

    SlotTable st(slot_cap, V, !giant, g);
    DBuf<uint32_t> ros("rank_of_slot", slot_cap);
    ros.fill(0xFF);
    DBuf<uint16_t> r16("rank16", c.use16 ? slot_cap : 1);
    r16.fill(0xFF);
    {   /* every rank's slot, or (giant V) those of the ranks in use */
        std::vector<uint32_t> rk;
        if (!giant) { rk.resize(V); for (uint32_t r = 0; r < V; ++r) rk[r] = r; }
        else { rk = c.main_ranks; std::sort(rk.begin(), rk.end()); rk.erase(std::unique(rk.begin(), rk.end()), rk.end()); }
        std::vector<uint32_t> sl(rk.size());
        for (size_t i = 0; i < rk.size(); ++i) sl[i] = st.of(rk[i]);
        {   /* the table is a bijection: no two ranks share a slot */
            std::vector<uint32_t> t = sl;
            std::sort(t.begin(), t.end());
            if (std::adjacent_find(t.begin(), t.end()) != t.end()) { printf("harness bug: two ranks share a slot\n"); exit(1); }
        }
        scatter(sl, rk, ros.p, slot_cap);
        if (c.use16) scatter(sl, rk, r16.p, slot_cap);
    }
    std::vector<uint32_t> recs(c.nrec_max, GUARD_WORD);   /* behind the records: never a valid slot or rank */
    for (uint64_t i = 0; i < nrec; ++i) recs[i] = st.of(c.main_ranks[i]);
    for (uint64_t i = 0; i < nm; ++i) recs[nrec + i] = c.merged_ranks[i];
    std::vector<uint32_t> xrec = recs;
    for (uint64_t i = 0; i < nrec; ++i) xrec[i] = c.main_ranks[i];
    std::vector<uint32_t> counts(V, 0);
    for (uint32_t r : c.main_ranks) ++counts[r];
    for (uint32_t r : c.merged_ranks) ++counts[r];

    DBuf<uint32_t> drec("rec_slot", c.nrec_max), ddf("df", V), dex("nrec_extra", 1);
    dex.up(std::vector<uint32_t>(1, (uint32_t)nm));
    std::vector<uint32_t> x(V);
    for (int acc = 0; acc < 2; ++acc) {
        const std::string what = c.name + (acc ? " accumulate" : " overwrite");
        drec.up(recs);
        if (acc) { for (uint32_t r = 0; r < V; ++r) x[r] = df_pattern(r); ddf.up(x); }
        else ddf.fill(0xCD);
        for (uint32_t r = 0; r < V; ++r) x[r] = (acc ? df_pattern(r) : 0u) + counts[r];
        begin_case((scratch + 255) & ~(size_t)255);
        end_stage(what + " launch_df_hist",
                  launch_df_hist(drec.p, nrec, c.extra_null ? nullptr : dex.p, c.nrec_max, ros.p, c.use16 ? r16.p : nullptr, V,
                                 slot_cap, g_status, ddf.p, g_ar, g_s, acc != 0));
        const std::vector<uint32_t> gd = ddf.down(), gr = drec.down();
        if (memcmp(gd.data(), x.data(), (size_t)V * 4))
            for (uint32_t r = 0; r < V; ++r) if (gd[r] != x[r]) fail(what, sz, r, "df");
        for (uint64_t i = 0; i < c.nrec_max; ++i)
            if (gr[i] != xrec[i]) fail(what, sz, i, i < nrec ? "record rewritten to its rank" : i < nrec + nm ? "merged record" : "record array behind the records");
    }
    if (c.force_wgs) unsetenv("TFIDF_DF_WGS");
}

/* n ranks: a share at the hot ranks, the rest uniform */
static std::vector<uint32_t> hot_ranks(uint64_t n, uint32_t V, const std::vector<uint32_t>& hot, Rng& g) {
    std::vector<uint32_t> r(n);
    for (auto& x : r) x = (!hot.empty() && g() % 10 < 7) ? hot[g() % hot.size()] : (uint32_t)(g() % V);
    return r;
}

static void df_group() {
    Rng g(777);
    /* ---- the LDS form, narrow ---- */
    for (uint32_t V : {1u, 2u, 3u, DFH_MAXV - 1, DFH_MAXV}) {
        std::vector<uint32_t> hot = {0u, V - 1, V > 1 ? V - 2 : 0u, V / 2};
        for (int use16 = 0; use16 < 2; ++use16) {
            struct Shape { uint64_t nrec, nm, slack; bool extra_null; const char* tag; };
            const Shape shapes[] = {
                {10007, 0, 0, true, "nrec_extra null"},
                {10007, 0, 500, false, "nrec_extra -> 0"},
                {10007, 3001, 0, false, "nrec_extra exact, ranked_from 10007 inside a workgroup"},
                {10007, 3001, 20000, false, "nrec_extra fewer: idle trailing workgroups"},
                {0, 5000, 0, false, "merged records only"},
                {200003, 0, 0, true, "several workgroups"},
            };
            for (const Shape& s : shapes) {
                DfCase c;
                c.name = fmt("df lds narrow V=%u %s, %s", V, use16 ? "rank16" : "rank_of_slot", s.tag);
                c.V = V;
                c.main_ranks = hot_ranks(s.nrec, V, hot, g);
                c.merged_ranks = hot_ranks(s.nm, V, hot, g);
                c.nrec_max = s.nrec + s.nm + s.slack;
                c.extra_null = s.extra_null;
                c.use16 = use16 != 0;
                c.form = DF_LDS_NARROW;
                run_df(c, g);
            }
            printf("ok  df lds narrow V=%u %s\n", V, use16 ? "rank16" : "rank_of_slot");
            fflush(stdout);
        }
    }
    /* ---- the LDS form, wide: two workgroups of 200 000 records; inside one of them a rank
     * occurs exactly c times, so its u16 counter meets every carry-out edge ---- */
    {
        const uint32_t V = 1000;
        const uint64_t per = 200000, nm = 1000;
        auto wide_case = [&](const std::string& name, int wg, const std::vector<std::pair<uint32_t, uint32_t>>& hotc, bool use16) {
            DfCase c;
            c.name = name;
            c.V = V;
            c.nrec_max = 2 * per;
            c.use16 = use16;
            c.force_wgs = 2;
            c.form = DF_LDS_WIDE;
            auto is_hot = [&](uint32_t r) { for (auto& h : hotc) if (h.first == r) return true; return false; };
            auto cold = [&]() { uint32_t r; do r = (uint32_t)(g() % V); while (is_hot(r)); return r; };
            /* workgroup wg's range: the hot ranks exactly c times each; the other range: 3 times */
            std::vector<uint32_t> half[2];
            for (int h = 0; h < 2; ++h) {
                const uint64_t len = h == 0 ? per : per - nm;   /* the merged records end workgroup 1's range */
                for (auto& hc : hotc) half[h].insert(half[h].end(), h == wg ? hc.second : 3u, hc.first);
                if (half[h].size() > len) { printf("harness bug: hot records over a workgroup's range\n"); exit(1); }
                while (half[h].size() < len) half[h].push_back(cold());
                std::shuffle(half[h].begin(), half[h].end(), g);
            }
            c.main_ranks = half[0];
            c.main_ranks.insert(c.main_ranks.end(), half[1].begin(), half[1].end());
            for (uint64_t i = 0; i < nm; ++i) c.merged_ranks.push_back(cold());
            run_df(c, g);
        };
        int k = 0;
        for (uint32_t cnt : {0x7FFFu, 0x8000u, 0x8001u, 0xFFFFu, 0x10000u, 0x17FFFu, 0x18000u, 0x20001u})
            for (uint32_t rank : {500u, 501u}) {
                const std::string name = fmt("df lds wide rank %u x 0x%x", rank, cnt);
                wide_case(name, k & 1, {{rank, cnt}}, (k >> 1) & 1);
                ++k;
                printf("ok  %s\n", name.c_str());
                fflush(stdout);
            }
        wide_case("df lds wide both halves of a bin word", 0, {{500u, 0x8000u}, {501u, 0xFFFFu}}, false);
        printf("ok  df lds wide both halves of a bin word (0x8000 and 0xffff)\n");
    }
    /* ---- the sliced form ---- */
    for (uint32_t V : {DFH_MAXV + 1, 3 * DFS_SLICE, 3 * DFS_SLICE + 1, 5 * DFS_SLICE - 1}) {
        std::vector<uint32_t> hot = {0u, V - 1};
        for (uint32_t e = DFS_SLICE; e < V; e += DFS_SLICE) { hot.push_back(e - 1); hot.push_back(e); }
        for (uint64_t n : {(uint64_t)1, DFS_TILE - 1, DFS_TILE, DFS_TILE + 1, 3 * DFS_TILE + 1})
            for (int merged = 0; merged < 2; ++merged) {
                DfCase c;
                c.V = V;
                c.nrec_max = n;
                c.form = DF_SLICED;
                uint64_t nrec = n, nm = 0;
                if (merged) { nrec = n * 6 / 10; nm = n - nrec - (n > 10 ? 3 : 0); }
                c.extra_null = !merged;
                c.name = fmt("df sliced V=%u nrec_max=%llu%s", V, (unsigned long long)n, merged ? " with merged records" : "");
                c.main_ranks = hot_ranks(nrec, V, hot, g);
                c.merged_ranks = hot_ranks(nm, V, hot, g);
                run_df(c, g);
            }
        printf("ok  df sliced V=%u\n", V);
        fflush(stdout);
    }
    /* ---- the last V the sliced form takes, and the atomic fallback one past it ---- */
    for (int past = 0; past < 2; ++past) {
        const uint32_t V = DFS_MAXSL * DFS_SLICE + (uint32_t)past;
        std::vector<uint32_t> hot = {0u, V - 1, V - 2, DFS_SLICE - 1, DFS_SLICE, (DFS_MAXSL - 1) * DFS_SLICE - 1, (DFS_MAXSL - 1) * DFS_SLICE};
        for (int q = 0; q < 20; ++q) { const uint32_t e = (uint32_t)(1 + g() % (DFS_MAXSL - 1)) * DFS_SLICE; hot.push_back(e - 1); hot.push_back(e); }
        DfCase c;
        c.V = V;
        c.form = past ? DF_ATOMIC : DF_SLICED;
        c.name = fmt("df %s V=%u", past ? "atomic fallback" : "sliced, last V", V);
        c.main_ranks = hot_ranks(30011, V, hot, g);
        c.merged_ranks = hot_ranks(19997, V, hot, g);
        c.nrec_max = 30011 + 19997 + 5;
        run_df(c, g);
        printf("ok  %s\n", c.name.c_str());
        fflush(stdout);
    }
}

/* ======================================================================= score ==== */
/* documents and their records as K5 reads them (ranks in the records, as after DF) */
struct Corpus {
    uint32_t V = 0;
    std::vector<uint32_t> np, dsize, rrank, rcnt;
    std::vector<uint64_t> recoff;
    std::vector<uint8_t> flags;
    void add(const std::vector<uint32_t>& ranks, bool presorted, Rng& g) {
        if (!presorted && ranks.size() > (size_t)K5_MAX_PAIRS) { printf("harness bug: unsorted document over K5_MAX_PAIRS\n"); exit(1); }
        np.push_back((uint32_t)ranks.size());
        recoff.push_back(ranks.empty() ? 0 : rrank.size());
        flags.push_back(presorted ? (uint8_t)(DF_PARTIAL | DF_PRESORTED) : (uint8_t)0);
        dsize.push_back(g() % 8 == 0 ? 0xFFFFFFFFu : 1u + (uint32_t)(g() % 1000000));
        for (uint32_t r : ranks) {
            if (r >= V) { printf("harness bug: rank past V\n"); exit(1); }
            rrank.push_back(r);
            rcnt.push_back(g() % 16 == 0 ? 70000u : 1u + (uint32_t)(g() % 70000));
        }
    }
};
enum RankOrder { RO_RANDOM, RO_ASC, RO_DESC };
/* n distinct ranks below V, one from each of n strata; the ends 0 and V - 1 half of the time */
static std::vector<uint32_t> some_ranks(uint32_t n, uint32_t V, RankOrder o, Rng& g) {
    if (n > V) { printf("harness bug: %u distinct ranks below %u\n", n, V); exit(1); }
    std::vector<uint32_t> r(n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t lo = (uint64_t)i * V / n, hi = (uint64_t)(i + 1) * V / n;
        r[i] = (uint32_t)(lo + g() % (hi - lo));
    }
    if (n && g() % 2) r[0] = 0;
    if (n > 1 && g() % 2) r[n - 1] = V - 1;
    if (o == RO_RANDOM) std::shuffle(r.begin(), r.end(), g);
    if (o == RO_DESC) std::reverse(r.begin(), r.end());
    return r;
}
static std::vector<uint32_t> consecutive(uint32_t first, uint32_t n, bool shuffled, Rng& g) {
    std::vector<uint32_t> r(n);
    for (uint32_t i = 0; i < n; ++i) r[i] = first + i;
    if (shuffled) std::shuffle(r.begin(), r.end(), g);
    return r;
}
static uint32_t rank_bits_of(uint32_t V) { return V > 1 ? 32u - (uint32_t)__builtin_clz(V - 1) : 1u; }
/* the fullest bucket of a document under a bucket sort by the top nbb of rank_bits bits */
static uint32_t bucket_max(const uint32_t* r, uint32_t n, uint32_t rank_bits, uint32_t nbb) {
    const uint32_t hsh = rank_bits > nbb ? rank_bits - nbb : 0u;
    std::unordered_map<uint32_t, uint32_t> h;
    uint32_t mx = 0;
    for (uint32_t i = 0; i < n; ++i) mx = std::max(mx, ++h[r[i] >> hsh]);
    return mx;
}
/* n ranks of which exactly `target` share one bucket (nbb bucket bits) and no other bucket
 * holds as many */
static std::vector<uint32_t> bucket_doc(uint32_t n, uint32_t V, uint32_t nbb, uint32_t target, Rng& g) {
    const uint32_t rb = rank_bits_of(V), hsh = rb > nbb ? rb - nbb : 0u, w = 1u << hsh, nb = V / w;
    if (w < target || n < target || nb < 3 || target < 3) { printf("harness bug: bucket_doc\n"); exit(1); }
    const uint32_t hb = nb / 2;
    std::vector<uint32_t> r = consecutive(hb * w, w, true, g);
    r.resize(target);
    for (uint32_t pass = 0, b = 0; r.size() < n; ++b) {
        if (b == nb) { b = 0; ++pass; }
        if (pass >= target - 1 || pass >= w) { printf("harness bug: bucket_doc cannot spread the rest\n"); exit(1); }
        if (b != hb) r.push_back(b * w + (pass * 7 + 3) % w);
    }
    std::shuffle(r.begin(), r.end(), g);
    return r;
}
/* k_score_large's bucket bits for a document of n pairs (launch_score_large's two instances) */
static uint32_t large_nbb(uint32_t n) { return n <= (uint32_t)K5_MAX_PAIRS / 2 ? 10u : 11u; }

/* the idf table K5 is given and the host's view of it */
struct IdfTable {
    bool full;
    uint32_t V, Ntot, dflt;
    std::vector<uint32_t> dfv;                          /* df of every rank (V <= 2^23) */
    std::unordered_map<uint32_t, uint32_t> patch;       /* or the default and the ranks in use */
    std::vector<uint32_t> idx;                          /* distinct table: df -> index */
    std::vector<double> idf;
    uint32_t df_of(uint32_t r) const {
        if (!dfv.empty()) return dfv[r];
        auto it = patch.find(r);
        return it == patch.end() ? dflt : it->second;
    }
    double idf_of(uint32_t r) const { const uint32_t d = df_of(r); return full ? idf[d] : idf[idx[d]]; }
    IdfTable(bool full_, uint32_t V_, const std::vector<uint32_t>& used_ranks, Rng& g) : full(full_), V(V_), Ntot(1000003) {
        std::vector<uint32_t> vals;   /* the df values in use */
        if (full) {
            idf.resize((size_t)Ntot + 1);
            idf[0] = 0.0;
            for (uint32_t k = 1; k <= Ntot; ++k) idf[k] = log(1.0 * (double)Ntot / (double)k);
        } else {
            for (int k = 0; k < 97; ++k) vals.push_back(1 + (uint32_t)(g() % Ntot));
            std::sort(vals.begin(), vals.end());
            vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
            idx.assign((size_t)Ntot + 2, 0);   /* the exclusive scan of the presence flags */
            for (size_t k = 0, x = 0; x < idx.size(); ++x) { idx[x] = (uint32_t)k; if (k < vals.size() && vals[k] == x) ++k; }
            idf.resize(vals.size() + 1, 0.0);
            for (size_t k = 0; k < vals.size(); ++k) idf[k] = log(1.0 * (double)Ntot / (double)vals[k]);
        }
        auto pick = [&]() { return full ? 1 + (uint32_t)(g() % Ntot) : vals[g() % vals.size()]; };
        dflt = pick();
        if (V <= (1u << 23)) { dfv.resize(V); for (auto& d : dfv) d = pick(); }
        else for (uint32_t r : used_ranks) patch[r] = pick();
    }
};

/* what K5 is run on: device arrays and the host's view of them */
struct ScoreIn {
    uint32_t N, V;
    uint64_t rec_total;
    const uint32_t *d_np, *d_dsize, *d_rslot, *d_rcnt, *d_df, *d_idf_idx;
    const uint64_t* d_recoff;
    const uint8_t* d_flags;
    const double* d_idf;
    bool full_table, with_split;
    const std::vector<uint32_t>*np, *dsize, *rrank, *rcnt;
    const std::vector<uint64_t>* recoff;
    const std::vector<uint8_t>* flags;
    std::function<double(uint32_t)> idf_of;
};
struct ScorePaths { uint32_t nsmall = 0, nwave = 0, nlarge = 0, ntasks = 0, nhand = 0; };

static ScorePaths run_score(const std::string& what, const ScoreIn& in, Rng& g) {
    const uint32_t N = in.N, V = in.V;
    const uint32_t rank_bits = rank_bits_of(V);
    const bool wide = rank_bits + K5_IDX_BITS > 32;
    const uint32_t by_df = (in.full_table && V > (1u << 21)) ? 1u : 0u;
    const std::string sz = fmt("ndocs=%u V=%u records=%llu %s idf table%s%s", N, V, (unsigned long long)in.rec_total,
                               in.full_table ? "full" : "distinct-df", by_df ? " (idf by df)" : "", in.with_split ? "" : " split_count=null");
    std::vector<uint32_t> order(N);
    for (uint32_t i = 0; i < N; ++i) order[i] = i;
    std::shuffle(order.begin(), order.end(), g);
    if (N > 1 && std::is_sorted(order.begin(), order.end())) std::swap(order[0], order[1]);
    /* the host's expectation: offsets, classes, hand-offs, chunk tasks, pairs */
    ScorePaths x;
    std::vector<uint64_t> xoff(N + 1, 0);
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t d = order[i], n = (*in.np)[d];
        const bool pres = ((*in.flags)[d] & DF_PRESORTED) != 0;
        xoff[i + 1] = xoff[i] + n;
        if (n && (*in.recoff)[d] + n > in.rec_total) { printf("harness bug: records past rec_total\n"); exit(1); }
        if (n == 0) continue;
        if (n <= K5_SMALL_DOC) ++x.nsmall;
        else if (n <= K5_WAVE) {
            ++x.nwave;
            if (wide && !pres && bucket_max(in.rrank->data() + (*in.recoff)[d], n, rank_bits, K5_NB_BITS) > K5_GROUP_MAX) ++x.nhand;
        } else if (pres && n > K5_PS_SPLIT && in.with_split) x.ntasks += (n + K5_PS_SPLIT - 1) / K5_PS_SPLIT;
        else ++x.nlarge;
    }
    const uint64_t P = xoff[N], Pmax = in.rec_total;
    std::vector<uint32_t> xterm(Pmax, 0xFFFFFFFFu), xcnt(Pmax, 0xFFFFFFFFu);
    std::vector<uint64_t> xscore(Pmax, ~0ull);
    std::vector<std::pair<uint32_t, uint32_t>> rc;
    for (uint32_t i = 0; i < N; ++i) {
        const uint32_t d = order[i], n = (*in.np)[d];
        const uint64_t rb = n ? (*in.recoff)[d] : 0;
        rc.resize(n);
        for (uint32_t j = 0; j < n; ++j) rc[j] = {(*in.rrank)[rb + j], (*in.rcnt)[rb + j]};
        if (!((*in.flags)[d] & DF_PRESORTED))
            std::sort(rc.begin(), rc.end(), [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) { return a.first < b.first; });
        const double ds = (double)(*in.dsize)[d];
        for (uint32_t j = 0; j < n; ++j) {
            const double score = ((double)rc[j].second / ds) * in.idf_of(rc[j].first);
            xterm[xoff[i] + j] = rc[j].first;
            xcnt[xoff[i] + j] = rc[j].second;
            memcpy(&xscore[xoff[i] + j], &score, 8);
        }
    }
    /* the buffers, sized as the engine sizes them */
    DBuf<uint32_t> dorder("order", N), lists("large_list + cls_list", 2ull * N + 4), clsoff("cls_off", 3ull * ((N + 255) / 256) + 8),
        oterm("out_term", Pmax + 1), ocnt("out_cnt", Pmax + 1), ros("rank_of_slot", 4096);
    const uint64_t cap_t = 2 * in.rec_total / 4096 + 64;
    DBuf<uint2> split("split_tasks", cap_t + 1);
    DBuf<uint64_t> npo("npairs_ord", (uint64_t)N + 1), ooff("out_off", (uint64_t)N + 1);
    DBuf<uint4> meta("doc_meta", (uint64_t)N + 1);
    DBuf<double> oscore("out_score", Pmax + 1), idfr("idf_rank", (uint64_t)V + 1);
    dorder.up(order);
    lists.fill(0xCD); clsoff.fill(0xCD); split.fill(0xCD); npo.fill(0xCD); ooff.fill(0xCD); meta.fill(0xCD); idfr.fill(0xCD);
    ros.fill(0xFF);
    oterm.fill(0xFF); ocnt.fill(0xFF); oscore.fill(0xFF);
    begin_case(g_ar_bytes);
    end_stage(what + " launch_gather_meta",
              launch_gather_meta(dorder.p, in.d_np, in.d_recoff, in.d_dsize, in.d_flags, N, npo.p, meta.p, g_s));
    end_stage(what + " scan_excl_u64", scan_excl_u64(npo.p, ooff.p, N, g_ar, g_s));
    K5Args a{};
    a.order = dorder.p;
    a.meta = meta.p;
    a.out_off = ooff.p;
    a.doc_recoff = in.d_recoff;
    a.doc_npairs = in.d_np;
    a.doc_size = in.d_dsize;
    a.doc_flags = in.d_flags;
    a.rec_slot = in.d_rslot;
    a.rec_cnt = in.d_rcnt;
    a.rank_of_slot = ros.p;
    a.df_of_rank = in.d_df;
    a.idf_idx = in.full_table ? nullptr : in.d_idf_idx;
    a.idf = in.d_idf;
    a.idf_rank = idfr.p;
    a.idf_by_df = by_df;
    a.large_list = lists.p + 1;
    a.large_count = lists.p;
    a.cls_nblk = (N + 255) / 256;
    a.cls_list = lists.p + N + 2;
    a.cls_off = clsoff.p;
    a.split_count = in.with_split ? (uint32_t*)split.p : nullptr;
    a.split_tasks = split.p + 1;
    a.split_cap = (uint32_t)cap_t;
    a.ndocs = N;
    a.nterms = V;
    a.rank_bits = rank_bits;
    a.rec_total = in.rec_total;
    a.slot_cap = 4096;
    a.status = g_status;
    a.out_term = oterm.p;
    a.out_cnt = ocnt.p;
    a.out_score = oscore.p;
    end_stage(what + " launch_score_order", launch_score_order(a, g_ar, g_s, g_s2, g_ev0, g_ev1));
    const std::vector<uint64_t> goff = ooff.down();
    for (uint32_t i = 0; i <= N; ++i) if (goff[i] != xoff[i]) fail(what, sz, i, "out_off");
    /* the paths taken */
    const uint32_t nb = a.cls_nblk;
    const uint32_t c1 = word_at(clsoff.p + nb), c2 = word_at(clsoff.p + 2 * nb), c3 = word_at(clsoff.p + 3 * nb);
    const uint32_t nhand = word_at(lists.p), ntasks = in.with_split ? word_at((const uint32_t*)split.p) : 0u;
    if (c1 != x.nsmall || c2 - c1 != x.nwave || c3 - c2 != x.nlarge || nhand != x.nhand || ntasks != x.ntasks) {
        printf("MISMATCH %s (%s): classes small/wave/large %u/%u/%u, handed off %u, chunk tasks %u; expected %u/%u/%u, %u, %u\n",
               what.c_str(), sz.c_str(), c1, c2 - c1, c3 - c2, nhand, ntasks, x.nsmall, x.nwave, x.nlarge, x.nhand, x.ntasks);
        exit(1);
    }
    const std::vector<uint32_t> gt = oterm.down(), gc = ocnt.down();
    const std::vector<double> gsd = oscore.down();
    for (uint64_t o = 0; o < Pmax; ++o) {
        uint64_t sb;
        memcpy(&sb, &gsd[o], 8);
        if (o < P && gt[o] == 0xFFFFFFFFu) fail(what, sz, o, "out_term never written");
        if (o < P && gc[o] == 0xFFFFFFFFu) fail(what, sz, o, "out_cnt never written");
        if (o < P && sb == ~0ull) fail(what, sz, o, "out_score never written");
        if (gt[o] != xterm[o]) fail(what, sz, o, o < P ? "out_term" : "out_term behind the pairs");
        if (gc[o] != xcnt[o]) fail(what, sz, o, o < P ? "out_cnt" : "out_cnt behind the pairs");
        if (sb != xscore[o]) fail(what, sz, o, o < P ? "out_score bits" : "out_score behind the pairs");
    }
    return x;
}

/* a corpus through K5 with the full and/or the distinct-df idf table */
enum Tables { T_BOTH, T_FULL, T_DISTINCT };
static ScorePaths score_corpus(const std::string& what, const Corpus& c, Tables t, bool with_split, Rng& g) {
    const uint32_t N = (uint32_t)c.np.size(), V = c.V;
    const uint64_t R = c.rrank.size();
    DBuf<uint32_t> dnp("doc_npairs", N), dds("doc_size", N), drs("rec_slot", R), drc("rec_cnt", R), ddf("df_of_rank", V);
    DBuf<uint64_t> dro("doc_recoff", N);
    DBuf<uint8_t> dfl("doc_flags", N);
    dnp.up(c.np); dds.up(c.dsize); drs.up(c.rrank); drc.up(c.rcnt); dro.up(c.recoff); dfl.up(c.flags);
    std::vector<uint32_t> used;
    if (V > (1u << 23)) { used = c.rrank; std::sort(used.begin(), used.end()); used.erase(std::unique(used.begin(), used.end()), used.end()); }
    ScorePaths p;
    for (int full = 1; full >= 0; --full) {
        if ((full && t == T_DISTINCT) || (!full && t == T_FULL)) continue;
        IdfTable tab(full != 0, V, used, g);
        if (!tab.dfv.empty()) ddf.up(tab.dfv);
        else {   /* a device fill and the ranks in use patched: the host never holds V words */
            CK(hipMemsetD32Async((hipDeviceptr_t)ddf.p, (int)tab.dflt, V, g_s));
            std::vector<uint32_t> vals(used.size());
            for (size_t i = 0; i < used.size(); ++i) vals[i] = tab.patch.at(used[i]);
            scatter(used, vals, ddf.p, V);
        }
        DBuf<double> didf("idf", tab.idf.size());
        DBuf<uint32_t> didx("idf_idx", tab.idx.empty() ? 1 : tab.idx.size());
        didf.up(tab.idf);
        if (!tab.idx.empty()) didx.up(tab.idx);
        ScoreIn in{};
        in.N = N; in.V = V; in.rec_total = R;
        in.d_np = dnp.p; in.d_dsize = dds.p; in.d_rslot = drs.p; in.d_rcnt = drc.p; in.d_df = ddf.p;
        in.d_idf_idx = didx.p; in.d_recoff = dro.p; in.d_flags = dfl.p; in.d_idf = didf.p;
        in.full_table = full != 0; in.with_split = with_split;
        in.np = &c.np; in.dsize = &c.dsize; in.rrank = &c.rrank; in.rcnt = &c.rcnt; in.recoff = &c.recoff; in.flags = &c.flags;
        in.idf_of = [&tab](uint32_t r) { return tab.idf_of(r); };
        p = run_score(what, in, g);
    }
    return p;
}

static void fillers(Corpus& c, uint32_t count, uint32_t maxn, Rng& g) {
    for (uint32_t q = 0; q < count; ++q) {
        const uint32_t n = (uint32_t)(g() % (std::min(maxn, c.V) + 1));
        c.add(some_ranks(n, c.V, g() % 4 ? RO_RANDOM : RO_ASC, g), g() % 4 == 0, g);
    }
}
/* documents of every class over V terms, unsorted and presorted */
static Corpus mixed_corpus(uint32_t V, Rng& g) {
    Corpus c;
    c.V = V;
    for (uint32_t n : {0u, 1u, 5u, 64u, 65u, 128u, 129u, 300u, 1024u, 1025u, 2048u, 2049u, 4096u}) {
        if (n > V) continue;
        c.add(some_ranks(n, V, RO_RANDOM, g), false, g);
        c.add(some_ranks(n, V, RO_ASC, g), true, g);
    }
    if (V >= 4097) c.add(some_ranks(4097, V, RO_ASC, g), true, g);
    fillers(c, 40, 200, g);
    return c;
}
#define REQUIRE_PATH(cond, why) do { if (!(cond)) bad_case(name, why); } while (0)

static void score_group() {
    Rng g(4242);
    const uint32_t class_sizes[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 130, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096};
    /* ---- the classes, V = 30 000 ---- */
    for (RankOrder o : {RO_RANDOM, RO_ASC, RO_DESC}) {
        const std::string name = fmt("score classes, unsorted documents in %s rank order", o == RO_RANDOM ? "random" : o == RO_ASC ? "ascending" : "descending");
        Corpus c;
        c.V = 30000;
        for (uint32_t n : class_sizes) c.add(some_ranks(n, c.V, o, g), false, g);
        const ScorePaths p = score_corpus(name, c, T_BOTH, true, g);
        REQUIRE_PATH(p.nsmall == 10 && p.nwave == 7 && p.nlarge == 6 && p.ntasks == 0, "class totals");
        printf("ok  %s\n", name.c_str());
    }
    for (int with_split = 1; with_split >= 0; --with_split) {
        const std::string name = fmt("score classes, presorted documents, %s", with_split ? "chunk tasks" : "split_count null");
        Corpus c;
        c.V = 30000;
        for (uint32_t n : class_sizes) c.add(some_ranks(n, c.V, RO_ASC, g), true, g);
        for (uint32_t n : {4097u, 8191u, 8192u, 8193u, 3u * 4096u + 1u}) c.add(some_ranks(n, c.V, RO_ASC, g), true, g);
        fillers(c, 10, 200, g);
        const ScorePaths p = score_corpus(name, c, T_BOTH, with_split != 0, g);
        /* over K5_PS_SPLIT pairs: 2 + 2 + 2 + 3 + 4 chunks, or whole documents of k_score_large */
        REQUIRE_PATH(with_split ? p.ntasks == 13 : p.ntasks == 0, "chunk tasks");
        REQUIRE_PATH(p.nlarge == (with_split ? 6u : 11u), "documents of k_score_large");
        printf("ok  %s\n", name.c_str());
    }
    /* ---- bucket fill at the switch between the bucket sort and the radix passes ---- */
    {
        const uint32_t V = 1u << 17, rb = rank_bits_of(V);
        struct B { uint32_t n, nbb, target; const char* tag; };
        const B bs[] = {
            {200, K5_NB_BITS, K5_GROUP_MAX, "wave class, a bucket of K5_GROUP_MAX"},
            {200, K5_NB_BITS, K5_GROUP_MAX + 1, "wave class, a bucket of K5_GROUP_MAX + 1"},
            {1500, large_nbb(1500), K5L_GROUP_MAX, "large class 1500 pairs, a bucket of K5L_GROUP_MAX"},
            {1500, large_nbb(1500), K5L_GROUP_MAX + 1, "large class 1500 pairs, a bucket of K5L_GROUP_MAX + 1"},
            {3000, large_nbb(3000), K5L_GROUP_MAX, "large class 3000 pairs, a bucket of K5L_GROUP_MAX"},
            {3000, large_nbb(3000), K5L_GROUP_MAX + 1, "large class 3000 pairs, a bucket of K5L_GROUP_MAX + 1"},
        };
        for (const B& b : bs) {
            const std::string name = fmt("score bucket fill: %s", b.tag);
            Corpus c;
            c.V = V;
            fillers(c, 5, 200, g);
            for (int q = 0; q < 3; ++q) {
                const std::vector<uint32_t> r = bucket_doc(b.n, V, b.nbb, b.target, g);
                REQUIRE_PATH(bucket_max(r.data(), b.n, rb, b.nbb) == b.target, "the fullest bucket");
                c.add(r, false, g);
            }
            fillers(c, 5, 200, g);
            const ScorePaths p = score_corpus(name, c, T_BOTH, true, g);
            REQUIRE_PATH((b.n <= K5_WAVE ? p.nwave : p.nlarge) >= 3, "the documents' class");
            printf("ok  %s\n", name.c_str());
        }
        const std::string name = "score documents of 129, 1024, 2048 and 4096 consecutive ranks";
        Corpus c;
        c.V = 30000;
        for (uint32_t n : {129u, 1024u, 2048u, 4096u}) {
            c.add(consecutive((uint32_t)(g() % (c.V - n)), n, true, g), false, g);
            c.add(consecutive(c.V - n, n, true, g), false, g);
        }
        score_corpus(name, c, T_BOTH, true, g);
        printf("ok  %s\n", name.c_str());
    }
    /* ---- rank width ---- */
    {
        const std::string name = "score V=2^8: fewer rank bits than bucket bits";
        Corpus c;
        c.V = 1u << 8;
        for (uint32_t n : {129u, 130u, 191u, 200u, 255u, 256u}) c.add(some_ranks(n, c.V, RO_RANDOM, g), false, g);
        c.add(consecutive(0, 256, false, g), true, g);
        fillers(c, 20, 128, g);
        const ScorePaths p = score_corpus(name, c, T_BOTH, true, g);
        REQUIRE_PATH(p.nwave == 7, "wave-class documents");
        printf("ok  %s\n", name.c_str());
    }
    for (uint32_t V : {(1u << 9) + 1, 1u << 16, (1u << 16) + 1, 1u << 21}) {
        const std::string name = fmt("score V=%u", V);
        const Corpus c = mixed_corpus(V, g);
        const ScorePaths p = score_corpus(name, c, T_BOTH, true, g);
        REQUIRE_PATH(p.nhand == 0 && p.nsmall && p.nwave, "narrow ranks");
        printf("ok  %s\n", name.c_str());
    }
    for (uint32_t V : {1024u, 2048u, 4096u}) {
        const std::string name = fmt("score documents holding every term, V=n=%u", V);
        Corpus c;
        c.V = V;
        fillers(c, 6, 128, g);
        c.add(consecutive(0, V, true, g), false, g);
        c.add(consecutive(0, V, false, g), true, g);
        c.add(some_ranks(V, V, RO_DESC, g), false, g);
        fillers(c, 6, 128, g);
        score_corpus(name, c, T_BOTH, true, g);
        printf("ok  %s\n", name.c_str());
    }
    /* ---- wide ranks: the wave kernel's wide instance and its hand-off through large_list ---- */
    for (uint32_t V : {(1u << 21) + 1, (1u << 22) + 5, (1u << 27) + 1})
        for (Tables t : {T_FULL, T_DISTINCT}) {
            if (V > (1u << 23) && t == T_DISTINCT) continue;   /* one case at the widest ranks: idf by df */
            const std::string name = fmt("score wide ranks V=%u, %s idf table", V, t == T_FULL ? "full" : "distinct-df");
            Corpus c = mixed_corpus(V, g);
            for (uint32_t n : {129u, 300u, 1024u}) {   /* skewed wave-class documents at both ends of the ranks */
                c.add(consecutive(0, n, true, g), false, g);
                c.add(consecutive(V - n, n, true, g), false, g);
            }
            c.add(consecutive(V - 2000, 2000, true, g), false, g);
            c.add(consecutive(V - 5000, 5000, false, g), true, g);
            c.add(consecutive(0, 100, true, g), false, g);
            const ScorePaths p = score_corpus(name, c, t, true, g);
            REQUIRE_PATH(p.nhand == 6, "documents handed to k_score_large");
            REQUIRE_PATH(p.ntasks >= 4 && p.nlarge >= 4, "classes");
            printf("ok  %s\n", name.c_str());
            fflush(stdout);
        }
    /* ---- persistence: more documents than one trip of each kernel's resident waves ---- */
    {
        const uint32_t C = g_ncu, V = 30000;
        {
            const std::string name = "score persistence: k_score_small across two batch refills";
            Corpus c;
            c.V = V;
            const uint32_t N = 130u * (C * (uint32_t)K5S_OCC * (uint32_t)K5S_WG) + 7u;
            std::vector<uint32_t> r;
            for (uint32_t d = 0; d < N; ++d) {
                const uint32_t n = d % 40000 == 17 ? 128u : d % 1000 == 500 ? 0u : 1u + (uint32_t)(g() % 3);   /* few empty ones: they join no list */
                r.resize(n);
                if (n <= 3) { const uint32_t b = (uint32_t)(g() % (V - 3000)); for (uint32_t j = 0; j < n; ++j) r[j] = b + (n - 1 - j) * 1000 + (uint32_t)(g() % 1000); }
                else r = some_ranks(n, V, RO_RANDOM, g);
                c.add(r, false, g);
            }
            const ScorePaths p = score_corpus(name, c, T_FULL, true, g);
            /* documents per wave: over two batches of 64 */
            REQUIRE_PATH(p.nwave == 0 && p.nlarge == 0 && p.nsmall > 128u * (C * (uint32_t)K5S_OCC * (uint32_t)K5S_WG), "documents per wave");
            printf("ok  %s (documents, records sized from the CU count)\n", name.c_str());
            fflush(stdout);
        }
        {
            const std::string name = "score persistence: k_score_wave's third trip";
            Corpus c;
            c.V = V;
            const uint32_t N = 3u * (C * 16u) + 5u;
            for (uint32_t d = 0; d < N; ++d) c.add(some_ranks(129 + (uint32_t)(g() % 32), V, RO_RANDOM, g), d % 11 == 3, g);
            const ScorePaths p = score_corpus(name, c, T_DISTINCT, true, g);
            REQUIRE_PATH(p.nwave == N, "wave-class documents");
            printf("ok  %s (documents, records sized from the CU count)\n", name.c_str());
            fflush(stdout);
        }
        {
            const std::string name = "score persistence: k_score_large's second trip";
            Corpus c;
            c.V = V;
            const uint32_t N = 2048 + 3;
            for (uint32_t d = 0; d < N; ++d) c.add(some_ranks(1025 + (uint32_t)(g() % 76), V, d % 5 == 1 ? RO_ASC : RO_RANDOM, g), d % 5 == 1, g);
            const ScorePaths p = score_corpus(name, c, T_FULL, true, g);
            REQUIRE_PATH(p.nlarge == N, "large-class documents");
            printf("ok  %s\n", name.c_str());
        }
    }
}

/* ======================================================================= chain ==== */
/* merge -> DF -> score, each stage on what the one before left on the device */
static void chain_group() {
    Rng g(99);
    const std::string name = "chain merge -> df -> score";
    const uint32_t V = 30000, N = 310;
    const uint64_t slot_cap = 1ull << 18;
    SlotTable st(slot_cap, V, true, g);
    /* main documents: slot records; the partial ones own no main record */
    const uint32_t partial_docs[] = {5, 77, 150, 151, 200, 309};
    const uint32_t partial_n[] = {1, 130, 1500, 5000, 64, 9000};
    Corpus c;   /* the documents as K5 will see them: main ones first, the merged ones set below */
    c.V = V;
    const uint32_t sizes[] = {0, 1, 2, 3, 50, 64, 100, 128, 129, 400, 1024, 1025, 2048, 2049, 4096};
    for (uint32_t d = 0; d < N; ++d) {
        const bool part = std::find(std::begin(partial_docs), std::end(partial_docs), d) != std::end(partial_docs);
        const uint32_t n = part ? 0u : d < 2 * 15 ? sizes[d % 15] : (uint32_t)(g() % 200);
        c.add(some_ranks(n, V, RO_RANDOM, g), false, g);
    }
    const uint64_t nrec = c.rrank.size();
    std::vector<PRec> pr;
    for (size_t q = 0; q < 6; ++q) {
        const std::vector<uint32_t> ranks = some_ranks(partial_n[q], V, RO_ASC, g);
        for (uint32_t r : ranks) {
            const uint32_t len = g() % 50 == 0 ? 70u : 1u + (uint32_t)(g() % 4);
            for (uint32_t e = 0; e < len; ++e) pr.push_back(PRec{partial_docs[q], r, 1u + (uint32_t)(g() % 20000)});
        }
    }
    std::sort(pr.begin(), pr.end(), [](const PRec& a, const PRec& b) { return a.doc != b.doc ? a.doc < b.doc : a.rank < b.rank; });
    const uint64_t Q = pr.size(), rec_total = nrec + Q;
    std::vector<uint64_t> keys(Q);
    std::vector<uint32_t> seq(Q), pcnt(Q);
    for (uint64_t i = 0; i < Q; ++i) { keys[i] = ((uint64_t)pr[i].doc << 32) | pr[i].rank; seq[i] = (uint32_t)i; }
    std::shuffle(seq.begin(), seq.end(), g);
    for (uint64_t i = 0; i < Q; ++i) pcnt[seq[i]] = pr[i].cnt;
    /* the host's merge: appended to the corpus's records behind the main ones */
    uint64_t U = 0;
    for (uint64_t i = 0; i < Q; ++i) {
        const bool head = i == 0 || keys[i] != keys[i - 1];
        const uint32_t d = pr[i].doc;
        if (head) {
            if (i == 0 || pr[i - 1].doc != d) { c.recoff[d] = nrec + U; c.np[d] = 0; c.flags[d] = DF_PARTIAL | DF_PRESORTED; }
            c.rrank.push_back(pr[i].rank);
            c.rcnt.push_back(0);
            ++c.np[d];
            ++U;
        }
        c.rcnt.back() += pr[i].cnt;
    }
    std::vector<uint32_t> xdf(V, 0);
    for (uint32_t r : c.rrank) ++xdf[r];
    /* device state */
    DBuf<uint32_t> ros("rank_of_slot", slot_cap), drs("rec_slot", rec_total), drc("rec_cnt", rec_total), dnp("doc_npairs", N),
        dds("doc_size", N), ddf("df", V), dseq("seq", Q), dpc("part_cnt", Q), dhead("head", Q + 1), dsor("slot_of_rank", 1);
    DBuf<uint64_t> dkeys("keys", Q), dro("doc_recoff", N);
    DBuf<uint8_t> dfl("doc_flags", N);
    ros.fill(0xFF);
    {
        std::vector<uint32_t> rk(V), sl(V);
        for (uint32_t r = 0; r < V; ++r) { rk[r] = r; sl[r] = st.of(r); }
        scatter(sl, rk, ros.p, slot_cap);
    }
    {
        std::vector<uint32_t> s0(rec_total, GUARD_WORD), c0(rec_total, GUARD_WORD), np0 = c.np;
        std::vector<uint64_t> ro0 = c.recoff;
        std::vector<uint8_t> fl0 = c.flags;
        for (uint64_t i = 0; i < nrec; ++i) { s0[i] = st.of(c.rrank[i]); c0[i] = c.rcnt[i]; }
        for (uint32_t d : partial_docs) { np0[d] = 0; ro0[d] = 0; fl0[d] = 0; }
        drs.up(s0); drc.up(c0); dnp.up(np0); dro.up(ro0); dfl.up(fl0);
    }
    dds.up(c.dsize); dkeys.up(keys); dseq.up(seq); dpc.up(pcnt);
    dhead.fill(0xCD); ddf.fill(0xCD);
    const size_t scratch = df_hist_scratch(rec_total, V);
    begin_case(g_ar_bytes);
    end_stage(name + ": launch_part_heads", launch_part_heads(dkeys.p, Q, dhead.p, g_s));
    end_stage(name + ": scan_excl_u32", scan_excl_u32(dhead.p, dhead.p, Q, g_ar, g_s));
    end_stage(name + ": launch_part_merge",
              launch_part_merge(dkeys.p, dseq.p, dpc.p, dhead.p, Q, dsor.p, nrec, drs.p, drc.p, dro.p, dnp.p, dfl.p, g_s));
    g_ar.cap = (scratch + 255) & ~(size_t)255;
    end_stage(name + ": launch_df_hist",
              launch_df_hist(drs.p, nrec, dhead.p + Q, rec_total, ros.p, nullptr, V, slot_cap, g_status, ddf.p, g_ar, g_s, false));
    const std::string sz = fmt("ndocs=%u V=%u main records=%llu partial records=%llu merged=%llu", N, V, (unsigned long long)nrec,
                               (unsigned long long)Q, (unsigned long long)U);
    {
        const std::vector<uint32_t> gs = drs.down(), gc = drc.down(), gn = dnp.down(), gd = ddf.down();
        const std::vector<uint64_t> go = dro.down();
        const std::vector<uint8_t> gf = dfl.down();
        if (word_at(dhead.p + Q) != (uint32_t)U) fail(name, sz, Q, "merged record count");
        for (uint64_t i = 0; i < nrec + U; ++i) {
            if (gs[i] != c.rrank[i]) fail(name, sz, i, i < nrec ? "record rewritten to its rank" : "merged rec_slot");
            if (gc[i] != c.rcnt[i]) fail(name, sz, i, "rec_cnt");
        }
        for (uint64_t i = nrec + U; i < rec_total; ++i) {
            if (gs[i] != GUARD_WORD) fail(name, sz, i, "rec_slot behind the merged records");
            if (gc[i] != 0) fail(name, sz, i, "rec_cnt behind the merged records");
        }
        for (uint32_t d = 0; d < N; ++d) {
            if (gn[d] != c.np[d]) fail(name, sz, d, "doc_npairs");
            if (c.np[d] && go[d] != c.recoff[d]) fail(name, sz, d, "doc_recoff");
            if (gf[d] != c.flags[d]) fail(name, sz, d, "doc_flags");
        }
        for (uint32_t r = 0; r < V; ++r) if (gd[r] != xdf[r]) fail(name, sz, r, "df");
    }
    /* idf over every df value 0..N, as a run with the full table */
    std::vector<double> idf((size_t)N + 1, 0.0);
    for (uint32_t k = 1; k <= N; ++k) idf[k] = log(1.0 * (double)N / (double)k);
    DBuf<double> didf("idf", idf.size());
    DBuf<uint32_t> didx("idf_idx", 1);
    didf.up(idf);
    ScoreIn in{};
    in.N = N; in.V = V; in.rec_total = rec_total;
    in.d_np = dnp.p; in.d_dsize = dds.p; in.d_rslot = drs.p; in.d_rcnt = drc.p; in.d_df = ddf.p;
    in.d_idf_idx = didx.p; in.d_recoff = dro.p; in.d_flags = dfl.p; in.d_idf = didf.p;
    in.full_table = true; in.with_split = true;
    in.np = &c.np; in.dsize = &c.dsize; in.rrank = &c.rrank; in.rcnt = &c.rcnt; in.recoff = &c.recoff; in.flags = &c.flags;
    in.idf_of = [&](uint32_t r) { return idf[xdf[r]]; };
    const ScorePaths p = run_score(name, in, g);
    REQUIRE_PATH(p.ntasks == 2 + 3 && p.nsmall && p.nwave && p.nlarge, "classes of the main and the merged documents");
    printf("ok  %s (%s)\n", name.c_str(), sz.c_str());
}

int main(int argc, char** argv) {
    const std::string grp = argc > 1 ? argv[1] : "";
    if (grp != "merge" && grp != "df" && grp != "score" && grp != "chain") {
        fprintf(stderr, "usage: %s merge|df|score|chain\n", argv[0]);
        return 2;
    }
    CK(hipSetDevice(0));
    int ncu = 0;
    CK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0));
    g_ncu = (uint32_t)ncu;
    CK(hipStreamCreate(&g_s));
    CK(hipStreamCreate(&g_s2));
    CK(hipEventCreateWithFlags(&g_ev0, hipEventDisableTiming));
    CK(hipEventCreateWithFlags(&g_ev1, hipEventDisableTiming));
    g_ar_bytes = 256ull << 20;
    CK(hipMalloc((void**)&g_ar.base, g_ar_bytes));
    CK(hipMalloc((void**)&g_status, 4));
    if (grp == "merge") merge_group();
    if (grp == "df") df_group();
    if (grp == "score") score_group();
    if (grp == "chain") chain_group();
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
