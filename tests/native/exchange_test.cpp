/* GPU test of the multi-rank half of csrc/finalize.hip (its "multi-GPU union" section), each
 * launcher on inputs crafted for it and compared with a plain host loop: the hash-owner DF
 * exchange (launch_owner_partition, launch_owner_offsets, launch_owner_aggregate,
 * launch_owner_aggregate_buckets, launch_owner_back), the dense exchange in both numberings
 * (launch_keys_by_rank, launch_dense_ids, launch_dense_scatter, launch_dense_gather,
 * launch_dense_merge_ids), the cross-rank check of long terms (launch_long_list,
 * launch_long_bytes, launch_long_verify) and the in-process transport's kernels (launch_xcopy,
 * launch_xsum_slice, launch_sum_rows_u32).  Links only build/finalize.o and build/prims.o: no
 * engine, no corpus, no transport threads; the ranks of a case are simulated one after another
 * on one device and the host moves their data.
 *
 *   exchange_test owner | dense | long | xport | chain
 *
 * One "ok  " line per case; "ALL OK" at the end.  Any HIP error or negative launcher return
 * ends the program at once (exit 2) without another launch; a mismatch prints the case, its
 * sizes, the first differing index and the field and ends it too (exit 1).  Everything is an
 * integer or a byte and is compared exactly.  The references are host loops over the same
 * inputs: std::unordered_map / std::map on the 128-bit keys, sums in uint32_t, memcmp.  Every
 * output is prefilled with all-ones words and every expected position must have been written;
 * the 1024 elements behind every buffer must still hold their fill; the status word must be
 * zero except where a case expects ST_LONG_COLLIDE (and then only that bit); used, vg and the
 * trailers must equal the host's counts.
 *
 * owner_of is restated here from dev_common.h's mix64 and finalize.hip's formula: it is the
 * cross-rank protocol (every rank must pick the same owner for a key), and this test pins it.
 *
 * Only inputs the launchers accept are fed: table capacities are a power of two >= 1.5 n
 * (engine.cpp's table_cap), keys are valid identity keys (a short key is its bytes, a TAB,
 * then zeros; a long key has byte 15 = 0xFF), no bucket of the bucketed aggregation holds more
 * than 2048 distinct keys, the terms of one rank are distinct.  The ST_BOUNDS guards are not
 * under test.
 *
 * Out of scope: the three-pass bucket sort of launch_owner_aggregate_buckets (lg > 16) needs
 * more than 33 554 432 received records on one owner, about 0.7 GB of records plus scratch;
 * the R > XO_MAXR fallbacks of k_owner_back and xb_seg cannot be reached through the launchers
 * (launch_owner_partition refuses R > 1024 and the group cannot be opened with more).  A
 * bucket of exactly 1024 or 1025 records is reached with records that all carry one key (they
 * share one bucket whatever the bucket hash is); with other keys beside it the bucket's size
 * follows the bucket hash, which this test does not restate. */
#include "kernels.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <random>
#include <set>
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

static hipStream_t g_s;
static uint32_t* g_status;       /* the device status word */

typedef std::mt19937_64 Rng;

[[noreturn]] static void fail(const std::string& what, const std::string& sizes, uint64_t idx, const char* field) {
    printf("MISMATCH %s (%s) first differing index %llu (%s)\n", what.c_str(), sizes.c_str(), (unsigned long long)idx, field);
    fflush(stdout);
    exit(1);
}
[[noreturn]] static void bad_case(const std::string& what, const char* why) {
    printf("MISMATCH %s: the case is not what it was built for: %s\n", what.c_str(), why);
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
static void ok_line(const std::string& what, const std::string& sz) {
    printf("ok  %s (%s)\n", what.c_str(), sz.c_str());
    fflush(stdout);
}

/* ------------------------------------------------------- guarded buffers ---- */
constexpr uint64_t GUARD = 1024;       /* elements behind every buffer */
constexpr int GUARD_BYTE = 0xA7;
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
        if (!h.empty()) {
            CK(hipMemcpyAsync((void*)(p + at), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, g_s));
            CK(hipStreamSynchronize(g_s));   /* h may be a temporary */
        }
    }
    std::vector<T> down(uint64_t count = ~0ull, uint64_t at = 0) const {
        if (count == ~0ull) count = n - at;
        if (at + count > n) { printf("harness bug: download past a buffer\n"); exit(1); }
        std::vector<T> h(count);
        CK(hipStreamSynchronize(g_s));
        if (count) CK(hipMemcpy(h.data(), (const void*)(p + at), count * sizeof(T), hipMemcpyDeviceToHost));
        return h;
    }
};

static uint32_t word_at(const uint32_t* dev) {
    uint32_t v = 0;
    CK(hipMemcpy(&v, dev, 4, hipMemcpyDeviceToHost));
    return v;
}
static void begin_case() { CK(hipMemsetAsync(g_status, 0, 4, g_s)); }
/* a stage returned: its return value, the stream, the status word, the guards */
static void end_stage(const std::string& what, int rc, uint32_t want_status = 0) {
    if (rc < 0) {
        printf("%s returned %d\n", what.c_str(), rc);
        fflush(stdout);
        exit(2);
    }
    CK(hipStreamSynchronize(g_s));
    CK(hipGetLastError());
    const uint32_t st = word_at(g_status);
    if (st != want_status) {
        printf("MISMATCH %s: status word 0x%x, expected 0x%x\n", what.c_str(), st, want_status);
        fflush(stdout);
        exit(1);
    }
    std::vector<uint8_t> g;
    for (const GuardRef& r : g_guards) {
        g.assign(r.bytes, 0);
        CK(hipMemcpy(g.data(), r.p, r.bytes, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < r.bytes; ++i)
            if (g[i] != (uint8_t)GUARD_BYTE) fail(what, fmt("guard behind %s", r.name), i, "guard byte overwritten");
    }
}

/* ------------------------------------------------------------------ keys ---- */
struct K128 {
    uint64_t lo, hi;
    bool operator==(const K128& o) const { return lo == o.lo && hi == o.hi; }
    bool operator<(const K128& o) const { return hi != o.hi ? hi < o.hi : lo < o.lo; }
};
static uint64_t splitmix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
struct K128Hash {
    size_t operator()(const K128& k) const { return (size_t)splitmix(k.lo ^ splitmix(k.hi)); }
};
static K128 k128(const uint4& k) { return K128{((uint64_t)k.y << 32) | k.x, ((uint64_t)k.w << 32) | k.z}; }
static K128 rec_key(const uint32_t* r) { return K128{((uint64_t)r[1] << 32) | r[0], ((uint64_t)r[3] << 32) | r[2]}; }
static bool same(const uint4& a, const uint4& b) { return memcmp(&a, &b, 16) == 0; }
static uint4 key_of_bytes(const uint8_t* b) {
    uint4 k;
    memcpy(&k, b, 16);
    return k;
}
/* a short term's identity key: its bytes, a TAB, zeros */
static uint4 short_key_str(const std::string& s) {
    if (s.empty() || s.size() > 15) { printf("harness bug: a short term of %zu bytes\n", s.size()); exit(1); }
    uint8_t b[16] = {0};
    memcpy(b, s.data(), s.size());
    b[s.size()] = 0x09;
    return key_of_bytes(b);
}
/* distinct ids give distinct short terms of 7..15 letters (the first 7 spell the id) */
static uint4 short_key(uint64_t id) {
    std::string s(7 + id % 9, 'q');
    uint64_t v = id;
    for (int i = 6; i >= 0; --i) { s[(size_t)i] = (char)('a' + v % 26); v /= 26; }
    if (v) { printf("harness bug: term id too large\n"); exit(1); }
    return short_key_str(s);
}
/* a long term's identity key: a 120-bit hash under the tag byte 0xFF */
static uint4 long_key(uint64_t id) {
    const uint64_t lo = splitmix(id ^ 0x1234ABCDull), hi = (splitmix(id + 0x77ull) & 0x00FFFFFFFFFFFFFFull) | 0xFF00000000000000ull;
    return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}
static bool id_is_long(uint64_t id) { return id % 7 == 3; }
static uint4 ident_of(uint64_t id) { return id_is_long(id) ? long_key(id) : short_key(id); }
/* the vocabulary sort's key of a short term: its identity key byte-reversed */
static uint4 sort_key(const uint4& k) {
    return make_uint4(__builtin_bswap32(k.w), __builtin_bswap32(k.z), __builtin_bswap32(k.y), __builtin_bswap32(k.x));
}
/* engine.cpp's table_cap */
static uint64_t table_cap(uint64_t n) {
    uint64_t t = 1024;
    while (t < n + n / 2) t *= 2;
    return t;
}
/* the owner of a key: dev_common.h's mix64 and finalize.hip's owner_of, restated */
static uint64_t h_mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t h_owner_of(const K128& k, uint32_t R) {
    const uint64_t h = h_mix64(k.lo ^ (k.hi * 0x9E3779B97F4A7C15ull) ^ 0x5851F42D4C957F2Dull);
    return (uint32_t)(((h >> 32) * (uint64_t)R) >> 32);
}

/* ==================================================================== owner ==== */
/* one rank's terms as the engine holds them: the sort keys in term-rank order, the slot
 * table and the vocabulary's keys (read only for long terms), the local df */
struct Terms {
    std::vector<uint4> skey, vkeys, ident;
    std::vector<uint32_t> sor, df;
};
static Terms make_terms(const std::vector<uint64_t>& ids, Rng& rng) {
    const uint64_t V = ids.size();
    Terms t;
    t.skey.resize(V); t.vkeys.resize(V); t.ident.resize(V); t.sor.resize(V); t.df.resize(V);
    uint64_t a = 1000003;
    while (V && std::gcd(a, V) != 1) ++a;
    /* byte 15 of a long term's sort key is the term's 16th byte: anything but NUL and TAB */
    static const uint8_t b15[] = {'a', 'z', 0x01, 0x08, 0x10, 0xFF, 'm', '0'};
    for (uint64_t i = 0; i < V; ++i) {
        const uint32_t slot = (uint32_t)((i * a + 12345) % V);
        t.sor[i] = slot;
        t.ident[i] = ident_of(ids[i]);
        t.df[i] = 1 + (uint32_t)(rng() % 1000);
        if (id_is_long(ids[i])) {
            const uint64_t x = rng(), y = rng();
            t.skey[i] = make_uint4(((uint32_t)x & ~0xFFu) | b15[(ids[i] / 7) % sizeof b15], (uint32_t)(x >> 32), (uint32_t)y,
                                   (uint32_t)(y >> 32));
            t.vkeys[slot] = t.ident[i];
        } else {
            t.skey[i] = sort_key(t.ident[i]);
            t.vkeys[slot] = long_key(ids[i] + (1ull << 40));   /* a short term's key is not read from here */
        }
    }
    return t;
}
static std::vector<uint64_t> id_range(uint64_t id0, uint64_t V) {
    std::vector<uint64_t> ids(V);
    std::iota(ids.begin(), ids.end(), id0);
    return ids;
}

struct PartBufs {
    DBuf<uint4> skey, vkeys;
    DBuf<uint32_t> sor, df, cnt, cur, srec, sidx;
    PartBufs(uint64_t V, uint32_t R)
        : skey("skey", V), vkeys("vkeys", V), sor("slot_of_rank", V), df("df", V), cnt("cnt", R), cur("cur", R),
          srec("srec", 5 * V), sidx("sidx", V) {}
};
/* launch_owner_partition of one rank's terms and its checks; leaves cnt, srec, sidx on the host */
static void run_partition(const std::string& what, const std::string& sz, const Terms& t, uint32_t R, PartBufs& b,
                          std::vector<uint32_t>& cnt, std::vector<uint32_t>& srec, std::vector<uint32_t>& sidx) {
    const uint32_t V = (uint32_t)t.ident.size();
    b.skey.up(t.skey); b.vkeys.up(t.vkeys); b.sor.up(t.sor); b.df.up(t.df);
    b.cnt.fill(0xFF); b.cur.fill(0xFF); b.srec.fill(0xFF); b.sidx.fill(0xFF);
    OwnerKeySrc ks;
    memset(&ks, 0, sizeof ks);
    ks.skey = b.skey.p;
    ks.slot_of_rank = b.sor.p;
    ks.vkeys = b.vkeys.p;
    end_stage(what + " launch_owner_partition",
              launch_owner_partition(ks, b.df.p, V, R, b.cnt.p, b.cur.p, b.srec.p, b.sidx.p, g_s));
    cnt = b.cnt.down(R);
    srec = b.srec.down(5ull * V);
    sidx = b.sidx.down(V);
    std::vector<uint32_t> xcnt(R, 0);
    for (uint32_t i = 0; i < V; ++i) ++xcnt[h_owner_of(k128(t.ident[i]), R)];
    for (uint32_t o = 0; o < R; ++o)
        if (cnt[o] != xcnt[o]) fail(what, sz, o, "cnt (terms per owner)");
    /* sidx a permutation, srec[p] = (key, df) of term sidx[p], p inside the segment of that key's
     * owner: with cnt right, every segment holds exactly the host's multiset for its owner */
    std::vector<uint8_t> seen(V, 0);
    uint32_t o = 0;
    uint64_t end = R ? xcnt[0] : 0;
    for (uint32_t p = 0; p < V; ++p) {
        while (p >= end) end += xcnt[++o];
        const uint32_t r = sidx[p];
        if (r >= V) fail(what, sz, p, "sidx (not a term rank)");
        if (seen[r]) fail(what, sz, p, "sidx (a term rank twice)");
        seen[r] = 1;
        if (memcmp(&srec[5ull * p], &t.ident[r], 16) != 0) fail(what, sz, p, "srec key of term sidx[p]");
        if (srec[5ull * p + 4] != t.df[r]) fail(what, sz, p, "srec df of term sidx[p]");
        if (h_owner_of(k128(t.ident[r]), R) != o) fail(what, sz, p, "srec (record in another owner's segment)");
    }
}

/* prefix offsets of n items over R segments; the first `lead`, the last `trail` and `mid`
 * segments from R / 2 on are empty (as far as R allows), the others share n at random */
static std::vector<uint32_t> layout(uint64_t n, uint32_t R, uint32_t lead, uint32_t trail, uint32_t mid, Rng& rng) {
    std::vector<uint32_t> open;
    for (uint32_t p = 0; p < R; ++p)
        if (!(p < lead || p + trail >= R || (p >= R / 2 && p < R / 2 + mid))) open.push_back(p);
    if (open.empty()) open.push_back(R / 2);
    std::vector<uint64_t> cut(open.size() + 1, 0);
    for (size_t i = 1; i < open.size(); ++i) cut[i] = rng() % (n + 1);
    cut[open.size()] = n;
    std::sort(cut.begin(), cut.end());
    std::vector<uint32_t> c(R, 0), off(R + 1, 0);
    for (size_t i = 0; i < open.size(); ++i) c[open[i]] = (uint32_t)(cut[i + 1] - cut[i]);
    for (uint32_t p = 0; p < R; ++p) off[p + 1] = off[p] + c[p];
    return off;
}

/* the owner's answer to n received records in segments roff: reply[i + sender] = the summed
 * df of record i's key, reply[roff[p + 1] + p] = the distinct keys */
static void ref_reply(const std::vector<uint32_t>& rrec, const std::vector<uint32_t>& roff, uint32_t R,
                      std::vector<uint32_t>& xreply, uint64_t& distinct) {
    const uint64_t n = rrec.size() / 5;
    std::unordered_map<K128, uint32_t, K128Hash> sum;
    sum.reserve(n);
    for (uint64_t i = 0; i < n; ++i) sum[rec_key(&rrec[5 * i])] += rrec[5 * i + 4];
    distinct = sum.size();
    xreply.assign(n + R, 0xFFFFFFFFu);
    for (uint32_t p = 0; p < R; ++p) {
        for (uint64_t i = roff[p]; i < roff[p + 1]; ++i) xreply[i + p] = sum[rec_key(&rrec[5 * i])];
        xreply[(uint64_t)roff[p + 1] + p] = (uint32_t)distinct;
    }
}
struct AggBufs {
    DBuf<uint32_t> rrec, roff, reply, tdf, rslot;
    DBuf<unsigned long long> used;
    DBuf<uint4> tkey;
    DBuf<uint8_t> scratch;
    AggBufs(uint64_t n, uint32_t R)
        : rrec("rrec", 5 * n), roff("roff", R + 1), reply("reply", n + R), tdf("tdf", table_cap(n)), rslot("rslot", n),
          used("used", 1), tkey("tkey", table_cap(n)), scratch("scratch", owner_bucket_scratch(n)) {}
};
/* the three forms of the aggregation on the same records: form 0 the table in memory, 1 the
 * buckets staged in LDS up to 1024 records, 2 every bucket compared in memory */
static std::vector<uint32_t> run_agg_form(const std::string& what, const std::string& sz, int form,
                                          const std::vector<uint32_t>& rrec, const std::vector<uint32_t>& roff, uint32_t R,
                                          AggBufs& b, const std::vector<uint32_t>& xreply, uint64_t distinct) {
    const uint64_t n = rrec.size() / 5;
    b.reply.fill(0xFF);
    b.used.fill(0xFF);
    b.rslot.fill(0xFF);
    int rc;
    if (form == 0)
        rc = launch_owner_aggregate(b.rrec.p, n, b.roff.p, R, b.tkey.p, table_cap(n), b.tdf.p, b.rslot.p, b.reply.p, b.used.p,
                                    g_status, g_s);
    else
        rc = launch_owner_aggregate_buckets(b.rrec.p, n, b.roff.p, R, b.scratch.p, owner_bucket_scratch(n), b.reply.p,
                                            b.used.p, g_status, form == 1 ? 1024u : 0u, g_s);
    end_stage(what, rc);
    const std::vector<uint32_t> got = b.reply.down(n + R);
    if (b.used.down(1)[0] != distinct) fail(what, sz, 0, "used (distinct keys)");
    for (uint64_t i = 0; i < n + R; ++i)
        if (got[i] != xreply[i]) {
            uint32_t p = 0;
            while (p < R && (uint64_t)roff[p + 1] + p < i) ++p;
            fail(what, sz, i, i == (uint64_t)roff[p + 1] + p ? "reply trailer" : "reply df");
        }
    return got;
}
static const char* const AGG_FORM[3] = {"table", "buckets staged up to 1024", "buckets in memory"};
static void run_agg(const std::string& what, const std::vector<uint32_t>& rrec, const std::vector<uint32_t>& roff, uint32_t R) {
    const uint64_t n = rrec.size() / 5;
    if (roff[R] != n) bad_case(what, "the segments do not add up to the records");
    std::vector<uint32_t> xreply;
    uint64_t distinct;
    ref_reply(rrec, roff, R, xreply, distinct);
    const std::string sz = fmt("n=%llu R=%u distinct=%llu", (unsigned long long)n, R, (unsigned long long)distinct);
    AggBufs b(n, R);
    b.rrec.up(rrec);
    b.roff.up(roff);
    for (int form = 0; form < 3; ++form) {
        begin_case();
        const std::string w = what + ", " + AGG_FORM[form];
        run_agg_form(w, sz, form, rrec, roff, R, b, xreply, distinct);
        ok_line(w, sz);
    }
}
static void push_rec(std::vector<uint32_t>& rrec, const uint4& k, uint32_t df) {
    rrec.push_back(k.x); rrec.push_back(k.y); rrec.push_back(k.z); rrec.push_back(k.w); rrec.push_back(df);
}
/* n records over a pool of ids (about `copies` records per key), shuffled */
static std::vector<uint32_t> random_recs(uint64_t n, uint64_t copies, uint64_t id0, Rng& rng) {
    std::vector<uint32_t> rrec;
    rrec.reserve(5 * n);
    const uint64_t pool = n / copies + 1;
    for (uint64_t i = 0; i < n; ++i) push_rec(rrec, ident_of(id0 + rng() % pool), (uint32_t)rng());
    return rrec;
}

/* launch_owner_back on a reply buffer of V words in R segments, each followed by a trailer */
static void check_back(const std::string& what, const std::string& sz, const std::vector<uint32_t>& back,
                       const std::vector<uint32_t>& soff, uint32_t R, const std::vector<uint32_t>& sidx, uint32_t V,
                       const std::vector<uint32_t>& got, uint32_t vg) {
    std::vector<uint32_t> x(V, 0xFFFFFFFFu);
    uint32_t xvg = 0;
    for (uint32_t p = 0; p < R; ++p) {
        for (uint32_t j = soff[p]; j < soff[p + 1]; ++j) x[sidx[j]] = back[(uint64_t)j + p];
        xvg += back[(uint64_t)soff[p + 1] + p];
    }
    for (uint32_t r = 0; r < V; ++r)
        if (got[r] != x[r]) fail(what, sz, r, "df_global");
    if (vg != xvg) fail(what, sz, 0, "vg (the trailers' sum)");
}
static void run_back(uint32_t R, uint32_t V, Rng& rng) {
    const std::string what = "owner back", sz = fmt("R=%u V=%u", R, V);
    /* empty owners in front, behind and in the middle wherever R leaves room for them */
    const std::vector<uint32_t> soff = layout(V, R, R > 3 ? 2 : 0, R > 3 ? 1 : 0, R > 8 ? 3 : 0, rng);
    std::vector<uint32_t> back((uint64_t)V + R), sidx(V);
    for (uint32_t& w : back) w = (uint32_t)rng();
    std::iota(sidx.begin(), sidx.end(), 0u);
    std::shuffle(sidx.begin(), sidx.end(), rng);
    DBuf<uint32_t> dback("back", back.size()), dsoff("soff", R + 1), dsidx("sidx", V), ddfg("df_global", V), dvg("vg", 1);
    dback.up(back); dsoff.up(soff); dsidx.up(sidx);
    ddfg.fill(0xFF); dvg.fill(0xFF);
    begin_case();
    end_stage(what + " launch_owner_back", launch_owner_back(dback.p, dsoff.p, R, dsidx.p, V, ddfg.p, dvg.p, g_s));
    check_back(what, sz, back, soff, R, sidx, V, ddfg.down(), dvg.down()[0]);
    ok_line(what, sz);
}

static void owner_group() {
    Rng rng(0x0E0E0E01u);
    static const uint32_t RS[] = {1, 2, 3, 255, 256, 257, 1024};
    /* ---- partition: V around one workgroup's 2048 terms and past the count kernel's 1024
     * workgroups; R around one trip of the 256-thread loops over owners and at XO_MAXR ---- */
    for (uint32_t V : {0u, 1u, 2047u, 2048u, 2049u, 2100000u}) {
        const Terms t = make_terms(id_range(1000 + V, V), rng);
        for (uint32_t R : RS) {
            const std::string what = "owner partition", sz = fmt("V=%u R=%u", V, R);
            PartBufs b(V, R);
            std::vector<uint32_t> cnt, srec, sidx;
            begin_case();
            run_partition(what, sz, t, R, b, cnt, srec, sidx);
            ok_line(what, sz);
        }
    }
    /* ---- offsets: this rank's row and column of the count matrix, with zero rows and columns ---- */
    for (uint32_t R : {1u, 3u, 257u, 1024u}) {
        const uint32_t me = R / 3;
        const std::string what = "owner offsets", sz = fmt("R=%u me=%u", R, me);
        std::vector<uint32_t> m((uint64_t)R * (R + 1));
        for (uint32_t p = 0; p < R; ++p)
            for (uint32_t q = 0; q <= R; ++q) {
                const bool zero = R > 1 && (p % 5 == 1 || q % 7 == 2);   /* rows 1, 6, .. and columns 2, 9, .. */
                m[(uint64_t)p * (R + 1) + q] = q == R ? 0xDEAD0000u + p /* the status column is not a count */
                                                      : zero ? 0u : (uint32_t)(rng() % 5000);
            }
        std::vector<uint32_t> xs(R + 1, 0), xr(R + 1, 0);
        for (uint32_t p = 0; p < R; ++p) {
            xs[p + 1] = xs[p] + m[(uint64_t)me * (R + 1) + p];
            xr[p + 1] = xr[p] + m[(uint64_t)p * (R + 1) + me];
        }
        DBuf<uint32_t> dm("count matrix", m.size()), dso("soff", R + 1), dro("roff", R + 1);
        dm.up(m);
        dso.fill(0xFF); dro.fill(0xFF);
        begin_case();
        end_stage(what + " launch_owner_offsets", launch_owner_offsets(dm.p, R, me, dso.p, dro.p, g_s));
        const std::vector<uint32_t> gs = dso.down(), gr = dro.down();
        for (uint32_t p = 0; p <= R; ++p) {
            if (gs[p] != xs[p]) fail(what, sz, p, "soff");
            if (gr[p] != xr[p]) fail(what, sz, p, "roff");
        }
        ok_line(what, sz);
    }
    /* ---- aggregate, all three forms per case.  n: no record, one (a bucket of the two stays
     * empty), the radix digit mask's switch at 131072 -> 131073 records (lg 8 -> 9), and past
     * the insert kernel's 8192 workgroups; layouts with empty senders in front, behind, in a
     * row, and more senders than records ---- */
    {
        struct C { uint64_t n; uint32_t R, lead, trail, mid; };
        for (const C& c : {C{0, 3, 0, 0, 0}, C{1, 1024, 500, 200, 0}, C{2, 257, 3, 0, 100}, C{131072, 8, 1, 1, 2},
                           C{131073, 255, 2, 3, 40}, C{2100000, 3, 0, 0, 0}}) {
            const std::vector<uint32_t> roff = layout(c.n, c.R, c.lead, c.trail, c.mid, rng);
            run_agg(fmt("owner aggregate random keys, %u+%u+%u senders empty", c.lead, c.trail, c.mid),
                    random_recs(c.n, 3, 5000000, rng), roff, c.R);
        }
        /* a term that every one of up to 1024 ranks holds: its copies fill one bucket past the
         * 1024 records staged in LDS and past the 2048 slots of the largest LDS table */
        for (uint32_t copies : {1023u, 1024u, 1025u, 2048u, 2049u, 5000u}) {
            std::vector<uint32_t> rrec;
            for (uint32_t i = 0; i < copies; ++i) push_rec(rrec, ident_of(77), 1 + (uint32_t)(rng() % 9));
            for (uint32_t i = 0; i < 300; ++i) push_rec(rrec, ident_of(9000 + i), (uint32_t)rng());
            /* shuffle the records (5 words each) */
            const uint64_t n = rrec.size() / 5;
            for (uint64_t i = n - 1; i > 0; --i) {
                const uint64_t j = rng() % (i + 1);
                for (int w = 0; w < 5; ++w) std::swap(rrec[5 * i + w], rrec[5 * j + w]);
            }
            run_agg(fmt("owner aggregate one key %u times beside 300 keys", copies), rrec, layout(n, 1024, 0, 0, 0, rng), 1024);
        }
        /* every record one key: one bucket of exactly n records (1024: all four per-thread
         * slots of the staged path full; 1025: the first size past it), every other bucket empty */
        for (uint32_t n : {1024u, 1025u, 5000u}) {
            std::vector<uint32_t> rrec;
            for (uint32_t i = 0; i < n; ++i) push_rec(rrec, ident_of(10), (uint32_t)rng());
            run_agg("owner aggregate every record one key", rrec, layout(n, 64, 1, 1, 2, rng), 64);
        }
        /* three keys over 16 buckets: at most three occupied, runs of empty ones around them */
        run_agg("owner aggregate 5000 records of three keys", random_recs(5000, 2000, 600, rng), layout(5000, 3, 0, 0, 0, rng), 3);
    }
    /* ---- back ---- */
    for (uint32_t R : RS)
        for (uint32_t V : {0u, 1u, 257u}) run_back(R, V, rng);
}

/* ==================================================================== dense ==== */
struct RankList { std::vector<uint4> keys; std::vector<uint32_t> df; };

static void run_keys_by_rank(uint32_t V, Rng& rng) {
    const std::string what = "keys by rank", sz = fmt("V=%u", V);
    const uint32_t cap = 2 * V + 3;
    std::vector<uint4> vkeys(cap);
    for (uint32_t i = 0; i < cap; ++i) vkeys[i] = ident_of(rng() % 1000000);
    std::vector<uint32_t> sor(V);
    for (uint32_t& s : sor) s = (uint32_t)(rng() % cap);
    DBuf<uint4> dv("vkeys", cap), dout("out", V);
    DBuf<uint32_t> ds("slot_of_rank", V);
    dv.up(vkeys); ds.up(sor);
    dout.fill(0xFF);
    begin_case();
    end_stage(what + " launch_keys_by_rank", launch_keys_by_rank(dv.p, ds.p, V, dout.p, g_s));
    const std::vector<uint4> got = dout.down();
    for (uint32_t r = 0; r < V; ++r)
        if (!same(got[r], vkeys[sor[r]])) fail(what, sz, r, "key of term rank r");
    ok_line(what, sz);
}

/* the table numbering: R lists of distinct keys gathered into blocks of maxv keys padded with
 * EMPTY keys; ids -> scatter per rank -> sum of the R vectors -> gather per rank */
static void run_dense_table(const std::string& what, const std::vector<RankList>& L, uint64_t maxv) {
    const uint32_t R = (uint32_t)L.size();
    const uint64_t n = (uint64_t)R * maxv;
    uint64_t sumv = 0;
    std::vector<uint4> g(n, make_uint4(0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu));
    std::vector<uint32_t> df(n, 0xFFFFFFFFu);
    struct Ref { uint32_t minpos, sum; };
    std::unordered_map<K128, Ref, K128Hash> ref;
    for (uint32_t r = 0; r < R; ++r) {
        if (L[r].keys.size() > maxv) bad_case(what, "a list longer than maxv");
        sumv += L[r].keys.size();
        for (uint64_t i = 0; i < L[r].keys.size(); ++i) {
            const uint64_t at = r * maxv + i;
            g[at] = L[r].keys[i];
            df[at] = L[r].df[i];
            auto it = ref.find(k128(g[at]));
            if (it == ref.end()) ref.emplace(k128(g[at]), Ref{(uint32_t)at, df[at]});   /* ascending at: the first is the smallest */
            else it->second.sum += df[at];
        }
    }
    const uint64_t tcap = table_cap(sumv);
    const std::string sz = fmt("R=%u maxv=%llu n=%llu sumv=%llu distinct=%zu", R, (unsigned long long)maxv,
                               (unsigned long long)n, (unsigned long long)sumv, ref.size());
    DBuf<uint4> dg("gkeys", n), dtkey("tkey", tcap);
    DBuf<uint32_t> ddf("df", n), dtpos("tpos", tcap), dpos("pos", n), drows("dense rows", (uint64_t)R * n), dsum("dense sum", n),
        ddfg("df_global", n);
    DBuf<unsigned long long> dused("used", 1);
    dg.up(g); ddf.up(df);
    dtkey.fill(0x11); dtpos.fill(0x11); dused.fill(0xFF); dpos.fill(0xFF); dsum.fill(0xFF); ddfg.fill(0xFF);
    drows.fill(0);   /* the engine clears its dense vector before the scatter */
    begin_case();
    end_stage(what + " launch_dense_ids", launch_dense_ids(dg.p, n, dtkey.p, dtpos.p, tcap, dused.p, g_status, g_s));
    if (dused.down()[0] != ref.size()) fail(what, sz, 0, "used (distinct keys)");
    for (uint32_t r = 0; r < R; ++r)
        end_stage(what + " launch_dense_scatter",
                  launch_dense_scatter(dg.p + r * maxv, ddf.p + r * maxv, (uint32_t)L[r].keys.size(), dtkey.p, tcap, dtpos.p,
                                       dpos.p + r * maxv, drows.p + (uint64_t)r * n, g_status, g_s));
    const std::vector<uint32_t> pos = dpos.down();
    for (uint64_t at = 0; at < n; ++at) {
        const bool real = at % maxv < L[at / maxv].keys.size();
        const uint32_t x = real ? ref[k128(g[at])].minpos : 0xFFFFFFFFu;
        if (pos[at] != x) fail(what, sz, at, real ? "pos (the key's smallest gathered position)" : "pos behind the rank's terms");
    }
    const std::vector<uint32_t> rows = drows.down();
    for (uint32_t r = 0; r < R; ++r) {
        std::vector<uint32_t> x(n, 0);
        for (uint64_t i = 0; i < L[r].keys.size(); ++i) x[ref[k128(L[r].keys[i])].minpos] = L[r].df[i];
        for (uint64_t p = 0; p < n; ++p)
            if (rows[(uint64_t)r * n + p] != x[p]) fail(what, sz, (uint64_t)r * n + p, "dense (a rank's scattered df)");
    }
    end_stage(what + " launch_sum_rows_u32", launch_sum_rows_u32(drows.p, R, n, dsum.p, g_s));
    {
        std::vector<uint32_t> x(n, 0);
        for (const auto& kv : ref) x[kv.second.minpos] = kv.second.sum;
        const std::vector<uint32_t> got = dsum.down();
        for (uint64_t p = 0; p < n; ++p)
            if (got[p] != x[p]) fail(what, sz, p, "dense sum");
    }
    for (uint32_t r = 0; r < R; ++r)
        end_stage(what + " launch_dense_gather",
                  launch_dense_gather(dsum.p, dpos.p + r * maxv, (uint32_t)L[r].keys.size(), ddfg.p + r * maxv, g_s));
    const std::vector<uint32_t> dfg = ddfg.down();
    for (uint64_t at = 0; at < n; ++at) {
        const bool real = at % maxv < L[at / maxv].keys.size();
        const uint32_t x = real ? ref[k128(g[at])].sum : 0xFFFFFFFFu;
        if (dfg[at] != x) fail(what, sz, at, real ? "df_global" : "df_global behind the rank's terms");
    }
    ok_line(what, sz);
}

static bool term_less(const uint4& a, const uint4& b) { return memcmp(&a, &b, 16) < 0; }   /* big-endian byte order */

/* the merge numbering: lists of short keys in term order, padded with all-ones keys */
static void run_dense_merge(const std::string& what, std::vector<RankList> L) {
    const uint32_t R = (uint32_t)L.size();
    uint64_t maxv = 1, sumv = 0;
    for (RankList& l : L) {   /* into term order, df along */
        std::vector<uint32_t> o(l.keys.size());
        std::iota(o.begin(), o.end(), 0u);
        std::sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return term_less(l.keys[a], l.keys[b]); });
        RankList s;
        for (uint32_t i : o) { s.keys.push_back(l.keys[i]); s.df.push_back(l.df[i]); }
        l = s;
        maxv = std::max<uint64_t>(maxv, l.keys.size());
        sumv += l.keys.size();
    }
    const uint64_t n = (uint64_t)R * maxv;
    std::vector<uint4> g(n, make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu)), all;
    std::vector<uint32_t> df(n, 0xFFFFFFFFu);
    std::unordered_map<K128, uint32_t, K128Hash> ref;
    for (uint32_t r = 0; r < R; ++r)
        for (uint64_t i = 0; i < L[r].keys.size(); ++i) {
            g[r * maxv + i] = L[r].keys[i];
            df[r * maxv + i] = L[r].df[i];
            ref[k128(L[r].keys[i])] += L[r].df[i];
            all.push_back(L[r].keys[i]);
        }
    std::sort(all.begin(), all.end(), term_less);
    const std::string sz = fmt("R=%u maxv=%llu sumv=%llu distinct=%zu", R, (unsigned long long)maxv, (unsigned long long)sumv,
                               ref.size());
    DBuf<uint4> dg("gkeys", n);
    DBuf<uint32_t> ddf("df", n), dlbm("lbm", n), dpos("pos", n), ddense("dense", sumv + 1), ddfg("df_global", n);
    dg.up(g); ddf.up(df);
    dpos.fill(0xFF); ddfg.fill(0xFF);
    std::vector<uint32_t> hsum(sumv + 1, 0);
    begin_case();
    for (uint32_t me = 0; me < R; ++me) {
        const uint32_t V = (uint32_t)L[me].keys.size();
        ddense.fill(0);   /* the engine clears sumv + 1 words before the launch */
        dlbm.fill(0xFF);
        end_stage(what + " launch_dense_merge_ids",
                  launch_dense_merge_ids(dg.p, maxv, R, me, V, dlbm.p, ddf.p + me * maxv, sumv, dpos.p + me * maxv, ddense.p,
                                         g_s));
        const std::vector<uint32_t> d = ddense.down();
        /* this rank's vector: its df at its positions, nothing else (checked below through the sum
         * and the positions), the keys it holds first at [sumv] */
        uint32_t first = 0;
        for (uint32_t i = 0; i < V; ++i) {
            bool held = false;
            for (uint32_t q = 0; q < me && !held; ++q)
                held = std::binary_search(L[q].keys.begin(), L[q].keys.end(), L[me].keys[i], term_less);
            first += !held;
        }
        if (d[sumv] != first) fail(what, sz, me, "dense[sumv] (keys this rank holds first)");
        for (uint64_t p = 0; p <= sumv; ++p) hsum[p] += d[p];
    }
    /* the position of a key = the keys below it over all lists: equal keys equal positions,
     * distinct keys distinct ones, all below sumv */
    const std::vector<uint32_t> pos = dpos.down();
    std::map<uint32_t, K128> key_at;
    for (uint64_t at = 0; at < n; ++at) {
        const bool real = at % maxv < L[at / maxv].keys.size();
        if (!real) {
            if (pos[at] != 0xFFFFFFFFu) fail(what, sz, at, "pos behind the rank's terms");
            continue;
        }
        const uint32_t x = (uint32_t)(std::lower_bound(all.begin(), all.end(), g[at], term_less) - all.begin());
        if (pos[at] >= sumv) fail(what, sz, at, "pos (not below sumv)");
        if (pos[at] != x) fail(what, sz, at, "pos (the keys below this one over all lists)");
        auto it = key_at.emplace(pos[at], k128(g[at])).first;
        if (!(it->second == k128(g[at]))) fail(what, sz, at, "pos (two distinct keys at one position)");
    }
    if (key_at.size() != ref.size()) fail(what, sz, 0, "pos (equal keys at different positions)");
    if (hsum[sumv] != ref.size()) fail(what, sz, sumv, "dense[sumv] summed over the ranks (distinct keys)");
    {
        std::vector<uint32_t> x(sumv + 1, 0);
        for (const auto& kv : key_at) x[kv.first] = ref[kv.second];
        x[sumv] = (uint32_t)ref.size();
        for (uint64_t p = 0; p <= sumv; ++p)
            if (hsum[p] != x[p]) fail(what, sz, p, "dense summed over the ranks");
    }
    ddense.up(hsum);
    for (uint32_t me = 0; me < R; ++me)
        end_stage(what + " launch_dense_gather",
                  launch_dense_gather(ddense.p, dpos.p + me * maxv, (uint32_t)L[me].keys.size(), ddfg.p + me * maxv, g_s));
    const std::vector<uint32_t> dfg = ddfg.down();
    for (uint64_t at = 0; at < n; ++at) {
        const bool real = at % maxv < L[at / maxv].keys.size();
        const uint32_t x = real ? ref[k128(g[at])] : 0xFFFFFFFFu;
        if (dfg[at] != x) fail(what, sz, at, real ? "df_global" : "df_global behind the rank's terms");
    }
    ok_line(what, sz);
}

/* R lists: a few ids on most ranks, many on one only (shared: ids below 20); rank R / 2 has no
 * term when R >= 3; short_only leaves out the ids of long terms */
static std::vector<RankList> random_lists(uint32_t R, uint32_t vmax, bool short_only, Rng& rng) {
    std::vector<RankList> L(R);
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t V = (R >= 3 && r == R / 2) ? 0 : 1 + (uint32_t)(rng() % vmax);
        std::set<uint64_t> ids;
        while (ids.size() < V) {
            const uint64_t id = rng() % 3 == 0 ? rng() % 20 : 1000 + rng() % 100000000;
            if (short_only && id_is_long(id)) continue;
            ids.insert(id);
        }
        for (uint64_t id : ids) {
            L[r].keys.push_back(short_only ? short_key(id) : ident_of(id));
            L[r].df.push_back((uint32_t)rng());   /* sums wrap 2^32 */
        }
        /* gathered order is free for the table numbering */
        for (size_t i = L[r].keys.size(); i > 1; --i) {
            const size_t j = rng() % i;
            std::swap(L[r].keys[i - 1], L[r].keys[j]);
            std::swap(L[r].df[i - 1], L[r].df[j]);
        }
    }
    return L;
}

static void dense_group() {
    Rng rng(0x0D0D0D02u);
    for (uint32_t V : {0u, 1u, 1000u}) run_keys_by_rank(V, rng);
    /* ---- the table numbering ---- */
    for (uint32_t R : {1u, 3u, 64u}) {
        const std::vector<RankList> L = random_lists(R, 400, false, rng);
        uint64_t maxv = 0;
        for (const RankList& l : L) maxv = std::max<uint64_t>(maxv, l.keys.size());
        run_dense_table("dense table numbering", L, maxv + 5);
    }
    {   /* past k_dense_insert's 8192 workgroups: n = 2 x 1 050 000 gathered positions, half the keys shared */
        std::vector<RankList> L(2);
        for (uint32_t r = 0; r < 2; ++r)
            for (uint64_t i = 0; i < 1050000 - 1000 * (uint64_t)r; ++i) {
                L[r].keys.push_back(ident_of(20000000 + i + 500000 * (uint64_t)r));
                L[r].df.push_back((uint32_t)rng());
            }
        run_dense_table("dense table numbering past 8192 workgroups", L, 1050000);
    }
    /* ---- the merge numbering ---- */
    {
        const std::string a15(15, 'a');
        std::string b = a15, c = a15, d = a15, e = a15;
        b[0] = 'b';                      /* differs from a15 in the first byte only */
        c[14] = 'b';                     /* ... in the last byte only */
        for (int i = 8; i < 15; ++i) d[(size_t)i] = 'z';   /* equal to a15 in the first 64-bit half */
        e[0] = 'z';                      /* equal to a15 in the second half */
        auto list = [&](std::initializer_list<std::string> terms) {
            RankList l;
            for (const std::string& t : terms) { l.keys.push_back(short_key_str(t)); l.df.push_back((uint32_t)rng()); }
            return l;
        };
        /* rank 0 the longest list (no padding: a later rank's "zzz" is above all of it, lo == maxv);
         * a15 on every list that has terms; rank 2 has none; "m" only on the last */
        run_dense_merge("dense merge numbering, key shapes",
                        {list({a15, b, c, d, e, "a", "zz"}), list({c, a15}), list({}), list({"zzz", a15, d}), list({"m", a15, "b"})});
    }
    for (uint32_t R : {1u, 2u, 3u, 64u, 1024u})
        run_dense_merge("dense merge numbering", random_lists(R, R == 1024 ? 24 : 300, true, rng));
}

/* ===================================================================== long ==== */
static void run_long_list(uint32_t V, Rng& rng) {
    const std::string what = "long list", sz = fmt("V=%u", V);
    const Terms t = make_terms(id_range(31, V), rng);   /* vkeys[slot_of_rank[r]]: long keys, and other long keys for short terms */
    std::vector<uint4> vkeys = t.vkeys;
    std::vector<uint64_t> vrep(V);
    struct E { K128 k; uint32_t len; uint64_t src; bool operator<(const E& o) const { return k < o.k; } };
    std::vector<E> want;
    uint64_t bytes = 0;
    for (uint32_t r = 0; r < V; ++r) {
        const uint32_t sl = t.sor[r], len = 16 + (uint32_t)(rng() % 5000);
        const uint64_t off = rng() & ((1ull << 40) - 1);
        vrep[sl] = ((uint64_t)len << 40) | off;
        if (id_is_long(31 + r)) { want.push_back(E{k128(vkeys[sl]), len, off}); bytes += len; }
        else vkeys[sl] = short_key(31 + r);   /* here the table holds the short term's own key */
    }
    DBuf<uint4> dv("vkeys", V);
    DBuf<uint64_t> drep("vrep", V), dsrc("src", V);
    DBuf<uint32_t> dsor("slot_of_rank", V);
    DBuf<LongEnt> dents("ents", V);
    DBuf<unsigned long long> dcnt("cnt", 2);
    dv.up(vkeys); drep.up(vrep); dsor.up(t.sor);
    dents.fill(0xFF); dsrc.fill(0xFF); dcnt.fill(0xFF);
    begin_case();
    end_stage(what + " launch_long_list", launch_long_list(dv.p, drep.p, dsor.p, V, dents.p, dsrc.p, dcnt.p, g_s));
    const std::vector<unsigned long long> cnt = dcnt.down();
    if (cnt[0] != want.size()) fail(what, sz, 0, "cnt[0] (entries)");
    if (cnt[1] != bytes) fail(what, sz, 1, "cnt[1] (bytes)");
    const std::vector<LongEnt> ents = dents.down();
    const std::vector<uint64_t> src = dsrc.down();
    std::vector<E> got;
    std::vector<std::pair<uint64_t, uint32_t>> span;
    for (uint64_t e = 0; e < want.size(); ++e) {
        got.push_back(E{k128(ents[e].key), ents[e].len, src[e]});
        span.push_back({ents[e].boff, ents[e].len});
        if (ents[e].pad != 0) fail(what, sz, e, "pad");
    }
    for (uint64_t e = want.size(); e < V; ++e)
        if (ents[e].len != 0xFFFFFFFFu || src[e] != ~0ull) fail(what, sz, e, "entry behind the list written");
    std::sort(want.begin(), want.end());
    std::sort(got.begin(), got.end());
    for (uint64_t e = 0; e < want.size(); ++e) {
        if (!(got[e].k == want[e].k)) fail(what, sz, e, "key (entries sorted by key)");
        if (got[e].len != want[e].len) fail(what, sz, e, "len");
        if (got[e].src != want[e].src) fail(what, sz, e, "src (the corpus offset of vrep)");
    }
    std::sort(span.begin(), span.end());
    uint64_t at = 0;
    for (uint64_t e = 0; e < span.size(); ++e) {
        if (span[e].first != at) fail(what, sz, e, "boff (ranges disjoint and without gaps, sorted by boff)");
        at += span[e].second;
    }
    ok_line(what, sz);
}

static void run_long_bytes(Rng& rng) {
    const std::string what = "long bytes";
    std::vector<LongEnt> ents;
    std::vector<uint64_t> src;
    uint64_t corpus = 3, total = 0;
    for (uint32_t len : {16u, 17u, 63u, 64u, 65u, 300u, 5000u})
        for (uint32_t res = 0; res < 16; ++res) {
            while (corpus % 16 != res) ++corpus;
            LongEnt e;
            memset(&e, 0, sizeof e);
            e.key = long_key(ents.size());
            e.len = len;
            ents.push_back(e);
            src.push_back(corpus);
            corpus += len + rng() % 40;
            total += len;
        }
    std::vector<uint32_t> order(ents.size());
    std::iota(order.begin(), order.end(), 0u);
    std::shuffle(order.begin(), order.end(), rng);
    uint64_t at = 0;
    for (uint32_t e : order) { ents[e].boff = at; at += ents[e].len; }
    std::vector<uint8_t> bytes(corpus), x(total);
    for (uint8_t& c : bytes) c = (uint8_t)rng();
    for (size_t e = 0; e < ents.size(); ++e) memcpy(&x[ents[e].boff], &bytes[src[e]], ents[e].len);
    const std::string sz = fmt("entries=%zu bytes=%llu", ents.size(), (unsigned long long)total);
    DBuf<LongEnt> dents("ents", ents.size());
    DBuf<uint64_t> dsrc("src", src.size());
    DBuf<uint8_t> dbytes("corpus", corpus), dblob("blob", total);
    dents.up(ents); dsrc.up(src); dbytes.up(bytes);
    dblob.fill(0xFF);
    begin_case();
    end_stage(what + " launch_long_bytes", launch_long_bytes(dents.p, dsrc.p, (uint32_t)ents.size(), dbytes.p, dblob.p, g_s));
    const std::vector<uint8_t> got = dblob.down();
    if (memcmp(got.data(), x.data(), total) != 0)
        for (uint64_t i = 0; i < total; ++i)
            if (got[i] != x[i]) fail(what, sz, i, "blob byte");
    ok_line(what, sz);
}

enum LongDiff { LD_NONE, LD_LEN, LD_BYTE0, LD_BYTE63, LD_BYTE64, LD_LAST };
static const char* const LD_NAME[] = {"equal bytes", "length only", "byte 0", "byte 63", "byte 64", "the last byte only"};
/* R blocks of lcap entries (EMPTY padding between and behind them) and blobs of bcap bytes;
 * term 0 on every block, term 1 on block R - 1 only, the others on random blocks; with a
 * difference, the last block's copy of term 0 (300 bytes) is altered */
static void run_long_verify(uint32_t R, LongDiff diff, Rng& rng) {
    const std::string what = fmt("long verify, %s", LD_NAME[diff]);
    const uint32_t nterms = 40;
    std::vector<std::vector<uint8_t>> text(nterms);
    static const uint32_t LENS[] = {300, 16, 17, 63, 64, 65, 128, 129, 5000, 1000};
    for (uint32_t t = 0; t < nterms; ++t) {
        text[t].resize(LENS[t % 10] + (t >= 10 ? t : 0));
        for (uint8_t& c : text[t]) c = (uint8_t)('a' + rng() % 26);
    }
    std::vector<std::vector<uint32_t>> held(R);
    uint64_t maxb = 0, maxe = 0;
    for (uint32_t r = 0; r < R; ++r) {
        for (uint32_t t = 0; t < nterms; ++t)
            if (t == 0 || (t == 1 ? r == R - 1 : rng() % 3 == 0)) held[r].push_back(t);
        std::shuffle(held[r].begin(), held[r].end(), rng);
        uint64_t b = 0;
        for (uint32_t t : held[r]) b += text[t].size();
        maxb = std::max(maxb, b);
        maxe = std::max<uint64_t>(maxe, held[r].size());
    }
    const uint64_t lcap = 2 * maxe + 3, bcap = (maxb + 16) & ~15ull, n = R * lcap, tcap = table_cap(n);
    LongEnt empty;
    memset(&empty, 0xEE, sizeof empty);
    std::vector<LongEnt> g(n, empty);
    std::vector<uint8_t> blob(R * bcap, 0x55);
    for (uint32_t r = 0; r < R; ++r) {
        uint64_t b = 0;
        for (size_t i = 0; i < held[r].size(); ++i) {
            const uint32_t t = held[r][i];
            LongEnt& e = g[r * lcap + 2 * i + (r & 1)];   /* padding entries between the real ones */
            memset(&e, 0, sizeof e);
            e.key = long_key(1000 + t);
            e.len = (uint32_t)text[t].size();
            e.boff = b;
            memcpy(&blob[r * bcap + b], text[t].data(), text[t].size());
            if (t == 0 && r == R - 1) {
                uint8_t* p = &blob[r * bcap + b];
                switch (diff) {
                case LD_NONE: break;
                case LD_LEN: e.len -= 1; break;
                case LD_BYTE0: p[0] ^= 1; break;
                case LD_BYTE63: p[63] ^= 1; break;
                case LD_BYTE64: p[64] ^= 1; break;
                case LD_LAST: p[text[t].size() - 1] ^= 1; break;
                }
            }
            b += text[t].size();
        }
    }
    /* reference: every entry against the first entry of its key, length then bytes */
    uint32_t want = 0;
    {
        std::map<K128, uint64_t> first;
        for (uint64_t i = 0; i < n; ++i) {
            if (memcmp(&g[i], &empty, sizeof empty) == 0) continue;
            const auto it = first.emplace(k128(g[i].key), i).first;
            const uint64_t j = it->second;
            if (g[i].len != g[j].len ||
                memcmp(&blob[(i / lcap) * bcap + g[i].boff], &blob[(j / lcap) * bcap + g[j].boff], g[i].len) != 0)
                want = ST_LONG_COLLIDE;
        }
    }
    if ((diff != LD_NONE) != (want != 0)) bad_case(what, "the reference does not see the difference the case was built with");
    const std::string sz = fmt("R=%u lcap=%llu bcap=%llu", R, (unsigned long long)lcap, (unsigned long long)bcap);
    DBuf<LongEnt> dg("gathered entries", n);
    DBuf<uint8_t> dblob("gathered blobs", blob.size());
    DBuf<uint4> dtkey("tkey", tcap);
    DBuf<uint32_t> dtpos("tpos", tcap);
    dg.up(g); dblob.up(blob);
    dtkey.fill(0x11); dtpos.fill(0x11);
    begin_case();
    end_stage(what + " launch_long_verify", launch_long_verify(dg.p, n, lcap, dblob.p, bcap, dtkey.p, dtpos.p, tcap, g_status, g_s),
              want);
    ok_line(what, sz);
}

static void long_group() {
    Rng rng(0x0C0C0C03u);
    for (uint32_t V : {0u, 1u, 1000u}) run_long_list(V, rng);
    run_long_bytes(rng);
    for (uint32_t R : {2u, 3u, 64u}) run_long_verify(R, LD_NONE, rng);
    for (LongDiff d : {LD_LEN, LD_BYTE0, LD_BYTE63, LD_BYTE64, LD_LAST}) run_long_verify(3, d, rng);
}

/* ==================================================================== xport ==== */
/* segments of the given word counts, each at an odd word offset of one source and one
 * destination buffer with gaps between them; the destination's other words keep their fill */
static void run_xcopy(const std::string& what, const std::vector<uint64_t>& words, Rng& rng) {
    const uint32_t nseg = (uint32_t)words.size();
    std::vector<uint64_t> so(nseg), dof(nseg);
    uint64_t sa = 1, da = 3, total = 0;
    for (uint32_t i = 0; i < nseg; ++i) {
        so[i] = sa; dof[i] = da;
        sa += words[i] + 2 * (rng() % 4);      /* odd offsets stay odd... */
        da += words[i] + 2 * (rng() % 4);
        if (words[i] % 2) { sa += 1; da += 1; }   /* ... also behind an odd segment */
        total += words[i];
    }
    const std::string sz = fmt("segments=%u words=%llu", nseg, (unsigned long long)total);
    std::vector<uint32_t> src(sa + 8), x(da + 8, 0xFFFFFFFFu);
    for (uint32_t& w : src) w = (uint32_t)rng();
    DBuf<uint32_t> dsrc("xcopy src", src.size()), ddst("xcopy dst", x.size());
    dsrc.up(src);
    ddst.fill(0xFF);
    XCopyList l;
    memset(&l, 0, sizeof l);
    l.n = nseg;
    for (uint32_t i = 0; i < nseg; ++i) {
        l.src[i] = dsrc.p + so[i];
        l.dst[i] = ddst.p + dof[i];
        l.off[i + 1] = l.off[i] + words[i];
        if (words[i]) memcpy(&x[dof[i]], &src[so[i]], words[i] * 4);
    }
    begin_case();
    end_stage(what + " launch_xcopy", launch_xcopy(l, g_s));
    const std::vector<uint32_t> got = ddst.down();
    if (memcmp(got.data(), x.data(), x.size() * 4) != 0)
        for (uint64_t i = 0; i < x.size(); ++i)
            if (got[i] != x[i]) fail(what, sz, i, x[i] == 0xFFFFFFFFu ? "destination word (outside every segment?)" : "destination word");
    ok_line(what, sz);
}
/* sources: windows of one random buffer at odd distances */
static void run_xsum(bool rows, uint32_t nsrc, uint64_t len, Rng& rng) {
    const std::string what = rows ? "sum rows" : "xsum slice";
    const uint64_t lo = rows ? 0 : 37;
    const std::string sz = fmt("sources=%u len=%llu lo=%llu", nsrc, (unsigned long long)len, (unsigned long long)lo);
    const uint64_t stride = rows ? len : 2 * (len % 1000) + 1;
    std::vector<uint32_t> src(stride * (nsrc - 1) + lo + len), x(len, 0);
    for (uint32_t& w : src) w = (uint32_t)rng();   /* full-range words: with two or more sources the sums wrap 2^32 */
    for (uint32_t r = 0; r < nsrc; ++r)
        for (uint64_t i = 0; i < len; ++i) x[i] += src[r * stride + lo + i];
    DBuf<uint32_t> dsrc("sum src", src.size()), dout("sum out", len);
    dsrc.up(src);
    dout.fill(0xFF);
    begin_case();
    if (rows) {
        end_stage(what + " launch_sum_rows_u32", launch_sum_rows_u32(dsrc.p, nsrc, len, dout.p, g_s));
    } else {
        XCopyList l;
        memset(&l, 0, sizeof l);
        l.n = nsrc;
        for (uint32_t r = 0; r < nsrc; ++r) l.src[r] = dsrc.p + r * stride;
        end_stage(what + " launch_xsum_slice", launch_xsum_slice(l, lo, len, dout.p, g_s));
    }
    const std::vector<uint32_t> got = dout.down();
    for (uint64_t i = 0; i < len; ++i)
        if (got[i] != x[i]) fail(what, sz, i, "sum");
    ok_line(what, sz);
}

static void xport_group() {
    Rng rng(0x0B0B0B04u);
    /* a tile is 1024 words */
    run_xcopy("xcopy a tile across three boundaries", {100, 50, 30, 2000}, rng);
    run_xcopy("xcopy segments shorter than a tile, empty ones among them", {0, 5, 0, 0, 1023, 1, 0}, rng);
    {
        std::vector<uint64_t> w(XCOPY_MAX);
        for (uint64_t& x : w) x = rng() % 4 ? rng() % 3000 : 0;
        run_xcopy("xcopy 64 segments", w, rng);
    }
    run_xcopy("xcopy one tile exactly", {1024}, rng);
    run_xcopy("xcopy one word past a tile", {1025}, rng);
    run_xcopy("xcopy past 4096 workgroups", {2000001, 0, 2200123, 77}, rng);   /* 4 200 201 words > 4 194 304 */
    for (uint32_t n : {0u, (uint32_t)XCOPY_MAX + 1}) {
        XCopyList l;
        memset(&l, 0, sizeof l);
        l.n = n;
        const int rc = launch_xcopy(l, g_s);
        CK(hipStreamSynchronize(g_s));
        if (rc != -3) fail("xcopy refuses the list", fmt("segments=%u", n), 0, "return value (-3 expected)");
        ok_line("xcopy refuses the list", fmt("segments=%u", n));
    }
    /* len around one workgroup and past xgrid's 4096 workgroups (1 048 576 elements) */
    for (uint32_t nsrc : {1u, 2u, 64u})
        for (uint64_t len : {1ull, 255ull, 256ull, 257ull, 1100000ull}) run_xsum(false, nsrc, len, rng);
    for (uint32_t nsrc : {1u, 2u, 64u})
        for (uint64_t len : {1ull, 255ull, 256ull, 257ull}) run_xsum(true, nsrc, len, rng);
    for (uint32_t nsrc : {1u, 2u}) run_xsum(true, nsrc, 1100000, rng);
}

/* ==================================================================== chain ==== */
/* the whole owner exchange for R ranks simulated one after another: partition on each rank,
 * the count all-gather and both all-to-alls by the host, aggregation in the table and the
 * bucketed form (their replies must agree word for word), back on each rank */
static void run_chain(uint32_t R, uint32_t vper, Rng& rng) {
    const std::string what = "owner exchange chain";
    /* sharing: 6 terms on every rank, term 100 + j on every (j + 2)-th rank, the rest on one rank */
    std::vector<std::vector<uint64_t>> ids(R);
    std::vector<Terms> T(R);
    std::unordered_map<K128, uint32_t, K128Hash> gdf;
    uint64_t total = 0, vmaxr = 0;
    for (uint32_t r = 0; r < R; ++r) {
        if (!(R >= 3 && r == R / 2)) {
            for (uint64_t c = 0; c < 6; ++c) ids[r].push_back(c);
            for (uint64_t j = 0; j < 40; ++j)
                if (r % (j + 2) == 0) ids[r].push_back(100 + j);
            const uint32_t own = vper / 2 + (uint32_t)(rng() % vper);
            for (uint32_t i = 0; i < own; ++i) ids[r].push_back(1000000 + (uint64_t)r * 100000 + i);
            std::shuffle(ids[r].begin(), ids[r].end(), rng);
        }
        T[r] = make_terms(ids[r], rng);
        for (size_t i = 0; i < ids[r].size(); ++i) gdf[k128(T[r].ident[i])] += T[r].df[i];
        total += ids[r].size();
        vmaxr = std::max<uint64_t>(vmaxr, ids[r].size());
    }
    const std::string sz = fmt("R=%u terms=%llu distinct=%zu", R, (unsigned long long)total, gdf.size());
    begin_case();
    /* 1. partition */
    std::vector<std::vector<uint32_t>> cnt(R), srec(R), sidx(R);
    {
        PartBufs b(vmaxr, R);
        for (uint32_t r = 0; r < R; ++r)
            run_partition(what, sz + fmt(" rank %u", r), T[r], R, b, cnt[r], srec[r], sidx[r]);
    }
    /* 2. the count all-gather: R rows of R counts + 1 status word */
    std::vector<uint32_t> m((uint64_t)R * (R + 1), 0);
    for (uint32_t r = 0; r < R; ++r) memcpy(&m[(uint64_t)r * (R + 1)], cnt[r].data(), R * 4ull);
    std::vector<std::vector<uint32_t>> soff(R), roff(R), reply(R);
    uint64_t nmax = 0;
    {
        DBuf<uint32_t> dm("count matrix", m.size()), dso("soff", R + 1), dro("roff", R + 1);
        dm.up(m);
        for (uint32_t r = 0; r < R; ++r) {
            dso.fill(0xFF); dro.fill(0xFF);
            end_stage(what + " launch_owner_offsets", launch_owner_offsets(dm.p, R, r, dso.p, dro.p, g_s));
            soff[r] = dso.down();
            roff[r] = dro.down();
            if (soff[r][R] != ids[r].size()) fail(what, sz, r, "soff[R] (the rank's terms)");
            nmax = std::max<uint64_t>(nmax, roff[r][R]);
        }
    }
    /* 3. the records to their owners, aggregated in both forms */
    uint64_t vsum = 0;
    {
        AggBufs b(nmax, R);
        for (uint32_t o = 0; o < R; ++o) {
            std::vector<uint32_t> rrec;
            for (uint32_t p = 0; p < R; ++p) {
                if (roff[o][p] != rrec.size() / 5) fail(what, sz, o, "roff (the senders' counts)");
                rrec.insert(rrec.end(), srec[p].begin() + 5ll * soff[p][o], srec[p].begin() + 5ll * soff[p][o + 1]);
            }
            std::vector<uint32_t> xreply;
            uint64_t distinct;
            ref_reply(rrec, roff[o], R, xreply, distinct);
            b.rrec.up(rrec);
            b.roff.up(roff[o]);
            const std::string zo = sz + fmt(" owner %u n=%zu", o, rrec.size() / 5);
            const std::vector<uint32_t> a = run_agg_form(what + ", table", zo, 0, rrec, roff[o], R, b, xreply, distinct);
            reply[o] = run_agg_form(what + ", buckets", zo, 1, rrec, roff[o], R, b, xreply, distinct);
            if (a != reply[o]) fail(what, zo, 0, "the two forms' replies differ");
            vsum += distinct;
        }
    }
    if (vsum != gdf.size()) bad_case(what, "the owners' distinct keys do not add up to the distinct terms");
    /* 4. the replies back to the senders */
    {
        DBuf<uint32_t> dback("back", vmaxr + R), dsoff("soff", R + 1), dsidx("sidx", vmaxr), ddfg("df_global", vmaxr), dvg("vg", 1);
        for (uint32_t r = 0; r < R; ++r) {
            const uint32_t V = (uint32_t)ids[r].size();
            std::vector<uint32_t> back;
            for (uint32_t o = 0; o < R; ++o)   /* owner o's segment for sender r and its trailer */
                back.insert(back.end(), reply[o].begin() + (roff[o][r] + r), reply[o].begin() + (roff[o][r + 1] + r + 1));
            if (back.size() != (uint64_t)V + R) fail(what, sz, r, "the replies to a rank: V + R words");
            dback.up(back); dsoff.up(soff[r]); dsidx.up(sidx[r]);
            ddfg.fill(0xFF); dvg.fill(0xFF);
            end_stage(what + " launch_owner_back", launch_owner_back(dback.p, dsoff.p, R, dsidx.p, V, ddfg.p, dvg.p, g_s));
            const std::vector<uint32_t> got = ddfg.down(V);
            for (uint32_t i = 0; i < V; ++i)
                if (got[i] != gdf[k128(T[r].ident[i])]) fail(what, sz + fmt(" rank %u", r), i, "df_global");
            if (dvg.down()[0] != gdf.size()) fail(what, sz, r, "vg (the distinct terms of all ranks)");
        }
    }
    ok_line(what, sz);
}
static void chain_group() {
    Rng rng(0x0A0A0A05u);
    run_chain(1, 3000, rng);
    run_chain(3, 3000, rng);
    run_chain(257, 300, rng);
    run_chain(1024, 200, rng);
}

int main(int argc, char** argv) {
    const std::string grp = argc > 1 ? argv[1] : "";
    if (grp != "owner" && grp != "dense" && grp != "long" && grp != "xport" && grp != "chain") {
        fprintf(stderr, "usage: %s owner|dense|long|xport|chain\n", argv[0]);
        return 64;
    }
    CK(hipSetDevice(0));
    CK(hipStreamCreate(&g_s));
    CK(hipMalloc((void**)&g_status, 4));
    if (grp == "owner") owner_group();
    if (grp == "dense") dense_group();
    if (grp == "long") long_group();
    if (grp == "xport") xport_group();
    if (grp == "chain") chain_group();
    CK(hipStreamSynchronize(g_s));
    CK(hipFree(g_status));
    CK(hipStreamDestroy(g_s));
    printf("ALL OK\n");
    return 0;
}
