/* GPU test of the device-wide primitives of csrc/prims.hip against host references:
 * exclusive scans (one tile, the fused two-launch form, the recursive three-launch form,
 * in place and out of place), the LSD radix sorts (fused scatter up to 1024 tiles, scanned
 * histogram above; byte masks with an odd, an even and no digit pass), the two-launch tile
 * sorts up to SORT_TILE_MAXN, and the varying-byte probes.  Links only build/prims.o.
 *
 *   prims_test scan | radix | tile | mask
 *
 * One "ok  " line per (primitive, n); "ALL OK" at the end.  Any HIP error or error return
 * ends the program at once (exit 2) without another launch; a mismatch prints the case, n and
 * the first differing index and ends it too (exit 1). */
#include "prims.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

typedef unsigned __int128 u128;   /* memory layout of uint4 {x, y, z, w}; its order is (w, z, y, x) */

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
static Arena g_ar;

static void sync_or_die(const char* what, int rc, bool neg_is_error = true) {
    if (neg_is_error && rc < 0) {
        printf("%s returned %d\n", what, rc);
        fflush(stdout);
        exit(2);
    }
    CK(hipStreamSynchronize(g_s));
    CK(hipGetLastError());
    if (g_ar.used != 0) {
        printf("%s left %zu arena bytes in use\n", what, g_ar.used);
        exit(1);
    }
}

static void mismatch(const std::string& what, uint64_t n, uint64_t idx, const char* field) {
    printf("MISMATCH %s n=%llu first differing index %llu (%s)\n", what.c_str(), (unsigned long long)n,
           (unsigned long long)idx, field);
    fflush(stdout);
    exit(1);
}

/* ---------------------------------------------------------------- dispatch ---- */
static int scan_excl(const uint32_t* i, uint32_t* o, uint64_t n) { return scan_excl_u32(i, o, n, g_ar, g_s); }
static int scan_excl(const uint64_t* i, uint64_t* o, uint64_t n) { return scan_excl_u64(i, o, n, g_ar, g_s); }
static int radix(uint64_t* k0, uint32_t* v0, uint64_t* k1, uint32_t* v1, uint64_t n, uint32_t m) {
    return radix_sort_u64(k0, v0, k1, v1, n, m, g_ar, g_s);
}
static int radix(u128* k0, uint32_t* v0, u128* k1, uint32_t* v1, uint64_t n, uint32_t m) {
    return radix_sort_u128((uint4*)k0, v0, (uint4*)k1, v1, n, m, g_ar, g_s);
}
static int tile(const uint64_t* k0, const uint32_t* v0, uint64_t* k1, uint32_t* v1, uint64_t n) {
    return tile_sort_u64(k0, v0, k1, v1, n, g_ar, g_s);
}
static int tile(const u128* k0, const uint32_t* v0, u128* k1, uint32_t* v1, uint64_t n) {
    return tile_sort_u128((const uint4*)k0, v0, (uint4*)k1, v1, n, g_ar, g_s);
}
static int varying(const uint64_t* k, uint64_t n, uint32_t* m) { return key_varying_bytes_u64(k, n, m, g_ar, g_s); }
static int varying(const u128* k, uint64_t n, uint32_t* m) { return key_varying_bytes_u128((const uint4*)k, n, m, g_ar, g_s); }

template <typename H> constexpr const char* tname();
template <> constexpr const char* tname<uint32_t>() { return "u32"; }
template <> constexpr const char* tname<uint64_t>() { return "u64"; }
template <> constexpr const char* tname<u128>() { return "u128"; }

template <typename T>
static T* dalloc(uint64_t count) {
    T* p = nullptr;
    CK(hipMalloc((void**)&p, (count ? count : 1) * sizeof(T)));
    return p;
}

/* ------------------------------------------------------------------- scans ---- */
template <typename T>
static void scan_group() {
    const uint64_t sizes[] = {0, 1, 7, 8, 9, 2047, 2048, 2049, 2048ull * 1024, 2048ull * 1024 + 1,
                              2 * 2048ull * 1024 + 5};
    const uint64_t maxn = 2 * 2048ull * 1024 + 5;
    T* din = dalloc<T>(maxn + 1);
    T* dout = dalloc<T>(maxn + 1);
    std::vector<T> in, ref, got;
    std::mt19937_64 rng(12345);
    const int ninputs = sizeof(T) == 8 ? 3 : 2;
    for (uint64_t n : sizes) {
        for (int input = 0; input < ninputs; ++input) {
            in.assign(n + 1, 0);
            for (uint64_t i = 0; i < n; ++i)
                in[i] = input == 0 ? (T)1 : input == 1 ? (T)(rng() & 15u) : (T)(1ull << 33);
            in[n] = (T)0x5A5A5A5Au;   /* the slot after the input: never read as input */
            ref.assign(n + 1, 0);
            T run = 0;
            for (uint64_t i = 0; i < n; ++i) { ref[i] = run; run += in[i]; }
            ref[n] = run;
            for (int inplace = 0; inplace < 2; ++inplace) {
                const std::string what = std::string("scan_excl_") + tname<T>() + (input == 0 ? " ones" : input == 1 ? " random" : " 2^33") +
                                         (inplace ? " in-place" : " out-of-place");
                CK(hipMemcpyAsync(din, in.data(), (n + 1) * sizeof(T), hipMemcpyHostToDevice, g_s));
                CK(hipMemsetAsync(dout, 0xCD, (n + 1) * sizeof(T), g_s));
                T* o = inplace ? din : dout;
                sync_or_die(what.c_str(), scan_excl(din, o, n));
                got.assign(n + 1, 0);
                CK(hipMemcpy(got.data(), o, (n + 1) * sizeof(T), hipMemcpyDeviceToHost));
                for (uint64_t i = 0; i <= n; ++i)
                    if (got[i] != ref[i]) mismatch(what, n, i, "prefix sum");
            }
        }
        printf("ok  scan_excl_%s n=%llu\n", tname<T>(), (unsigned long long)n);
    }
    CK(hipFree(din));
    CK(hipFree(dout));
}

/* -------------------------------------------------------------------- keys ---- */
template <typename H>
static H rnd(std::mt19937_64& g) {
    H v = (H)g();
    if constexpr (sizeof(H) == 16) v = (v << 64) | (H)g();
    return v;
}
template <typename H>
static H mask_bits(uint32_t byte_mask) {
    H r = 0;
    for (unsigned p = 0; p < sizeof(H); ++p)
        if ((byte_mask >> p) & 1u) r |= (H)0xFF << (8 * p);
    return r;
}
template <typename H>
static H fill_byte(uint8_t b) {
    H r = 0;
    for (unsigned p = 0; p < sizeof(H); ++p) r |= (H)b << (8 * p);
    return r;
}

enum KeySet { KS_RANDOM, KS_256, KS_EQUAL, KS_SORTED, KS_REVERSED, KS_CONST_UNMASKED, KS_VARY_UNMASKED, KS_ALL_ONES_MIXED, KS_COUNT };
static const char* const KS_NAME[] = {"random", "256-distinct", "all-equal", "sorted", "reversed",
                                      "constant-unmasked-bytes", "varying-unmasked-bytes", "all-ones-mixed"};

template <typename H>
static std::vector<H> gen_keys(int set, uint64_t n, uint32_t byte_mask, uint64_t seed) {
    std::mt19937_64 g(seed * 0x9E3779B97F4A7C15ull + 77);
    std::vector<H> k(n);
    const H mb = mask_bits<H>(byte_mask);
    switch (set) {
    case KS_RANDOM:
    case KS_VARY_UNMASKED:
    case KS_SORTED:
    case KS_REVERSED:
        for (auto& x : k) x = rnd<H>(g);
        if (set == KS_SORTED) std::sort(k.begin(), k.end());
        if (set == KS_REVERSED) std::sort(k.begin(), k.end(), [](H a, H b) { return a > b; });
        break;
    case KS_256: {
        H tab[256];
        for (auto& t : tab) t = rnd<H>(g);
        for (auto& x : k) x = tab[g() & 255];
        break;
    }
    case KS_EQUAL: {
        const H c = rnd<H>(g);
        for (auto& x : k) x = c;
        break;
    }
    case KS_CONST_UNMASKED:
        for (auto& x : k) x = (rnd<H>(g) & mb) | (fill_byte<H>(0xA5) & ~mb);
        break;
    case KS_ALL_ONES_MIXED: {
        H tab[8];
        for (auto& t : tab) t = rnd<H>(g);
        tab[7] = ~(H)0 - 1;   /* the largest key below the padding value */
        for (auto& x : k) {
            const uint64_t r = g();
            x = (r & 3) == 0 ? ~(H)0 : (r & 4) ? tab[(r >> 8) & 7] : rnd<H>(g);
        }
        break;
    }
    }
    return k;
}

/* stable order of the input indices by the key with the unmasked bytes cleared */
template <typename H>
static std::vector<uint32_t> ref_order(const std::vector<H>& k, uint32_t byte_mask) {
    struct Ent { H k; uint32_t i; };
    const H mb = mask_bits<H>(byte_mask);
    std::vector<Ent> e(k.size());
    for (size_t i = 0; i < k.size(); ++i) e[i] = Ent{(H)(k[i] & mb), (uint32_t)i};
    std::stable_sort(e.begin(), e.end(), [](const Ent& a, const Ent& b) { return a.k < b.k; });
    std::vector<uint32_t> o(k.size());
    for (size_t i = 0; i < k.size(); ++i) o[i] = e[i].i;
    return o;
}

template <typename H>
struct Case {
    int set;
    uint32_t mask;
    std::vector<H> keys;
    std::vector<uint32_t> order;
};

/* keys and references of all cases of one n, on up to 16 host threads */
template <typename H>
static void prepare(std::vector<Case<H>>& cs, uint64_t n, uint64_t seed0) {
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t c; (c = next.fetch_add(1)) < cs.size();) {
            cs[c].keys = gen_keys<H>(cs[c].set, n, cs[c].mask, seed0 + c);
            cs[c].order = ref_order<H>(cs[c].keys, cs[c].mask);
        }
    };
    const size_t nth = n < 100000 ? 1 : std::min<size_t>(16, cs.size());
    std::vector<std::thread> th;
    for (size_t t = 1; t < nth; ++t) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
}

template <typename H>
static void compare_sorted(const std::string& what, const Case<H>& c, uint64_t n, const std::vector<H>& gk,
                           const std::vector<uint32_t>& gv) {
    for (uint64_t i = 0; i < n; ++i) {
        if (gv[i] != c.order[i]) mismatch(what, n, i, "value");
        if (gk[i] != c.keys[c.order[i]]) mismatch(what, n, i, "key");
    }
}

template <typename H>
struct SortBufs {
    H *k0, *k1;
    uint32_t *v0, *v1;
    std::vector<uint32_t> iota;
    explicit SortBufs(uint64_t maxn) : iota(maxn) {
        k0 = dalloc<H>(maxn); k1 = dalloc<H>(maxn); v0 = dalloc<uint32_t>(maxn); v1 = dalloc<uint32_t>(maxn);
        for (uint64_t i = 0; i < maxn; ++i) iota[i] = (uint32_t)i;
    }
    ~SortBufs() { (void)hipFree(k0); (void)hipFree(k1); (void)hipFree(v0); (void)hipFree(v1); }
    void load(const std::vector<H>& keys, uint64_t n) {
        if (n) {
            CK(hipMemcpyAsync(k0, keys.data(), n * sizeof(H), hipMemcpyHostToDevice, g_s));
            CK(hipMemcpyAsync(v0, iota.data(), n * 4, hipMemcpyHostToDevice, g_s));
        }
        CK(hipMemsetAsync(k1, 0xCD, (n ? n : 1) * sizeof(H), g_s));
        CK(hipMemsetAsync(v1, 0xCD, (n ? n : 1) * 4, g_s));
    }
    void read(int buf, uint64_t n, std::vector<H>& gk, std::vector<uint32_t>& gv) {
        gk.assign(n, 0); gv.assign(n, 0);
        if (!n) return;
        CK(hipMemcpy(gk.data(), buf ? k1 : k0, n * sizeof(H), hipMemcpyDeviceToHost));
        CK(hipMemcpy(gv.data(), buf ? v1 : v0, n * 4, hipMemcpyDeviceToHost));
    }
};

/* ------------------------------------------------------------- radix sorts ---- */
template <typename H>
static void radix_group() {
    const uint64_t sizes[] = {0, 1, 2, 64, 65, 2047, 2048, 2049, 131073, 2097152, 2097153, 3000001};
    constexpr bool W = sizeof(H) == 16;
    const uint32_t full = W ? 0xFFFFu : 0xFFu;
    /* odd pass count / even / one pass / even across the first and last bytes */
    const uint32_t partial[] = {W ? 0x7FFFu : 0x7Fu, W ? 0x0FF0u : 0x3Cu, W ? 0x0100u : 0x01u, W ? 0x8001u : 0x81u};
    SortBufs<H> b(3000001);
    std::vector<H> gk;
    std::vector<uint32_t> gv;
    uint64_t seed = W ? 1000 : 0;
    for (uint64_t n : sizes) {
        std::vector<Case<H>> cs;
        for (int set : {KS_RANDOM, KS_256, KS_EQUAL, KS_SORTED, KS_REVERSED}) cs.push_back({set, full, {}, {}});
        cs.push_back({KS_RANDOM, 0u, {}, {}});
        const int np = n > 200000 ? 2 : 4;   /* the large sizes: the odd and the even pass count */
        for (int p = 0; p < np; ++p)
            for (int set : {KS_CONST_UNMASKED, KS_VARY_UNMASKED, KS_256}) cs.push_back({set, partial[p], {}, {}});
        prepare(cs, n, seed);
        seed += cs.size();
        for (const auto& c : cs) {
            char tag[128];
            snprintf(tag, sizeof tag, "radix_sort_%s %s byte_mask=0x%x", tname<H>(), KS_NAME[c.set], c.mask);
            b.load(c.keys, n);
            const int rc = radix(b.k0, b.v0, b.k1, b.v1, n, c.mask);
            sync_or_die(tag, rc);
            const int want = (n <= 1 || c.mask == 0) ? 0 : (__builtin_popcount(c.mask & full) & 1);
            if (rc != want) {
                printf("MISMATCH %s n=%llu: result reported in buffer %d, expected %d\n", tag, (unsigned long long)n, rc, want);
                exit(1);
            }
            b.read(rc, n, gk, gv);
            compare_sorted(tag, c, n, gk, gv);
        }
        printf("ok  radix_sort_%s n=%llu (%zu cases)\n", tname<H>(), (unsigned long long)n, cs.size());
        fflush(stdout);
    }
}

/* -------------------------------------------------------------- tile sorts ---- */
template <typename H>
static void tile_group() {
    const uint64_t sizes[] = {0, 1, 2, 2047, 2048, 2049, 16384, 16385, 131071, 131072};
    constexpr bool W = sizeof(H) == 16;
    const uint32_t full = W ? 0xFFFFu : 0xFFu;
    SortBufs<H> b(SORT_TILE_MAXN + 1);
    std::vector<H> gk, rk;
    std::vector<uint32_t> gv, rv;
    uint64_t seed = W ? 3000 : 2000;
    for (uint64_t n : sizes) {
        std::vector<Case<H>> cs;
        for (int set : {KS_RANDOM, KS_256, KS_EQUAL, KS_SORTED, KS_REVERSED, KS_ALL_ONES_MIXED}) cs.push_back({set, full, {}, {}});
        cs.push_back({KS_CONST_UNMASKED, W ? 0x0FF0u : 0x3Cu, {}, {}});
        prepare(cs, n, seed);
        seed += cs.size();
        for (auto& c : cs) {
            /* the tile sort orders by the whole key, whatever bytes the generator varied */
            c.order = ref_order<H>(c.keys, full);
            char tag[128];
            snprintf(tag, sizeof tag, "tile_sort_%s %s", tname<H>(), KS_NAME[c.set]);
            b.load(c.keys, n);
            const int rc = tile(b.k0, b.v0, b.k1, b.v1, n);
            sync_or_die(tag, rc);
            if (rc != 1) {
                printf("MISMATCH %s n=%llu: returned %d, expected 1\n", tag, (unsigned long long)n, rc);
                exit(1);
            }
            b.read(1, n, gk, gv);
            compare_sorted(tag, c, n, gk, gv);
            /* prims.h: the same result as the radix sort over all bytes */
            b.load(c.keys, n);
            const int rr = radix(b.k0, b.v0, b.k1, b.v1, n, full);
            sync_or_die("radix sort for the tile sort", rr);
            b.read(rr, n, rk, rv);
            for (uint64_t i = 0; i < n; ++i) {
                if (rv[i] != gv[i]) mismatch(std::string(tag) + " vs radix", n, i, "value");
                if (rk[i] != gk[i]) mismatch(std::string(tag) + " vs radix", n, i, "key");
            }
        }
        printf("ok  tile_sort_%s n=%llu (%zu cases)\n", tname<H>(), (unsigned long long)n, cs.size());
        fflush(stdout);
    }
    {   /* one key over the limit: refused before any launch */
        const uint64_t n = SORT_TILE_MAXN + 1;
        std::vector<H> keys = gen_keys<H>(KS_RANDOM, n, full, seed);
        b.load(keys, n);
        const int rc = tile(b.k0, b.v0, b.k1, b.v1, n);
        sync_or_die("tile sort over the limit", rc, false);
        if (rc != -3) {
            printf("MISMATCH tile_sort_%s n=%llu: returned %d, expected -3\n", tname<H>(), (unsigned long long)n, rc);
            exit(1);
        }
        b.read(1, n, gk, gv);
        for (uint64_t i = 0; i < n; ++i)
            if (gv[i] != 0xCDCDCDCDu) mismatch("tile sort over the limit wrote output", n, i, "value");
        printf("ok  tile_sort_%s n=%llu returns -3\n", tname<H>(), (unsigned long long)n);
    }
}

/* ----------------------------------------------------- varying-byte masks ---- */
template <typename H>
static uint32_t host_varying(const std::vector<H>& k) {
    H a = ~(H)0, o = 0;
    for (H x : k) { a &= x; o |= x; }
    uint32_t m = 0;
    for (unsigned p = 0; p < sizeof(H); ++p)
        if ((uint8_t)((a ^ o) >> (8 * p))) m |= 1u << p;
    return m;
}

template <typename H>
static void mask_one(const char* what, const std::vector<H>& k, H* dk, bool expect_given, uint32_t expect) {
    const uint64_t n = k.size();
    CK(hipMemcpyAsync(dk, k.data(), n * sizeof(H), hipMemcpyHostToDevice, g_s));
    uint32_t got = 0xDEADBEEFu;
    sync_or_die(what, varying(dk, n, &got));
    const uint32_t want = host_varying<H>(k);
    if (expect_given && want != expect) {
        printf("MISMATCH %s n=%llu: the host reference gives 0x%x, the case was built for 0x%x\n", what, (unsigned long long)n, want, expect);
        exit(1);
    }
    if (got != want) {
        printf("MISMATCH key_varying_bytes_%s %s n=%llu: mask 0x%x, expected 0x%x\n", tname<H>(), what, (unsigned long long)n, got, want);
        exit(1);
    }
}

template <typename H>
static void mask_group() {
    const uint64_t maxn = 2048 * 100 + 1;
    H* dk = dalloc<H>(maxn);
    std::mt19937_64 g(sizeof(H) * 31);
    for (uint64_t n : {(uint64_t)2, (uint64_t)2049, maxn})
        mask_one<H>("constant keys", std::vector<H>(n, rnd<H>(g)), dk, true, 0u);
    printf("ok  key_varying_bytes_%s constant keys\n", tname<H>());
    for (int r = 0; r < 4; ++r) mask_one<H>("n = 1", std::vector<H>(1, r == 0 ? ~(H)0 : r == 1 ? (H)0 : rnd<H>(g)), dk, true, 0u);
    printf("ok  key_varying_bytes_%s n=1\n", tname<H>());
    /* one byte differs, in the last element only; the larger n wraps the grid-stride loop */
    for (uint64_t n : {(uint64_t)2049, 3 * (uint64_t)2048 + 1, maxn})
        for (unsigned p = 0; p < sizeof(H); ++p)
            for (int flip = 0; flip < 2; ++flip) {   /* a bit set only there / cleared only there */
                std::vector<H> k(n, flip ? ~(H)0 : (H)0);
                k[n - 1] ^= (H)(p & 1 ? 0x80 : 0x01) << (8 * p);
                mask_one<H>("last element differs in one byte", k, dk, true, 1u << p);
            }
    printf("ok  key_varying_bytes_%s last element differs in one byte\n", tname<H>());
    for (uint64_t n : {(uint64_t)2, (uint64_t)3, (uint64_t)255, (uint64_t)4097, maxn})
        for (uint32_t bm : {0xFFFFu, 0x0FF0u, 0x8001u, 0x0055u}) {
            std::vector<H> k = gen_keys<H>(KS_CONST_UNMASKED, n, bm, n + bm);
            mask_one<H>("random keys", k, dk, false, 0u);
        }
    printf("ok  key_varying_bytes_%s random keys\n", tname<H>());
    CK(hipFree(dk));
}

int main(int argc, char** argv) {
    const std::string grp = argc > 1 ? argv[1] : "";
    if (grp != "scan" && grp != "radix" && grp != "tile" && grp != "mask") {
        fprintf(stderr, "usage: %s scan|radix|tile|mask\n", argv[0]);
        return 2;
    }
    CK(hipSetDevice(0));
    CK(hipStreamCreate(&g_s));
    g_ar.cap = 64ull << 20;
    CK(hipMalloc((void**)&g_ar.base, g_ar.cap));
    if (grp == "scan") { scan_group<uint32_t>(); scan_group<uint64_t>(); }
    if (grp == "radix") { radix_group<uint64_t>(); radix_group<u128>(); }
    if (grp == "tile") { tile_group<uint64_t>(); tile_group<u128>(); }
    if (grp == "mask") { mask_group<uint64_t>(); mask_group<u128>(); }
    CK(hipStreamSynchronize(g_s));
    CK(hipFree(g_ar.base));
    CK(hipStreamDestroy(g_s));
    printf("ALL OK\n");
    return 0;
}
