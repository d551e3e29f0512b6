/*
 * topk_test — k_query_topk (csrc/query.hip) through launch_query_topk on crafted arrays, round by
 * round, against plain host sorts: no engine, no corpus (tests/test_gpu_topk_native.py runs it;
 * links query.o alone).  The driver here is the program's own and follows the contract of QTopkArgs
 * (csrc/kernels.h): round 1 over the N output positions in ceil(N / QT_SLICE) slices, every later
 * round over the nsl lists of k as nsl * k inputs, nsl <- ceil(nsl * k / QT_SLICE), until one slice
 * is left, the two candidate buffers swapped every round.
 *
 *   rounds   N in {1, 4095, 4096, 4097, 16384, 16385, 20000, 65537, 70001} x k in {1, 10, 1000,
 *            1024} (65537 at k = 1024: four launches, [17, 5, 2, 1]) x six hit patterns: every
 *            position, none, the last position alone, the last slice alone, fewer than k in every
 *            slice, a random 30 %.  One or three queries.  Scores from seven values (ties are the
 *            rule), among them +0.0, the smallest subnormal and DBL_MAX.  Ids through a permuted
 *            order and arbitrary 32-bit doc_ids, through a permuted order with doc_ids null
 *            (index + 1), and all above 2^31.
 *   clauses  need != null in the first round: count words on both sides of every field boundary
 *            of CL_INC_* / CL_FIELD against the rule of kernels.h written out below
 *
 * Before every launch the whole output buffer is filled with all-ones; after it the buffer must be
 * exactly the host's image of that round: the expected lists, and all-ones everywhere else, so an
 * entry past a list's count that a later round took up, or a write outside [0, out_n), shows.
 * nmatch is zeroed before round 1, equals the hit count after it and stays.  The last round's list
 * must equal a direct sort of all hits.  Prints one "ok  " line per case and "ALL OK"; ends at the
 * first HIP error or mismatch with a non-zero status.
 */
#include <hip/hip_runtime.h>

#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

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

template <typename T> static T* up(const std::vector<T>& h) {
    T* d = nullptr;
    CK(hipMalloc((void**)&d, (h.size() + 1) * sizeof(T)));
    if (!h.empty()) CK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
template <typename T> static std::vector<T> down(const T* d, size_t n) {
    std::vector<T> h(n);
    if (n) CK(hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
    return h;
}
static void fail(const char* what, const char* field, unsigned round, uint64_t idx) {
    printf("MISMATCH %s: %s in round %u at index %llu\n", what, field, round, (unsigned long long)idx);
    exit(1);
}
static uint64_t bits(double x) {
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
}

struct Hit {
    uint64_t s;   /* the score's bit pattern */
    uint32_t id;
};
/* a before b: score descending (the patterns of scores >= +0.0 order like the values), id ascending */
static bool before(const Hit& a, const Hit& b) { return a.s != b.s ? a.s > b.s : a.id < b.id; }
typedef std::vector<Hit> List;

/* the clause test of a count word as kernels.h states it: need = |M| << 12 | min_should; no must_not
 * term (bits 24..31), every must term (bits 12..23), enough should terms (bits 0..11), and at least
 * one scoring term */
static bool clause_hit(uint32_t cnt, uint32_t need) {
    const uint32_t nots = cnt >> 24, must = (cnt >> 12) & 0xFFFu, should = cnt & 0xFFFu;
    if (nots != 0u) return false;
    if (must != need >> 12) return false;
    if (should < (need & 0xFFFu)) return false;
    return must + should != 0u;
}

struct Input {
    uint32_t N, k, nq;
    std::vector<double> acc;     /* [nq][N] */
    std::vector<uint32_t> cnt;   /* [nq][N] */
    std::vector<uint32_t> order, doc_ids, need;   /* doc_ids / need empty: null */
};

/* one slice of a round on the host: the valid inputs, sorted, cut at k */
static List best_of(List in, uint32_t k) {
    std::sort(in.begin(), in.end(), before);
    if (in.size() > k) in.resize(k);
    return in;
}

static void run_case(const char* what, const Input& in) {
    static_assert(CL_INC_SHOULD == 1u && CL_INC_MUST == 1u << 12 && CL_INC_NOT == 1u << 24 && CL_FIELD == 0xFFFu,
                  "clause_hit above is written for these fields");
    const uint32_t N = in.N, k = in.k, nq = in.nq;
    const uint64_t nsl0 = ((uint64_t)N + QT_SLICE - 1) / QT_SLICE;
    const size_t cand_el = (size_t)nq * nsl0 * k, n_el = (size_t)nq * nsl0;
    /* ---- the host's first round, and the direct reference ---- */
    std::vector<std::vector<List>> lists(nq, std::vector<List>(nsl0));
    std::vector<List> want(nq);
    std::vector<uint64_t> nhit(nq, 0);
    for (uint32_t q = 0; q < nq; ++q) {
        List all;
        for (uint64_t sl = 0; sl < nsl0; ++sl) {
            List mine;
            for (uint64_t e = sl * QT_SLICE; e < N && e < (sl + 1) * QT_SLICE; ++e) {
                const uint32_t c = in.cnt[(size_t)q * N + e];
                if (!(in.need.empty() ? c != 0u : clause_hit(c, in.need[q]))) continue;
                const uint32_t d = in.order[e];
                mine.push_back(Hit{bits(in.acc[(size_t)q * N + e]), in.doc_ids.empty() ? d + 1u : in.doc_ids[d]});
            }
            all.insert(all.end(), mine.begin(), mine.end());
            lists[q][sl] = best_of(mine, k);
        }
        nhit[q] = all.size();
        want[q] = best_of(all, k);
    }
    /* ---- the device ---- */
    double* d_acc = up(in.acc);
    uint32_t* d_cnt = up(in.cnt);
    uint32_t* d_order = up(in.order);
    uint32_t* d_ids = in.doc_ids.empty() ? nullptr : up(in.doc_ids);
    uint32_t* d_need = in.need.empty() ? nullptr : up(in.need);
    uint64_t* d_s[2];
    uint32_t *d_id[2], *d_n[2];
    for (int c = 0; c < 2; ++c) {
        CK(hipMalloc((void**)&d_s[c], cand_el * 8 + 8));
        CK(hipMalloc((void**)&d_id[c], cand_el * 4 + 4));
        CK(hipMalloc((void**)&d_n[c], n_el * 4 + 4));
    }
    unsigned long long* d_nm = nullptr;
    CK(hipMalloc((void**)&d_nm, (size_t)nq * 8));
    CK(hipMemset(d_nm, 0, (size_t)nq * 8));
    unsigned round = 1, launches = 0;
    int cur = 0;
    uint64_t nsl = nsl0, n_in = N;
    for (;;) {
        const uint64_t out_slices = round == 1 ? nsl0 : (n_in + QT_SLICE - 1) / QT_SLICE;
        QTopkArgs a{};
        if (round == 1) {
            a.acc = d_acc;
            a.cnt = d_cnt;
            a.need = d_need;
            a.order = d_order;
            a.doc_ids = d_ids;
        } else {
            a.in_s = d_s[cur ^ 1];
            a.in_id = d_id[cur ^ 1];
            a.in_n = d_n[cur ^ 1];
            a.in_slices = (uint32_t)nsl;
            /* the host's model of this round: the nsl lists as nsl * k inputs, cut into slices */
            std::vector<std::vector<List>> next(nq, std::vector<List>(out_slices));
            for (uint32_t q = 0; q < nq; ++q)
                for (uint64_t o = 0; o < out_slices; ++o) {
                    List mine;
                    for (uint64_t e = o * QT_SLICE; e < n_in && e < (o + 1) * QT_SLICE; ++e) {
                        const List& l = lists[q][e / k];
                        if (e % k < l.size()) mine.push_back(l[e % k]);
                    }
                    next[q][o] = best_of(mine, k);
                }
            lists.swap(next);
        }
        a.n_in = n_in;
        a.kk = k;
        a.out_s = d_s[cur];
        a.out_id = d_id[cur];
        a.out_n = d_n[cur];
        a.out_slices = (uint32_t)out_slices;
        a.nmatch = d_nm;
        CK(hipMemsetAsync(d_s[cur], 0xFF, cand_el * 8, g_s));
        CK(hipMemsetAsync(d_id[cur], 0xFF, cand_el * 4, g_s));
        CK(hipMemsetAsync(d_n[cur], 0xFF, n_el * 4, g_s));
        if (launch_query_topk(a, nq, g_s)) { printf("%s: the launch of round %u failed\n", what, round); exit(2); }
        CK(hipStreamSynchronize(g_s));
        ++launches;
        /* the buffer is the host's image of the round: the lists, all-ones everywhere else */
        std::vector<uint64_t> img_s(cand_el, ~0ull);
        std::vector<uint32_t> img_id(cand_el, ~0u), img_n(n_el, ~0u);
        for (uint32_t q = 0; q < nq; ++q)
            for (uint64_t o = 0; o < out_slices; ++o) {
                const List& l = lists[q][o];
                const size_t row = (size_t)q * out_slices + o;
                img_n[row] = (uint32_t)l.size();
                for (size_t i = 0; i < l.size(); ++i) {
                    if (l[i].id == ~0u || l[i].s == ~0ull) { printf("harness bug: %s holds an all-ones entry\n", what); exit(1); }
                    img_s[row * k + i] = l[i].s;
                    img_id[row * k + i] = l[i].id;
                }
            }
        const auto g_n = down(d_n[cur], n_el);
        const auto g_sc = down(d_s[cur], cand_el);
        const auto g_id = down(d_id[cur], cand_el);
        for (size_t i = 0; i < n_el; ++i) if (g_n[i] != img_n[i]) fail(what, "out_n", round, i);
        for (size_t i = 0; i < cand_el; ++i) {
            if (g_id[i] != img_id[i]) fail(what, "out_id", round, i);
            if (g_sc[i] != img_s[i]) fail(what, "out_s", round, i);
        }
        const auto g_nm = down(d_nm, nq);
        for (uint32_t q = 0; q < nq; ++q) if (g_nm[q] != nhit[q]) fail(what, "nmatch", round, q);
        if (out_slices <= 1) break;
        nsl = out_slices;
        n_in = nsl * k;
        cur ^= 1;
        ++round;
    }
    /* the rule's own count of launches, and the last list against the direct sort */
    unsigned expect = 1;
    for (uint64_t s = nsl0; s > 1; s = (s * k + QT_SLICE - 1) / QT_SLICE) ++expect;
    if (launches != expect) fail(what, "the number of launches", launches, expect);
    for (uint32_t q = 0; q < nq; ++q) {
        const List& l = lists[q][0];
        if (l.size() != want[q].size()) fail(what, "the result's length", round, q);
        for (size_t i = 0; i < l.size(); ++i)
            if (l[i].s != want[q][i].s || l[i].id != want[q][i].id) fail(what, "the result", round, (uint64_t)q * k + i);
    }
    CK(hipFree(d_acc)); CK(hipFree(d_cnt)); CK(hipFree(d_order));
    if (d_ids) CK(hipFree(d_ids));
    if (d_need) CK(hipFree(d_need));
    for (int c = 0; c < 2; ++c) { CK(hipFree(d_s[c])); CK(hipFree(d_id[c])); CK(hipFree(d_n[c])); }
    CK(hipFree(d_nm));
    printf("ok  %s: %u launches\n", what, launches);
}

/* ------------------------------------------------------------------ inputs -- */

static double score_value(uint32_t i) {
    double sub;
    const uint64_t one = 1ull;
    memcpy(&sub, &one, 8);   /* the smallest subnormal */
    const double v[7] = {0.0, sub, DBL_MIN, 0.5, 1.0, 2.5, DBL_MAX};
    return v[i % 7u];
}

enum IdMode { ID_PERM_IDS, ID_PERM_NULL, ID_HIGH };
static const char* const ID_NAME[3] = {"permuted order and 32-bit ids", "permuted order, ids null", "ids above 2^31"};

static void make_ids(Input& in, IdMode mode, std::mt19937& rng) {
    in.order.resize(in.N);
    std::iota(in.order.begin(), in.order.end(), 0u);
    if (mode != ID_HIGH) std::shuffle(in.order.begin(), in.order.end(), rng);
    if (mode == ID_PERM_NULL) return;
    in.doc_ids.resize(in.N);
    for (uint32_t d = 0; d < in.N; ++d) {
        /* an odd multiplier is a bijection of the 32-bit words: distinct ids over the whole range; the
         * all-ones word (the poison) would be document 0xFFFFFFFF / 2654435761's, far past any N here */
        in.doc_ids[d] = mode == ID_HIGH ? 0x80000001u + 3u * d : (d + 1u) * 2654435761u;
        if (in.doc_ids[d] == ~0u) { printf("harness bug: an all-ones id\n"); exit(1); }
    }
}

enum Pattern { P_ALL, P_NONE, P_LAST, P_LAST_SLICE, P_SHORT, P_RANDOM, P_COUNT };
static const char* const P_NAME[P_COUNT] = {"every position a hit", "no hit", "one hit at the last position",
                                            "hits in the last slice alone", "fewer than k hits in every slice", "a random 30 %"};

static void rounds_group() {
    const uint32_t Ns[] = {1u, 4095u, 4096u, 4097u, 16384u, 16385u, 20000u, 65537u, 70001u};
    const uint32_t ks[] = {1u, 10u, 1000u, 1024u};
    unsigned ncase = 0;
    for (uint32_t N : Ns)
        for (uint32_t k : ks)
            for (int p = 0; p < P_COUNT; ++p, ++ncase) {
                std::mt19937 rng(1000u * ncase + 17u);
                Input in;
                in.N = N; in.k = k;
                in.nq = (ncase + ncase / P_COUNT) % 2u ? 3u : 1u;   /* both for every (N, k) */
                const IdMode mode = (IdMode)((ncase + ncase / P_COUNT) % 3u);
                make_ids(in, mode, rng);
                in.acc.resize((size_t)in.nq * N);
                in.cnt.assign((size_t)in.nq * N, 0u);
                const uint32_t last0 = (N - 1u) / QT_SLICE * QT_SLICE;   /* the last slice's first position */
                for (uint32_t q = 0; q < in.nq; ++q) {
                    uint32_t* cnt = in.cnt.data() + (size_t)q * N;
                    switch (p) {
                    case P_ALL: for (uint32_t e = 0; e < N; ++e) cnt[e] = 1u + rng() % 5u; break;
                    case P_NONE: break;
                    case P_LAST: cnt[N - 1u] = 1u; break;
                    case P_LAST_SLICE: for (uint32_t e = last0; e < N; ++e) cnt[e] = 1u + rng() % 5u; break;
                    case P_SHORT:
                        for (uint32_t e0 = 0, sl = 0; e0 < N; e0 += QT_SLICE, ++sl) {
                            const uint32_t len = N - e0 < QT_SLICE ? N - e0 : QT_SLICE;
                            std::vector<uint32_t> at(len);
                            std::iota(at.begin(), at.end(), e0);
                            std::shuffle(at.begin(), at.end(), rng);
                            uint32_t n = (sl + q) % 2u ? (k - 1u) / 2u : k - 1u;   /* k = 1: none */
                            if (n > len) n = len;
                            for (uint32_t i = 0; i < n; ++i) cnt[at[i]] = 1u + rng() % 5u;
                        }
                        break;
                    default: for (uint32_t e = 0; e < N; ++e) cnt[e] = rng() % 10u < 3u ? 1u + rng() % 5u : 0u; break;
                    }
                    /* scores from seven values; where there is no hit, a value that would win if it were taken */
                    for (uint32_t e = 0; e < N; ++e) in.acc[(size_t)q * N + e] = cnt[e] ? score_value(rng()) : DBL_MAX;
                }
                char what[160];
                snprintf(what, sizeof what, "N=%u k=%u nq=%u %s, %s", N, k, in.nq, P_NAME[p], ID_NAME[mode]);
                run_case(what, in);
            }
}

static void clauses_group() {
    /* need words: no clause at all, one must term, three must terms and two should terms, should terms
     * alone (2, and the full field), both fields full */
    const std::vector<uint32_t> need = {0u, 1u << 12, 3u << 12 | 2u, 2u, 0xFFFu, 0xFFFu << 12 | 0xFFFu};
    const uint32_t Ns[] = {4097u, 20000u, 65537u};
    const uint32_t ks[] = {10u, 1000u, 1024u};
    unsigned ncase = 0;
    for (uint32_t N : Ns)
        for (uint32_t k : ks) {
            std::mt19937 rng(77u + ncase);
            Input in;
            in.N = N; in.k = k; in.nq = (uint32_t)need.size();
            in.need = need;
            make_ids(in, (IdMode)(ncase++ % 3u), rng);
            in.acc.resize((size_t)in.nq * N);
            in.cnt.resize((size_t)in.nq * N);
            uint64_t nhits = 0, edge[6] = {0, 0, 0, 0, 0, 0};
            for (uint32_t q = 0; q < in.nq; ++q) {
                const uint32_t M = need[q] >> 12, m = need[q] & 0xFFFu;
                for (uint32_t e = 0; e < N; ++e) {
                    uint32_t nots = 0, must = M, should = m + rng() % 3u;
                    if (should > 0xFFFu) should = 0xFFFu;
                    if (rng() % 10u >= 6u) {   /* 40 %: a value at a field's boundary */
                        const uint32_t nv[3] = {0u, 1u, 0xFFu};
                        const uint32_t mv[3] = {M ? M - 1u : 0u, M, M < 0xFFFu ? M + 1u : M};
                        const uint32_t sv[4] = {m ? m - 1u : 0u, m, 0xFFFu, 0u};
                        nots = nv[rng() % 3u];
                        must = mv[rng() % 3u];
                        should = sv[rng() % 4u];
                    }
                    const uint32_t c = nots << 24 | must << 12 | should;
                    in.cnt[(size_t)q * N + e] = c;
                    const bool hit = clause_hit(c, need[q]);
                    nhits += hit;
                    edge[0] += nots == 1u; edge[1] += nots == 0xFFu;
                    edge[2] += must + 1u == M; edge[3] += must == M + 1u;
                    edge[4] += m && should + 1u == m;
                    edge[5] += (c & 0xFFFFFFu) == 0u;
                    in.acc[(size_t)q * N + e] = hit ? score_value(rng()) : DBL_MAX;
                }
            }
            for (uint64_t x : edge) if (!x) { printf("harness bug: a boundary of the count word is not reached\n"); exit(1); }
            if (nhits < (uint64_t)N || nhits > (uint64_t)in.nq * N * 9 / 10) { printf("harness bug: %llu hits\n", (unsigned long long)nhits); exit(1); }
            char what[160];
            snprintf(what, sizeof what, "clauses N=%u k=%u nq=%u, %llu of %llu count words pass", N, k, in.nq,
                     (unsigned long long)nhits, (unsigned long long)in.nq * N);
            run_case(what, in);
        }
}

int main(int argc, char** argv) {
    const char* group = argc > 1 ? argv[1] : "all";
    CK(hipSetDevice(0));
    CK(hipStreamCreate(&g_s));
    if (!strcmp(group, "rounds") || !strcmp(group, "all")) rounds_group();
    if (!strcmp(group, "clauses") || !strcmp(group, "all")) clauses_group();
    CK(hipStreamDestroy(g_s));
    printf("ALL OK\n");
    return 0;
}
