/*
 * nb_test — the count, reduction and predict kernels of csrc/nb.hip on crafted arrays against
 * plain host loops: no engine, no corpus (tests/test_gpu_nb_native.py runs it; links nb.o alone).
 *
 *   count    documents of one class whose counts of one term are 0xFFFFFFFF each: the sum passes
 *            2^32, which no corpus of test size reaches; FC, F and T against the loops, both
 *            feature modes, unlabelled documents and an empty one between them
 *   predict  crafted W rows: two classes that tie exactly (the lowest wins); a negative score
 *            whose bit pattern is the largest beside a positive winner; scores that are all
 *            negative; the winner in each of the four accumulator slots of a lane; rows of 0, 1,
 *            63, 64, 65 and 200 pairs; a row the caller marks as not held
 *
 * Every comparison is exact (doubles as bit patterns).  Prints one "ok  " line per case and
 * "ALL OK"; ends at the first HIP error or mismatch with a non-zero status.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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
static uint32_t g_ncu;

template <typename T> static T* up(const std::vector<T>& h, size_t extra = 0) {
    T* d = nullptr;
    CK(hipMalloc((void**)&d, (h.size() + extra + 1) * sizeof(T)));
    CK(hipMemset(d, 0, (h.size() + extra + 1) * sizeof(T)));
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
static uint64_t bits(double x) {
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
}

struct Rows {
    std::vector<uint64_t> off{0};
    std::vector<uint32_t> term, cnt;
    void add(const std::vector<uint32_t>& t, const std::vector<uint32_t>& c) {
        term.insert(term.end(), t.begin(), t.end());
        cnt.insert(cnt.end(), c.begin(), c.end());
        off.push_back(term.size());
    }
    uint32_t n() const { return (uint32_t)off.size() - 1; }
};

/* ------------------------------------------------------------------- count -- */

static void count_case(const char* what, const Rows& r, const std::vector<uint32_t>& lab, uint32_t V, uint32_t K, bool binary) {
    const uint32_t N = r.n();
    std::vector<uint64_t> FC((size_t)V * K, 0), F(V, 0), T(K, 0);
    for (uint32_t j = 0; j < N; ++j) {
        if (lab[j] >= K) continue;
        for (uint64_t p = r.off[j]; p < r.off[j + 1]; ++p) FC[(size_t)r.term[p] * K + lab[j]] += binary ? 1u : r.cnt[p];
    }
    uint64_t amax = 0;
    for (uint32_t t = 0; t < V; ++t)
        for (uint32_t c = 0; c < K; ++c) {
            const uint64_t v = FC[(size_t)t * K + c];
            F[t] += v;
            T[c] += v;
            amax = v > amax ? v : amax;
        }
    NbFitArgs a{};
    uint64_t* d_off = up(r.off);
    uint32_t* d_term = up(r.term);
    uint32_t* d_cnt = up(r.cnt);
    uint32_t* d_lab = up(lab);
    uint64_t* d_FC = up(std::vector<uint64_t>((size_t)V * K, ~0ull));   /* the launch clears it */
    uint64_t* d_F = up(std::vector<uint64_t>(V, ~0ull));
    uint64_t* d_T = up(std::vector<uint64_t>(K, ~0ull));
    uint64_t* d_misc = up(std::vector<uint64_t>(4, ~0ull));
    a.off = d_off; a.term = d_term; a.cnt = d_cnt;
    a.npairs = r.term.size();
    a.ndocs = N; a.V = V; a.K = K;
    a.binary = binary;
    a.lab = d_lab;
    a.FC = d_FC; a.F = d_F; a.T = d_T; a.misc = d_misc;
    a.lut_n = (uint64_t)NB_LUT_MAX + 1;
    if (launch_nb_count(a, g_ncu, g_s) || launch_nb_sums(a, g_ncu, g_s) || launch_nb_argmax(a, g_ncu, g_s)) {
        printf("%s: a launch failed\n", what);
        exit(2);
    }
    CK(hipStreamSynchronize(g_s));
    const auto gFC = down(d_FC, FC.size());
    const auto gF = down(d_F, V);
    const auto gT = down(d_T, K);
    const auto gm = down(d_misc, 2);
    for (size_t i = 0; i < FC.size(); ++i) if (gFC[i] != FC[i]) fail(what, "FC", i);
    for (uint32_t t = 0; t < V; ++t) if (gF[t] != F[t]) fail(what, "F", t);
    for (uint32_t c = 0; c < K; ++c) if (gT[c] != T[c]) fail(what, "T", c);
    uint64_t past = 0;
    for (uint64_t v : FC) past += v > NB_LUT_MAX;
    if (gm[0] != amax) fail(what, "the largest argument", 0);
    if (gm[1] != past) fail(what, "the arguments past the table", 0);
    CK(hipFree(d_off)); CK(hipFree(d_term)); CK(hipFree(d_cnt)); CK(hipFree(d_lab));
    CK(hipFree(d_FC)); CK(hipFree(d_F)); CK(hipFree(d_T)); CK(hipFree(d_misc));
    printf("ok  %s\n", what);
}

static void count_group() {
    {   /* the 64-bit accumulation */
        Rows r;
        r.add({2}, {0xFFFFFFFFu});
        r.add({}, {});
        r.add({2}, {0xFFFFFFFFu});
        r.add({0, 2}, {7, 9});          /* unlabelled */
        r.add({1, 2}, {5, 1});
        const std::vector<uint32_t> lab = {1, 1, 1, NB_NO_CLASS, 0};
        count_case("count two documents of 0xFFFFFFFF sum to 2^33-2", r, lab, 3, 3, false);
        count_case("count the same, binary", r, lab, 3, 3, true);
    }
    for (uint32_t K : {1u, 64u, 65u, 129u, 256u}) {   /* many documents: every wave strides */
        Rows r;
        std::vector<uint32_t> lab;
        const uint32_t V = 301, N = 3000;
        uint32_t x = 12345u;
        for (uint32_t j = 0; j < N; ++j) {
            std::vector<uint32_t> t, c;
            const uint32_t n = j % 7 == 3 ? 0u : 1u + (j * 37u) % 150u;
            uint32_t at = j % V;
            for (uint32_t i = 0; i < n && at < V; ++i) {
                x = x * 1664525u + 1013904223u;
                t.push_back(at);
                c.push_back(1u + (x >> 20));
                at += 1u + (x >> 8) % 3u;
            }
            r.add(t, c);
            lab.push_back(j % 5 == 4 ? NB_NO_CLASS : (j * 7u) % K);
        }
        char what[96];
        snprintf(what, sizeof what, "count 3000 documents K=%u", K);
        count_case(what, r, lab, V, K, false);
    }
}

/* ----------------------------------------------------------------- predict -- */

static void predict_case(const char* what, const Rows& r, const std::vector<uint32_t>& pos, uint32_t ndocs,
                         const std::vector<double>& W, const std::vector<double>& prior, uint32_t V, uint32_t K, bool binary,
                         const std::vector<uint32_t>* want_label) {
    const uint32_t R = pos.empty() ? r.n() : (uint32_t)pos.size();
    std::vector<uint32_t> label(R);
    std::vector<double> score(R), all((size_t)R * K);
    for (uint32_t i = 0; i < R; ++i) {
        const uint32_t j = pos.empty() ? i : pos[i];
        if (j >= ndocs) {
            label[i] = NB_NO_CLASS;
            score[i] = 0.0;
            continue;
        }
        for (uint32_t c = 0; c < K; ++c) {
            double s = prior[c];
            for (uint64_t p = r.off[j]; p < r.off[j + 1]; ++p) {
                const double x = binary ? 1.0 : (double)r.cnt[p];
                const double prod = x * W[(size_t)r.term[p] * K + c];
                s = s + prod;
            }
            all[(size_t)i * K + c] = s;
            if (c == 0 || s > score[i]) { score[i] = s; label[i] = c; }
        }
    }
    if (want_label)
        for (uint32_t i = 0; i < R; ++i)
            if (label[i] != (*want_label)[i]) { printf("harness bug: %s row %u is built for class %u, the loop says %u\n", what, i, (*want_label)[i], label[i]); exit(1); }
    NbPredictArgs a{};
    uint64_t* d_off = up(r.off);
    uint32_t* d_term = up(r.term);
    uint32_t* d_cnt = up(r.cnt);
    uint32_t* d_pos = up(pos);
    double* d_W = up(W);
    double* d_prior = up(prior);
    uint32_t* d_label = up(std::vector<uint32_t>(R, 0xABABABABu));
    double* d_score = up(std::vector<double>(R, -1.0));
    double* d_all = up(std::vector<double>((size_t)R * K, -1.0));
    a.off = d_off; a.term = d_term; a.cnt = d_cnt;
    a.npairs = r.term.size();
    a.ndocs = ndocs;
    a.pos = pos.empty() ? nullptr : d_pos;
    a.nrows = R; a.V = V; a.K = K;
    a.binary = binary;
    a.W = d_W; a.prior = d_prior;
    a.label = d_label; a.score = d_score; a.all = d_all;
    if (launch_nb_predict(a, g_ncu, g_s)) { printf("%s: the launch failed\n", what); exit(2); }
    CK(hipStreamSynchronize(g_s));
    const auto gl = down(d_label, R);
    const auto gs = down(d_score, R);
    const auto ga = down(d_all, (size_t)R * K);
    for (uint32_t i = 0; i < R; ++i) {
        if (gl[i] != label[i]) fail(what, "label", i);
        if (bits(gs[i]) != bits(score[i])) fail(what, "score", i);
    }
    for (size_t i = 0; i < ga.size(); ++i) if (bits(ga[i]) != bits(all[i])) fail(what, "scores", i);
    a.all = nullptr;   /* the same without the score matrix */
    CK(hipMemset(d_label, 0xCD, (size_t)R * 4));
    if (launch_nb_predict(a, g_ncu, g_s)) { printf("%s: the launch failed\n", what); exit(2); }
    CK(hipStreamSynchronize(g_s));
    const auto gl2 = down(d_label, R);
    for (uint32_t i = 0; i < R; ++i) if (gl2[i] != label[i]) fail(what, "label without scores", i);
    CK(hipFree(d_off)); CK(hipFree(d_term)); CK(hipFree(d_cnt)); CK(hipFree(d_pos)); CK(hipFree(d_W));
    CK(hipFree(d_prior)); CK(hipFree(d_label)); CK(hipFree(d_score)); CK(hipFree(d_all));
    printf("ok  %s\n", what);
}

static void predict_group() {
    {   /* ties: classes 3 and 5 hold the same column and the best score; 3 wins.  K = 8 */
        const uint32_t V = 4, K = 8;
        std::vector<double> W((size_t)V * K), prior(K, -0.5);
        for (uint32_t t = 0; t < V; ++t)
            for (uint32_t c = 0; c < K; ++c) W[(size_t)t * K + c] = c == 3 || c == 5 ? -0.25 * (t + 1) : -1.0 - 0.125 * (t + c);
        Rows r;
        r.add({0, 1, 3}, {2, 1, 5});
        r.add({2}, {1});
        r.add({}, {});   /* every class scores the prior: class 0 */
        const std::vector<uint32_t> want = {3, 3, 0};
        predict_case("predict an exact tie: the lowest class wins", r, {}, r.n(), W, prior, V, K, false, &want);
    }
    {   /* signs: class 1 scores negative (the largest bit pattern), class 2 positive and wins; then all negative */
        const uint32_t V = 2, K = 3;
        const std::vector<double> W = {/* t0 */ -3.0, -7.0, 0.5, /* t1 */ -2.0, -1.5, -1.0};
        const std::vector<double> prior = {0.0, 0.0, 0.0};
        Rows r;
        r.add({0}, {4});        /* -12, -28, +2: class 2 */
        r.add({1}, {3});        /* -6, -4.5, -3: class 2, the smallest magnitude */
        r.add({0, 1}, {1, 9});  /* -21, -20.5, -8.5: class 2 */
        r.add({0, 1}, {2, 1});  /* -8, -15.5, 0.0: class 2 with exactly +0.0 above the negatives */
        const std::vector<uint32_t> want = {2, 2, 2, 2};
        predict_case("predict a positive winner beside negative scores, and all negative", r, {}, r.n(), W, prior, V, K, false, &want);
    }
    for (uint32_t slot = 0; slot < 4; ++slot) {   /* K = 256: the winner in accumulator `slot` of lane 17 */
        const uint32_t V = 70, K = 256, win = 64u * slot + 17u;
        std::vector<double> W((size_t)V * K), prior(K);
        for (uint32_t c = 0; c < K; ++c) prior[c] = -0.001 * (double)(c % 13);
        for (uint32_t t = 0; t < V; ++t)
            for (uint32_t c = 0; c < K; ++c) W[(size_t)t * K + c] = c == win ? -1.0 : -1.0 - 0.01 * (double)(1 + (t * 31 + c * 7) % 97);
        Rows r;
        std::vector<uint32_t> want;
        for (uint32_t n : {1u, 3u, 63u, 64u, 65u, 66u, 67u}) {
            std::vector<uint32_t> t, c;
            for (uint32_t i = 0; i < n; ++i) { t.push_back(i); c.push_back(1 + i % 4); }
            r.add(t, c);
            want.push_back(win);
        }
        char what[96];
        snprintf(what, sizeof what, "predict K=256 the winner in accumulator %u", slot);
        predict_case(what, r, {}, r.n(), W, prior, V, K, false, &want);
    }
    for (uint32_t K : {1u, 2u, 64u, 65u, 128u, 129u, 192u, 193u}) {   /* both sides of every accumulator boundary, many rows, a position list */
        const uint32_t V = 257, N = 700;
        std::vector<double> W((size_t)V * K), prior(K);
        uint32_t x = 99u + K;
        for (auto& w : W) { x = x * 1664525u + 1013904223u; w = -((double)(x >> 8) / 1048576.0) - 0.125; }
        for (auto& p : prior) { x = x * 1664525u + 1013904223u; p = -((double)(x >> 12) / 65536.0); }
        Rows r;
        for (uint32_t j = 0; j < N; ++j) {
            std::vector<uint32_t> t, c;
            const uint32_t n = j % 11 == 5 ? 0u : (j == 13 ? 200u : 1u + (j * 29u) % 90u);
            uint32_t at = j % 50u;
            for (uint32_t i = 0; i < n && at < V; ++i) {
                x = x * 1664525u + 1013904223u;
                t.push_back(at);
                c.push_back(1u + (x >> 27));
                at += 1u + (x >> 9) % 2u;
            }
            r.add(t, c);
        }
        std::vector<uint32_t> pos;
        for (uint32_t i = 0; i < 900; ++i) pos.push_back(i % 97 == 0 ? 0xFFFFFFFFu : (i * 389u) % N);
        char what[96];
        snprintf(what, sizeof what, "predict 700 rows K=%u", K);
        predict_case(what, r, {}, N, W, prior, V, K, false, nullptr);
        snprintf(what, sizeof what, "predict 900 listed rows K=%u binary, some not held", K);
        predict_case(what, r, pos, N, W, prior, V, K, true, nullptr);
    }
}

int main(int argc, char** argv) {
    const char* group = argc > 1 ? argv[1] : "all";
    CK(hipSetDevice(0));
    CK(hipStreamCreate(&g_s));
    int ncu = 0;
    CK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0));
    g_ncu = argc > 2 ? (uint32_t)atoi(argv[2]) : (uint32_t)ncu;   /* a second argument: the CU count the grids take */
    if (!strcmp(group, "count") || !strcmp(group, "all")) count_group();
    if (!strcmp(group, "predict") || !strcmp(group, "all")) predict_group();
    CK(hipStreamDestroy(g_s));
    printf("ALL OK\n");
    return 0;
}
