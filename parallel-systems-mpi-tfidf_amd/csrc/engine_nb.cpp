/*
 * engine_nb.cpp — tfidf_nb_fit, tfidf_nb_predict, tfidf_nb_predict_rows, tfidf_nb_export (nb.hip).
 * The context and the helpers every engine file shares: engine_ctx.h.
 */
#include "engine_ctx.h"

#include <math.h>

#include <algorithm>

/* ---------------------------------------------------------------- classify ----
 * Naive Bayes over the resident result (nb.hip).  The fit: the labelled ids become output
 * positions by the keyword path's lookup, the host turns them into one class word per position
 * (an id the context does not hold refuses the call there), and the device counts, reduces and
 * reports the largest log argument.  The host then takes every logarithm: a table over the
 * arguments 0..min(max, NB_LUT_MAX), the sorted distinct arguments beyond it, and one per class;
 * the device does the one subtraction per entry.  A predict call is one kernel per batch of rows
 * over the resident pairs or over uploaded rows.  Nothing of the run's result is written. */

namespace {

constexpr uint64_t NB_OUT_BYTES = 64ull << 20;   /* a predict batch's labels and scores on the device */

/* the words of nb_work behind F: T, lc, prior (K each), misc (3 used of 4), then the labels by position */
struct NbWork {
    uint64_t* F;
    uint64_t* T;
    double* lc;
    double* prior;
    uint64_t* misc;
    uint32_t* lab;
};
NbWork nb_work(tfidf_ctx* ctx, uint32_t V, uint32_t K) {
    NbWork w;
    w.F = ctx->nb_work.as<uint64_t>();
    w.T = w.F + V;
    w.lc = (double*)(w.T + K);
    w.prior = w.lc + K;
    w.misc = (uint64_t*)(w.prior + K);
    w.lab = (uint32_t*)(w.misc + 4);
    return w;
}
uint64_t nb_work_bytes(uint32_t N, uint32_t V, uint32_t K) { return (uint64_t)V * 8 + (uint64_t)K * 24 + 32 + (uint64_t)N * 4 + 64; }

struct LabelsGuard {   /* an error return leaves *out zeroed */
    tfidf_nb_labels* l;
    ~LabelsGuard() { if (l) tfidf_nb_labels_free(l); }
};

int labels_alloc(tfidf_nb_labels* out, uint32_t R, uint32_t K, bool all) {
    out->ndocs = R;
    out->nclasses = K;
    out->doc = (uint32_t*)calloc((size_t)R + 1, 4);
    out->pos = (uint32_t*)calloc((size_t)R + 1, 4);
    out->label = (uint32_t*)calloc((size_t)R + 1, 4);
    out->score = (double*)calloc((size_t)R + 1, 8);
    if (all) out->scores = (double*)calloc((size_t)R * K + 1, 8);
    return out->doc && out->pos && out->label && out->score && (!all || out->scores) ? TFIDF_OK : TFIDF_E_NOMEM;
}

/* the rows of `a` (off, term, cnt, npairs, ndocs, pos set by the caller) in batches into out */
int predict_batches(tfidf_ctx* ctx, NbPredictArgs a, uint32_t R, bool all, tfidf_nb_labels* out) {
    hipStream_t s = ctx->stream;
    const uint32_t K = ctx->nb_K;
    const uint64_t per_row = 12 + (all ? (uint64_t)K * 8 : 0);
    uint64_t B = NB_OUT_BYTES / per_row;
    B = B < 1 ? 1 : (B > R ? R : B);
    ENSURE(ctx->nb_out, (size_t)B * per_row + 64);
    a.V = ctx->nb_V;
    a.K = K;
    a.binary = ctx->nb_feature == TFIDF_NB_BINARY;
    a.W = ctx->nb_W.as<double>();
    a.prior = ctx->nb_prior_dev;
    a.score = ctx->nb_out.as<double>();
    a.all = all ? a.score + B : nullptr;
    a.label = (uint32_t*)(a.score + B + (all ? B * K : 0));
    const uint64_t* off0 = a.off;
    const uint32_t* pos0 = a.pos;
    const uint32_t nd0 = a.ndocs;
    double ms = 0;
    for (uint64_t r0 = 0; r0 < R; r0 += B) {
        const uint32_t nb = (uint32_t)(R - r0 < B ? R - r0 : B);
        a.nrows = nb;
        if (pos0) {
            a.pos = pos0 + r0;
        } else {   /* row r is position r0 + r: the offsets from r0 on */
            a.off = off0 + r0;
            a.ndocs = nd0 - (uint32_t)r0;
        }
        HIPCHK(hipEventRecord(ctx->ev_nb[0], s));
        LAUNCH(launch_nb_predict(a, ctx->ncu, s));
        HIPCHK(hipEventRecord(ctx->ev_nb[1], s));
        HIPCHK(hipMemcpyAsync(out->label + r0, a.label, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->score + r0, a.score, (size_t)nb * 8, hipMemcpyDeviceToHost, s));
        if (all) HIPCHK(hipMemcpyAsync(out->scores + r0 * K, a.all, (size_t)nb * K * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        ms += ev_ms(ctx->ev_nb[0], ctx->ev_nb[1]);
    }
    ctx->nbinfo.predict_rows = R;
    ctx->nbinfo.ms_predict = ms;
    return TFIDF_OK;
}

}  // namespace

extern "C" int tfidf_nb_fit(tfidf_ctx* ctx, const tfidf_nb_params* params) {
    if (!ctx) return TFIDF_E_INVAL;
    if (const int rc = tfidf_nb_check(params)) return rc;
    if (!ctx->have_result || ctx->model_only) return TFIDF_E_STATE;
    const uint32_t N = ctx->ndocs, V = ctx->V, K = params->nclasses;
    const uint64_t n = params->nlabelled, KV = (uint64_t)K * V;
    const uint64_t matrix = KV * 16, work = nb_work_bytes(N, V, K);
    if (matrix + work > ctx->nb_bytes) return TFIDF_E_CAPACITY;
    const auto wall0 = std::chrono::steady_clock::now();
    ctx->nb_valid = false;
    if (const int rc = call_begin(ctx, ctx->ev_nb)) return rc;
    hipStream_t s = ctx->stream;
    const bool comp = params->variant == TFIDF_NB_COMPLEMENT;
    const double alpha = params->alpha == 0.0 ? 1.0 : params->alpha;
    tfidf_nb_info ni{};
    ni.nclasses = K;
    ni.nterms = V;
    ni.nlabelled = n;
    ni.matrix_bytes = matrix;

    /* ---- labelled ids -> output positions -> a class word per position ---- */
    std::vector<uint32_t> h_pos((size_t)n + 1), h_lab((size_t)N + 1, NB_NO_CLASS);
    if (const int rc = lookup_ids(ctx, ctx->nb_ids, params->doc, (uint32_t)n, nullptr)) return rc;
    HIPCHK(hipMemcpyAsync(h_pos.data(), ctx->nb_ids.as<uint32_t>() + n, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ctx->nb_class_docs.assign(K, 0);
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t j = h_pos[i];
        if (j >= N || h_lab[j] != NB_NO_CLASS) return TFIDF_E_INVAL;   /* not held, or two entries of one document */
        h_lab[j] = params->label[i];
        ctx->nb_class_docs[params->label[i]] += 1u;
    }

    ENSURE(ctx->nb_FC, (size_t)KV * 8 + 64);
    ENSURE(ctx->nb_W, (size_t)KV * 8 + 64);
    ENSURE(ctx->nb_work, work);
    const NbWork w = nb_work(ctx, V, K);
    NbFitArgs a{};
    a.off = ctx->out_off.as<uint64_t>();
    a.term = ctx->out_term.as<uint32_t>();
    a.cnt = ctx->out_cnt.as<uint32_t>();
    a.npairs = ctx->npairs;
    a.ndocs = N;
    a.V = V;
    a.K = K;
    a.complement = comp;
    a.binary = params->feature == TFIDF_NB_BINARY;
    a.lab = w.lab;
    a.FC = ctx->nb_FC.as<uint64_t>();
    a.F = w.F;
    a.T = w.T;
    a.misc = w.misc;
    a.lc = w.lc;
    a.W = ctx->nb_W.as<double>();
    a.lut_n = (uint64_t)NB_LUT_MAX + 1;   /* what the table can hold: the arguments from here on are counted */

    /* ---- count, reduce, the arguments' maximum ---- */
    if (N) HIPCHK(hipMemcpyAsync(w.lab, h_lab.data(), (size_t)N * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(ctx->ev_nb[0], s));
    LAUNCH(launch_nb_count(a, ctx->ncu, s));
    LAUNCH(launch_nb_sums(a, ctx->ncu, s));
    LAUNCH(launch_nb_argmax(a, ctx->ncu, s));
    HIPCHK(hipEventRecord(ctx->ev_nb[1], s));
    std::vector<uint64_t> h_T(K);
    uint64_t h_misc[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h_T.data(), w.T, (size_t)K * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_misc, w.misc, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    ni.ms_count = ev_ms(ctx->ev_nb[0], ctx->ev_nb[1]);

    /* ---- the list of the arguments past the table ---- */
    const uint64_t amax = h_misc[0], past = h_misc[1];
    const uint64_t lut_n = (amax < NB_LUT_MAX ? amax : NB_LUT_MAX) + 1;
    std::vector<uint64_t> keys;
    if (past) {
        ENSURE(ctx->nb_list, (size_t)past * 16 + 64);   /* the raw list, then keys and values in its place */
        a.list = ctx->nb_list.as<uint64_t>();
        a.list_cap = past;
        LAUNCH(launch_nb_list(a, ctx->ncu, s));
        keys.resize((size_t)past);
        HIPCHK(hipMemcpyAsync(keys.data(), a.list, (size_t)past * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        std::sort(keys.begin(), keys.end());
        keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    }

    /* ---- every logarithm, on the host ---- */
    const auto logs0 = std::chrono::steady_clock::now();
    std::vector<double> lut((size_t)lut_n), vals(keys.size()), lc(K), prior(K);
    for (uint64_t m = 0; m < lut_n; ++m) {
        const double x = (double)m + alpha;
        lut[(size_t)m] = log(x);
    }
    for (size_t i = 0; i < keys.size(); ++i) {
        const double x = (double)keys[i] + alpha;
        vals[i] = log(x);
    }
    uint64_t Ttot = 0;
    for (uint32_t c = 0; c < K; ++c) Ttot += h_T[c];
    const double aV = alpha * (double)V;
    ni.nlogs = lut_n + keys.size() + K;
    const double ln_n = comp || params->uniform_prior ? 0.0 : log((double)n);
    for (uint32_t c = 0; c < K; ++c) {
        const double x = (double)(comp ? Ttot - h_T[c] : h_T[c]) + aV;
        lc[c] = log(x);
        if (comp || params->uniform_prior) {
            prior[c] = 0.0;
        } else {
            const double ln_c = log((double)ctx->nb_class_docs[c]);
            prior[c] = ln_c - ln_n;
        }
    }
    if (!comp && !params->uniform_prior) ni.nlogs += (uint64_t)K + 1;
    ni.nlisted = keys.size();
    ni.ms_logs_host = wall_ms(logs0);

    /* ---- the tables up, one subtraction per entry ---- */
    ENSURE(ctx->nb_lut, (size_t)lut_n * 8 + 64);
    HIPCHK(hipMemcpyAsync(ctx->nb_lut.p, lut.data(), (size_t)lut_n * 8, hipMemcpyHostToDevice, s));
    if (!keys.empty()) {
        uint64_t* d_key = ctx->nb_list.as<uint64_t>();
        double* d_val = (double*)(d_key + past);
        HIPCHK(hipMemcpyAsync(d_key, keys.data(), keys.size() * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_val, vals.data(), vals.size() * 8, hipMemcpyHostToDevice, s));
        a.list_key = d_key;
        a.list_val = d_val;
        a.list_n = keys.size();
    }
    HIPCHK(hipMemcpyAsync(w.lc, lc.data(), (size_t)K * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(w.prior, prior.data(), (size_t)K * 8, hipMemcpyHostToDevice, s));
    a.lut = ctx->nb_lut.as<double>();
    a.lut_n = lut_n;
    HIPCHK(hipEventRecord(ctx->ev_nb[2], s));
    LAUNCH(launch_nb_weights(a, ctx->ncu, s));
    HIPCHK(hipEventRecord(ctx->ev_nb[3], s));
    HIPCHK(hipStreamSynchronize(s));   /* the host tables are on this frame */
    ni.ms_weights = ev_ms(ctx->ev_nb[2], ctx->ev_nb[3]);

    ctx->nb_K = K;
    ctx->nb_V = V;
    ctx->nb_variant = params->variant;
    ctx->nb_feature = params->feature;
    ctx->nb_uniform = params->uniform_prior ? 1u : 0u;
    ctx->nb_alpha = alpha;
    ctx->nb_n = n;
    ctx->nb_prior_dev = w.prior;
    ctx->nb_T_dev = w.T;
    ctx->nb_valid = true;
    ni.ms_total = wall_ms(wall0);
    ctx->nbinfo = ni;
    return TFIDF_OK;
}

extern "C" int tfidf_nb_predict(tfidf_ctx* ctx, const uint32_t* doc_ids, uint32_t ndocs, uint32_t flags, tfidf_nb_labels* out) {
    if (!ctx || !out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (flags & ~TFIDF_NB_ALL_SCORES) return TFIDF_E_INVAL;
    if (!ctx->nb_valid || !ctx->have_result) return TFIDF_E_STATE;
    if (const int rc = call_begin(ctx, ctx->ev_nb)) return rc;
    hipStream_t s = ctx->stream;
    const uint32_t N = ctx->ndocs, R = doc_ids ? ndocs : N;
    const bool all = (flags & TFIDF_NB_ALL_SCORES) != 0;
    LabelsGuard guard{out};
    if (const int rc = labels_alloc(out, R, ctx->nb_K, all)) return rc;
    NbPredictArgs a{};
    a.off = ctx->out_off.as<uint64_t>();
    a.term = ctx->out_term.as<uint32_t>();
    a.cnt = ctx->out_cnt.as<uint32_t>();
    a.npairs = ctx->npairs;
    a.ndocs = N;
    ENSURE(ctx->nb_ids, (size_t)R * 8 + 8);
    uint32_t* d_ids = ctx->nb_ids.as<uint32_t>();
    if (doc_ids && R) {
        if (const int rc = lookup_ids(ctx, ctx->nb_ids, doc_ids, R, nullptr)) return rc;   /* the same size: d_ids stays */
        HIPCHK(hipMemcpyAsync(out->pos, d_ids + R, (size_t)R * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        memcpy(out->doc, doc_ids, (size_t)R * 4);
        a.pos = d_ids + R;
    } else if (R) {
        LAUNCH(launch_km_docs(ctx->order, ctx->dev_ids, N, d_ids, s));
        HIPCHK(hipMemcpyAsync(out->doc, d_ids, (size_t)R * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (uint32_t r = 0; r < R; ++r) out->pos[r] = r;
    }
    if (const int rc = predict_batches(ctx, a, R, all, out)) return rc;
    guard.l = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_nb_predict_rows(tfidf_ctx* ctx, const tfidf_rows* rows, uint32_t flags, tfidf_nb_labels* out) {
    if (!ctx || !out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!rows || (flags & ~TFIDF_NB_ALL_SCORES)) return TFIDF_E_INVAL;
    if (!ctx->nb_valid) return TFIDF_E_STATE;
    const uint32_t R = rows->ndocs;
    const uint64_t P = rows->npairs;
    if (R && !rows->row_off) return TFIDF_E_INVAL;
    if (P && (!rows->term || !rows->count || !R)) return TFIDF_E_INVAL;
    if (R && (rows->row_off[0] != 0 || rows->row_off[R] != P)) return TFIDF_E_INVAL;
    for (uint32_t r = 0; r < R; ++r)
        if (rows->row_off[r + 1] < rows->row_off[r]) return TFIDF_E_INVAL;
    for (uint64_t q = 0; q < P; ++q)
        if (rows->term[q] >= ctx->nb_V) return TFIDF_E_INVAL;   /* a merged group transform carries UINT32_MAX */
    if (const int rc = call_begin(ctx, ctx->ev_nb)) return rc;
    hipStream_t s = ctx->stream;
    const bool all = (flags & TFIDF_NB_ALL_SCORES) != 0;
    LabelsGuard guard{out};
    if (const int rc = labels_alloc(out, R, ctx->nb_K, all)) return rc;
    for (uint32_t r = 0; r < R; ++r) out->doc[r] = out->pos[r] = r;
    const size_t o_term = al256(((size_t)R + 1) * 8), o_cnt = o_term + al256((size_t)P * 4 + 4);
    ENSURE(ctx->nb_rows, o_cnt + (size_t)P * 4 + 64);
    uint8_t* base = ctx->nb_rows.as<uint8_t>();
    NbPredictArgs a{};
    a.off = (const uint64_t*)base;
    a.term = (const uint32_t*)(base + o_term);
    a.cnt = (const uint32_t*)(base + o_cnt);
    a.npairs = P;
    a.ndocs = R;
    if (R) HIPCHK(hipMemcpyAsync(base, rows->row_off, ((size_t)R + 1) * 8, hipMemcpyHostToDevice, s));
    if (P) {
        HIPCHK(hipMemcpyAsync(base + o_term, rows->term, (size_t)P * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(base + o_cnt, rows->count, (size_t)P * 4, hipMemcpyHostToDevice, s));
    }
    if (const int rc = predict_batches(ctx, a, R, all, out)) return rc;
    guard.l = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_nb_export(tfidf_ctx* ctx, tfidf_nb_model* out) {
    if (!ctx || !out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!ctx->nb_valid) return TFIDF_E_STATE;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint32_t K = ctx->nb_K, V = ctx->nb_V;
    const size_t KV = (size_t)K * V;
    struct ModelGuard {
        tfidf_nb_model* m;
        ~ModelGuard() { if (m) tfidf_nb_model_free(m); }
    } guard{out};
    out->class_docs = (uint64_t*)calloc((size_t)K + 1, 8);
    out->class_total = (uint64_t*)calloc((size_t)K + 1, 8);
    out->feature_count = (uint64_t*)calloc(KV + 1, 8);
    out->prior = (double*)calloc((size_t)K + 1, 8);
    out->weight = (double*)calloc(KV + 1, 8);
    if (!out->class_docs || !out->class_total || !out->feature_count || !out->prior || !out->weight) return TFIDF_E_NOMEM;
    memcpy(out->class_docs, ctx->nb_class_docs.data(), (size_t)K * 8);
    HIPCHK(hipMemcpyAsync(out->class_total, ctx->nb_T_dev, (size_t)K * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out->prior, ctx->nb_prior_dev, (size_t)K * 8, hipMemcpyDeviceToHost, s));
    if (KV) {
        HIPCHK(hipMemcpyAsync(out->feature_count, ctx->nb_FC.p, KV * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->weight, ctx->nb_W.p, KV * 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    out->size = sizeof(*out);
    out->nclasses = K;
    out->nterms = V;
    out->variant = ctx->nb_variant;
    out->feature = ctx->nb_feature;
    out->uniform_prior = ctx->nb_uniform;
    out->alpha = ctx->nb_alpha;
    out->nlabelled = ctx->nb_n;
    guard.m = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_last_nb_info(const tfidf_ctx* ctx, tfidf_nb_info* info) {
    return ctx ? copy_info(info, ctx->nbinfo) : TFIDF_E_INVAL;
}
