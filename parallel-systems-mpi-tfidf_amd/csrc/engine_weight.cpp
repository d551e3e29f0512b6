/*
 * engine_weight.cpp — tfidf_reweight and the weighting helpers tfidf_transform shares (reweight.hip).
 * The context and the helpers every engine file shares: engine_ctx.h.
 */
#include <algorithm>

#include "engine_ctx.h"

/* --------------------------------------------------------------- weighting ----
 * Weighting schemes over the resident result (reweight.hip; the check, the formulas of the
 * tables and the host form are weight_host.c).  Tables (the scheme's idf in the layout of
 * idf_vals, the sublinear tf table, the idf by rank), then the pair pass into prune's spare
 * score buffer, which changes places with out_score when every step has succeeded.  idf_vals is
 * never written: the reference scheme reads it again. */

/* The scheme's idf for every df the run's table covers, in that table's layout, on the
 * context's workers; kept until the next run or import (a prune leaves the index a superset). */
static int rw_idf_table(tfidf_ctx* ctx, uint32_t mode, uint64_t* nlogs) {
    if (mode == TFIDF_IDF_REF || mode == TFIDF_IDF_NONE || ctx->rw_idf_mode == mode) return TFIDF_OK;
    const uint64_t Nt = ctx->ndocs_total;
    if (!ctx->V || !Nt) return TFIDF_OK;
    hipStream_t s = ctx->stream;
    if (const int q = idf_pin_quiesce(ctx)) return q;
    const double keep_host = ctx->ms_idf_host, keep_wait = ctx->ms_idf_wait;   /* the run's, in tfidf_last_run_info */
    std::vector<uint32_t> vals;
    uint64_t n = Nt + 1;   /* entries of the table */
    if (Nt > IDF_FULL_MAX) {   /* the distinct df values through the run's index, listed again */
        if (arena_scratch(ctx, (size_t)(Nt + 2) * 4 + 8192)) return TFIDF_E_NOMEM;
        uint32_t* vals_dev = (uint32_t*)ctx->arena.get((size_t)(Nt + 2) * 4);
        if (!vals_dev) return TFIDF_E_NOMEM;
        uint32_t* present = ctx->present.as<uint32_t>();
        if (!present || ctx->present.cap < (Nt + 2) * 4) return TFIDF_E_STATE;
        LAUNCH(launch_df_list(present, Nt + 1, vals_dev, s));
        uint32_t K = 0;
        HIPCHK(hipMemcpyAsync(&K, present + Nt + 1, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (K == 0 || (uint64_t)K > Nt + 1) return TFIDF_E_STATE;
        vals.resize(K);
        HIPCHK(hipMemcpyAsync(vals.data(), vals_dev, (size_t)K * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        n = K;
    }
    ENSURE(ctx->rw_idf, (size_t)n * 8 + 8);
    if (idf_pin_reserve(ctx, (size_t)n + 1)) return TFIDF_E_NOMEM;
    if (vals.empty()) {
        ctx->idf_pin[0] = 0.0;   /* df >= 1 for every term that occurs */
        idf_post(ctx, ctx->idf_pin, Nt, nullptr, Nt, mode);
        *nlogs += Nt;
    } else {
        idf_post(ctx, ctx->idf_pin, Nt, vals.data(), n, mode);
        *nlogs += n;
    }
    idf_join(ctx);
    ctx->ms_idf_host = keep_host;
    ctx->ms_idf_wait = keep_wait;
    HIPCHK(hipMemcpyAsync(ctx->rw_idf.p, ctx->idf_pin, (size_t)n * 8, hipMemcpyHostToDevice, s));
    ctx->idf_pin_busy = true;
    HIPCHK(hipStreamSynchronize(s));
    ctx->idf_pin_busy = false;
    ctx->rw_idf_mode = mode;
    return TFIDF_OK;
}

/* sublinear tf, first half: the largest of n counts (n_dev: the total still on the device) and
 * the list of those above RW_LUT_MAX, into rw_misc[RWM_CMAX..] and rw_list */
int rw_cmax_launch(tfidf_ctx* ctx, const uint32_t* count, uint64_t n, const uint32_t* n_dev) {
    ENSURE(ctx->rw_misc, 256);
    ENSURE(ctx->rw_list, (size_t)RW_LIST_MAX * 4);
    ENSURE(ctx->rw_lut, ((size_t)RW_LUT_MAX + 1) * 8);
    uint32_t* misc = ctx->rw_misc.as<uint32_t>();
    HIPCHK(hipMemsetAsync(misc + RWM_CMAX, 0, 8, ctx->stream));
    LAUNCH(launch_rw_cmax(count, n, n_dev, misc + RWM_CMAX, ctx->rw_list.as<uint32_t>(), RW_LIST_MAX, ctx->stream));
    return TFIDF_OK;
}
/* second half, with the two words on the host: the table fl(1 + log c) up to min(cmax,
 * RW_LUT_MAX) (grown, never rebuilt: its values do not depend on the run) and the listed
 * counts, sorted and distinct, with their values.  Synchronises the stream. */
int rw_tf_finish(tfidf_ctx* ctx, uint32_t cmax, uint32_t nlist, uint32_t* nlisted, uint64_t* nlogs) {
    hipStream_t s = ctx->stream;
    *nlisted = 0;
    if (nlist > RW_LIST_MAX) return TFIDF_E_CAPACITY;   /* the list is bounded; nothing has been scored */
    const uint32_t need = cmax < RW_LUT_MAX ? cmax : RW_LUT_MAX;
    bool wait = false;
    if (need > ctx->rw_lut_n || ctx->rw_lut_host.empty()) {
        if (ctx->rw_lut_host.empty()) ctx->rw_lut_host.assign((size_t)RW_LUT_MAX + 1, 0.0);
        const uint32_t first = ctx->rw_lut_n + 1u;
        for (uint32_t c = first; c <= need; ++c) ctx->rw_lut_host[c] = tfidf_weight_tf_log(c);
        const uint32_t from = ctx->rw_lut_n ? first : 0u;
        if (need + 1u > from) {
            HIPCHK(hipMemcpyAsync(ctx->rw_lut.as<double>() + from, ctx->rw_lut_host.data() + from, (size_t)(need + 1u - from) * 8,
                                  hipMemcpyHostToDevice, s));
            wait = true;
        }
        if (need >= first) *nlogs += need - first + 1u;
    }
    if (nlist) {
        std::vector<uint32_t>& lc = ctx->rw_list_host;
        lc.resize(nlist);
        HIPCHK(hipMemcpyAsync(lc.data(), ctx->rw_list.p, (size_t)nlist * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        std::sort(lc.begin(), lc.end());
        lc.erase(std::unique(lc.begin(), lc.end()), lc.end());
        std::vector<double>& lv = ctx->rw_listv_host;
        lv.resize(lc.size());
        for (size_t i = 0; i < lc.size(); ++i) lv[i] = tfidf_weight_tf_log(lc[i]);
        ENSURE(ctx->rw_listv, lc.size() * 8 + 8);
        HIPCHK(hipMemcpyAsync(ctx->rw_list.p, lc.data(), lc.size() * 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(ctx->rw_listv.p, lv.data(), lv.size() * 8, hipMemcpyHostToDevice, s));
        *nlisted = (uint32_t)lc.size();
        *nlogs += lc.size();
        wait = true;
    }
    if (wait) HIPCHK(hipStreamSynchronize(s));   /* the uploads read pageable host memory of the context */
    if (need > ctx->rw_lut_n) ctx->rw_lut_n = need;
    return TFIDF_OK;
}

/* the scheme-dependent members of a pair pass's arguments */
void rw_scheme_args(tfidf_ctx* ctx, RwArgs& a, uint32_t tf, uint32_t norm, uint32_t nlisted) {
    a.tf_mode = tf;
    a.norm = norm;
    a.tf_lut = ctx->rw_lut.as<double>();
    a.lut_n = ctx->rw_lut_n;
    a.nlisted = nlisted;
    a.listed_c = ctx->rw_list.as<uint32_t>();
    a.listed_v = ctx->rw_listv.as<double>();
    a.big_list = ctx->rw_big.as<uint32_t>();
    a.misc = ctx->rw_misc.as<uint32_t>();
}

extern "C" int tfidf_reweight(tfidf_ctx* ctx, const tfidf_weighting* w) {
    if (!ctx || tfidf_weighting_check(w) != TFIDF_OK) return TFIDF_E_INVAL;
    if (!ctx->have_result && !ctx->have_model) return TFIDF_E_STATE;
    if (tfidf_weighting_check_n(w, ctx->ndocs_total) != TFIDF_OK) return TFIDF_E_INVAL;
    const auto wall0 = std::chrono::steady_clock::now();
    if (const int rc = call_begin(ctx, ctx->ev_rw)) return rc;
    hipStream_t s = ctx->stream;
    const bool pairs = ctx->have_result && !ctx->model_only;
    const uint32_t V = ctx->V, N = pairs ? ctx->ndocs : 0u;
    const uint64_t P = pairs ? ctx->npairs : 0u, Nt = ctx->ndocs_total;
    tfidf_reweight_info ri{};
    ri.tf = w->tf;
    ri.idf = w->idf;
    ri.norm = w->norm;
    ri.npairs = P;
    ri.ndocs = N;
    if (w->tf == ctx->wt_tf && w->idf == ctx->wt_idf && w->norm == ctx->wt_norm) {   /* active already: no byte changes */
        ri.ms_total = wall_ms(wall0);
        ctx->rwinfo = ri;
        return TFIDF_OK;
    }
    ri.changed = 1;
    HIPCHK(hipEventRecord(ctx->ev_rw[0], s));
    if (const int rc = rw_idf_table(ctx, w->idf, &ri.nlogs)) return rc;
    if (P && N) {
        if (ensure_spare(ctx->pr_score, ctx->out_score, (size_t)P * 8 + 8)) return TFIDF_E_NOMEM;
        ENSURE(ctx->rw_misc, 256);
        ENSURE(ctx->rw_big, (size_t)N * 4 + 4);
        uint32_t nlisted = 0;
        if (w->tf == TFIDF_TF_LOG) {
            if (const int rc = rw_cmax_launch(ctx, ctx->out_cnt.as<uint32_t>(), P, nullptr)) return rc;
            uint32_t cw[2] = {0, 0};
            HIPCHK(hipMemcpyAsync(cw, ctx->rw_misc.as<uint32_t>() + RWM_CMAX, 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (const int rc = rw_tf_finish(ctx, cw[0], cw[1], &nlisted, &ri.nlogs)) return rc;
            ri.max_count = cw[0];
            ri.listed_counts = nlisted;
        }
        RwArgs a{};
        a.off = ctx->out_off.as<uint64_t>();
        a.npairs = P;
        a.ndocs = N;
        a.order = ctx->order;
        a.doc_size = ctx->doc_size.as<uint32_t>();
        a.count = ctx->out_cnt.as<uint32_t>();
        a.key = ctx->out_term.as<uint32_t>();
        a.key_n = V;
        if (w->idf != TFIDF_IDF_NONE) {   /* the idf by rank: one 8-byte gather per pair in the pair pass */
            ENSURE(ctx->idf_rank, (size_t)V * 8 + 8);
            const double* tab = w->idf == TFIDF_IDF_REF ? ctx->idf_vals.as<double>() : ctx->rw_idf.as<double>();
            const uint32_t* idx = Nt <= IDF_FULL_MAX ? nullptr : ctx->present.as<uint32_t>();
            LAUNCH(launch_rw_idf_rank(df_of_run(ctx), V, tab, idx, Nt + 1, ctx->idf_rank.as<double>(), s));
            a.idf = ctx->idf_rank.as<double>();
        }
        a.score = ctx->pr_score.as<double>();
        rw_scheme_args(ctx, a, w->tf, w->norm, nlisted);
        HIPCHK(hipEventRecord(ctx->ev_rw[1], s));
        LAUNCH(launch_rw_pairs(a, ctx->ncu, s));
        HIPCHK(hipEventRecord(ctx->ev_rw[2], s));
        uint32_t mw[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(mw, ctx->rw_misc.as<uint32_t>() + RWM_BIG, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));   /* the spare is written: from here on the call cannot fail */
        std::swap(ctx->out_score, ctx->pr_score);
        result_changed(ctx, RC_SCORES);
        ri.big_docs = mw[0] < N ? mw[0] : N;
        ri.zero_norm_docs = mw[1];
        ri.ms_tables = ev_ms(ctx->ev_rw[0], ctx->ev_rw[1]);
        ri.ms_pairs = ev_ms(ctx->ev_rw[1], ctx->ev_rw[2]);
    }
    ctx->wt_tf = w->tf;
    ctx->wt_idf = w->idf;
    ctx->wt_norm = w->norm;
    ri.ms_total = wall_ms(wall0);
    ctx->rwinfo = ri;
    return TFIDF_OK;
}

extern "C" int tfidf_weighting_get(const tfidf_ctx* ctx, tfidf_weighting* out) {
    if (!ctx || !out || out->size < sizeof(tfidf_weighting)) return TFIDF_E_INVAL;
    out->tf = ctx->wt_tf;
    out->idf = ctx->wt_idf;
    out->norm = ctx->wt_norm;
    out->reserved = 0;
    return TFIDF_OK;
}

extern "C" int tfidf_last_reweight_info(const tfidf_ctx* ctx, tfidf_reweight_info* info) {
    return ctx ? copy_info(info, ctx->rwinfo) : TFIDF_E_INVAL;
}
