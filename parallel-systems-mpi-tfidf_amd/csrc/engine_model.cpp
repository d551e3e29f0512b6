/*
 * engine_model.cpp — tfidf_model_export, tfidf_model_import (model.hip).
 * The context and the helpers every engine file shares: engine_ctx.h.
 */
#include <math.h>

#include "engine_ctx.h"

/* ------------------------------------------------------------------- model ----
 * The model tfidf_transform reads, as an object (include/tfidf.h, model.hip; the host-only
 * check and file format are model_io.c).  Export gathers the term table on the device with the
 * keyword path's word gather (term metadata, a scan of the lengths, launch_terms_words over
 * every rank) and copies offsets, bytes and df.  Import builds what a run leaves behind from the
 * list: the slot table and rank_of_slot (launch_model_build), df by rank, the idf table in
 * run_post's two forms, V and N; the uploaded term bytes stand where the run's corpus does. */

namespace {
struct ModelGuard {   /* an error return leaves *out zeroed */
    tfidf_model* m;
    ~ModelGuard() { if (m) tfidf_model_free(m); }
};
}  // namespace

extern "C" int tfidf_model_export(tfidf_ctx* ctx, tfidf_model* out) {
    if (!ctx || !out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!ctx->have_model) return TFIDF_E_STATE;
    const auto wall0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint32_t V = ctx->V;
    ModelGuard guard{out};
    out->size = sizeof(tfidf_model);
    out->ndocs_total = ctx->ndocs_total;
    out->nterms = V;
    out->term_off = (uint64_t*)calloc((size_t)V + 1, 8);
    out->term_df = (uint32_t*)calloc((size_t)V + 1, 4);
    if (!out->term_off || !out->term_df) return TFIDF_E_NOMEM;
    const uint8_t* d_words = nullptr;
    if (ctx->model_only) {   /* the imported list is the table */
        if (V) HIPCHK(hipMemcpyAsync(out->term_off, ctx->m_off.p, ((size_t)V + 1) * 8, hipMemcpyDeviceToHost, s));
        d_words = ctx->m_blob.as<uint8_t>();
    } else if (V) {
        if (const int rc = ensure_term_meta(ctx)) return rc;
        ENSURE(ctx->tm_term, (size_t)V * 4 + 4);
        ENSURE(ctx->tm_woff, ((size_t)V + 1) * 8 + 16);
        uint64_t* d_woff = ctx->tm_woff.as<uint64_t>();
        LAUNCH(launch_model_lens(ctx->t_len.as<uint32_t>(), V, ctx->tm_term.as<uint32_t>(), d_woff, s));
        if (arena_scratch(ctx, scan_scratch(V) + 4096)) return TFIDF_E_NOMEM;
        SCAN(scan_excl_u64(d_woff, d_woff, V, ctx->arena, s));
        HIPCHK(hipMemcpyAsync(out->term_off, d_woff, ((size_t)V + 1) * 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    const uint64_t total = out->term_off[V];
    if (ctx->model_only && total != ctx->m_blob_bytes) return TFIDF_E_STATE;
    out->term_bytes = (uint8_t*)malloc((size_t)total + 1);
    if (!out->term_bytes) return TFIDF_E_NOMEM;
    if (!ctx->model_only && V) {
        ENSURE(ctx->tm_words, total + 16);
        TWordArgs wa{ctx->tm_term.as<uint32_t>(), ctx->tm_woff.as<uint64_t>(), V, ctx->t_key.as<uint4>(), V,
                     ctx->dev_bytes, ctx->corpus.nbytes, ctx->tm_words.as<uint8_t>()};
        LAUNCH(launch_terms_words(wa, s));
        d_words = ctx->tm_words.as<uint8_t>();
    }
    if (total) HIPCHK(hipMemcpyAsync(out->term_bytes, d_words, (size_t)total, hipMemcpyDeviceToHost, s));
    if (V) HIPCHK(hipMemcpyAsync(out->term_df, df_of_run(ctx), (size_t)V * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    tfidf_model_info mi{};
    mi.nterms = V;
    mi.table_slots = ctx->vcap;
    mi.blob_bytes = total;
    mi.ms_total = wall_ms(wall0);
    ctx->minfo = mi;
    guard.m = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_model_import(tfidf_ctx* ctx, const tfidf_model* m) {
    if (!ctx || !m) return TFIDF_E_INVAL;
    if (tfidf_model_check(m) != TFIDF_OK) return TFIDF_E_INVAL;
    const uint32_t V = m->nterms;
    const uint64_t Nt = m->ndocs_total;
    if (V && Nt > 0xFFFFFFFFull) return TFIDF_E_INVAL;   /* as tfidf_run: df and N are 32-bit */
    const auto wall0 = std::chrono::steady_clock::now();
    if (const int rc = call_begin(ctx, ctx->ev_m)) return rc;
    hipStream_t s = ctx->stream;
    const uint64_t base = V ? m->term_off[0] : 0, nbytes = V ? m->term_off[V] - base : 0;
    /* the table: the smallest size from the context's current one on that keeps V under the
     * run's load limits (run_local), chosen before anything is inserted */
    uint64_t cap = ctx->vcap;
    while (cap <= K1_VS_MAX_CAP &&
           (uint64_t)V * 100 > cap * (cap < VOCAB_LOW_LOAD_CAP ? ctx->vload_pct : ctx->vload_big_pct))
        cap *= 2;
    if (cap > K1_VS_MAX_CAP) return TFIDF_E_CAPACITY;
    /* from here on the previous result or model is gone */
    result_changed(ctx, RC_SCORES | RC_TERMS | RC_NEW);
    if (const int q = idf_pin_quiesce(ctx)) return q;
    ctx->vcap = cap;
    DevBuf& dfb = ctx->xp ? ctx->df_global : ctx->df_local;   /* df_of_run */
    ENSURE(ctx->vkeys, cap * 16);
    ENSURE(ctx->vrep, cap * 8);
    ENSURE(ctx->rank_of_slot, cap * 4);
    ENSURE(dfb, (size_t)V * 4 + 4);
    ENSURE(ctx->m_off, ((size_t)V + 1) * 8);
    ENSURE(ctx->m_blob, nbytes + 64);
    ENSURE(ctx->m_stat, 256);
    /* the device's offsets index the uploaded bytes from 0: the caller's own array when it
     * starts there (an exported or loaded model), else a rebased copy */
    std::vector<uint64_t> rebased;
    const uint64_t zero_off = 0;
    const uint64_t* h_off = V ? m->term_off : &zero_off;
    if (base) {
        rebased.resize((size_t)V + 1);
        for (uint32_t t = 0; t <= V; ++t) rebased[t] = m->term_off[t] - base;
        h_off = rebased.data();
    }
    uint64_t nlong = 0;
    for (uint32_t t = 0; t < V; ++t) nlong += (h_off[t + 1] - h_off[t]) >= 16u ? 1u : 0u;
    /* ---- idf: log(1.0 * N / df) on this host's libm, in run_post's forms.  Up to
     * IDF_FULL_MAX documents every df = 1..N, tabulated by the context's workers while the
     * device builds the table ---- */
    const bool full_lut = Nt <= IDF_FULL_MAX;
    IdfJoin idf_guard{ctx};
    if (V && full_lut) {
        if (idf_pin_reserve(ctx, (size_t)Nt + 1)) return TFIDF_E_NOMEM;
        ctx->idf_full_n = 0;
        ctx->idf_pin[0] = 0.0;
        idf_post(ctx, ctx->idf_pin, Nt, nullptr, Nt);
    }
    /* ---- upload, clear, build ---- */
    HIPCHK(hipMemcpyAsync(ctx->m_off.p, h_off, ((size_t)V + 1) * 8, hipMemcpyHostToDevice, s));
    if (nbytes) HIPCHK(hipMemcpyAsync(ctx->m_blob.p, m->term_bytes + base, (size_t)nbytes, hipMemcpyHostToDevice, s));
    if (V) HIPCHK(hipMemcpyAsync(dfb.p, m->term_df, (size_t)V * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(ctx->ev_m[0], s));
    {
        FillList fl{};
        fl.p[0] = ctx->vkeys.p;        fl.bytes[0] = cap * 16; fl.val[0] = 0xEEEEEEEEu;   /* KEY_EMPTY_HI */
        fl.p[1] = ctx->rank_of_slot.p; fl.bytes[1] = cap * 4;  fl.val[1] = 0xFFFFFFFFu;   /* QUERY_NO_TERM */
        fl.p[2] = ctx->m_stat.p;       fl.bytes[2] = 256;      fl.val[2] = 0u;
        fl.n = 3;
        LAUNCH(launch_fill_multi(fl, s));
    }
    ModelBuild mb{ctx->m_off.as<uint64_t>(), ctx->m_blob.as<uint8_t>(), nbytes, V, ctx->vkeys.as<uint4>(),
                  ctx->vrep.as<uint64_t>(), cap - 1, ctx->rank_of_slot.as<uint32_t>(), ctx->m_stat.as<uint32_t>()};
    LAUNCH(launch_model_build(mb, s));
    HIPCHK(hipEventRecord(ctx->ev_m[1], s));
    uint32_t st = 0;
    HIPCHK(hipMemcpyAsync(&st, ctx->m_stat.p, 4, hipMemcpyDeviceToHost, s));
    if (V && full_lut) {
        ENSURE(ctx->idf_vals, (size_t)(Nt + 1) * 8);
        idf_join(ctx);
        HIPCHK(hipMemcpyAsync(ctx->idf_vals.p, ctx->idf_pin, (size_t)(Nt + 1) * 8, hipMemcpyHostToDevice, s));
        ctx->idf_pin_busy = true;
        HIPCHK(hipStreamSynchronize(s));
        ctx->idf_pin_busy = false;
        ctx->idf_full_n = Nt;
    } else if (V) {   /* the distinct df values, listed on the device as run_post lists them */
        ctx->idf_full_n = 0;
        {
            const size_t want = (size_t)(Nt + 2) * 4 + scan_scratch(Nt + 1) + 8192;
            if (arena_reset(ctx, want > ctx->arena_buf.cap ? want : ctx->arena_buf.cap) != 0) return TFIDF_E_NOMEM;
        }
        Arena& ar = ctx->arena;
        ENSURE(ctx->present, (Nt + 2) * 4);
        uint32_t* present = ctx->present.as<uint32_t>();
        HIPCHK(hipMemsetAsync(present, 0, (Nt + 2) * 4, s));
        uint32_t* vals_dev = (uint32_t*)ar.get((size_t)(Nt + 2) * 4);
        if (!vals_dev) return TFIDF_E_NOMEM;
        LAUNCH(launch_df_mark(dfb.as<uint32_t>(), V, present, s) || scan_excl_u32(present, present, Nt + 1, ar, s) ||
            launch_df_list(present, Nt + 1, vals_dev, s));
        uint32_t K = 0;
        HIPCHK(hipMemcpyAsync(&K, present + Nt + 1, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (K == 0 || K > V) return TFIDF_E_STATE;
        std::vector<uint32_t> vals(K);
        HIPCHK(hipMemcpyAsync(vals.data(), vals_dev, (size_t)K * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        ENSURE(ctx->idf_vals, (size_t)K * 8 + 8);
        if (idf_pin_reserve(ctx, (size_t)K + 1)) return TFIDF_E_NOMEM;
        if (K < 2 * 16384) {
            for (uint32_t k = 0; k < K; ++k) ctx->idf_pin[k] = log(1.0 * (double)Nt / (double)vals[k]);
        } else {
            idf_post(ctx, ctx->idf_pin, Nt, vals.data(), K);
            idf_join(ctx);
        }
        HIPCHK(hipMemcpyAsync(ctx->idf_vals.p, ctx->idf_pin, (size_t)K * 8, hipMemcpyHostToDevice, s));
        ctx->idf_pin_busy = true;
        HIPCHK(hipStreamSynchronize(s));
        ctx->idf_pin_busy = false;
    } else {
        HIPCHK(hipStreamSynchronize(s));
    }
    /* the build's status, read as run_local reads K1's */
    if (st & ST_BOUNDS) {
        fprintf(stderr, "tfidf: model import: internal bounds check tripped (status 0x%x)\n", st);
        return TFIDF_E_STATE;
    }
    if (st & ST_LONG_COLLIDE) {   /* dev_vocab.h: reported, never merged */
        fprintf(stderr, "tfidf: two distinct terms of 16 bytes or more share their 120-bit identity key\n");
        return TFIDF_E_CAPACITY;
    }
    if (st & (ST_VOCAB_FULL | ST_VOCAB_SPIN | ST_TERM_LONG)) return TFIDF_E_CAPACITY;   /* not at these loads: no retry */
    if (st & ST_MODEL_DUP) return TFIDF_E_STATE;
    ctx->local_long = nlong != 0;
    ctx->V = V;
    ctx->Vg = V;
    ctx->ndocs_total = Nt;
    ctx->ndocs = 0;
    ctx->npairs = 0;
    ctx->info_npairs = 0;
    ctx->info_V = V;
    ctx->wt_tf = ctx->wt_idf = ctx->wt_norm = 0;   /* the model file records no scheme */
    ctx->rw_idf_mode = 0;
    ctx->corpus = tfidf_corpus{};
    ctx->corpus.nbytes = nbytes;   /* VocabRO.corpus_bytes: the blob stands where the corpus does */
    ctx->dev_bytes = ctx->m_blob.as<uint8_t>();
    ctx->dev_ids = nullptr;
    ctx->m_blob_bytes = nbytes;
    ctx->have_model = true;
    ctx->model_only = true;
    tfidf_model_info mi{};
    mi.nterms = V;
    mi.table_slots = cap;
    mi.blob_bytes = nbytes;
    mi.long_terms = nlong;
    mi.ms_build = ev_ms(ctx->ev_m[0], ctx->ev_m[1]);
    mi.ms_total = wall_ms(wall0);
    ctx->minfo = mi;
    return TFIDF_OK;
}

extern "C" int tfidf_last_model_info(const tfidf_ctx* ctx, tfidf_model_info* info) {
    return ctx ? copy_info(info, ctx->minfo) : TFIDF_E_INVAL;
}
