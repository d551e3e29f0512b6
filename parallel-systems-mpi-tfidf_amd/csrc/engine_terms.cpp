/*
 * engine_terms.cpp — tfidf_top_terms (terms.hip).
 * The context and the helpers every engine file shares: engine_ctx.h.
 */
#include "engine_ctx.h"

/* ---------------------------------------------------------------- keywords ----
 * Per-document top-k terms over the resident result (terms.hip).  The rows (every output
 * position, or the positions of the requested ids) are cut into batches whose device result
 * buffers stay under the context's budget; a batch is one selection pass, a scan of the
 * selected words' lengths and a gather of their bytes, copied straight into the caller's
 * arrays.  Nothing of the run's result is written. */

/* ---- the preambles the calls over the result share (engine_ctx.h): emit.hip's term metadata
 * and terms.hip's id lookup ---- */
int ensure_term_meta(tfidf_ctx* ctx) {
    if (ctx->tmeta_valid) return TFIDF_OK;
    const uint32_t V = ctx->V;
    ENSURE(ctx->t_key, (size_t)V * 16 + 16);
    ENSURE(ctx->t_len, (size_t)V * 4 + 4);
    LAUNCH(launch_term_meta(ctx->vkeys.as<uint4>(), ctx->vrep.as<uint64_t>(), ctx->slot_of_rank.as<uint32_t>(), V,
                            ctx->t_key.as<uint4>(), ctx->t_len.as<uint32_t>(), ctx->stream));
    ctx->tmeta_valid = true;
    return TFIDF_OK;
}

int lookup_ids(tfidf_ctx* ctx, DevBuf& ids, const uint32_t* host_ids, uint32_t n, uint32_t* d_pos) {
    ENSURE(ids, (size_t)n * (d_pos ? 4 : 8) + 8);
    uint32_t* d_ids = ids.as<uint32_t>();
    HIPCHK(hipMemcpyAsync(d_ids, host_ids, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    TLookupArgs la{d_ids, n, ctx->order, ctx->dev_ids, ctx->ndocs, d_pos ? d_pos : d_ids + n};
    LAUNCH(launch_terms_lookup(la, ctx->stream));
    return TFIDF_OK;
}

extern "C" void tfidf_doc_terms_free(tfidf_doc_terms* t) {
    if (!t) return;
    free(t->doc); free(t->pos); free(t->npairs); free(t->nterms); free(t->term); free(t->count);
    free(t->score); free(t->pair); free(t->word_off); free(t->word_bytes);
    memset(t, 0, sizeof(*t));
}

extern "C" int tfidf_top_terms(tfidf_ctx* ctx, const uint32_t* doc_ids, uint32_t ndocs, uint32_t k, tfidf_doc_terms* out) {
    if (!ctx || !out) return TFIDF_E_INVAL;
    if (k == 0 || k > TFIDF_TERMS_MAX_K) return TFIDF_E_INVAL;
    if (!ctx->have_result) return TFIDF_E_STATE;
    const auto wall0 = std::chrono::steady_clock::now();
    if (const int rc = call_begin(ctx, ctx->ev_t)) return rc;
    hipStream_t s = ctx->stream;
    const uint32_t N = ctx->ndocs, V = ctx->V;
    const uint32_t R = doc_ids ? ndocs : N;
    const size_t RK = (size_t)R * k;
    memset(out, 0, sizeof(*out));
    out->ndocs = R;
    out->k = k;
    out->doc = (uint32_t*)calloc((size_t)R + 1, 4);
    out->pos = (uint32_t*)calloc((size_t)R + 1, 4);
    out->npairs = (uint64_t*)calloc((size_t)R + 1, 8);
    out->nterms = (uint32_t*)calloc((size_t)R + 1, 4);
    out->term = (uint32_t*)calloc(RK + 1, 4);
    out->count = (uint32_t*)calloc(RK + 1, 4);
    out->score = (double*)calloc(RK + 1, 8);
    out->pair = (uint64_t*)calloc(RK + 1, 8);
    out->word_off = (uint64_t*)calloc(RK + 1, 8);
    out->word_bytes = (uint8_t*)calloc(1, 1);
    struct TermsGuard {   /* an error return leaves *out zeroed */
        tfidf_doc_terms* t;
        ~TermsGuard() { if (t) tfidf_doc_terms_free(t); }
    } guard{out};
    if (!out->doc || !out->pos || !out->npairs || !out->nterms || !out->term || !out->count || !out->score ||
        !out->pair || !out->word_off || !out->word_bytes)
        return TFIDF_E_NOMEM;
    tfidf_terms_info ti{};
    ti.ndocs = R;
    ti.k = k;

    /* ---- the selected words' lengths and byte sources: the formatter's term metadata ---- */
    if (V)
        if (const int rc = ensure_term_meta(ctx)) return rc;

    /* ---- lookup: one lane per requested id ---- */
    const uint32_t* d_pos = nullptr;
    if (doc_ids && R) {
        HIPCHK(hipEventRecord(ctx->ev_t[0], s));
        if (const int rc = lookup_ids(ctx, ctx->tm_ids, doc_ids, R, nullptr)) return rc;
        HIPCHK(hipEventRecord(ctx->ev_t[1], s));
        d_pos = ctx->tm_ids.as<uint32_t>() + R;
        HIPCHK(hipMemcpyAsync(out->pos, d_pos, (size_t)R * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        ti.ms_lookup = ev_ms(ctx->ev_t[0], ctx->ev_t[1]);
        ti.out_bytes += (uint64_t)R * 4;
    } else {
        for (uint32_t r = 0; r < R; ++r) out->pos[r] = r;
    }

    /* ---- batches of rows under the budget: 32 bytes per entry, 20 per row ---- */
    const uint64_t per_row = (uint64_t)k * 32 + 20;
    uint64_t B = ctx->terms_bytes / per_row;
    B = B < 1 ? 1 : B;
    if (B > R) B = R;
    const size_t BK = (size_t)B * k;
    if (R) {
        ENSURE(ctx->tm_rows, (size_t)B * 16 + 16);
        ENSURE(ctx->tm_score, BK * 8 + 8);
        ENSURE(ctx->tm_pair, BK * 8 + 8);
        ENSURE(ctx->tm_term, BK * 4 + 4);
        ENSURE(ctx->tm_cnt, BK * 4 + 4);
        ENSURE(ctx->tm_woff, BK * 8 + 16);
        ENSURE(ctx->tm_big, (size_t)B * 4 + 16);
    }
    std::vector<uint64_t> h_woff(BK + 1);
    std::vector<uint32_t> h_doc(B);
    uint64_t wbase = 0;
    for (uint64_t r0 = 0; r0 < R; r0 += B) {
        const uint32_t nb = (uint32_t)(R - r0 < B ? R - r0 : B);
        const size_t nbk = (size_t)nb * k;
        ++ti.nbatches;
        TSelArgs sa{};
        sa.out_off = ctx->out_off.as<uint64_t>();
        sa.out_term = ctx->out_term.as<uint32_t>();
        sa.out_cnt = ctx->out_cnt.as<uint32_t>();
        sa.out_score = ctx->out_score.as<double>();
        sa.order = ctx->order;
        sa.doc_ids = ctx->dev_ids;
        sa.tlen = ctx->t_len.as<uint32_t>();
        sa.ndocs = N;
        sa.nterms = V;
        sa.npairs = ctx->npairs;
        sa.pos = d_pos;
        sa.row0 = (uint32_t)r0;
        sa.nrows = nb;
        sa.k = k;
        sa.rnpairs = ctx->tm_rows.as<uint64_t>();
        sa.rnterms = (uint32_t*)(sa.rnpairs + B);
        sa.rdoc = sa.rnterms + B;
        sa.score = ctx->tm_score.as<uint64_t>();
        sa.pair = ctx->tm_pair.as<uint64_t>();
        sa.term = ctx->tm_term.as<uint32_t>();
        sa.cnt = ctx->tm_cnt.as<uint32_t>();
        sa.wlen = ctx->tm_woff.as<uint64_t>();
        sa.big_list = ctx->tm_big.as<uint32_t>();
        sa.big_count = sa.big_list + B;
        HIPCHK(hipEventRecord(ctx->ev_t[0], s));
        LAUNCH(launch_terms_select(sa, ctx->ncu, s));
        HIPCHK(hipEventRecord(ctx->ev_t[1], s));
        /* word lengths -> offsets inside the batch, in place; [nbk] = the batch's word bytes */
        ctx->arena.used = 0;   /* as format_prepare: nothing of the result lives in the arena */
        SCAN(scan_excl_u64(sa.wlen, sa.wlen, nbk, ctx->arena, s));
        HIPCHK(hipEventRecord(ctx->ev_t[2], s));
        uint32_t nbig = 0;
        HIPCHK(hipMemcpyAsync(h_woff.data(), sa.wlen, (nbk + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&nbig, sa.big_count, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const uint64_t wtotal = h_woff[nbk];
        ENSURE(ctx->tm_words, wtotal + 16);
        TWordArgs wa{sa.term, sa.wlen, nbk, ctx->t_key.as<uint4>(), V, ctx->dev_bytes, ctx->corpus.nbytes,
                     ctx->tm_words.as<uint8_t>()};
        HIPCHK(hipEventRecord(ctx->ev_t[3], s));
        LAUNCH(launch_terms_words(wa, s));
        HIPCHK(hipEventRecord(ctx->ev_t[4], s));
        uint8_t* wb = (uint8_t*)realloc(out->word_bytes, (size_t)(wbase + wtotal) + 1);
        if (!wb) return TFIDF_E_NOMEM;
        out->word_bytes = wb;
        const size_t e0 = (size_t)r0 * k;
        HIPCHK(hipMemcpyAsync(out->npairs + r0, sa.rnpairs, (size_t)nb * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->nterms + r0, sa.rnterms, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_doc.data(), sa.rdoc, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->score + e0, sa.score, nbk * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->pair + e0, sa.pair, nbk * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->term + e0, sa.term, nbk * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->count + e0, sa.cnt, nbk * 4, hipMemcpyDeviceToHost, s));
        if (wtotal) HIPCHK(hipMemcpyAsync(wb + wbase, ctx->tm_words.p, wtotal, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        ti.ms_select += ev_ms(ctx->ev_t[0], ctx->ev_t[1]);
        ti.ms_words += ev_ms(ctx->ev_t[1], ctx->ev_t[2]);
        ti.ms_words += ev_ms(ctx->ev_t[3], ctx->ev_t[4]);
        ti.big_docs += nbig < nb ? nbig : nb;
        ti.out_bytes += (uint64_t)nb * 16 + nbk * 32 + wtotal;
        for (uint32_t i = 0; i < nb; ++i) out->doc[r0 + i] = doc_ids ? doc_ids[r0 + i] : h_doc[i];
        for (size_t i = 0; i < nbk; ++i) out->word_off[e0 + i] = wbase + h_woff[i];
        wbase += wtotal;
    }
    out->word_off[RK] = wbase;
    ti.ms_total = wall_ms(wall0);
    ctx->tinfo = ti;
    guard.t = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_last_terms_info(const tfidf_ctx* ctx, tfidf_terms_info* info) {
    return ctx ? copy_info(info, ctx->tinfo) : TFIDF_E_INVAL;
}
