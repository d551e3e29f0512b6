/*
 * engine_transform.cpp — tfidf_transform (transform.hip).
 * The context and the helpers every engine file shares: engine_ctx.h.
 */
#include "engine_ctx.h"

/* --------------------------------------------------------------- transform ----
 * Unseen documents against the resident model (transform.hip).  The run leaves vkeys / vrep /
 * rank_of_slot, df_of_run, idf_vals and (N over IDF_FULL_MAX) its `present` index in buffers of
 * the context that nothing after the run writes (engine_query.cpp's note; the query, keyword
 * and similarity calls use their own buffers and the arena only as scratch), so the scores
 * read the very doubles the run multiplied with.  The batch is cut into slices at document
 * boundaries; a slice is: boundaries (counted, scanned, written) -> one round trip for the
 * token total -> resolve -> stable sort of (row << 32 | rank, token index) -> run heads, scan,
 * pairs -> copies into the caller's arrays. */

extern "C" void tfidf_rows_free(tfidf_rows* r) {
    if (!r) return;
    free(r->row_off); free(r->doc_size); free(r->doc_oov); free(r->term); free(r->count); free(r->df);
    free(r->score); free(r->word_off); free(r->word_len);
    memset(r, 0, sizeof(*r));
}

namespace {
struct RowsGuard {   /* an error return leaves *out zeroed */
    tfidf_rows* r;
    ~RowsGuard() { if (r) tfidf_rows_free(r); }
};
template <typename T> bool grow_host(T*& p, uint64_t n) {
    void* q = realloc(p, (size_t)(n + 1) * sizeof(T));
    if (!q) return false;
    p = (T*)q;
    return true;
}
}  // namespace

extern "C" int tfidf_transform(tfidf_ctx* ctx, const tfidf_corpus* batch, tfidf_rows* out) {
    return tfidf_ctx_transform(ctx, batch, out, true);
}

int tfidf_ctx_transform(tfidf_ctx* ctx, const tfidf_corpus* batch, tfidf_rows* out, bool norm) {
    if (!ctx || !batch || !out) return TFIDF_E_INVAL;
    const uint32_t N = batch->ndocs;
    if (N && !batch->doc_off) return TFIDF_E_INVAL;   /* an argument error comes before a state error */
    if (!ctx->have_model) return TFIDF_E_STATE;       /* a run's model or an imported one */
    const auto wall0 = std::chrono::steady_clock::now();
    if (const int rc = call_begin(ctx, ctx->ev_tr)) return rc;
    hipStream_t s = ctx->stream;
    /* the offsets on the host: the slices are cut here */
    std::vector<uint64_t> off_copy;
    const uint64_t* off = nullptr;
    if (const int rc = corpus_offsets(ctx, *batch, off_copy, &off)) return rc;
    if (N && off[N] > off[0] && !batch->bytes) return TFIDF_E_INVAL;   /* an empty window needs no bytes */
    /* the run's own host corpus lives in in_bytes: a host batch gets its own buffers */
    const uint8_t* d_bytes = nullptr;
    const uint64_t* d_off = nullptr;
    if (const int rc = stage_window(ctx, *batch, off, ctx->tr_bytes, ctx->tr_off, &d_bytes, &d_off)) return rc;

    memset(out, 0, sizeof(*out));
    RowsGuard guard{out};
    out->ndocs = N;
    out->row_off = (uint64_t*)calloc((size_t)N + 1, 8);
    out->doc_size = (uint32_t*)calloc((size_t)N + 1, 4);
    out->doc_oov = (uint32_t*)calloc((size_t)N + 1, 4);
    if (!out->row_off || !out->doc_size || !out->doc_oov) return TFIDF_E_NOMEM;
    if (!grow_host(out->term, 0) || !grow_host(out->count, 0) || !grow_host(out->df, 0) || !grow_host(out->score, 0) ||
        !grow_host(out->word_off, 0) || !grow_host(out->word_len, 0))
        return TFIDF_E_NOMEM;

    tfidf_transform_info ti{};
    ti.ndocs = N;
    const uint32_t V = ctx->V;
    const bool full_lut = ctx->ndocs_total <= IDF_FULL_MAX;   /* run_post: idf_vals by df, else through `present` */
    /* the active weighting scheme (tfidf_reweight); the reference's takes the path it always took */
    const uint32_t wtf = ctx->wt_tf, widf = ctx->wt_idf, wnorm = norm ? ctx->wt_norm : (uint32_t)TFIDF_NORM_NONE;
    const bool ref_scheme = wtf == TFIDF_TF_RATIO && widf == TFIDF_IDF_REF && ctx->wt_norm == TFIDF_NORM_NONE;
    if (!ref_scheme) ENSURE(ctx->rw_misc, 256);
    uint64_t Ptot = 0;
    std::vector<uint64_t> h_rowoff;
    for (uint32_t d0 = 0; d0 < N;) {
        /* ---- the slice: documents [d0, d1) whose scratch bound stays under the budget ---- */
        uint32_t d1 = d0 + 1;
        while (d1 < N && tr_bound(off[d1 + 1] - off[d0], (uint64_t)d1 + 1 - d0) <= ctx->transform_bytes) ++d1;
        const uint32_t nd = d1 - d0;
        const uint64_t b0 = off[d0], b1 = off[d1];
        ++ti.nslices;
        for (uint32_t r = 0; r <= nd; ++r) out->row_off[d0 + r] = Ptot;   /* rows without a token stay empty */
        if (b1 == b0) { d0 = d1; continue; }
        TrSlice sl{};
        sl.bytes = d_bytes;
        sl.nbytes = batch->nbytes;
        sl.doc_off = d_off;
        sl.d0 = d0;
        sl.d1 = d1;
        sl.b0 = b0;
        sl.b1 = b1;
        /* tr_a: status, per-document words; behind them the bitmap and the per-tile counts */
        const size_t a_dsize = 256, a_doov = al256(a_dsize + (size_t)nd * 4);
        const size_t a_rowoff = al256(a_doov + (size_t)nd * 4), a_head = al256(a_rowoff + ((size_t)nd + 1) * 8);
        size_t a_end = 0;
        if (const int rc = token_scratch(ctx, sl, ctx->tr_a, a_head, &a_end)) return rc;
        uint8_t* A = ctx->tr_a.as<uint8_t>();
        HIPCHK(hipMemsetAsync(A, 0, a_rowoff, s));   /* status, doc_size, doc_oov */
        HIPCHK(hipEventRecord(ctx->ev_tr[0], s));
        uint64_t T = 0;
        if (const int rc = token_bounds(ctx, sl, "transform", &T)) return rc;
        if (T == 0) {   /* whitespace only */
            const uint64_t sb = a_end;
            if (sb > ti.scratch_bytes) ti.scratch_bytes = sb;
            d0 = d1;
            continue;
        }
        /* tr_b: token records, sort buffers, pairs (sized by the slice's tokens) */
        size_t bo = 0;
        auto take = [&bo](size_t bytes) { const size_t at = bo; bo = al256(bo + bytes); return at; };
        const size_t b_ts = take(T * 8), b_te = take(T * 8), b_tl = take(T * 4);
        const size_t b_k0 = take(T * 8), b_k1 = take(T * 8), b_v0 = take(T * 4), b_v1 = take(T * 4);
        const size_t b_pos = take((T + 1) * 4);
        const size_t b_prow = take(T * 4), b_pterm = take(T * 4), b_pcnt = take(T * 4), b_pdf = take(T * 4);
        const size_t b_psc = take(T * 8), b_pwo = take(T * 8), b_pwl = take(T * 4);
        ENSURE(ctx->tr_b, bo);
        if (a_end + bo > ti.scratch_bytes) ti.scratch_bytes = a_end + bo;
        uint8_t* B = ctx->tr_b.as<uint8_t>();
        /* the arena: the sort's histograms and the scans' block sums */
        if (const int rc = token_write(ctx, sl, (uint64_t*)(B + b_ts), (uint64_t*)(B + b_te), T,
                                       (size_t)(T / 2 + T / 64) + (8u << 20)))
            return rc;
        HIPCHK(hipEventRecord(ctx->ev_tr[1], s));
        TrResolve ra{};
        ra.sl = sl;
        ra.ntok = T;
        ra.voc = VocabRO{ctx->vkeys.as<uint4>(), ctx->vrep.as<uint64_t>(), ctx->vcap - 1, ~1ull,
                         ctx->rank_of_slot.as<uint32_t>(), ctx->dev_bytes, ctx->corpus.nbytes, V};
        ra.key = (uint64_t*)(B + b_k0);
        ra.val = (uint32_t*)(B + b_v0);
        ra.tlen = (uint32_t*)(B + b_tl);
        LAUNCH(launch_tr_resolve(ra, s));
        HIPCHK(hipEventRecord(ctx->ev_tr[2], s));
        /* only the bytes that vary are sorted: the ranks 0..V below, the rows d0..d1-1 above */
        uint32_t byte_mask = 0;
        for (uint32_t b = 0; b < 4; ++b) {
            if ((V >> (8 * b)) != 0) byte_mask |= 1u << b;
            if (((d0 ^ (d1 - 1)) >> (8 * b)) != 0) byte_mask |= 1u << (4 + b);
        }
        const int where = radix_sort_u64(ra.key, ra.val, (uint64_t*)(B + b_k1), (uint32_t*)(B + b_v1), T, byte_mask,
                                         ctx->arena, s);
        if (where < 0) { HIPCHK(hipGetLastError()); return where == -2 ? TFIDF_E_NOMEM : TFIDF_E_HIP; }
        HIPCHK(hipEventRecord(ctx->ev_tr[3], s));
        TrPairs pa{};
        pa.key = where ? (uint64_t*)(B + b_k1) : ra.key;
        pa.val = where ? (uint32_t*)(B + b_v1) : ra.val;
        pa.ntok = T;
        pa.d0 = d0;
        pa.d1 = d1;
        pa.V = V;
        pa.doc_off = d_off;
        pa.tok_start = sl.tok_start;
        pa.tlen = ra.tlen;
        pa.flag = (uint32_t*)(B + b_pos);
        pa.pos = pa.flag;   /* scanned in place */
        pa.df = df_of_run(ctx);
        pa.idf_idx = full_lut ? nullptr : ctx->present.as<uint32_t>();
        pa.idf = ctx->idf_vals.as<double>();
        pa.Nt = ctx->ndocs_total;
        pa.doc_size = (uint32_t*)(A + a_dsize);
        pa.doc_oov = (uint32_t*)(A + a_doov);
        pa.row_off = (uint64_t*)(A + a_rowoff);
        pa.p_row = (uint32_t*)(B + b_prow);
        pa.p_term = (uint32_t*)(B + b_pterm);
        pa.p_count = (uint32_t*)(B + b_pcnt);
        pa.p_df = (uint32_t*)(B + b_pdf);
        pa.p_score = (double*)(B + b_psc);
        pa.p_woff = (uint64_t*)(B + b_pwo);
        pa.p_wlen = (uint32_t*)(B + b_pwl);
        pa.status = sl.status;
        LAUNCH(launch_tr_flags(pa, s) || scan_excl_u32(pa.flag, pa.flag, T, ctx->arena, s) ||
            (ref_scheme ? launch_tr_pairs(pa, s) : launch_tr_pairs_w(pa, s)));
        uint32_t cw[2] = {0, 0};   /* sublinear tf: the slice's largest count and its counts above the table */
        if (!ref_scheme && wtf == TFIDF_TF_LOG) {
            if (const int rc = rw_cmax_launch(ctx, pa.p_count, T, pa.pos + T)) return rc;
            HIPCHK(hipMemcpyAsync(cw, ctx->rw_misc.as<uint32_t>() + RWM_CMAX, 8, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipEventRecord(ctx->ev_tr[4], s));
        /* ---- back to the host: the slice's words first (the pair total sizes the rest) ---- */
        uint32_t P32 = 0, st = 0;
        h_rowoff.resize((size_t)nd + 1);
        HIPCHK(hipMemcpyAsync(&P32, pa.pos + T, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&st, sl.status, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->doc_size + d0, pa.doc_size, (size_t)nd * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->doc_oov + d0, pa.doc_oov, (size_t)nd * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_rowoff.data(), pa.row_off, ((size_t)nd + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (st & ST_BOUNDS) {
            fprintf(stderr, "tfidf: transform: internal bounds check tripped (status 0x%x)\n", st);
            return TFIDF_E_STATE;
        }
        const uint64_t P = P32;
        if (!ref_scheme && P) {   /* the rows' scores by the scheme: w, then the norm over each row's pairs */
            uint32_t nlisted = 0;
            uint64_t nlogs = 0;
            if (wtf == TFIDF_TF_LOG)
                if (const int rc = rw_tf_finish(ctx, cw[0], cw[1], &nlisted, &nlogs)) return rc;
            ENSURE(ctx->rw_big, (size_t)nd * 4 + 4);
            RwArgs wa{};
            wa.off = pa.row_off;
            wa.npairs = P;
            wa.ndocs = nd;
            wa.doc_size = pa.doc_size;
            wa.count = pa.p_count;
            wa.key = pa.p_df;
            wa.key_n = ctx->ndocs_total + 1;
            if (widf != TFIDF_IDF_NONE) {
                wa.idf = widf == TFIDF_IDF_REF ? ctx->idf_vals.as<double>() : ctx->rw_idf.as<double>();
                wa.idf_idx = pa.idf_idx;
            }
            wa.score = pa.p_score;
            rw_scheme_args(ctx, wa, wtf, wnorm, nlisted);
            LAUNCH(launch_rw_pairs(wa, ctx->ncu, s));
        }
        if (!grow_host(out->term, Ptot + P) || !grow_host(out->count, Ptot + P) || !grow_host(out->df, Ptot + P) ||
            !grow_host(out->score, Ptot + P) || !grow_host(out->word_off, Ptot + P) || !grow_host(out->word_len, Ptot + P))
            return TFIDF_E_NOMEM;
        if (P) {
            HIPCHK(hipMemcpyAsync(out->term + Ptot, pa.p_term, (size_t)P * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out->count + Ptot, pa.p_count, (size_t)P * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out->df + Ptot, pa.p_df, (size_t)P * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out->score + Ptot, pa.p_score, (size_t)P * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out->word_off + Ptot, pa.p_woff, (size_t)P * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(out->word_len + Ptot, pa.p_wlen, (size_t)P * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        for (uint32_t r = 0; r <= nd; ++r) out->row_off[d0 + r] = Ptot + h_rowoff[r];
        Ptot += P;
        ti.ntokens += T;
        ti.ms_tokens += ev_ms(ctx->ev_tr[0], ctx->ev_tr[1]);
        ti.ms_resolve += ev_ms(ctx->ev_tr[1], ctx->ev_tr[2]);
        ti.ms_sort += ev_ms(ctx->ev_tr[2], ctx->ev_tr[3]);
        ti.ms_pairs += ev_ms(ctx->ev_tr[3], ctx->ev_tr[4]);
        d0 = d1;
    }
    if (N) out->row_off[N] = Ptot;
    out->npairs = Ptot;
    out->ntokens = ti.ntokens;
    for (uint32_t d = 0; d < N; ++d) ti.noov += out->doc_oov[d];
    ti.npairs = Ptot;
    ti.ms_total = wall_ms(wall0);
    ctx->trinfo = ti;
    guard.r = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_last_transform_info(const tfidf_ctx* ctx, tfidf_transform_info* info) {
    return ctx ? copy_info(info, ctx->trinfo) : TFIDF_E_INVAL;
}
