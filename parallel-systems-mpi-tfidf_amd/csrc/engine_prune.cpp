/*
 * engine_prune.cpp — tfidf_prune (prune.hip).
 * The context and the helpers every engine file shares: engine_ctx.h.
 */
#include "engine_ctx.h"

/* ------------------------------------------------------------------- prune ----
 * Vocabulary pruning by document frequency over the resident result (prune.hip; the parameter
 * check and the model form are prune_host.c).  Select (flags, the max_features sort, bitmap, new
 * ranks), the term arrays, the pair pass.  Everything is written into spare buffers of the
 * context, which change places with the resident ones when every step has succeeded; only
 * rank_of_slot is rewritten in place, by the last launch.  idf_rank is the score stage's scratch
 * and has no reader after a run (transform reads the idf by df), so it is left alone. */

/* a spare as large as the buffer it will change places with: after the swap neither a run nor
 * the next prune has anything to grow */
int ensure_spare(DevBuf& spare, const DevBuf& orig, size_t need) {
    const size_t want = orig.cap > need ? orig.cap : need;
    if (spare.p && spare.cap >= want) return 0;
    return spare.exact(want);
}

extern "C" int tfidf_prune(tfidf_ctx* ctx, const tfidf_prune_params* params) {
    if (!ctx || tfidf_prune_check(params) != TFIDF_OK) return TFIDF_E_INVAL;
    if (!ctx->have_result || ctx->model_only) return TFIDF_E_STATE;
    if (ctx->xp && params->max_features) return TFIDF_E_INVAL;   /* the ranks share no term table */
    const auto wall0 = std::chrono::steady_clock::now();
    if (const int rc = call_begin(ctx, ctx->ev_pr)) return rc;
    hipStream_t s = ctx->stream;
    const uint32_t V = ctx->V, N = ctx->ndocs, M = params->max_features;
    const uint64_t P = ctx->npairs, Nt = ctx->ndocs_total;
    const uint64_t ntiles = P / PR_TILE + 1u;
    const bool cut = M != 0u && M < V;   /* M >= V cannot remove a survivor */
    DevBuf& dfb = ctx->xp ? ctx->df_global : ctx->df_local;   /* df_of_run */
    ENSURE(ctx->pr_flag, ((size_t)V + 1) * 4 + 4);
    ENSURE(ctx->pr_bits, (((size_t)V + 63) / 64) * 8 + 16);
    ENSURE(ctx->pr_tcnt, (size_t)(ntiles + 1) * 8);
    ENSURE(ctx->pr_tdoc, (size_t)(ntiles + 1) * 4);
    ENSURE(ctx->pr_misc, 256);
    if (cut) {
        ENSURE(ctx->pr_k0, (size_t)V * 8 + 8);
        ENSURE(ctx->pr_k1, (size_t)V * 8 + 8);
        ENSURE(ctx->pr_v0, (size_t)V * 4 + 4);
        ENSURE(ctx->pr_v1, (size_t)V * 4 + 4);
    }
    if (ensure_spare(ctx->pr_sor, ctx->slot_of_rank, (size_t)V * 4 + 4) || ensure_spare(ctx->pr_df, dfb, (size_t)V * 4 + 4) ||
        ensure_spare(ctx->pr_term, ctx->out_term, (size_t)P * 4 + 4) || ensure_spare(ctx->pr_cnt, ctx->out_cnt, (size_t)P * 4 + 4) ||
        ensure_spare(ctx->pr_score, ctx->out_score, (size_t)P * 8 + 8) || ensure_spare(ctx->pr_off, ctx->out_off, ((size_t)N + 1) * 8))
        return TFIDF_E_NOMEM;
    {   /* the scans' block sums and the sort's histograms */
        const uint64_t nb = ((uint64_t)V + 2047) / 2048;
        const size_t want = scan_scratch((uint64_t)V + 1) + scan_scratch(ntiles + 1) +
                            (cut ? (size_t)(256 * nb + 1) * 4 + scan_scratch(256 * nb) : 0) + 8192;
        if (arena_scratch(ctx, want)) return TFIDF_E_NOMEM;
    }
    uint32_t* flag = ctx->pr_flag.as<uint32_t>();   /* the keep flags, then in place the new ranks */
    uint32_t* bits = ctx->pr_bits.as<uint32_t>();
    /* ---- select ---- */
    HIPCHK(hipEventRecord(ctx->ev_pr[0], s));
    LAUNCH(launch_pr_range(df_of_run(ctx), V, Nt, params->min_df, params->max_df, flag,
                        cut ? ctx->pr_k0.as<uint64_t>() : nullptr, ctx->pr_v0.as<uint32_t>(), s));
    uint64_t cut_keys[2] = {PR_KEY_DEAD, PR_KEY_DEAD};   /* the sorted keys at positions M - 1 and M */
    if (cut) {
        uint32_t byte_mask = 1u << 4;   /* PR_KEY_DEAD's bit; below it the bytes Nt - df can reach */
        for (int b = 0; b < 4; ++b)
            if ((Nt >> (8 * b)) != 0) byte_mask |= 1u << b;
        const int where = radix_sort_u64(ctx->pr_k0.as<uint64_t>(), ctx->pr_v0.as<uint32_t>(), ctx->pr_k1.as<uint64_t>(),
                                         ctx->pr_v1.as<uint32_t>(), V, byte_mask, ctx->arena, s);
        if (where < 0) { HIPCHK(hipGetLastError()); return where == -2 ? TFIDF_E_NOMEM : TFIDF_E_HIP; }
        const uint64_t* ks = where ? ctx->pr_k1.as<uint64_t>() : ctx->pr_k0.as<uint64_t>();
        const uint32_t* vs = where ? ctx->pr_v1.as<uint32_t>() : ctx->pr_v0.as<uint32_t>();
        LAUNCH(launch_pr_take(ks, vs, V, M, flag, s));
        HIPCHK(hipMemcpyAsync(cut_keys, ks + (M - 1u), 16, hipMemcpyDeviceToHost, s));   /* M < V: both exist */
    }
    LAUNCH(launch_pr_bitmap(flag, V, bits, s));
    SCAN(scan_excl_u32(flag, flag, V, ctx->arena, s));
    HIPCHK(hipEventRecord(ctx->ev_pr[1], s));
    uint32_t V2 = 0;
    HIPCHK(hipMemcpyAsync(&V2, flag + V, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (V2 > V) return TFIDF_E_STATE;
    tfidf_prune_info pi{};
    pi.nterms_before = V;
    pi.npairs_before = P;
    /* the cut removed a survivor of the range test exactly when position M holds one */
    if (cut && cut_keys[1] != PR_KEY_DEAD && cut_keys[0] <= Nt) pi.cut_df = (uint32_t)(Nt - cut_keys[0]);
    pi.ms_select = ev_ms(ctx->ev_pr[0], ctx->ev_pr[1]);
    if (V2 == V) {   /* nothing to remove: every byte stays */
        pi.nterms_after = V;
        pi.npairs_after = P;
        pi.ms_total = wall_ms(wall0);
        ctx->pinfo = pi;
        return TFIDF_OK;
    }
    /* ---- terms ---- */
    PrTerms ta{bits, flag, V, ctx->slot_of_rank.as<uint32_t>(), df_of_run(ctx), ctx->pr_sor.as<uint32_t>(),
               ctx->pr_df.as<uint32_t>()};
    LAUNCH(launch_pr_terms(ta, s));
    HIPCHK(hipEventRecord(ctx->ev_pr[2], s));
    /* ---- pairs ---- */
    HIPCHK(hipMemsetAsync(ctx->pr_misc.p, 0, 16, s));
    PrPairs pa{};
    pa.out_off = ctx->out_off.as<uint64_t>();
    pa.out_term = ctx->out_term.as<uint32_t>();
    pa.out_cnt = ctx->out_cnt.as<uint32_t>();
    pa.out_score = ctx->out_score.as<double>();
    pa.npairs = P;
    pa.ndocs = N;
    pa.V = V;
    pa.bits = bits;
    pa.new_rank = flag;
    pa.ntiles = ntiles;
    pa.tile_cnt = ctx->pr_tcnt.as<uint64_t>();
    pa.tile_doc = ctx->pr_tdoc.as<uint32_t>();
    pa.new_term = ctx->pr_term.as<uint32_t>();
    pa.new_cnt = ctx->pr_cnt.as<uint32_t>();
    pa.new_score = ctx->pr_score.as<double>();
    pa.new_off = ctx->pr_off.as<uint64_t>();
    pa.emptied = ctx->pr_misc.as<uint32_t>();
    LAUNCH(launch_pr_tiledoc(pa, s) || launch_pr_count(pa, ctx->ncu, s));
    SCAN(scan_excl_u64(pa.tile_cnt, pa.tile_cnt, ntiles, ctx->arena, s));
    LAUNCH(launch_pr_write(pa, ctx->ncu, s) || launch_pr_emptied(pa, s));
    HIPCHK(hipEventRecord(ctx->ev_pr[3], s));
    uint64_t P2 = 0;
    uint32_t emptied = 0;
    HIPCHK(hipMemcpyAsync(&P2, pa.tile_cnt + ntiles, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&emptied, pa.emptied, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));   /* every spare is written: from here on the call cannot fail half-way */
    if (P2 > P) return TFIDF_E_STATE;
    LAUNCH(launch_pr_slots(ta, ctx->rank_of_slot.as<uint32_t>(), ctx->vcap, s));
    HIPCHK(hipStreamSynchronize(s));
    std::swap(ctx->slot_of_rank, ctx->pr_sor);
    std::swap(dfb, ctx->pr_df);
    std::swap(ctx->out_term, ctx->pr_term);
    std::swap(ctx->out_cnt, ctx->pr_cnt);
    std::swap(ctx->out_score, ctx->pr_score);
    std::swap(ctx->out_off, ctx->pr_off);
    ctx->V = V2;
    ctx->npairs = P2;
    result_changed(ctx, RC_SCORES | RC_TERMS);   /* the classifier's matrices are indexed by the old ranks */
    pi.nterms_after = V2;
    pi.npairs_after = P2;
    pi.docs_emptied = emptied;
    pi.ms_terms = ev_ms(ctx->ev_pr[1], ctx->ev_pr[2]);
    pi.ms_pairs = ev_ms(ctx->ev_pr[2], ctx->ev_pr[3]);
    pi.ms_total = wall_ms(wall0);
    ctx->pinfo = pi;
    return TFIDF_OK;
}

extern "C" int tfidf_last_prune_info(const tfidf_ctx* ctx, tfidf_prune_info* info) {
    return ctx ? copy_info(info, ctx->pinfo) : TFIDF_E_INVAL;
}
