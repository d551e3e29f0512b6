/*
 * engine_kmeans.cpp — tfidf_kmeans (kmeans.hip).
 * The context and the helpers every engine file shares: engine_ctx.h.
 */
#include "engine_ctx.h"

/* ---------------------------------------------------------------- clusters ----
 * Spherical k-means over the resident result (kmeans.hip).  The norms are tfidf_similar's.  The
 * host validates the seeds against the documents' ids and norms (copied once), then loops over
 * the passes: an assignment, a 4-byte copy of the changed-label count, and unless the loop
 * stops an update.  Labels, sims and sizes come to the host once, after the last pass; the
 * matrix never does: the clusters' top terms are selected on the device and their words
 * gathered by the keyword path's k_terms_words.  Nothing of the run's result is written. */

extern "C" void tfidf_clusters_free(tfidf_clusters* c) {
    if (!c) return;
    free(c->doc); free(c->label); free(c->sim); free(c->size); free(c->seed); free(c->nterms); free(c->term);
    free(c->weight); free(c->word_off); free(c->word_bytes);
    memset(c, 0, sizeof(*c));
}

extern "C" int tfidf_kmeans(tfidf_ctx* ctx, const tfidf_kmeans_params* params, tfidf_clusters* out) {
    if (!ctx || !params || !out) return TFIDF_E_INVAL;
    if (params->size < sizeof(tfidf_kmeans_params)) return TFIDF_E_INVAL;
    const uint32_t K = params->k, T = params->nterms;
    const uint32_t max_iter = params->max_iter ? params->max_iter : TFIDF_KMEANS_DEFAULT_ITER;
    if (K == 0 || K > TFIDF_KMEANS_MAX_K || T > TFIDF_KMEANS_MAX_TERMS) return TFIDF_E_INVAL;
    if (params->seeds && params->nseeds != K) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!ctx->have_result) return TFIDF_E_STATE;
    const uint32_t N = ctx->ndocs, V = ctx->V;
    const uint64_t matrix = (uint64_t)K * V * 8;
    const uint64_t work = (uint64_t)N * 24 + (uint64_t)K * 24 + 64;
    if (matrix + work > ctx->kmeans_bytes) return TFIDF_E_CAPACITY;
    const auto wall0 = std::chrono::steady_clock::now();
    int rc = call_begin(ctx, ctx->ev_s);   /* sim_norms' events */
    if (!rc) rc = call_begin(ctx, ctx->ev_k);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    tfidf_kmeans_info ki{};
    ki.ndocs = N;
    ki.k = K;
    ki.matrix_bytes = matrix;
    ki.work_bytes = work;
    tfidf_similar_info si{};
    rc = sim_norms(ctx, si);
    if (rc) return rc;
    ki.ms_norms = si.ms_norms;
    ENSURE(ctx->km_work, work);
    ENSURE(ctx->km_C, matrix + 64);

    KmArgs a{};
    a.out_off = ctx->out_off.as<uint64_t>();
    a.out_term = ctx->out_term.as<uint32_t>();
    a.out_score = ctx->out_score.as<double>();
    a.norm = ctx->sm_norm.as<double>() + N;
    a.ndocs = N;
    a.npairs = ctx->npairs;
    a.V = V;
    a.K = K;
    a.C = ctx->km_C.as<double>();
    a.sim = ctx->km_work.as<double>();
    a.cnorm = a.sim + N;
    uint32_t* d_ids = (uint32_t*)(a.cnorm + K);
    uint32_t* d_lab[2] = {d_ids + N, d_ids + 2 * (size_t)N};
    a.members = d_ids + 3 * (size_t)N;
    a.size = a.members + N;
    a.moff = a.size + K;
    uint32_t* d_seedpos = a.moff + K + 1;
    a.seedpos = d_seedpos;
    a.changed = d_seedpos + K;

    /* ---- ids and norms by output position: the seeds are checked on the host ---- */
    std::vector<uint32_t> h_id((size_t)N + 1);
    std::vector<double> h_norm((size_t)N + 1);
    if (N) {
        LAUNCH(launch_km_docs(ctx->order, ctx->dev_ids, N, d_ids, s));
        HIPCHK(hipMemcpyAsync(h_id.data(), d_ids, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_norm.data(), a.norm, (size_t)N * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    std::vector<uint32_t> clus;   /* the clusterable positions, ascending */
    for (uint32_t j = 0; j < N; ++j)
        if (h_norm[j] > 0.0) clus.push_back(j);
    const uint64_t M = clus.size();
    ki.clusterable = (uint32_t)M;
    if (K > M) return TFIDF_E_INVAL;
    std::vector<uint32_t> h_seedpos(K), h_seed(K);
    if (params->seeds) {
        std::unordered_map<uint32_t, uint32_t> pos_of;
        pos_of.reserve((size_t)N * 2);
        for (uint32_t j = 0; j < N; ++j) pos_of.emplace(h_id[j], j);
        std::unordered_map<uint32_t, int> seen;
        for (uint32_t c = 0; c < K; ++c) {
            const uint32_t id = params->seeds[c];
            const auto it = pos_of.find(id);
            if (it == pos_of.end() || !(h_norm[it->second] > 0.0) || !seen.emplace(id, 1).second) return TFIDF_E_INVAL;
            h_seedpos[c] = it->second;
            h_seed[c] = id;
        }
    } else {
        for (uint32_t c = 0; c < K; ++c) {
            h_seedpos[c] = clus[(size_t)((uint64_t)c * M / K)];
            h_seed[c] = h_id[h_seedpos[c]];
        }
    }

    const size_t KT = (size_t)K * T;
    out->ndocs = N;
    out->k = K;
    out->t = T;
    out->doc = (uint32_t*)calloc((size_t)N + 1, 4);
    out->label = (uint32_t*)calloc((size_t)N + 1, 4);
    out->sim = (double*)calloc((size_t)N + 1, 8);
    out->size = (uint32_t*)calloc((size_t)K + 1, 4);
    out->seed = (uint32_t*)calloc((size_t)K + 1, 4);
    out->nterms = (uint32_t*)calloc((size_t)K + 1, 4);
    out->term = (uint32_t*)calloc(KT + 1, 4);
    out->weight = (double*)calloc(KT + 1, 8);
    out->word_off = (uint64_t*)calloc(KT + 1, 8);
    out->word_bytes = (uint8_t*)calloc(1, 1);
    struct ClustersGuard {   /* an error return leaves *out zeroed */
        tfidf_clusters* c;
        ~ClustersGuard() { if (c) tfidf_clusters_free(c); }
    } guard{out};
    if (!out->doc || !out->label || !out->sim || !out->size || !out->seed || !out->nterms || !out->term || !out->weight ||
        !out->word_off || !out->word_bytes)
        return TFIDF_E_NOMEM;
    memcpy(out->doc, h_id.data(), (size_t)N * 4);
    memcpy(out->seed, h_seed.data(), (size_t)K * 4);

    /* ---- centroid 0 ---- */
    HIPCHK(hipMemcpyAsync(d_seedpos, h_seedpos.data(), (size_t)K * 4, hipMemcpyHostToDevice, s));
    LAUNCH(launch_km_seed(a, s));

    /* ---- the passes ---- */
    uint32_t split = ctx->kmeans_split;
    if (!split) {
        split = (2u * ctx->ncu + K - 1) / K;
        split = split < 1u ? 1u : (split > 64u ? 64u : split);
    }
    ki.split = split;
    int cur = 0;
    bool update_pending = false;
    for (uint32_t it = 1; it <= max_iter; ++it) {
        a.label = d_lab[cur];
        a.prev = it > 1 ? d_lab[cur ^ 1] : nullptr;
        uint32_t changed = 0;
        HIPCHK(hipEventRecord(ctx->ev_k[0], s));
        LAUNCH(launch_km_assign(a, ctx->ncu, s));
        HIPCHK(hipEventRecord(ctx->ev_k[1], s));
        HIPCHK(hipMemcpyAsync(&changed, a.changed, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        ki.ms_assign += ev_ms(ctx->ev_k[0], ctx->ev_k[1]);
        if (update_pending) {
            ki.ms_update += ev_ms(ctx->ev_k[2], ctx->ev_k[3]);
            update_pending = false;
        }
        ki.passes = it;
        if (it > 1 && changed == 0) { out->converged = 1; break; }
        if (it == max_iter) break;
        HIPCHK(hipEventRecord(ctx->ev_k[2], s));
        LAUNCH(launch_km_update(a, split, s));
        HIPCHK(hipEventRecord(ctx->ev_k[3], s));
        ++ki.updates;
        update_pending = true;
        cur ^= 1;
    }
    out->iterations = ki.passes;
    if (N) {
        HIPCHK(hipMemcpyAsync(out->label, a.label, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->sim, a.sim, (size_t)N * 8, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipMemcpyAsync(out->size, a.size, (size_t)K * 4, hipMemcpyDeviceToHost, s));

    /* ---- the clusters' best terms and their words ---- */
    if (T) {
        if (V)
            if (const int rc = ensure_term_meta(ctx)) return rc;
        ENSURE(ctx->km_top, (size_t)K * KM_TOP_SLICES * 16 + (size_t)K * 16 + KT * 8 + (KT + 1) * 8 + KT * 4 + (size_t)K * 4 + 64);
        KmTopArgs ta{};
        ta.C = a.C;
        ta.V = V;
        ta.K = K;
        ta.T = T;
        ta.tlen = ctx->t_len.as<uint32_t>();
        ta.part = ctx->km_top.as<uint64_t>();
        ta.prev = ta.part + (size_t)K * KM_TOP_SLICES * 2;
        ta.weight = ta.prev + (size_t)K * 2;
        ta.wlen = ta.weight + KT;
        ta.term = (uint32_t*)(ta.wlen + KT + 1);
        ta.n = ta.term + KT;
        HIPCHK(hipEventRecord(ctx->ev_k[0], s));
        LAUNCH(launch_km_top(ta, s));
        ctx->arena.used = 0;   /* as tfidf_top_terms: nothing of the result lives in the arena */
        SCAN(scan_excl_u64(ta.wlen, ta.wlen, KT, ctx->arena, s));   /* lengths -> offsets, in place */
        HIPCHK(hipMemcpyAsync(out->word_off, ta.wlen, (KT + 1) * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        const uint64_t wtotal = out->word_off[KT];
        ENSURE(ctx->km_words, wtotal + 16);
        TWordArgs wa{ta.term, ta.wlen, KT, ctx->t_key.as<uint4>(), V, ctx->dev_bytes, ctx->corpus.nbytes,
                     ctx->km_words.as<uint8_t>()};
        LAUNCH(launch_terms_words(wa, s));
        HIPCHK(hipEventRecord(ctx->ev_k[1], s));
        uint8_t* wb = (uint8_t*)realloc(out->word_bytes, (size_t)wtotal + 1);
        if (!wb) return TFIDF_E_NOMEM;
        out->word_bytes = wb;
        HIPCHK(hipMemcpyAsync(out->term, ta.term, KT * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->weight, ta.weight, KT * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(out->nterms, ta.n, (size_t)K * 4, hipMemcpyDeviceToHost, s));
        if (wtotal) HIPCHK(hipMemcpyAsync(wb, ctx->km_words.p, wtotal, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        ki.ms_terms = ev_ms(ctx->ev_k[0], ctx->ev_k[1]);
    } else {
        HIPCHK(hipStreamSynchronize(s));
    }
    ki.ms_total = wall_ms(wall0);
    ctx->kinfo = ki;
    guard.c = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_last_kmeans_info(const tfidf_ctx* ctx, tfidf_kmeans_info* info) {
    return ctx ? copy_info(info, ctx->kinfo) : TFIDF_E_INVAL;
}
