/*
 * engine_dedup.cpp — tfidf_minhash, tfidf_near_dups (dedup.hip).
 * The context and the helpers every engine file shares: engine_ctx.h.
 */
#include "engine_ctx.h"

/* ---------------------------------------------------------- near duplicates ----
 * Over the resident result (dedup.hip).  The host reads the pair offsets once (8 bytes per
 * document): they give n(d), the documents with pairs and with them the capacity check, before
 * any kernel runs.  Then: the h0 table (kept until the next run, prune or import), the signature
 * pass, and for tfidf_near_dups the band keys of all bands in one sort (band-major entries, a
 * stable radix sort of the 64-bit keys: entries of one band with equal keys stay adjacent and in
 * position order, which is the definition's (band key, pos) order band by band), the chain
 * candidates, a second sort that makes them a set, and the verification.  The integers come to
 * the host, which divides, compares with the threshold and builds the groups with dedup_host.c's
 * union-find.  Nothing of the run's result is written. */

namespace {

struct DdPlan {
    uint32_t H = 0, rows = 0, nb = 0;
    uint64_t seed = 0;
    uint32_t N = 0, M = 0;
    std::vector<uint32_t> n;      /* n(d) by position */
    std::vector<uint32_t> live;   /* the positions with pairs, ascending */
};

uint64_t dd_mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

/* parameters, state, offsets, capacity: everything that can refuse the call before a kernel runs */
int dd_begin(tfidf_ctx* ctx, const tfidf_dedup_params* params, DdPlan& pl, tfidf_dedup_info& di) {
    if (tfidf_dedup_check(params) != TFIDF_OK) return TFIDF_E_INVAL;
    if (!ctx->have_result || ctx->model_only) return TFIDF_E_STATE;
    pl.H = params->nhashes ? params->nhashes : TFIDF_DEDUP_DEFAULT_H;
    pl.rows = params->nhashes ? params->rows : TFIDF_DEDUP_DEFAULT_ROWS;
    pl.seed = params->nhashes ? params->seed : TFIDF_DEDUP_DEFAULT_SEED;
    pl.nb = pl.H / pl.rows;
    const uint32_t N = pl.N = ctx->ndocs;
    int rc = call_begin(ctx, ctx->ev_dd);
    if (rc) return rc;
    std::vector<uint64_t> off((size_t)N + 1, 0);
    if (N) {
        HIPCHK(hipMemcpyAsync(off.data(), ctx->out_off.p, ((size_t)N + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    pl.n.assign((size_t)N, 0);
    for (uint32_t j = 0; j < N; ++j) {   /* pair_range's clamp */
        uint64_t b = off[j], e = off[j + 1];
        if (e > ctx->npairs) e = ctx->npairs;
        if (b > e) b = e;
        if (e - b > 0xFFFFFFFFull) return TFIDF_E_CAPACITY;
        pl.n[j] = (uint32_t)(e - b);
        if (e > b) pl.live.push_back(j);
    }
    pl.M = (uint32_t)pl.live.size();
    di.ndocs = N;
    di.nhashes = pl.H;
    di.rows = pl.rows;
    di.clusterable = pl.M;
    di.sig_bytes = (uint64_t)N * pl.H * 4;
    const uint64_t cmax = pl.M ? (uint64_t)pl.nb * (pl.M - 1u) : 0u;
    if (di.sig_bytes + cmax * 16 > ctx->dedup_bytes) return TFIDF_E_CAPACITY;
    if ((uint64_t)pl.nb * pl.M > 0xFFFFFFFFull) return TFIDF_E_CAPACITY;
    return TFIDF_OK;
}

/* the h0 table when it is not this result's, and the signatures into dd_sig */
int dd_signatures(tfidf_ctx* ctx, const DdPlan& pl, tfidf_dedup_info& di) {
    hipStream_t s = ctx->stream;
    const uint32_t N = pl.N, V = ctx->V, H = pl.H;
    ENSURE(ctx->dd_h0, (size_t)V * 8 + 8);
    ENSURE(ctx->dd_sig, (size_t)N * H * 4 + 4);
    ENSURE(ctx->dd_fam, (size_t)DD_MAX_H * 12);
    ENSURE(ctx->dd_misc, (size_t)N * 4 + 64);
    HIPCHK(hipEventRecord(ctx->ev_dd[0], s));
    const bool hashed = !ctx->h0_valid;
    if (hashed) {
        if (V)
            if (const int rc = ensure_term_meta(ctx)) return rc;
        LAUNCH(launch_dd_h0(ctx->t_key.as<uint4>(), ctx->t_len.as<uint32_t>(), V, ctx->dev_bytes, ctx->corpus.nbytes,
                            ctx->dd_h0.as<uint64_t>(), s));
        ctx->h0_valid = true;
    }
    HIPCHK(hipEventRecord(ctx->ev_dd[1], s));
    /* the family: DD_MAX_H multipliers, then DD_MAX_H offsets (the unused ones 0) */
    uint64_t fam[DD_MAX_H + DD_MAX_H / 2] = {};
    uint32_t* fb = (uint32_t*)(fam + DD_MAX_H);
    uint64_t st = pl.seed;
    for (uint32_t i = 0; i < H; ++i) {
        st += 0x9E3779B97F4A7C15ull;
        fam[i] = dd_mix64(st) | 1ull;
        st += 0x9E3779B97F4A7C15ull;
        fb[i] = (uint32_t)(dd_mix64(st) >> 32);
    }
    HIPCHK(hipMemcpyAsync(ctx->dd_fam.p, fam, sizeof fam, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   /* fam is on this frame */
    DdSigArgs a{};
    a.off = ctx->out_off.as<uint64_t>();
    a.npairs = ctx->npairs;
    a.ndocs = N;
    a.H = H;
    a.V = V;
    a.term = ctx->out_term.as<uint32_t>();
    a.h0 = ctx->dd_h0.as<uint64_t>();
    a.fam_a = ctx->dd_fam.as<uint64_t>();
    a.fam_b = (const uint32_t*)(a.fam_a + DD_MAX_H);
    a.sig = ctx->dd_sig.as<uint32_t>();
    a.big_count = ctx->dd_misc.as<uint32_t>();
    a.big_list = a.big_count + 16;
    LAUNCH(launch_dd_sig(a, ctx->ncu, s));
    HIPCHK(hipEventRecord(ctx->ev_dd[2], s));
    uint32_t nbig = 0;
    if (N) HIPCHK(hipMemcpyAsync(&nbig, a.big_count, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    di.big_docs = nbig < N ? nbig : N;
    di.ms_hash = hashed ? ev_ms(ctx->ev_dd[0], ctx->ev_dd[1]) : 0.0;
    di.ms_sig = ev_ms(ctx->ev_dd[1], ctx->ev_dd[2]);
    return TFIDF_OK;
}

/* doc[pos] = the global id, through tfidf_kmeans' kernel into dd_misc's list words */
int dd_doc_ids(tfidf_ctx* ctx, uint32_t N, uint32_t* doc) {
    if (!N) return TFIDF_OK;
    uint32_t* d_ids = ctx->dd_misc.as<uint32_t>() + 16;   /* the big list has been read */
    LAUNCH(launch_km_docs(ctx->order, ctx->dev_ids, N, d_ids, ctx->stream));
    HIPCHK(hipMemcpyAsync(doc, d_ids, (size_t)N * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return TFIDF_OK;
}

int sort_rc(tfidf_ctx* ctx, int where) {
    if (where >= 0) return TFIDF_OK;
    HIPCHK(hipGetLastError());
    return where == -2 ? TFIDF_E_NOMEM : TFIDF_E_HIP;
}

}  // namespace

extern "C" int tfidf_minhash(tfidf_ctx* ctx, const tfidf_dedup_params* params, tfidf_signatures* out) {
    if (!ctx || !params || !out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    const auto wall0 = std::chrono::steady_clock::now();
    DdPlan pl;
    tfidf_dedup_info di{};
    int rc = dd_begin(ctx, params, pl, di);
    if (rc) return rc;
    rc = dd_signatures(ctx, pl, di);
    if (rc) return rc;
    const uint32_t N = pl.N, H = pl.H;
    out->ndocs = N;
    out->nhashes = H;
    out->doc = (uint32_t*)calloc((size_t)N + 1, 4);
    out->npairs = (uint32_t*)calloc((size_t)N + 1, 4);
    out->sig = (uint32_t*)calloc((size_t)N * H + 1, 4);
    struct Guard {   /* an error return leaves *out zeroed */
        tfidf_signatures* p;
        ~Guard() { if (p) tfidf_signatures_free(p); }
    } guard{out};
    if (!out->doc || !out->npairs || !out->sig) return TFIDF_E_NOMEM;
    if (N) memcpy(out->npairs, pl.n.data(), (size_t)N * 4);
    rc = dd_doc_ids(ctx, N, out->doc);
    if (rc) return rc;
    if (N) {
        HIPCHK(hipMemcpyAsync(out->sig, ctx->dd_sig.p, (size_t)N * H * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    di.ms_total = wall_ms(wall0);
    ctx->ddinfo = di;
    guard.p = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_near_dups(tfidf_ctx* ctx, const tfidf_dedup_params* params, tfidf_dups* out) {
    if (!ctx || !params || !out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    const auto wall0 = std::chrono::steady_clock::now();
    DdPlan pl;
    tfidf_dedup_info di{};
    int rc = dd_begin(ctx, params, pl, di);
    if (rc) return rc;
    rc = dd_signatures(ctx, pl, di);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    const uint32_t N = pl.N, H = pl.H, M = pl.M;
    const uint64_t n = (uint64_t)pl.nb * M;                       /* band entries */
    const uint64_t cmax = M ? (uint64_t)pl.nb * (M - 1u) : 0u;    /* chain candidates at most */

    /* ---- the work buffer: two key and two value arrays of n entries, the flags / offsets, two
     * candidate arrays of cmax entries, the positions with pairs.  The verification's output
     * words and its list of big candidates lie over the key arrays, which are free by then. ---- */
    const size_t o_k0 = 0, o_k1 = o_k0 + al256((n + 1) * 8), o_v0 = o_k1 + al256((n + 1) * 8), o_v1 = o_v0 + al256((n + 1) * 4),
                 o_fl = o_v1 + al256((n + 1) * 4), o_c0 = o_fl + al256((n + 2) * 4), o_c1 = o_c0 + al256((cmax + 1) * 8),
                 o_lv = o_c1 + al256((cmax + 1) * 8), o_end = o_lv + al256(((size_t)M + 1) * 4);
    ENSURE(ctx->dd_work, o_end + 256);
    di.work_bytes = o_end;
    uint8_t* W = ctx->dd_work.as<uint8_t>();
    uint64_t* k0 = (uint64_t*)(W + o_k0);
    uint64_t* k1 = (uint64_t*)(W + o_k1);
    uint32_t* v0 = (uint32_t*)(W + o_v0);
    uint32_t* v1 = (uint32_t*)(W + o_v1);
    uint32_t* fl = (uint32_t*)(W + o_fl);
    uint64_t* c0 = (uint64_t*)(W + o_c0);
    uint64_t* c1 = (uint64_t*)(W + o_c1);
    uint32_t* live = (uint32_t*)(W + o_lv);
    {   /* the sorts' histograms and the scans' block sums */
        const uint64_t nt = n / 1024 + 2;
        if (arena_scratch(ctx, (size_t)(256 * nt + 1) * 4 + scan_scratch(256 * nt) + scan_scratch(n + 2) + 16384)) return TFIDF_E_NOMEM;
    }
    uint64_t nraw = 0, ncand = 0;
    HIPCHK(hipEventRecord(ctx->ev_dd[0], s));
    if (M >= 2) {
        HIPCHK(hipMemcpyAsync(live, pl.live.data(), (size_t)M * 4, hipMemcpyHostToDevice, s));
        LAUNCH(launch_dd_bandkeys(ctx->dd_sig.as<uint32_t>(), live, M, H, pl.rows, k0, v0, s));
        int where = radix_sort_u64(k0, v0, k1, v1, n, 0xFFu, ctx->arena, s);
        if ((rc = sort_rc(ctx, where))) return rc;
        const uint64_t* ks = where ? k1 : k0;
        const uint32_t* vs = where ? v1 : v0;
        LAUNCH(launch_dd_runflag(ks, vs, n, M, fl, s));
        SCAN(scan_excl_u32(fl, fl, n, ctx->arena, s));   /* flags -> offsets, in place */
        uint32_t tot = 0;
        HIPCHK(hipMemcpyAsync(&tot, fl + n, 4, hipMemcpyDeviceToHost, s));
        LAUNCH(launch_dd_runwrite(vs, fl, n, M, live, c0, s));
        HIPCHK(hipStreamSynchronize(s));
        nraw = tot;
        if (nraw > cmax) return TFIDF_E_HIP;   /* cannot be: a band chains at most M - 1 */
        if (nraw) {   /* the candidates as a set: positions are below N, so only their bytes vary */
            uint32_t byte_mask = 0;
            for (uint32_t b = 0; b < 4; ++b)
                if (((N - 1u) >> (8 * b)) != 0 || b == 0) byte_mask |= (1u << b) | (1u << (4 + b));
            /* the values ride along unused: the band stage's value arrays */
            where = radix_sort_u64(c0, v0, c1, v1, nraw, byte_mask, ctx->arena, s);
            if ((rc = sort_rc(ctx, where))) return rc;
            uint64_t* cs = where ? c1 : c0;
            uint64_t* cu = where ? c0 : c1;
            LAUNCH(launch_dd_uniqflag(cs, nraw, fl, s));
            SCAN(scan_excl_u32(fl, fl, nraw, ctx->arena, s));
            HIPCHK(hipMemcpyAsync(&tot, fl + nraw, 4, hipMemcpyDeviceToHost, s));
            LAUNCH(launch_dd_uniqwrite(cs, fl, nraw, cu, s));
            HIPCHK(hipStreamSynchronize(s));
            ncand = tot;
            if (ncand > nraw) return TFIDF_E_HIP;
            c0 = cu;   /* the set, ascending: (pos_a, pos_b) order */
        }
    }
    HIPCHK(hipEventRecord(ctx->ev_dd[1], s));

    /* ---- verification ---- */
    std::vector<uint64_t> h_cand((size_t)ncand + 1);
    std::vector<uint32_t> h_shared((size_t)ncand + 1), h_same((size_t)ncand + 1);
    if (ncand) {
        DdVerArgs va{};
        va.cand = c0;
        va.ncand = ncand;
        va.off = ctx->out_off.as<uint64_t>();
        va.npairs = ctx->npairs;
        va.ndocs = N;
        va.H = H;
        va.term = ctx->out_term.as<uint32_t>();
        va.sig = ctx->dd_sig.as<uint32_t>();
        va.shared = (uint32_t*)k0;                 /* 2 * ncand words in n + 1 u64: ncand <= cmax < n */
        va.same = va.shared + ncand;
        va.big_list = (uint32_t*)k1;
        va.big_count = ctx->dd_misc.as<uint32_t>();
        LAUNCH(launch_dd_verify(va, ctx->ncu, s));
        HIPCHK(hipMemcpyAsync(h_cand.data(), c0, (size_t)ncand * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_shared.data(), va.shared, (size_t)ncand * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_same.data(), va.same, (size_t)ncand * 4, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipEventRecord(ctx->ev_dd[2], s));
    HIPCHK(hipStreamSynchronize(s));
    di.ms_bands = ev_ms(ctx->ev_dd[0], ctx->ev_dd[1]);
    di.ms_verify = ev_ms(ctx->ev_dd[1], ctx->ev_dd[2]);

    /* ---- the division, the threshold, the groups: on the host over the fetched integers ---- */
    uint64_t ne = 0;
    for (uint64_t c = 0; c < ncand; ++c) {
        const uint32_t a = (uint32_t)(h_cand[c] >> 32), b = (uint32_t)h_cand[c];
        if (a >= N || b >= N) return TFIDF_E_HIP;
        const uint32_t uni = pl.n[a] + pl.n[b] - h_shared[c];
        if ((double)h_shared[c] / (double)uni >= params->threshold) ++ne;
    }
    out->ndocs = N;
    out->ncand = ncand;
    out->nedges = ne;
    out->doc = (uint32_t*)calloc((size_t)N + 1, 4);
    out->group = (uint32_t*)calloc((size_t)N + 1, 4);
    out->a_pos = (uint32_t*)calloc((size_t)ne + 1, 4);
    out->b_pos = (uint32_t*)calloc((size_t)ne + 1, 4);
    out->a_doc = (uint32_t*)calloc((size_t)ne + 1, 4);
    out->b_doc = (uint32_t*)calloc((size_t)ne + 1, 4);
    out->shared = (uint32_t*)calloc((size_t)ne + 1, 4);
    out->uni = (uint32_t*)calloc((size_t)ne + 1, 4);
    out->same = (uint32_t*)calloc((size_t)ne + 1, 4);
    out->jaccard = (double*)calloc((size_t)ne + 1, 8);
    struct Guard {   /* an error return leaves *out zeroed */
        tfidf_dups* p;
        ~Guard() { if (p) tfidf_dups_free(p); }
    } guard{out};
    if (!out->doc || !out->group || !out->a_pos || !out->b_pos || !out->a_doc || !out->b_doc || !out->shared || !out->uni ||
        !out->same || !out->jaccard)
        return TFIDF_E_NOMEM;
    rc = dd_doc_ids(ctx, N, out->doc);
    if (rc) return rc;
    uint64_t k = 0;
    for (uint64_t c = 0; c < ncand; ++c) {
        const uint32_t a = (uint32_t)(h_cand[c] >> 32), b = (uint32_t)h_cand[c];
        const uint32_t uni = pl.n[a] + pl.n[b] - h_shared[c];
        const double jac = (double)h_shared[c] / (double)uni;
        if (!(jac >= params->threshold)) continue;
        out->a_pos[k] = a;
        out->b_pos[k] = b;
        out->a_doc[k] = out->doc[a];
        out->b_doc[k] = out->doc[b];
        out->shared[k] = h_shared[c];
        out->uni[k] = uni;
        out->same[k] = h_same[c];
        out->jaccard[k] = jac;
        ++k;
    }
    rc = tfidf_dedup_groups(N, out->a_pos, out->b_pos, ne, out->group, &out->ngroups);
    if (rc) return rc;
    di.ncand = ncand;
    di.nedges = ne;
    di.ngroups = out->ngroups;
    di.ms_total = wall_ms(wall0);
    ctx->ddinfo = di;
    guard.p = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_last_dedup_info(const tfidf_ctx* ctx, tfidf_dedup_info* info) {
    return ctx ? copy_info(info, ctx->ddinfo) : TFIDF_E_INVAL;
}
