/*
 * engine_similar.cpp — tfidf_similar and the two halves of tfidf_group_similar (similar.hip).
 * The context and the helpers every engine file shares: engine_ctx.h.
 */
#include "engine_ctx.h"

/* ----------------------------------------------------------------- similar ----
 * Top-k similar documents over the resident result (similar.hip).  The norms are computed by
 * the first call after a run.  The rows (every output position, or the positions of the
 * requested ids) are cut into groups of up to SG_MAX under the accumulator budget; a group is
 * a postings table (masks, offsets, weights) built on the device from the rows' vectors, one scan of the pairs that
 * leaves sim and the shared-term count per (row, output position), the top-k rounds of
 * tfidf_query over them, and a lookup of the neighbours' positions for their shared counts.
 * Nothing of the run's result is written. */

extern "C" void tfidf_neighbors_free(tfidf_neighbors* n) {
    if (!n) return;
    free(n->doc); free(n->pos); free(n->npairs); free(n->norm); free(n->nmatch); free(n->nnb);
    free(n->nb_doc); free(n->nb_shared); free(n->nb_score);
    memset(n, 0, sizeof(*n));
}

static int neighbors_alloc(tfidf_neighbors* out, uint32_t R, uint32_t k) {
    const size_t RK = (size_t)R * k;
    memset(out, 0, sizeof(*out));
    out->ndocs = R;
    out->k = k;
    out->doc = (uint32_t*)calloc((size_t)R + 1, 4);
    out->pos = (uint32_t*)calloc((size_t)R + 1, 4);
    out->npairs = (uint64_t*)calloc((size_t)R + 1, 8);
    out->norm = (double*)calloc((size_t)R + 1, 8);
    out->nmatch = (uint64_t*)calloc((size_t)R + 1, 8);
    out->nnb = (uint32_t*)calloc((size_t)R + 1, 4);
    out->nb_doc = (uint32_t*)calloc(RK + 1, 4);
    out->nb_shared = (uint32_t*)calloc(RK + 1, 4);
    out->nb_score = (double*)calloc(RK + 1, 8);
    if (!out->doc || !out->pos || !out->npairs || !out->norm || !out->nmatch || !out->nnb || !out->nb_doc ||
        !out->nb_shared || !out->nb_score) {
        tfidf_neighbors_free(out);
        return TFIDF_E_NOMEM;
    }
    return TFIDF_OK;
}

namespace {
struct NeighborsGuard {   /* an error return leaves *out zeroed */
    tfidf_neighbors* n;
    ~NeighborsGuard() { if (n) tfidf_neighbors_free(n); }
};
/* the call's rows on the device (sm_rows) */
struct SimCall {
    uint32_t R = 0;
    uint64_t* rb = nullptr;
    uint64_t* re = nullptr;
    double* rnorm = nullptr;
    double* rsq = nullptr;
    uint32_t* rpos = nullptr;
    uint32_t* rid = nullptr;
};
}  // namespace

static int sim_layout(tfidf_ctx* ctx, uint32_t R, SimCall& c) {
    ENSURE(ctx->sm_rows, (size_t)R * 40 + 64);
    c.R = R;
    c.rb = ctx->sm_rows.as<uint64_t>();
    c.re = c.rb + R;
    c.rnorm = (double*)(c.re + R);
    c.rsq = c.rnorm + R;
    c.rpos = (uint32_t*)(c.rsq + R);
    c.rid = c.rpos + R;
    return TFIDF_OK;
}

/* sq and norm by output position, once per run */
int sim_norms(tfidf_ctx* ctx, tfidf_similar_info& si) {
    if (ctx->norm_valid) return TFIDF_OK;
    hipStream_t s = ctx->stream;
    const uint32_t N = ctx->ndocs;
    ENSURE(ctx->sm_norm, (size_t)N * 16 + 16);
    HIPCHK(hipEventRecord(ctx->ev_s[4], s));
    LAUNCH(launch_sim_norms(ctx->out_off.as<uint64_t>(), ctx->out_score.as<double>(), N, ctx->npairs,
                         ctx->sm_norm.as<double>(), ctx->sm_norm.as<double>() + N, s));
    HIPCHK(hipEventRecord(ctx->ev_s[5], s));
    HIPCHK(hipStreamSynchronize(s));
    si.ms_norms = ev_ms(ctx->ev_s[4], ctx->ev_s[5]);
    ctx->norm_valid = true;
    return TFIDF_OK;
}

/* the rows of a call from the resident result: positions (ids looked up, or every position),
 * vector ranges, norms, ids; copied to the host arrays (R entries each) */
static int sim_resident_rows(tfidf_ctx* ctx, const uint32_t* doc_ids, uint32_t R, SimCall& c, uint64_t* h_rb,
                             uint64_t* h_re, double* h_norm, uint32_t* h_pos, uint32_t* h_id) {
    hipStream_t s = ctx->stream;
    int rc = sim_layout(ctx, R, c);
    if (rc) return rc;
    if (!R) return TFIDF_OK;
    if (doc_ids) {
        rc = lookup_ids(ctx, ctx->sm_ids, doc_ids, R, c.rpos);
        if (rc) return rc;
    }
    SimRowArgs ra{};
    ra.out_off = ctx->out_off.as<uint64_t>();
    ra.order = ctx->order;
    ra.doc_ids = ctx->dev_ids;
    ra.sq = ctx->sm_norm.as<double>();
    ra.norm = ra.sq + ctx->ndocs;
    ra.ndocs = ctx->ndocs;
    ra.npairs = ctx->npairs;
    ra.pos = doc_ids ? c.rpos : nullptr;   /* read and rewritten by the same thread */
    ra.nrows = R;
    ra.rb = c.rb;
    ra.re = c.re;
    ra.rnorm = c.rnorm;
    ra.rsq = c.rsq;
    ra.rpos = c.rpos;
    ra.rid = c.rid;
    LAUNCH(launch_sim_rows(ra, s));
    HIPCHK(hipMemcpyAsync(h_rb, c.rb, (size_t)R * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_re, c.re, (size_t)R * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_norm, c.rnorm, (size_t)R * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_pos, c.rpos, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_id, c.rid, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return TFIDF_OK;
}

/* the groups of a call: row i's vector is entries [h_rb[i], h_re[i]) of d_term / d_score
 * (nentries of them; terms >= V are words this shard does not hold).  Fills nmatch, nnb and
 * nb_* of `out`. */
static int similar_groups(tfidf_ctx* ctx, const SimCall& c, uint32_t k, const uint32_t* d_term, const double* d_score,
                          uint64_t nentries, const uint64_t* h_rb, const uint64_t* h_re, tfidf_neighbors* out,
                          tfidf_similar_info& si) {
    hipStream_t s = ctx->stream;
    const uint32_t N = ctx->ndocs, V = ctx->V, R = c.R;
    const TopkPlan plan = topk_plan(N, k, R, ctx->query_acc_bytes);
    const uint64_t G = plan.G;
    si.group_rows = (uint32_t)G;
    si.acc_bytes = G * plan.per_q;
    if (!N || !V || !R) return TFIDF_OK;
    uint64_t maxP = 0;   /* the largest group's postings */
    for (uint32_t g0 = 0; g0 < R; g0 += (uint32_t)G) {
        uint64_t pg = 0;
        for (uint32_t i = g0; i < R && i < g0 + G; ++i) pg += h_re[i] - h_rb[i];
        if (pg > maxP) maxP = pg;
    }
    if (maxP > 0x7FFFFFFFull) return TFIDF_E_CAPACITY;
    if (!maxP) return TFIDF_OK;   /* every row is empty */
    const int erc = topk_ensure(ctx, plan, N);
    if (erc) return erc;
    ENSURE(ctx->sm_mask, ((size_t)V + 2) * 8);
    ENSURE(ctx->sm_cnt, ((size_t)V + 2) * 4);
    ENSURE(ctx->sm_off, ((size_t)V + 2) * 4);
    ENSURE(ctx->sm_pw, (size_t)maxP * 8 + 16);
    ENSURE(ctx->sm_res, (size_t)G * k * 8 + 16);
    std::vector<uint64_t> h_s((size_t)G * k), h_nm(G);
    std::vector<uint32_t> h_id((size_t)G * k), h_sh((size_t)G * k), h_n(G);
    uint32_t* res_pos = ctx->sm_res.as<uint32_t>();
    uint32_t* res_sh = res_pos + (size_t)G * k;
    for (uint32_t g0 = 0; g0 < R; g0 += (uint32_t)G) {
        const uint32_t gn = R - g0 < G ? R - g0 : (uint32_t)G;
        uint64_t pg = 0;
        for (uint32_t i = g0; i < g0 + gn; ++i) pg += h_re[i] - h_rb[i];
        if (!pg) continue;   /* empty rows: no neighbours */
        ++si.ngroups;
        /* ---- the group's table ---- */
        SimTabArgs ta{};
        ta.term = d_term;
        ta.score = d_score;
        ta.rb = c.rb + g0;
        ta.re = c.re + g0;
        ta.nentries = nentries;
        ta.nrows = gn;
        ta.V = V;
        ta.mask = ctx->sm_mask.as<uint64_t>();
        ta.cnt = ctx->sm_cnt.as<uint32_t>();
        ta.post_off = ctx->sm_off.as<uint32_t>();
        ta.post_w = ctx->sm_pw.as<double>();
        ta.post_cap = (uint32_t)maxP;
        HIPCHK(hipEventRecord(ctx->ev_s[0], s));
        HIPCHK(hipMemsetAsync(ta.mask, 0, ((size_t)V + 1) * 8, s));
        LAUNCH(launch_sim_mark(ta, s));
        ctx->arena.used = 0;   /* as format_prepare: nothing of the result lives in the arena */
        SCAN(scan_excl_u32(ta.cnt, ctx->sm_off.as<uint32_t>(), V, ctx->arena, s));
        LAUNCH(launch_sim_fill(ta, s));
        HIPCHK(hipEventRecord(ctx->ev_s[1], s));
        /* ---- one scan of the pairs ---- */
        unsigned long long* d_nm = ctx->q_misc.as<unsigned long long>();
        HIPCHK(hipMemsetAsync(d_nm, 0, (size_t)G * 8, s));
        SimScoreArgs sa{};
        sa.out_off = ctx->out_off.as<uint64_t>();
        sa.out_term = ctx->out_term.as<uint32_t>();
        sa.out_score = ctx->out_score.as<double>();
        sa.ndocs = N;
        sa.npairs = ctx->npairs;
        sa.V = V;
        sa.mask = ta.mask;
        sa.post_off = ta.post_off;
        sa.post_w = ta.post_w;
        sa.post_cap = ta.post_cap;
        sa.nq = gn;
        sa.rnorm = c.rnorm + g0;
        sa.rpos = c.rpos + g0;
        sa.dnorm = ctx->sm_norm.as<double>() + N;
        sa.acc = ctx->q_acc.as<double>();
        sa.cnt = ctx->q_cnt.as<uint32_t>();
        sa.big_list = ctx->q_big.as<uint32_t>();
        sa.big_count = (uint32_t*)(d_nm + G);
        LAUNCH(launch_sim_score(sa, ctx->ncu, s));
        HIPCHK(hipEventRecord(ctx->ev_s[2], s));
        /* ---- top-k rounds (tfidf_query's) ---- */
        TopkCand res{};
        int rc = topk_rounds(ctx, plan, sa.acc, sa.cnt, N, k, gn, d_nm, &res);
        if (rc) return rc;
        /* ---- the neighbours' positions and shared-term counts ---- */
        TLookupArgs la{res.id, gn * k, ctx->order, ctx->dev_ids, N, res_pos};
        LAUNCH(launch_terms_lookup(la, s));
        LAUNCH(launch_sim_shared(sa.cnt, res_pos, res.n, gn, k, N, res_sh, s));
        HIPCHK(hipEventRecord(ctx->ev_s[3], s));
        uint32_t nbig = 0;
        HIPCHK(hipMemcpyAsync(h_sh.data(), res_sh, (size_t)gn * k * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&nbig, sa.big_count, 4, hipMemcpyDeviceToHost, s));
        rc = topk_read_back(ctx, res, d_nm, gn, k, h_s.data(), h_id.data(), h_n.data(), h_nm.data());
        if (rc) return rc;
        si.ms_table += ev_ms(ctx->ev_s[0], ctx->ev_s[1]);
        si.ms_score += ev_ms(ctx->ev_s[1], ctx->ev_s[2]);
        si.ms_topk += ev_ms(ctx->ev_s[2], ctx->ev_s[3]);
        si.big_docs = nbig < N ? nbig : N;
        for (uint32_t q = 0; q < gn; ++q) {
            const uint32_t n = h_n[q] < k ? h_n[q] : k;
            out->nnb[g0 + q] = n;
            out->nmatch[g0 + q] = h_nm[q];
            for (uint32_t i = 0; i < n; ++i) {
                const size_t o = (size_t)(g0 + q) * k + i, e = (size_t)q * k + i;
                out->nb_doc[o] = h_id[e];
                out->nb_shared[o] = h_sh[e];
                memcpy(&out->nb_score[o], &h_s[e], 8);
            }
        }
    }
    return TFIDF_OK;
}

extern "C" int tfidf_similar(tfidf_ctx* ctx, const uint32_t* doc_ids, uint32_t ndocs, uint32_t k, tfidf_neighbors* out) {
    if (!ctx || !out) return TFIDF_E_INVAL;
    if (k == 0 || k > TFIDF_SIMILAR_MAX_K) return TFIDF_E_INVAL;
    if (!ctx->have_result) return TFIDF_E_STATE;
    const auto wall0 = std::chrono::steady_clock::now();
    int rc = call_begin(ctx, ctx->ev_s);
    if (rc) return rc;
    const uint32_t R = doc_ids ? ndocs : ctx->ndocs;
    rc = neighbors_alloc(out, R, k);
    if (rc) return rc;
    NeighborsGuard guard{out};
    tfidf_similar_info si{};
    si.rows = R;
    si.k = k;
    rc = sim_norms(ctx, si);
    if (rc) return rc;
    SimCall c;
    std::vector<uint64_t> h_rb((size_t)R + 1), h_re((size_t)R + 1);
    std::vector<uint32_t> h_id((size_t)R + 1);
    rc = sim_resident_rows(ctx, doc_ids, R, c, h_rb.data(), h_re.data(), out->norm, out->pos, h_id.data());
    if (rc) return rc;
    for (uint32_t i = 0; i < R; ++i) {
        out->doc[i] = doc_ids ? doc_ids[i] : h_id[i];
        out->npairs[i] = h_re[i] - h_rb[i];
    }
    rc = similar_groups(ctx, c, k, ctx->out_term.as<uint32_t>(), ctx->out_score.as<double>(), ctx->npairs, h_rb.data(),
                        h_re.data(), out, si);
    if (rc) return rc;
    si.ms_total = wall_ms(wall0);
    ctx->sinfo = si;
    guard.n = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_last_similar_info(const tfidf_ctx* ctx, tfidf_similar_info* info) {
    return ctx ? copy_info(info, ctx->sinfo) : TFIDF_E_INVAL;
}

/* the rows' vectors as (word bytes, score): the word gather of tfidf_top_terms over every pair
 * of the rows' documents (short terms from their key, long terms from the corpus) */
int tfidf_ctx_similar_export(tfidf_ctx* ctx, const uint32_t* doc_ids, uint32_t ndocs, SimExport* e) {
    if (!ctx || !e) return TFIDF_E_INVAL;
    if (!ctx->have_result) return TFIDF_E_STATE;
    int rc = call_begin(ctx, ctx->ev_s);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    const uint32_t V = ctx->V;
    const uint32_t R = doc_ids ? ndocs : ctx->ndocs;
    tfidf_similar_info si{};
    rc = sim_norms(ctx, si);
    if (rc) return rc;
    if (V && (rc = ensure_term_meta(ctx)) != 0) return rc;
    SimCall c;
    std::vector<uint64_t> h_rb((size_t)R + 1), h_re((size_t)R + 1);
    e->id.assign((size_t)R + 1, 0);
    e->pos.assign((size_t)R + 1, 0);
    e->norm.assign((size_t)R + 1, 0.0);
    e->npairs.assign((size_t)R + 1, 0);
    e->voff.assign((size_t)R + 1, 0);
    rc = sim_resident_rows(ctx, doc_ids, R, c, h_rb.data(), h_re.data(), e->norm.data(), e->pos.data(), e->id.data());
    if (rc) return rc;
    for (uint32_t i = 0; i < R; ++i) {
        if (doc_ids) e->id[i] = doc_ids[i];
        e->npairs[i] = h_re[i] - h_rb[i];
        e->voff[i + 1] = e->voff[i] + e->npairs[i];
    }
    const uint64_t P = e->voff[R];
    e->woff.assign((size_t)P + 1, 0);
    e->score.assign((size_t)P + 1, 0.0);
    e->wbytes.clear();
    if (!P) return TFIDF_OK;
    ENSURE(ctx->sm_xoff, ((size_t)R + 1) * 8);
    ENSURE(ctx->sm_xterm, (size_t)P * 4 + 16);
    ENSURE(ctx->sm_xscore, (size_t)P * 8 + 16);
    ENSURE(ctx->sm_xwoff, (size_t)P * 8 + 16);
    HIPCHK(hipMemcpyAsync(ctx->sm_xoff.p, e->voff.data(), ((size_t)R + 1) * 8, hipMemcpyHostToDevice, s));
    SimExportArgs xa{};
    xa.out_term = ctx->out_term.as<uint32_t>();
    xa.out_score = ctx->out_score.as<double>();
    xa.tlen = ctx->t_len.as<uint32_t>();
    xa.V = V;
    xa.rb = c.rb;
    xa.re = c.re;
    xa.eoff = ctx->sm_xoff.as<uint64_t>();
    xa.nrows = R;
    xa.term = ctx->sm_xterm.as<uint32_t>();
    xa.score = ctx->sm_xscore.as<double>();
    xa.wlen = ctx->sm_xwoff.as<uint64_t>();
    LAUNCH(launch_sim_export(xa, s));
    ctx->arena.used = 0;
    SCAN(scan_excl_u64(xa.wlen, xa.wlen, P, ctx->arena, s));   /* lengths -> offsets, in place */
    HIPCHK(hipMemcpyAsync(e->woff.data(), xa.wlen, ((size_t)P + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(e->score.data(), xa.score, (size_t)P * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const uint64_t wtotal = e->woff[P];
    e->wbytes.assign((size_t)wtotal + 1, 0);
    ENSURE(ctx->sm_xwords, (size_t)wtotal + 16);
    TWordArgs wa{xa.term, xa.wlen, P, ctx->t_key.as<uint4>(), V, ctx->dev_bytes, ctx->corpus.nbytes,
                 ctx->sm_xwords.as<uint8_t>()};
    LAUNCH(launch_terms_words(wa, s));
    if (wtotal) HIPCHK(hipMemcpyAsync(e->wbytes.data(), ctx->sm_xwords.p, (size_t)wtotal, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return TFIDF_OK;
}

int tfidf_ctx_similar_ext(tfidf_ctx* ctx, const SimExport* rows, uint32_t k, tfidf_neighbors* out) {
    if (!ctx || !rows || !out) return TFIDF_E_INVAL;
    if (k == 0 || k > TFIDF_SIMILAR_MAX_K || rows->voff.empty()) return TFIDF_E_INVAL;
    if (!ctx->have_result) return TFIDF_E_STATE;
    const auto wall0 = std::chrono::steady_clock::now();
    int rc = call_begin(ctx, ctx->ev_s);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    const uint32_t R = (uint32_t)(rows->voff.size() - 1);
    const uint64_t P = rows->voff[R];
    if (rows->id.size() < R || rows->norm.size() < R || rows->woff.size() < P + 1 || rows->score.size() < P ||
        rows->wbytes.size() < rows->woff[P])
        return TFIDF_E_INVAL;
    if (P > 0xFFFFFFFFull) return TFIDF_E_CAPACITY;   /* one lookup lane per exported word */
    rc = neighbors_alloc(out, R, k);
    if (rc) return rc;
    NeighborsGuard guard{out};
    tfidf_similar_info si{};
    si.rows = R;
    si.k = k;
    rc = sim_norms(ctx, si);
    if (rc) return rc;
    SimCall c;
    rc = sim_layout(ctx, R, c);
    if (rc) return rc;
    for (uint32_t i = 0; i < R; ++i) out->doc[i] = rows->id[i];
    if (R && P && ctx->ndocs && ctx->V) {
        /* the rows' own documents by id (another shard's: no position here) */
        rc = lookup_ids(ctx, ctx->sm_ids, rows->id.data(), R, c.rpos);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(c.rb, rows->voff.data(), (size_t)R * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(c.re, rows->voff.data() + 1, (size_t)R * 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(c.rnorm, rows->norm.data(), (size_t)R * 8, hipMemcpyHostToDevice, s));
        /* the words -> this shard's term ranks (k_query_lookup; QUERY_NO_TERM: not in its vocabulary) */
        const size_t offb = ((size_t)P + 1) * 8;
        const uint64_t wtotal = rows->woff[P];
        ENSURE(ctx->q_terms, offb + wtotal + 16);
        ENSURE(ctx->q_rank, (size_t)P * 4 + 4);
        ENSURE(ctx->sm_escore, (size_t)P * 8 + 16);
        HIPCHK(hipMemcpyAsync(ctx->q_terms.p, rows->woff.data(), offb, hipMemcpyHostToDevice, s));
        if (wtotal)
            HIPCHK(hipMemcpyAsync(ctx->q_terms.as<uint8_t>() + offb, rows->wbytes.data(), wtotal, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(ctx->sm_escore.p, rows->score.data(), (size_t)P * 8, hipMemcpyHostToDevice, s));
        QLookupArgs la{};
        la.tbytes = ctx->q_terms.as<uint8_t>() + offb;
        la.toff = ctx->q_terms.as<uint64_t>();
        la.nterms = (uint32_t)P;
        la.vkeys = ctx->vkeys.as<uint4>();
        la.vrep = ctx->vrep.as<uint64_t>();
        la.mask = ctx->vcap - 1;
        la.home = ~1ull;
        la.rank_of_slot = ctx->rank_of_slot.as<uint32_t>();
        la.corpus = ctx->dev_bytes;
        la.corpus_bytes = ctx->corpus.nbytes;
        la.V = ctx->V;
        la.rank_out = ctx->q_rank.as<uint32_t>();
        LAUNCH(launch_query_lookup(la, s));
        HIPCHK(hipStreamSynchronize(s));   /* the host arrays are the caller's */
        rc = similar_groups(ctx, c, k, ctx->q_rank.as<uint32_t>(), ctx->sm_escore.as<double>(), P, rows->voff.data(),
                            rows->voff.data() + 1, out, si);
        if (rc) return rc;
    }
    si.ms_total = wall_ms(wall0);
    ctx->sinfo = si;
    guard.n = nullptr;
    return TFIDF_OK;
}
