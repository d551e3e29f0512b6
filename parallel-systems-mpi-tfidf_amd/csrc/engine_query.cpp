/*
 * engine_query.cpp — tfidf_query, tfidf_query_bm25, tfidf_query_clauses and the top-k driver they
 * share with tfidf_similar (query.hip, bm25.hip).
 * The context and the helpers every engine file shares: engine_ctx.h.
 */
#include <float.h>
#include <math.h>

#include <algorithm>
#include <string>
#include <unordered_map>

#include "engine_ctx.h"

/* ------------------------------------------------------------------- query ----
 * Top-k retrieval over the resident result (query.hip).  The host tokenises the batch
 * (fscanf("%s") tokens, terms cut at their first NUL: TFIDF.c:141-147,152), the device maps
 * the batch's distinct terms to term ranks, and every group of queries takes one pass over
 * the pairs and a few top-k rounds.  The vocabulary table is only read: no stage after K1
 * writes vkeys or vrep (the vocabulary stage reads them into its own sort keys and writes
 * rank_of_slot at the used slots; fetch and format read them again), and all three K1
 * kernels insert from the pair-aligned home (vocab_insert's default, VS_HOME). */

static inline bool query_is_ws(uint8_t c) { return c == 0x20u || (c >= 0x09u && c <= 0x0Du); }

extern "C" void tfidf_hits_free(tfidf_hits* h) {
    if (!h) return;
    free(h->nhits); free(h->nmatch); free(h->nterms_found); free(h->doc); free(h->score);
    memset(h, 0, sizeof(*h));
}

/* the exact sum of doc_size over the context's documents (BM25's default avgdl): a host sum
 * over one copy, kept until the next run */
int tfidf_ctx_bm25_lengths(tfidf_ctx* ctx, uint64_t* L, uint64_t* n) {
    if (!ctx || !L || !n) return TFIDF_E_INVAL;
    if (!ctx->have_result) return TFIDF_E_STATE;
    if (!ctx->bm25_L_valid) {
        HIPCHK(hipSetDevice(ctx->device));
        std::vector<uint32_t> dsz(ctx->ndocs);
        if (ctx->ndocs) {
            HIPCHK(hipMemcpyAsync(dsz.data(), ctx->doc_size.p, (size_t)ctx->ndocs * 4, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
        }
        uint64_t sum = 0;
        for (uint32_t v : dsz) sum += v;
        ctx->bm25_L = sum;
        ctx->bm25_L_valid = true;
    }
    *L = ctx->bm25_L;
    *n = ctx->ndocs;
    return TFIDF_OK;
}

int tfidf_bm25_params_check(const tfidf_bm25_params* p, Bm25Call* out) {
    Bm25Call c{TFIDF_BM25_DEFAULT_K1, TFIDF_BM25_DEFAULT_B, 0.0};
    if (p) {
        if (p->size < sizeof(tfidf_bm25_params)) return TFIDF_E_INVAL;
        c = Bm25Call{p->k1, p->b, p->avgdl};
    }
    /* written so that a NaN fails every test */
    if (!(c.k1 >= 0.0 && c.k1 <= TFIDF_BM25_MAX_K1)) return TFIDF_E_INVAL;
    if (!(c.b >= 0.0 && c.b <= 1.0)) return TFIDF_E_INVAL;
    if (!(c.avgdl == 0.0 || (c.avgdl >= TFIDF_BM25_MIN_AVGDL && c.avgdl <= DBL_MAX))) return TFIDF_E_INVAL;
    *out = c;
    return TFIDF_OK;
}

/* ---- what tfidf_query, tfidf_query_bm25 and tfidf_similar share on the host: the group
 * budget, the top-k rounds over a group's dense accumulators, the read-back of the result ---- */
static_assert(SG_MAX == QG_MAX, "queries and rows share one group budget");
TopkPlan topk_plan(uint32_t N, uint32_t k, uint32_t rows, uint64_t acc_bytes) {
    TopkPlan p{};
    p.nsl0 = ((uint64_t)N + QT_SLICE - 1) / QT_SLICE;
    p.per_q = (uint64_t)N * 12 + 2 * (p.nsl0 * k * 12 + p.nsl0 * 4) + 8;
    p.G = acc_bytes / p.per_q;
    p.G = p.G < 1 ? 1 : (p.G > QG_MAX ? QG_MAX : p.G);
    if (p.G > rows) p.G = rows ? rows : 1;
    p.cand_el = p.G * p.nsl0 * k;
    return p;
}
/* the plan's buffers: apart from the budget, because a call with nothing to scan allocates nothing */
int topk_ensure(tfidf_ctx* ctx, const TopkPlan& p, uint32_t N) {
    ENSURE(ctx->q_acc, p.G * N * 8);
    ENSURE(ctx->q_cnt, p.G * N * 4);
    ENSURE(ctx->q_big, (size_t)N * 4 + 4);
    ENSURE(ctx->q_cand0, p.cand_el * 12 + p.G * p.nsl0 * 4);
    ENSURE(ctx->q_cand1, p.cand_el * 12 + p.G * p.nsl0 * 4);
    ENSURE(ctx->q_misc, p.G * 8 + 16);
    return TFIDF_OK;
}
static TopkCand topk_cand(tfidf_ctx* ctx, const TopkPlan& p, int c) {
    uint64_t* s = (c ? ctx->q_cand1 : ctx->q_cand0).as<uint64_t>();
    uint32_t* id = (uint32_t*)(s + p.cand_el);
    return TopkCand{s, id, id + p.cand_el};
}
/* the top-k rounds of a group of gn queries (rows): the accumulators' slices, then the slices'
 * lists until one is left per query: row q = entries [q * k, q * k + n[q]) of *res */
int topk_rounds(tfidf_ctx* ctx, const TopkPlan& p, const double* acc, const uint32_t* cnt, uint32_t N, uint32_t k,
                uint32_t gn, unsigned long long* d_nm, TopkCand* res, const uint32_t* need) {
    hipStream_t s = ctx->stream;
    int cur = 0;
    TopkCand o = topk_cand(ctx, p, cur);
    QTopkArgs ta{};
    ta.acc = acc;
    ta.cnt = cnt;
    ta.need = need;
    ta.order = ctx->order;
    ta.doc_ids = ctx->dev_ids;
    ta.n_in = N;
    ta.kk = k;
    ta.out_s = o.s;
    ta.out_id = o.id;
    ta.out_n = o.n;
    ta.out_slices = (uint32_t)p.nsl0;
    ta.nmatch = d_nm;
    LAUNCH(launch_query_topk(ta, gn, s));
    uint64_t nsl = p.nsl0;
    while (nsl > 1) {
        const TopkCand in = o;
        QTopkArgs tb{};
        tb.in_s = in.s;
        tb.in_id = in.id;
        tb.in_n = in.n;
        tb.in_slices = (uint32_t)nsl;
        tb.n_in = nsl * k;
        tb.kk = k;
        nsl = (tb.n_in + QT_SLICE - 1) / QT_SLICE;
        cur ^= 1;
        o = topk_cand(ctx, p, cur);
        tb.out_s = o.s;
        tb.out_id = o.id;
        tb.out_n = o.n;
        tb.out_slices = (uint32_t)nsl;
        tb.nmatch = d_nm;
        LAUNCH(launch_query_topk(tb, gn, s));
    }
    *res = o;
    return TFIDF_OK;
}
/* the result of topk_rounds and the match counts on the host; waits for the stream */
int topk_read_back(tfidf_ctx* ctx, const TopkCand& res, const unsigned long long* d_nm, uint32_t gn, uint32_t k,
                   uint64_t* h_s, uint32_t* h_id, uint32_t* h_n, uint64_t* h_nm) {
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(h_s, res.s, (size_t)gn * k * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_id, res.id, (size_t)gn * k * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_n, res.n, (size_t)gn * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_nm, d_nm, (size_t)gn * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return TFIDF_OK;
}

/* a batch as tfidf_query takes it */
static int queries_check(const tfidf_queries* qs) {
    if (!qs || qs->nqueries > TFIDF_QUERY_MAX_QUERIES) return TFIDF_E_INVAL;
    const uint32_t nq = qs->nqueries;
    if (nq && !qs->q_off) return TFIDF_E_INVAL;
    for (uint32_t q = 0; q < nq; ++q)
        if (qs->q_off[q] > qs->q_off[q + 1]) return TFIDF_E_INVAL;
    if (nq && (qs->q_off[nq] > qs->nbytes || (qs->q_off[nq] > qs->q_off[0] && !qs->bytes))) return TFIDF_E_INVAL;
    return TFIDF_OK;
}

/* f(term bytes, length) for every token of query q of the batch, in order: tokens are maximal
 * runs of non-whitespace, a term is the token up to its first NUL (strcmp semantics) */
template <class F>
static void for_each_term(const tfidf_queries* qs, uint32_t q, F f) {
    const uint8_t* b = qs->bytes;
    const uint64_t e = qs->q_off[q + 1];
    for (uint64_t i = qs->q_off[q]; i < e;) {
        while (i < e && query_is_ws(b[i])) ++i;
        if (i >= e) break;
        const uint64_t t0 = i;
        while (i < e && !query_is_ws(b[i])) ++i;
        uint64_t tl = 0;
        while (t0 + tl < i && b[t0 + tl] != 0) ++tl;
        f((const char*)b + t0, (size_t)tl);
    }
}

/* with a clause plan (cl) qs is unused: the batch is the plan's three texts, a posting carries
 * the increment of its clause kinds and the first top-k round tests the count word against
 * need[q]; everything else is the one path */
int tfidf_ctx_query(tfidf_ctx* ctx, const tfidf_queries* qs, uint32_t k, tfidf_hits* out, std::vector<uint8_t>* found_out,
                    std::vector<uint64_t>* found_off_out, const Bm25Call* bm, const ClausePlan* cl) {
    if (!ctx || (!qs && !cl) || !out) return TFIDF_E_INVAL;
    if (k == 0 || k > TFIDF_QUERY_MAX_K) return TFIDF_E_INVAL;
    if (!cl) {
        if (const int rc = queries_check(qs)) return rc;
    }
    const uint32_t nq = cl ? cl->nqueries : qs->nqueries;
    if (!ctx->have_result) return TFIDF_E_STATE;
    const auto wall0 = std::chrono::steady_clock::now();
    if (const int rc = call_begin(ctx, ctx->ev_q)) return rc;
    hipStream_t s = ctx->stream;
    double avgdl = 0.0;   /* BM25: 0 = no document has a token, every row is empty */
    if (bm) {
        avgdl = bm->avgdl;
        if (!(avgdl > 0.0)) {
            uint64_t L = 0, n = 0;
            const int rc = tfidf_ctx_bm25_lengths(ctx, &L, &n);
            if (rc) return rc;
            avgdl = L ? (double)L / (double)n : 0.0;
        }
    }
    memset(out, 0, sizeof(*out));
    out->nqueries = nq;
    out->k = k;
    out->nhits = (uint32_t*)calloc((size_t)nq + 1, 4);
    out->nmatch = (uint64_t*)calloc((size_t)nq + 1, 8);
    out->nterms_found = (uint32_t*)calloc((size_t)nq + 1, 4);
    out->doc = (uint32_t*)calloc((size_t)nq * k + 1, 4);
    out->score = (double*)calloc((size_t)nq * k + 1, 8);
    struct HitsGuard {   /* an error return leaves *out zeroed */
        tfidf_hits* h;
        ~HitsGuard() { if (h) tfidf_hits_free(h); }
    } guard{out};
    if (!out->nhits || !out->nmatch || !out->nterms_found || !out->doc || !out->score) return TFIDF_E_NOMEM;

    /* ---- tokens -> the batch's distinct terms, per query (term, weight) in first-occurrence order ---- */
    std::unordered_map<std::string, uint32_t> term_id;
    std::vector<const std::string*> terms;
    std::vector<uint64_t> qt_off((size_t)nq + 1, 0);
    std::vector<uint32_t> qt_term, qt_w, qt_inc;   /* qt_inc: clauses only, the CL_INC_* of the term's texts, summed */
    for (uint32_t q = 0; q < nq; ++q) {
        std::unordered_map<uint32_t, size_t> seen;
        /* a token of a text that scores (w += 1) or of the must_not text; inc: the text's CL_INC_* */
        auto token = [&](const char* p, size_t n, uint32_t inc) {
            auto ins = term_id.emplace(std::string(p, n), (uint32_t)terms.size());
            if (ins.second) terms.push_back(&ins.first->first);
            auto at = seen.emplace(ins.first->second, qt_term.size());
            const bool scores = inc != CL_INC_NOT;
            if (at.second) {
                qt_term.push_back(ins.first->second);
                qt_w.push_back(scores ? 1u : 0u);
                if (cl) qt_inc.push_back(inc);
                return;
            }
            const size_t x = at.first->second;
            if (scores && qt_w[x] != 0xFFFFFFFFu) ++qt_w[x];
            const uint32_t field = inc == CL_INC_NOT ? 0xFF000000u : inc * CL_FIELD;
            if (cl && !(qt_inc[x] & field)) qt_inc[x] += inc;   /* once per text */
        };
        if (!cl) {
            for_each_term(qs, q, [&](const char* p, size_t n) { token(p, n, CL_INC_SHOULD); });
        } else {   /* the numbering every rank shares: must text, should text, then what is only in must_not */
            if (cl->must) for_each_term(cl->must, q, [&](const char* p, size_t n) { token(p, n, CL_INC_MUST); });
            if (cl->should) for_each_term(cl->should, q, [&](const char* p, size_t n) { token(p, n, CL_INC_SHOULD); });
            if (cl->must_not) for_each_term(cl->must_not, q, [&](const char* p, size_t n) { token(p, n, CL_INC_NOT); });
        }
        qt_off[q + 1] = qt_term.size();
    }
    const uint32_t nT = (uint32_t)terms.size();
    tfidf_clause_info qi{};   /* the widest of the three infos: the call's own is cut from it below */
    qi.nqueries = nq;
    qi.k = k;
    qi.nterms = nT;

    /* ---- lookup: one lane per distinct term ---- */
    std::vector<uint32_t> rank(nT, QUERY_NO_TERM), df_found(bm ? nT : 0, 0u);
    std::vector<uint64_t> toff((size_t)nT + 1, 0);
    std::string blob;
    if (nT && ctx->V) {
        for (uint32_t t = 0; t < nT; ++t) { toff[t] = blob.size(); blob += *terms[t]; }
        toff[nT] = blob.size();
        const size_t offb = ((size_t)nT + 1) * 8;
        ENSURE(ctx->q_terms, offb + blob.size() + 16);
        ENSURE(ctx->q_rank, (size_t)nT * (bm ? 8 : 4) + 4);   /* BM25: the found terms' df behind the ranks */
        HIPCHK(hipMemcpyAsync(ctx->q_terms.p, toff.data(), offb, hipMemcpyHostToDevice, s));
        if (!blob.empty())
            HIPCHK(hipMemcpyAsync(ctx->q_terms.as<uint8_t>() + offb, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
        QLookupArgs la{};
        la.tbytes = ctx->q_terms.as<uint8_t>() + offb;
        la.toff = ctx->q_terms.as<uint64_t>();
        la.nterms = nT;
        la.vkeys = ctx->vkeys.as<uint4>();
        la.vrep = ctx->vrep.as<uint64_t>();
        la.mask = ctx->vcap - 1;
        la.home = ~1ull;
        la.rank_of_slot = ctx->rank_of_slot.as<uint32_t>();
        la.corpus = ctx->dev_bytes;
        la.corpus_bytes = ctx->corpus.nbytes;
        la.V = ctx->V;
        la.rank_out = ctx->q_rank.as<uint32_t>();
        HIPCHK(hipEventRecord(ctx->ev_q[0], s));
        LAUNCH(launch_query_lookup(la, s));
        LAUNCH(bm && launch_bm25_df(la.rank_out, nT, df_of_run(ctx), ctx->V, la.rank_out + nT, s));
        HIPCHK(hipEventRecord(ctx->ev_q[1], s));
        HIPCHK(hipMemcpyAsync(rank.data(), ctx->q_rank.p, (size_t)nT * 4, hipMemcpyDeviceToHost, s));
        if (bm) HIPCHK(hipMemcpyAsync(df_found.data(), la.rank_out + nT, (size_t)nT * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        qi.ms_lookup = ev_ms(ctx->ev_q[0], ctx->ev_q[1]);
    }
    for (uint32_t t = 0; t < nT; ++t) qi.nterms_found += rank[t] != QUERY_NO_TERM;
    if (found_out) found_out->assign(qt_term.size(), 0);
    if (found_off_out) *found_off_out = qt_off;
    for (uint32_t q = 0; q < nq; ++q)
        for (uint64_t x = qt_off[q]; x < qt_off[q + 1]; ++x)
            if (rank[qt_term[x]] != QUERY_NO_TERM && qt_w[x] != 0u) {   /* w = 0: only in the must_not text */
                ++out->nterms_found[q];
                if (found_out) (*found_out)[x] = 1;
            }

    /* ---- clauses: need[q] = |M| << 12 | m, and the queries no document of this shard can satisfy ---- */
    std::vector<uint32_t> need(cl ? nq : 0, 0u);
    std::vector<uint8_t> dropped(cl ? nq : 0, 0);
    for (uint32_t q = 0; cl && q < nq; ++q) {
        uint32_t nM = 0, nS = 0;
        bool bad = false;
        for (uint64_t x = qt_off[q]; x < qt_off[q + 1]; ++x) {
            const uint32_t inc = qt_inc[x];
            const bool must = (inc >> 12) & CL_FIELD;
            nM += must;
            nS += (inc & CL_FIELD) != 0u;
            bad = bad || (must && (rank[qt_term[x]] == QUERY_NO_TERM || (inc >> 24)));
        }
        const uint32_t m = cl->min_should ? cl->min_should[q] : 0u;
        if (nM > TFIDF_CLAUSE_MAX_TERMS || nS > TFIDF_CLAUSE_MAX_TERMS || m > TFIDF_CLAUSE_MAX_TERMS) return TFIDF_E_INVAL;
        need[q] = nM << 12 | m;
        dropped[q] = bad || m > nS;
        qi.nq_unsatisfiable += dropped[q];
    }

    /* ---- BM25: idf per distinct found term, the host's libm log (one operation per line) ---- */
    std::vector<double> idf(bm ? nT : 0, 0.0);
    for (uint32_t t = 0; bm && t < nT; ++t) {
        if (rank[t] == QUERY_NO_TERM) continue;
        const uint64_t Nt = ctx->ndocs_total, df = df_found[t] < Nt ? df_found[t] : Nt;
        const double num = (double)(Nt - df) + 0.5;
        const double den = (double)df + 0.5;
        const double ratio = num / den;
        const double arg = 1.0 + ratio;
        idf[t] = log(arg);
    }

    /* ---- query groups under the accumulator budget ---- */
    /* BM25 with avgdl 0 (L = 0: no document of the context has a token, so there are no pairs):
     * N = 0 turns every group below off and the rows stay empty, as the header defines */
    const uint32_t N = bm && !(avgdl > 0.0) ? 0u : ctx->ndocs;
    const TopkPlan plan = topk_plan(N, k, nq, ctx->query_acc_bytes);
    const uint64_t G = plan.G;
    qi.group_queries = (uint32_t)G;
    qi.acc_bytes = G * plan.per_q;
    if (N && nq) {
        const int rc = topk_ensure(ctx, plan, N);
        if (rc) return rc;
    }
    std::vector<uint64_t> h_s((size_t)G * k), h_nm(G);
    std::vector<uint32_t> h_id((size_t)G * k), h_n(G);
    struct Post { uint32_t rank, q, w, term, inc; };
    std::vector<Post> posts;
    std::vector<uint32_t> tab;
    for (uint32_t g0 = 0; N && g0 < nq; g0 += (uint32_t)G) {
        const uint32_t gn = nq - g0 < G ? nq - g0 : (uint32_t)G;
        posts.clear();
        for (uint32_t q = 0; q < gn; ++q) {
            if (cl && dropped[g0 + q]) continue;
            for (uint64_t x = qt_off[g0 + q]; x < qt_off[g0 + q + 1]; ++x)
                if (rank[qt_term[x]] != QUERY_NO_TERM)
                    posts.push_back(Post{rank[qt_term[x]], q, qt_w[x], qt_term[x], cl ? qt_inc[x] : 1u});
        }
        if (posts.empty()) continue;   /* no term of the group is in the vocabulary: no hits */
        if (posts.size() > 0x7FFFFFFFull) return TFIDF_E_CAPACITY;
        ++qi.ngroups;
        std::sort(posts.begin(), posts.end(), [](const Post& a, const Post& b) { return a.rank != b.rank ? a.rank < b.rank : a.q < b.q; });
        /* the group's table: sorted distinct ranks, CSR offsets, postings' queries and weights */
        uint32_t nG = 0;
        for (size_t i = 0; i < posts.size(); ++i) nG += i == 0 || posts[i].rank != posts[i - 1].rank;
        const uint32_t nP = (uint32_t)posts.size();
        /* clauses: the postings' increments behind their queries, and behind the table the group's
         * need words.  BM25: the weights are binary64 W(q,t) = fl(w * idf), at the next even word */
        const size_t inc_at = (size_t)2 * nG + 1 + nP, w_base = inc_at + (cl ? nP : 0u);
        const size_t w_at = w_base + (bm ? w_base & 1u : 0u);
        const size_t tab_words = w_at + (bm ? 2 : 1) * (size_t)nP;
        tab.assign(tab_words + (cl ? gn : 0u), 0);
        uint32_t* gterm = tab.data();
        uint32_t* poff = gterm + nG;
        uint32_t* pq = poff + nG + 1;
        uint32_t* pw = gterm + w_at;
        for (uint32_t q = 0; cl && q < gn; ++q) tab[tab_words + q] = need[g0 + q];
        for (uint32_t i = 0, t = 0; i < nP; ++i) {
            if (i == 0 || posts[i].rank != posts[i - 1].rank) { gterm[t] = posts[i].rank; poff[t] = i; ++t; }
            pq[i] = posts[i].q;
            if (cl) gterm[inc_at + i] = posts[i].inc;
            if (bm) {
                /* a must_not-only posting: W = +0.0 whatever the idf, its product is +0.0 */
                const double W = posts[i].w ? (double)posts[i].w * idf[posts[i].term] : 0.0;
                memcpy(pw + 2 * (size_t)i, &W, 8);
            } else {
                pw[i] = posts[i].w;
            }
        }
        poff[nG] = nP;
        ENSURE(ctx->q_tab, tab.size() * 4 + 16);
        HIPCHK(hipMemcpyAsync(ctx->q_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
        unsigned long long* d_nm = ctx->q_misc.as<unsigned long long>();
        HIPCHK(hipMemsetAsync(d_nm, 0, (size_t)G * 8, s));
        DocScanArgs sa{};
        sa.out_off = ctx->out_off.as<uint64_t>();
        sa.out_term = ctx->out_term.as<uint32_t>();
        sa.ndocs = N;
        sa.npairs = ctx->npairs;
        sa.gterm = ctx->q_tab.as<uint32_t>();
        sa.ngterm = nG;
        sa.post_off = sa.gterm + nG;
        sa.post_q = sa.post_off + nG + 1;
        sa.post_w = sa.gterm + w_at;
        sa.tab_words = tab_words <= 0xFFFFFFFFull ? (uint32_t)tab_words : 0u;
        qi.ngroups_tab_lds += sa.tab_words != 0u && sa.tab_words <= QTAB_WORDS;
        sa.nq = gn;
        sa.acc = ctx->q_acc.as<double>();
        sa.cnt = ctx->q_cnt.as<uint32_t>();
        sa.big_list = ctx->q_big.as<uint32_t>();
        sa.big_count = (uint32_t*)(d_nm + G);
        HIPCHK(hipEventRecord(ctx->ev_q[0], s));
        int lrc;
        if (bm) {
            BScoreArgs ba{sa};
            ba.out_cnt = ctx->out_cnt.as<uint32_t>();
            ba.order = ctx->order;
            ba.doc_size = ctx->doc_size.as<uint32_t>();
            ba.k1 = bm->k1;
            ba.b = bm->b;
            ba.avgdl = avgdl;
            ba.k1_plus_1 = bm->k1 + 1.0;
            ba.one_minus_b = 1.0 - bm->b;
            lrc = cl ? launch_bm25_score_clauses(BClauseArgs{ba, sa.gterm + inc_at}, ctx->ncu, s) : launch_bm25_score(ba, ctx->ncu, s);
        } else {
            QScoreArgs ta{sa};
            ta.out_score = ctx->out_score.as<double>();
            lrc = cl ? launch_query_score_clauses(QClauseArgs{ta, sa.gterm + inc_at}, ctx->ncu, s) : launch_query_score(ta, ctx->ncu, s);
        }
        LAUNCH(lrc);
        HIPCHK(hipEventRecord(ctx->ev_q[1], s));
        TopkCand res{};
        int rc = topk_rounds(ctx, plan, sa.acc, sa.cnt, N, k, gn, d_nm, &res, cl ? sa.gterm + tab_words : nullptr);
        if (rc) return rc;
        HIPCHK(hipEventRecord(ctx->ev_q[2], s));
        rc = topk_read_back(ctx, res, d_nm, gn, k, h_s.data(), h_id.data(), h_n.data(), h_nm.data());
        if (rc) return rc;
        qi.ms_score += ev_ms(ctx->ev_q[0], ctx->ev_q[1]);
        qi.ms_topk += ev_ms(ctx->ev_q[1], ctx->ev_q[2]);
        for (uint32_t q = 0; q < gn; ++q) {
            const uint32_t n = h_n[q] < k ? h_n[q] : k;
            out->nhits[g0 + q] = n;
            out->nmatch[g0 + q] = h_nm[q];
            for (uint32_t i = 0; i < n; ++i) {
                out->doc[(size_t)(g0 + q) * k + i] = h_id[(size_t)q * k + i];
                memcpy(&out->score[(size_t)(g0 + q) * k + i], &h_s[(size_t)q * k + i], 8);
            }
        }
    }
    qi.ms_total = wall_ms(wall0);
    qi.avgdl = avgdl;
    /* the three infos share their leading fields (static_asserts below) */
    if (cl) ctx->cinfo = qi;
    else if (bm) memcpy(&ctx->binfo, &qi, sizeof(ctx->binfo));
    else memcpy(&ctx->qinfo, &qi, sizeof(ctx->qinfo));
    guard.h = nullptr;
    return TFIDF_OK;
}

static_assert(offsetof(tfidf_clause_info, avgdl) == offsetof(tfidf_bm25_info, avgdl) &&
                  offsetof(tfidf_bm25_info, avgdl) == sizeof(tfidf_query_info) &&
                  offsetof(tfidf_clause_info, nq_unsatisfiable) == sizeof(tfidf_bm25_info),
              "tfidf_clause_info extends tfidf_bm25_info, which extends tfidf_query_info");

extern "C" int tfidf_query(tfidf_ctx* ctx, const tfidf_queries* queries, uint32_t k, tfidf_hits* out) {
    return tfidf_ctx_query(ctx, queries, k, out, nullptr, nullptr);
}

extern "C" int tfidf_query_bm25(tfidf_ctx* ctx, const tfidf_queries* queries, uint32_t k, const tfidf_bm25_params* params,
                                tfidf_hits* out) {
    if (!ctx || !queries || !out) return TFIDF_E_INVAL;
    Bm25Call bm{};
    const int rc = tfidf_bm25_params_check(params, &bm);
    if (rc) return rc;
    return tfidf_ctx_query(ctx, queries, k, out, nullptr, nullptr, &bm);
}

extern "C" int tfidf_last_bm25_info(const tfidf_ctx* ctx, tfidf_bm25_info* info) {
    return ctx ? copy_info(info, ctx->binfo) : TFIDF_E_INVAL;
}

extern "C" int tfidf_last_query_info(const tfidf_ctx* ctx, tfidf_query_info* info) {
    return ctx ? copy_info(info, ctx->qinfo) : TFIDF_E_INVAL;
}

/* ------------------------------------------------------------------ clauses ---- */

int tfidf_clause_plan(const tfidf_clauses* c, ClausePlan* plan, Bm25Call* bm, bool* has_bm) {
    if (!c || c->size < sizeof(tfidf_clauses)) return TFIDF_E_INVAL;
    if (c->ranking != TFIDF_RANK_TFIDF && c->ranking != TFIDF_RANK_BM25) return TFIDF_E_INVAL;
    if (c->nqueries > TFIDF_QUERY_MAX_QUERIES) return TFIDF_E_INVAL;
    if (c->ranking == TFIDF_RANK_TFIDF && c->bm25) return TFIDF_E_INVAL;
    *has_bm = c->ranking == TFIDF_RANK_BM25;
    if (*has_bm) {
        if (const int rc = tfidf_bm25_params_check(c->bm25, bm)) return rc;
    }
    const tfidf_queries* text[3] = {c->must, c->should, c->must_not};
    const size_t limit[3] = {TFIDF_CLAUSE_MAX_TERMS, TFIDF_CLAUSE_MAX_TERMS, TFIDF_CLAUSE_MAX_NOT};
    for (int i = 0; i < 3; ++i) {
        if (!text[i]) continue;
        if (text[i]->nqueries != c->nqueries || queries_check(text[i])) return TFIDF_E_INVAL;
        for (uint32_t q = 0; q < c->nqueries; ++q) {
            std::unordered_map<std::string, int> distinct;
            for_each_term(text[i], q, [&](const char* p, size_t n) { distinct.emplace(std::string(p, n), 0); });
            if (distinct.size() > limit[i]) return TFIDF_E_INVAL;
        }
    }
    for (uint32_t q = 0; c->min_should && q < c->nqueries; ++q)
        if (c->min_should[q] > TFIDF_CLAUSE_MAX_TERMS) return TFIDF_E_INVAL;
    *plan = ClausePlan{c->nqueries, c->must, c->should, c->must_not, c->min_should};
    return TFIDF_OK;
}

extern "C" int tfidf_clauses_check(const tfidf_clauses* clauses) {
    ClausePlan plan{};
    Bm25Call bm{};
    bool has_bm = false;
    return tfidf_clause_plan(clauses, &plan, &bm, &has_bm);
}

extern "C" int tfidf_query_clauses(tfidf_ctx* ctx, const tfidf_clauses* clauses, uint32_t k, tfidf_hits* out) {
    if (out) memset(out, 0, sizeof(*out));
    if (!ctx || !clauses || !out) return TFIDF_E_INVAL;
    ClausePlan plan{};
    Bm25Call bm{};
    bool has_bm = false;
    if (const int rc = tfidf_clause_plan(clauses, &plan, &bm, &has_bm)) return rc;
    return tfidf_ctx_query(ctx, nullptr, k, out, nullptr, nullptr, has_bm ? &bm : nullptr, &plan);
}

extern "C" int tfidf_last_clause_info(const tfidf_ctx* ctx, tfidf_clause_info* info) {
    return ctx ? copy_info(info, ctx->cinfo) : TFIDF_E_INVAL;
}
