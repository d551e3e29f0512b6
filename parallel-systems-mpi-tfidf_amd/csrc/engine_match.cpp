/*
 * engine_match.cpp — tfidf_match_terms (match.hip).
 * The context and the helpers every engine file shares: engine_ctx.h.
 */
#include "engine_ctx.h"

/* ----------------------------------------------------------- term matching ----
 * Fuzzy and prefix patterns against the resident term table (include/tfidf.h, match.hip; the
 * check and the host twin are match_host.c).  The patterns go in groups of MT_GROUP, one scan of
 * the table per group.  A scan counts every pattern's matches exactly and appends them to the
 * device list; when the group's matches fit the list, one sort by (pattern, dist, ~df, rank)
 * puts every pattern's matches in the defined order, the first k of each segment are cut and
 * their words gathered.  When they do not fit, the counts are exact all the same: the group's
 * patterns are scanned again in batches whose summed counts fit, and for a single pattern with
 * more matches than the capacity the list grows once to that count (at most V records of 40
 * bytes).  Nothing of the result is written, and nothing depends on grid, group, batch or
 * capacity: the sort key is total. */

namespace {
constexpr uint64_t MT_DEFAULT_RECORDS = 262144;
constexpr uint32_t MT_KEY_BYTES = 0x11FFu;   /* the key's digits that vary: rank, ~df, dist, pattern in the group */

struct MatchGuard {   /* an error return leaves *out zeroed */
    tfidf_term_matches* m;
    ~MatchGuard() { if (m) tfidf_term_matches_free(m); }
};

struct MatchCall {
    tfidf_ctx* ctx;
    MtScanArgs sa;
    uint64_t cap;                    /* the list's capacity in records */
    uint32_t E;
    tfidf_term_matches* out;
    tfidf_match_info mi;
    std::vector<uint64_t> nmatch;    /* by pattern, as the last scan of it counted */
    std::vector<uint64_t> woff;      /* a batch's word offsets */
    uint64_t wbase = 0;
};

int list_ensure(MatchCall& c) {
    tfidf_ctx* ctx = c.ctx;
    ENSURE(ctx->mt_k0, c.cap * 16 + 16);
    ENSURE(ctx->mt_k1, c.cap * 16 + 16);
    ENSURE(ctx->mt_v0, c.cap * 4 + 4);
    ENSURE(ctx->mt_v1, c.cap * 4 + 4);
    c.sa.key = ctx->mt_k0.as<uint4>();
    c.sa.val = ctx->mt_v0.as<uint32_t>();
    c.sa.list_cap = c.cap;
    return TFIDF_OK;
}

/* one scan of the table for the patterns [b0, b0 + nb): their counts to c.nmatch, the records
 * appended (written or not) to *nrec */
int mt_scan(MatchCall& c, uint32_t b0, uint32_t nb, uint64_t* nrec) {
    tfidf_ctx* ctx = c.ctx;
    hipStream_t s = ctx->stream;
    c.sa.p0 = b0;
    c.sa.np = nb;
    HIPCHK(hipMemsetAsync(c.sa.nmatch + b0, 0, (size_t)nb * 8, s));
    HIPCHK(hipMemsetAsync(c.sa.nrec, 0, 8, s));
    HIPCHK(hipEventRecord(ctx->ev_mt[0], s));
    LAUNCH(launch_match_scan(c.sa, ctx->ncu, s));
    HIPCHK(hipEventRecord(ctx->ev_mt[1], s));
    HIPCHK(hipMemcpyAsync(c.nmatch.data() + b0, c.sa.nmatch + b0, (size_t)nb * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(nrec, c.sa.nrec, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    c.mi.ms_scan += ev_ms(ctx->ev_mt[0], ctx->ev_mt[1]);
    ++c.mi.ngroups;
    return TFIDF_OK;
}

/* the list of the scan before holds every match of the patterns [b0, b0 + nb), n records: sort,
 * cut, gather the words, copy the rows out */
int mt_select(MatchCall& c, uint32_t b0, uint32_t nb, uint64_t n) {
    tfidf_ctx* ctx = c.ctx;
    hipStream_t s = ctx->stream;
    const uint32_t E = c.E;
    const size_t nbe = (size_t)nb * E, e0 = (size_t)b0 * E;
    uint32_t seg[MT_GROUP + 1];
    seg[0] = 0;
    for (uint32_t i = 0; i < nb; ++i) seg[i + 1] = seg[i] + (uint32_t)c.nmatch[b0 + i];
    if (seg[nb] != n || n > c.cap) return TFIDF_E_STATE;
    const bool tile = n <= SORT_TILE_MAXN;
    if (arena_scratch(ctx, (size_t)n * (tile ? 32 : 4) + (2u << 20))) return TFIDF_E_NOMEM;
    HIPCHK(hipMemcpyAsync(ctx->mt_seg.p, seg, ((size_t)nb + 1) * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(ctx->ev_mt[2], s));
    uint4 *k0 = ctx->mt_k0.as<uint4>(), *k1 = ctx->mt_k1.as<uint4>();
    uint32_t *v0 = ctx->mt_v0.as<uint32_t>(), *v1 = ctx->mt_v1.as<uint32_t>();
    const int where = tile ? tile_sort_u128(k0, v0, k1, v1, n, ctx->arena, s)
                           : radix_sort_u128(k0, v0, k1, v1, n, MT_KEY_BYTES, ctx->arena, s);
    if (where == -2) return TFIDF_E_NOMEM;
    LAUNCH(where < 0);
    MtCutArgs ca{where ? k1 : k0, ctx->mt_seg.as<uint32_t>(), nb, E, c.sa.src, c.sa.V, ctx->mt_term.as<uint32_t>(),
                 ctx->mt_dist.as<uint8_t>(), ctx->mt_df.as<uint32_t>(), ctx->mt_woff.as<uint64_t>()};
    LAUNCH(launch_match_cut(ca, s));
    /* word lengths -> offsets inside the batch, in place; [nbe] = the batch's word bytes */
    SCAN(scan_excl_u64(ca.wlen, ca.wlen, nbe, ctx->arena, s));
    HIPCHK(hipEventRecord(ctx->ev_mt[3], s));
    HIPCHK(hipMemcpyAsync(c.woff.data(), ca.wlen, (nbe + 1) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const uint64_t wtotal = c.woff[nbe];
    ENSURE(ctx->mt_words, wtotal + 16);
    HIPCHK(hipEventRecord(ctx->ev_mt[4], s));
    if (c.sa.src.tkey) {
        TWordArgs wa{ca.term, ca.wlen, nbe, c.sa.src.tkey, c.sa.V, c.sa.src.corpus, c.sa.src.corpus_bytes,
                     ctx->mt_words.as<uint8_t>()};
        LAUNCH(launch_terms_words(wa, s));
    } else {
        LAUNCH(launch_match_words_model(ca.term, ca.wlen, nbe, c.sa.src, c.sa.V, ctx->mt_words.as<uint8_t>(), s));
    }
    HIPCHK(hipEventRecord(ctx->ev_mt[5], s));
    tfidf_term_matches* out = c.out;
    uint8_t* wb = (uint8_t*)realloc(out->word_bytes, (size_t)(c.wbase + wtotal) + 1);
    if (!wb) return TFIDF_E_NOMEM;
    out->word_bytes = wb;
    HIPCHK(hipMemcpyAsync(out->term + e0, ca.term, nbe * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out->dist + e0, ca.dist, nbe, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out->df + e0, ca.df, nbe * 4, hipMemcpyDeviceToHost, s));
    if (wtotal) HIPCHK(hipMemcpyAsync(wb + c.wbase, ctx->mt_words.p, wtotal, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    c.mi.ms_select += ev_ms(ctx->ev_mt[2], ctx->ev_mt[3]);
    c.mi.ms_words += ev_ms(ctx->ev_mt[4], ctx->ev_mt[5]);
    ++c.mi.nbatches;
    c.mi.nrecords += n;
    for (uint32_t i = 0; i < nb; ++i) {
        out->nmatch[b0 + i] = c.nmatch[b0 + i];
        out->nterms[b0 + i] = c.nmatch[b0 + i] < E ? (uint32_t)c.nmatch[b0 + i] : E;
    }
    for (size_t i = 0; i < nbe; ++i) out->word_off[e0 + i] = c.wbase + c.woff[i];
    c.wbase += wtotal;
    return TFIDF_OK;
}
}  // namespace

extern "C" int tfidf_match_terms(tfidf_ctx* ctx, const tfidf_patterns* ps, const tfidf_match_params* pr,
                                 tfidf_term_matches* out) {
    if (!out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!ctx || tfidf_match_check(ps, pr) != TFIDF_OK) return TFIDF_E_INVAL;
    if (!ctx->have_result && !ctx->have_model) return TFIDF_E_STATE;
    const auto wall0 = std::chrono::steady_clock::now();
    if (const int rc = call_begin(ctx, ctx->ev_mt)) return rc;
    hipStream_t s = ctx->stream;
    const uint32_t P = ps->npatterns, E = pr->max_expansions, V = ctx->V;
    const size_t PE = (size_t)P * E;
    out->npatterns = P;
    out->k = E;
    out->nmatch = (uint64_t*)calloc((size_t)P + 1, 8);
    out->nterms = (uint32_t*)calloc((size_t)P + 1, 4);
    out->term = (uint32_t*)calloc(PE + 1, 4);
    out->dist = (uint8_t*)calloc(PE + 1, 1);
    out->df = (uint32_t*)calloc(PE + 1, 4);
    out->word_off = (uint64_t*)calloc(PE + 1, 8);
    out->word_bytes = (uint8_t*)calloc(1, 1);
    MatchGuard guard{out};
    if (!out->nmatch || !out->nterms || !out->term || !out->dist || !out->df || !out->word_off || !out->word_bytes)
        return TFIDF_E_NOMEM;
    MatchCall c{};
    c.ctx = ctx;
    c.E = E;
    c.out = out;
    c.cap = pr->list_records ? pr->list_records : MT_DEFAULT_RECORDS;
    c.mi.npatterns = P;
    c.mi.k = E;
    if (P) {
        /* ---- the table's bytes: the run's term metadata, or the imported model's own list ---- */
        MtScanArgs& sa = c.sa;
        if (ctx->model_only) {
            sa.src = MtSrc{nullptr, nullptr, nullptr, ctx->m_blob_bytes, ctx->m_off.as<uint64_t>(), ctx->m_blob.as<uint8_t>()};
        } else {
            if (const int rc = ensure_term_meta(ctx)) return rc;
            sa.src = MtSrc{ctx->t_key.as<uint4>(), ctx->t_len.as<uint32_t>(), ctx->dev_bytes, ctx->corpus.nbytes, nullptr, nullptr};
        }
        sa.df = df_of_run(ctx);
        sa.V = V;
        sa.fixed_prefix = pr->fixed_prefix;
        sa.transpose = (pr->flags & TFIDF_MATCH_TRANSPOSE) ? 1u : 0u;
        /* ---- the pattern block: MT_PAT zero-padded bytes per pattern, then lengths, kinds, budgets ---- */
        std::vector<uint8_t> blk((size_t)P * (MT_PAT + 3), 0);
        for (uint32_t p = 0; p < P; ++p) {
            const uint32_t len = (uint32_t)(ps->p_off[p + 1] - ps->p_off[p]);
            memcpy(blk.data() + (size_t)p * MT_PAT, ps->bytes + ps->p_off[p], len);
            blk[(size_t)P * MT_PAT + p] = (uint8_t)len;
            blk[(size_t)P * (MT_PAT + 1) + p] = ps->kind[p];
            blk[(size_t)P * (MT_PAT + 2) + p] = ps->kind[p] == TFIDF_MATCH_PREFIX ? 0 : ps->max_edits[p];
        }
        ENSURE(ctx->mt_pat, blk.size() + 16);
        ENSURE(ctx->mt_cnt, ((size_t)P + 1) * 8);
        const size_t GE = (size_t)MT_GROUP * E;
        ENSURE(ctx->mt_seg, (MT_GROUP + 1) * 4);
        ENSURE(ctx->mt_term, GE * 4 + 4);
        ENSURE(ctx->mt_dist, GE + 4);
        ENSURE(ctx->mt_df, GE * 4 + 4);
        ENSURE(ctx->mt_woff, (GE + 1) * 8 + 16);
        if (const int rc = list_ensure(c)) return rc;
        HIPCHK(hipMemcpyAsync(ctx->mt_pat.p, blk.data(), blk.size(), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        sa.pat = ctx->mt_pat.as<uint8_t>();
        sa.plen = sa.pat + (size_t)P * MT_PAT;
        sa.pkind = sa.plen + P;
        sa.pbudget = sa.pkind + P;
        sa.nmatch = ctx->mt_cnt.as<unsigned long long>();
        sa.nrec = sa.nmatch + P;
        c.nmatch.assign(P, 0);
        c.woff.assign(GE + 1, 0);
        for (uint32_t g0 = 0; g0 < P; g0 += MT_GROUP) {
            const uint32_t g1 = P - g0 < MT_GROUP ? P : g0 + MT_GROUP;
            uint64_t n = 0;
            if (const int rc = mt_scan(c, g0, g1 - g0, &n)) return rc;
            if (n <= c.cap) {
                if (const int rc = mt_select(c, g0, g1 - g0, n)) return rc;
                continue;
            }
            /* the group's matches exceed the list: batches of patterns whose exact counts fit */
            for (uint32_t b = g0; b < g1;) {
                uint64_t sum = 0;
                uint32_t e = b;
                while (e < g1 && sum + c.nmatch[e] <= c.cap) sum += c.nmatch[e++];
                if (e == b) {   /* one pattern with more matches than the capacity: the list grows to its count */
                    c.cap = c.nmatch[b];
                    if (const int rc = list_ensure(c)) return rc;
                    e = b + 1;
                }
                if (const int rc = mt_scan(c, b, e - b, &n)) return rc;
                if (n > c.cap) return TFIDF_E_STATE;
                if (const int rc = mt_select(c, b, e - b, n)) return rc;
                b = e;
            }
        }
    }
    out->word_off[PE] = c.wbase;
    c.mi.list_records = c.cap;
    c.mi.ms_total = wall_ms(wall0);
    ctx->mtinfo = c.mi;
    guard.m = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_last_match_info(const tfidf_ctx* ctx, tfidf_match_info* info) {
    return ctx ? copy_info(info, ctx->mtinfo) : TFIDF_E_INVAL;
}
