/*
 * engine_snippets.cpp — tfidf_snippet (snippets.hip).
 * The context and the helpers every engine file shares: engine_ctx.h.
 */
#include "engine_ctx.h"

#include <algorithm>
#include <string>
#include <unordered_set>

/* ---------------------------------------------------------------- snippets ----
 * Best passage and match marks of (query, document) jobs over the resident corpus (include/tfidf.h,
 * snippets.hip; the check and the host twin are snippet_host.c).  The host tokenises the queries
 * into U(q); one lookup gives every term's key and whether the vocabulary holds it, and the host
 * builds each query's table of found terms from the keys.  The jobs go in order:
 *   batch      consecutive jobs whose tiles fit the tile half of the budget: one count pass, the
 *              scans of the tile counts, the per-job totals read back (exact sizes before anything
 *              is written);
 *   sub-batch  consecutive jobs of the batch whose matches fit the record half: the write pass over
 *              their tiles, select, emit, the per-job results read back, the marks' and texts'
 *              offsets up, fill, marks and text read back.
 * One job with more tiles or matches than its half of the budget grows that buffer once to its
 * size.  Nothing of the result is written, and nothing depends on grid, batch or budget. */

namespace {
constexpr uint64_t SN_DEFAULT_SCRATCH = 256ull << 20;
constexpr uint64_t SN_TILE_WORDS = 16;   /* budget bytes per tile: two counts, their scans' scratch, the job's words */
constexpr uint64_t SN_REC_BYTES = 16;

struct SnipGuard {   /* an error return leaves *out zeroed */
    tfidf_snippets* s;
    ~SnipGuard() { if (s) tfidf_snippets_free(s); }
};

inline bool ws(uint8_t c) { return c == 0x20u || (c >= 0x09u && c <= 0x0Du); }

struct QTerms {   /* U(q) of every query, flattened */
    std::vector<uint64_t> off;      /* nq + 1 */
    std::vector<uint64_t> pos;      /* in the query's bytes */
    std::vector<uint32_t> len;
    std::vector<uint8_t> truncated; /* per query */
};

void query_terms(const tfidf_queries* qs, QTerms& t) {
    const uint32_t nq = qs->nqueries;
    t.off.assign((size_t)nq + 1, 0);
    t.truncated.assign(nq, 0);
    for (uint32_t q = 0; q < nq; ++q) {
        const uint8_t* qb = qs->bytes + qs->q_off[q];
        const uint64_t qn = qs->q_off[q + 1] - qs->q_off[q];
        std::unordered_set<std::string> seen;
        size_t used = 0;
        for (uint64_t i = 0; i < qn;) {
            if (ws(qb[i])) { ++i; continue; }
            uint64_t e = i;
            while (e < qn && !ws(qb[e])) ++e;
            const void* z = memchr(qb + i, 0, (size_t)(e - i));
            const uint64_t tl = z ? (uint64_t)((const uint8_t*)z - (qb + i)) : e - i;
            std::string term((const char*)qb + i, (size_t)tl);
            if (!seen.count(term)) {
                if (used == TFIDF_SNIP_MAX_TERMS) {
                    t.truncated[q] = 1;
                } else {
                    seen.insert(std::move(term));
                    t.pos.push_back(i);
                    t.len.push_back((uint32_t)tl);
                    ++used;
                }
            }
            i = e;
        }
        t.off[q + 1] = t.pos.size();
    }
}

template <typename T> bool grow(T*& p, size_t n) {
    T* q = (T*)realloc(p, (n + 1) * sizeof(T));
    if (!q) return false;
    p = q;
    return true;
}
}  // namespace

extern "C" int tfidf_snippet(tfidf_ctx* ctx, const tfidf_queries* qs, const uint32_t* job_query, const uint32_t* job_doc,
                             uint32_t njobs, const tfidf_snippet_params* pr, tfidf_snippets* out) {
    if (!out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!ctx || !qs || tfidf_snippets_check(pr) != TFIDF_OK) return TFIDF_E_INVAL;
    if (njobs > TFIDF_SNIP_MAX_JOBS || (njobs && (!job_query || !job_doc))) return TFIDF_E_INVAL;
    const uint32_t nq = qs->nqueries;
    if (nq > TFIDF_QUERY_MAX_QUERIES || !qs->q_off || (qs->nbytes && !qs->bytes)) return TFIDF_E_INVAL;
    for (uint32_t q = 0; q < nq; ++q)
        if (qs->q_off[q + 1] < qs->q_off[q]) return TFIDF_E_INVAL;
    if (qs->q_off[nq] > qs->nbytes) return TFIDF_E_INVAL;
    for (uint32_t j = 0; j < njobs; ++j)
        if (job_query[j] >= nq) return TFIDF_E_INVAL;
    if (!ctx->have_result || ctx->model_only) return TFIDF_E_STATE;   /* a model-only context has no corpus */
    const auto wall0 = std::chrono::steady_clock::now();
    if (const int rc = call_begin(ctx, ctx->ev_sn)) return rc;
    hipStream_t s = ctx->stream;
    const uint32_t W = pr->window, M = pr->max_marks, want_text = (pr->flags & TFIDF_SNIP_TEXT) ? 1u : 0u;
    tfidf_snippet_info si{};
    si.njobs = njobs;
    si.scratch_bytes = pr->scratch_bytes ? pr->scratch_bytes : SN_DEFAULT_SCRATCH;
    uint64_t tile_cap = si.scratch_bytes / 2 / SN_TILE_WORDS, rec_cap = si.scratch_bytes / 2 / SN_REC_BYTES;
    if (tile_cap > SN_MAX_TILES) tile_cap = SN_MAX_TILES;

    /* ---- U(q) ---- */
    QTerms qt;
    query_terms(qs, qt);
    const size_t nT = qt.pos.size();
    out->njobs = njobs;
    out->nqueries = nq;
    out->flags = (uint32_t*)calloc((size_t)njobs + 1, 4);
    out->ntokens = (uint32_t*)calloc((size_t)njobs + 1, 4);
    out->nmatch = (uint32_t*)calloc((size_t)njobs + 1, 4);
    out->nterms_matched = (uint32_t*)calloc((size_t)njobs + 1, 4);
    out->win_tok = (uint32_t*)calloc(2 * (size_t)njobs + 1, 4);
    out->win_byte = (uint64_t*)calloc(2 * (size_t)njobs + 1, 8);
    out->cover = (uint32_t*)calloc((size_t)njobs + 1, 4);
    out->hits = (uint32_t*)calloc((size_t)njobs + 1, 4);
    out->mark_off = (uint64_t*)calloc((size_t)njobs + 1, 8);
    out->text_off = (uint64_t*)calloc((size_t)njobs + 1, 8);
    out->mark_byte = (uint64_t*)calloc(1, 8);
    out->mark_len = (uint32_t*)calloc(1, 4);
    out->mark_slot = (uint32_t*)calloc(1, 4);
    out->text = (uint8_t*)calloc(1, 1);
    out->qterm_off = (uint64_t*)calloc((size_t)nq + 1, 8);
    out->qterm_pos = (uint64_t*)calloc(nT + 1, 8);
    out->qterm_len = (uint32_t*)calloc(nT + 1, 4);
    out->qterm_found = (uint8_t*)calloc(nT + 1, 1);
    SnipGuard guard{out};
    if (!out->flags || !out->ntokens || !out->nmatch || !out->nterms_matched || !out->win_tok || !out->win_byte ||
        !out->cover || !out->hits || !out->mark_off || !out->text_off || !out->mark_byte || !out->mark_len ||
        !out->mark_slot || !out->text || !out->qterm_off || !out->qterm_pos || !out->qterm_len || !out->qterm_found)
        return TFIDF_E_NOMEM;
    memcpy(out->qterm_off, qt.off.data(), ((size_t)nq + 1) * 8);
    if (nT) {
        memcpy(out->qterm_pos, qt.pos.data(), nT * 8);
        memcpy(out->qterm_len, qt.len.data(), nT * 4);
    }

    /* ---- lookup: one lane per term; the keys and the found flags come back ---- */
    std::vector<uint64_t> toff(nT + 1, 0), keys(2 * nT, 0);
    std::vector<uint32_t> found(nT, 0);
    std::string blob;
    {
        size_t x = 0;
        for (uint32_t q = 0; q < nq; ++q)
            for (uint64_t u = qt.off[q]; u < qt.off[q + 1]; ++u, ++x) {
                toff[x] = blob.size();
                blob.append((const char*)qs->bytes + qs->q_off[q] + qt.pos[u], qt.len[u]);
            }
        toff[nT] = blob.size();
    }
    const size_t t_off_b = 0, t_blob_b = al256((nT + 1) * 8), t_key_b = al256(t_blob_b + blob.size() + 16),
                 t_found_b = t_key_b + nT * 16, t_end = t_found_b + nT * 4 + 16;
    ENSURE(ctx->sn_terms, t_end);
    uint8_t* d_terms = ctx->sn_terms.as<uint8_t>();
    if (nT) {
        HIPCHK(hipMemcpyAsync(d_terms + t_off_b, toff.data(), (nT + 1) * 8, hipMemcpyHostToDevice, s));
        if (!blob.empty()) HIPCHK(hipMemcpyAsync(d_terms + t_blob_b, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
        SnLookupArgs la{};
        la.tbytes = d_terms + t_blob_b;
        la.toff = (const uint64_t*)(d_terms + t_off_b);
        la.nterms = (uint32_t)nT;
        la.voc = VocabRO{ctx->vkeys.as<uint4>(), ctx->vrep.as<uint64_t>(), ctx->vcap - 1, ~1ull,
                         ctx->rank_of_slot.as<uint32_t>(), ctx->dev_bytes, ctx->corpus.nbytes, ctx->V};
        la.key = (uint64_t*)(d_terms + t_key_b);
        la.found = (uint32_t*)(d_terms + t_found_b);
        HIPCHK(hipEventRecord(ctx->ev_sn[0], s));
        LAUNCH(launch_sn_lookup(la, s));
        HIPCHK(hipEventRecord(ctx->ev_sn[1], s));
        HIPCHK(hipMemcpyAsync(keys.data(), la.key, nT * 16, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(found.data(), la.found, nT * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        si.ms_lookup = ev_ms(ctx->ev_sn[0], ctx->ev_sn[1]);
        for (size_t x = 0; x < nT; ++x) out->qterm_found[x] = (uint8_t)found[x];
    }

    /* ---- every query's table of found terms ---- */
    std::vector<SnQuery> hq((size_t)nq + 1);
    std::vector<SnEnt> htab;
    for (uint32_t q = 0; q < nq; ++q) {
        uint32_t nf = 0, lmax = 0;
        for (uint64_t u = qt.off[q]; u < qt.off[q + 1]; ++u)
            if (found[u]) { ++nf; if (qt.len[u] > lmax) lmax = qt.len[u]; }
        uint32_t size = 0;
        if (nf) for (size = 2; size < 2 * nf; size <<= 1) {}
        hq[q] = SnQuery{(uint32_t)htab.size(), size, lmax, 0};
        const size_t t0 = htab.size();
        htab.resize(t0 + size, SnEnt{0, SN_ENT_EMPTY, 0, 0, 0});
        for (uint64_t u = qt.off[q]; u < qt.off[q + 1]; ++u) {
            if (!found[u]) continue;
            uint32_t h = sn_hash(keys[2 * u], keys[2 * u + 1]) & (size - 1);
            while (htab[t0 + h].khi != SN_ENT_EMPTY) h = (h + 1) & (size - 1);
            htab[t0 + h] = SnEnt{keys[2 * u], keys[2 * u + 1], toff[u], qt.len[u], (uint32_t)(u - qt.off[q])};
        }
    }
    const size_t q_b = 0, tab_b = al256(((size_t)nq + 1) * sizeof(SnQuery));
    ENSURE(ctx->sn_tab, tab_b + (htab.size() + 1) * sizeof(SnEnt));
    HIPCHK(hipMemcpyAsync(ctx->sn_tab.as<uint8_t>() + q_b, hq.data(), ((size_t)nq + 1) * sizeof(SnQuery), hipMemcpyHostToDevice, s));
    if (!htab.empty())
        HIPCHK(hipMemcpyAsync(ctx->sn_tab.as<uint8_t>() + tab_b, htab.data(), htab.size() * sizeof(SnEnt), hipMemcpyHostToDevice, s));

    /* ---- the jobs' documents ---- */
    std::vector<SnJob> hjobs(njobs);
    const size_t j_q_b = al256((size_t)njobs * 8 + 8), j_job_b = al256(j_q_b + (size_t)njobs * 4 + 4);
    if (njobs) {
        ENSURE(ctx->sn_jobs, j_job_b + (size_t)njobs * sizeof(SnJob));
        uint8_t* dj = ctx->sn_jobs.as<uint8_t>();
        const uint64_t* d_off = (ctx->corpus.flags & TFIDF_CORPUS_DEVICE) ? ctx->corpus.doc_off : ctx->in_off.as<uint64_t>();
        /* ids at the buffer's start, their output positions behind them (lookup_ids) */
        HIPCHK(hipMemcpyAsync(dj, job_doc, (size_t)njobs * 4, hipMemcpyHostToDevice, s));
        TLookupArgs la{(const uint32_t*)dj, njobs, ctx->order, ctx->dev_ids, ctx->ndocs, (uint32_t*)dj + njobs};
        LAUNCH(launch_terms_lookup(la, s));
        HIPCHK(hipMemcpyAsync(dj + j_q_b, job_query, (size_t)njobs * 4, hipMemcpyHostToDevice, s));
        LAUNCH(launch_sn_jobs((const uint32_t*)dj + njobs, (const uint32_t*)(dj + j_q_b), njobs, ctx->order, d_off,
                              (SnJob*)(dj + j_job_b), s));
        HIPCHK(hipMemcpyAsync(hjobs.data(), dj + j_job_b, (size_t)njobs * sizeof(SnJob), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    const SnJob* d_jobs = njobs ? (const SnJob*)(ctx->sn_jobs.as<uint8_t>() + j_job_b) : nullptr;
    const SnQuery* d_q = (const SnQuery*)(ctx->sn_tab.as<uint8_t>() + q_b);
    const SnEnt* d_tab = (const SnEnt*)(ctx->sn_tab.as<uint8_t>() + tab_b);

    /* a job's tiles: from the 16-byte boundary at or below its first byte to its last byte */
    auto tiles_of = [&](const SnJob& jb) -> uint64_t {
        if (!jb.len) return 0;
        const uint64_t mis = (uint64_t)((uintptr_t)(ctx->dev_bytes + jb.base) & 15u);
        return (mis + jb.len + SN_TILE - 1) / SN_TILE;
    };

    uint64_t nmarks_all = 0, ntext_all = 0;
    std::vector<uint32_t> tile_first, slice_first, tot;
    std::vector<SnOut> hout;
    std::vector<uint64_t> moff, toff_j;
    for (uint32_t b0 = 0; b0 < njobs;) {
        /* ---- a batch: [b0, b1), its tiles under tile_cap (one larger job alone) ---- */
        uint64_t nt = 0;
        uint32_t b1 = b0;
        tile_first.assign(1, 0);
        while (b1 < njobs) {
            const uint64_t t = tiles_of(hjobs[b1]);
            if (b1 > b0 && nt + t > tile_cap) break;
            if (t > SN_MAX_TILES) return TFIDF_E_CAPACITY;   /* a document of 4 GiB: its token ordinals would pass 2^32 */
            nt += t;
            tile_first.push_back((uint32_t)nt);
            ++b1;
            if (nt > tile_cap) break;
        }
        const uint32_t nb = b1 - b0, ntiles = (uint32_t)nt;
        if (nt > tile_cap) si.scratch_bytes = std::max<uint64_t>(si.scratch_bytes, nt * SN_TILE_WORDS * 2);
        /* tile words: tile_first [nb + 1], tile_tok [ntiles + 1], tile_match [ntiles + 1], totals [2 nb],
         * slice_first [nb + 1], best [nb] u64, mask [4 nb] u64 */
        const size_t w_tf = 0, w_tok = al256(((size_t)nb + 1) * 4), w_mat = al256(w_tok + ((size_t)ntiles + 1) * 4),
                     w_tot = al256(w_mat + ((size_t)ntiles + 1) * 4), w_sf = al256(w_tot + (size_t)nb * 8),
                     w_best = al256(w_sf + ((size_t)nb + 1) * 4), w_mask = w_best + (size_t)nb * 8,
                     w_end = w_mask + (size_t)nb * 32;
        ENSURE(ctx->sn_tile, w_end + 16);
        if (arena_scratch(ctx, scan_scratch(ntiles) + (1u << 20))) return TFIDF_E_NOMEM;
        uint8_t* dw = ctx->sn_tile.as<uint8_t>();
        uint32_t* d_tf = (uint32_t*)(dw + w_tf);
        uint32_t* d_tok = (uint32_t*)(dw + w_tok);
        uint32_t* d_mat = (uint32_t*)(dw + w_mat);
        uint32_t* d_tot = (uint32_t*)(dw + w_tot);
        HIPCHK(hipMemcpyAsync(d_tf, tile_first.data(), ((size_t)nb + 1) * 4, hipMemcpyHostToDevice, s));
        SnScanArgs sa{};
        sa.corpus = ctx->dev_bytes;
        sa.jobs = d_jobs + b0;
        sa.tile_first = d_tf;
        sa.njobs = nb;
        sa.t0 = 0;
        sa.t1 = ntiles;
        sa.queries = d_q;
        sa.tab = d_tab;
        sa.tbytes = d_terms + t_blob_b;
        sa.tile_tok = d_tok;
        sa.tile_match = d_mat;
        HIPCHK(hipEventRecord(ctx->ev_sn[2], s));
        LAUNCH(launch_sn_scan(sa, ctx->ncu, s));
        SCAN(scan_excl_u32(d_tok, d_tok, ntiles, ctx->arena, s));
        SCAN(scan_excl_u32(d_mat, d_mat, ntiles, ctx->arena, s));
        LAUNCH(launch_sn_totals(d_tf, nb, d_tok, d_mat, d_tot, s));
        HIPCHK(hipEventRecord(ctx->ev_sn[3], s));
        tot.assign(2 * (size_t)nb, 0);
        HIPCHK(hipMemcpyAsync(tot.data(), d_tot, (size_t)nb * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        si.ms_count += ev_ms(ctx->ev_sn[2], ctx->ev_sn[3]);
        ++si.nbatches;
        si.ntiles += ntiles;
        for (uint32_t i = 0; i < nb; ++i) {
            si.nbytes += hjobs[b0 + i].len;
            si.ntokens += tot[2 * (size_t)i];
            si.nmatches += tot[2 * (size_t)i + 1];
        }

        /* ---- sub-batches: [c0, c1) of the batch, their matches under rec_cap (one larger job alone) ---- */
        for (uint32_t c0 = 0; c0 < nb;) {
            uint64_t nr = 0;
            uint32_t c1 = c0;
            slice_first.assign(1, 0);
            while (c1 < nb) {
                const uint64_t m = tot[2 * (size_t)c1 + 1];
                if (c1 > c0 && nr + m > rec_cap) break;
                nr += m;
                const uint32_t nsl = (uint32_t)((m + SN_SLICE - 1) / SN_SLICE);
                si.nbig += nsl > 1;
                slice_first.push_back(slice_first.back() + nsl);
                ++c1;
            }
            if (nr > rec_cap) {   /* one job with more matches than the capacity: the list grows to its count */
                rec_cap = nr;
                si.scratch_bytes = std::max<uint64_t>(si.scratch_bytes, nr * SN_REC_BYTES * 2);
            }
            const uint32_t nc = c1 - c0;
            ENSURE(ctx->sn_rec, (nr + 1) * SN_REC_BYTES);
            const size_t o_out = 0, o_moff = al256((size_t)nc * sizeof(SnOut)), o_toff = al256(o_moff + ((size_t)nc + 1) * 8),
                         o_end = o_toff + ((size_t)nc + 1) * 8;
            ENSURE(ctx->sn_out, o_end + 16);
            uint8_t* dout = ctx->sn_out.as<uint8_t>();
            uint32_t* d_sf = (uint32_t*)(dw + w_sf);
            unsigned long long* d_best = (unsigned long long*)(dw + w_best);
            unsigned long long* d_mask = (unsigned long long*)(dw + w_mask);
            HIPCHK(hipMemcpyAsync(d_sf, slice_first.data(), ((size_t)nc + 1) * 4, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemsetAsync(d_best, 0, (size_t)nc * 8, s));
            HIPCHK(hipMemsetAsync(d_mask, 0, (size_t)nc * 32, s));
            /* the write pass over the sub-batch's tiles */
            sa.t0 = tile_first[c0];
            sa.t1 = tile_first[c1];
            sa.rec = ctx->sn_rec.as<uint4>();
            uint64_t rec0 = 0;
            for (uint32_t i = 0; i < c0; ++i) rec0 += tot[2 * (size_t)i + 1];
            sa.rec0 = (uint32_t)rec0;
            HIPCHK(hipEventRecord(ctx->ev_sn[4], s));
            if (nr) LAUNCH(launch_sn_scan(sa, ctx->ncu, s));
            HIPCHK(hipEventRecord(ctx->ev_sn[5], s));
            sa.rec = nullptr;
            SnSelArgs se{};
            se.jobs = d_jobs + b0;
            se.tile_first = d_tf;
            se.tile_tok = d_tok;
            se.tile_match = d_mat;
            se.j0 = c0;
            se.j1 = c1;
            se.rec = ctx->sn_rec.as<uint4>();
            se.slice_first = d_sf;
            se.nslices = slice_first.back();
            se.best = d_best;
            se.mask = d_mask;
            se.window = W;
            se.max_marks = M;
            se.want_text = want_text;
            se.corpus = ctx->dev_bytes;
            se.out = (SnOut*)(dout + o_out);
            LAUNCH(launch_sn_select(se, ctx->ncu, s));
            HIPCHK(hipEventRecord(ctx->ev_sn[6], s));
            LAUNCH(launch_sn_emit(se, ctx->ncu, s));
            HIPCHK(hipEventRecord(ctx->ev_sn[7], s));
            hout.resize(nc);
            HIPCHK(hipMemcpyAsync(hout.data(), se.out, (size_t)nc * sizeof(SnOut), hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            si.ms_write += ev_ms(ctx->ev_sn[4], ctx->ev_sn[5]);
            si.ms_select += ev_ms(ctx->ev_sn[5], ctx->ev_sn[6]);
            si.ms_emit += ev_ms(ctx->ev_sn[6], ctx->ev_sn[7]);
            ++si.nsubbatches;
            moff.assign((size_t)nc + 1, 0);
            toff_j.assign((size_t)nc + 1, 0);
            for (uint32_t i = 0; i < nc; ++i) {
                const SnOut& o = hout[i];
                const size_t j = (size_t)b0 + c0 + i;
                out->flags[j] = o.flags | (qt.truncated[job_query[j]] && !(o.flags & TFIDF_SNIP_NO_DOC) ? TFIDF_SNIP_TRUNCATED : 0u);
                out->ntokens[j] = o.ntokens;
                out->nmatch[j] = o.nmatch;
                out->nterms_matched[j] = o.nterms_matched;
                out->win_tok[2 * j] = o.win_tok[0];
                out->win_tok[2 * j + 1] = o.win_tok[1];
                out->win_byte[2 * j] = o.win_byte[0];
                out->win_byte[2 * j + 1] = o.win_byte[1];
                out->cover[j] = o.cover;
                out->hits[j] = o.hits;
                out->mark_off[j] = nmarks_all + moff[i];
                out->text_off[j] = ntext_all + toff_j[i];
                moff[i + 1] = moff[i] + o.nmarks;
                toff_j[i + 1] = toff_j[i] + o.text_len;
            }
            const uint64_t nm = moff[nc], ntx = toff_j[nc];
            if (nm || ntx) {
                const size_t f_len = al256(nm * 8), f_slot = al256(f_len + nm * 4), f_text = al256(f_slot + nm * 4);
                ENSURE(ctx->sn_marks, f_text + ntx + 16);
                uint8_t* df = ctx->sn_marks.as<uint8_t>();
                HIPCHK(hipMemcpyAsync(dout + o_moff, moff.data(), ((size_t)nc + 1) * 8, hipMemcpyHostToDevice, s));
                HIPCHK(hipMemcpyAsync(dout + o_toff, toff_j.data(), ((size_t)nc + 1) * 8, hipMemcpyHostToDevice, s));
                SnFillArgs fa{d_jobs + b0, c0, c1, ctx->sn_rec.as<uint4>(), se.out, (const uint64_t*)(dout + o_moff),
                              (const uint64_t*)(dout + o_toff), ctx->dev_bytes, (uint64_t*)df, (uint32_t*)(df + f_len),
                              (uint32_t*)(df + f_slot), df + f_text};
                HIPCHK(hipEventRecord(ctx->ev_sn[8], s));
                LAUNCH(launch_sn_fill(fa, ctx->ncu, s));
                HIPCHK(hipEventRecord(ctx->ev_sn[9], s));
                if (!grow(out->mark_byte, (size_t)(nmarks_all + nm)) || !grow(out->mark_len, (size_t)(nmarks_all + nm)) ||
                    !grow(out->mark_slot, (size_t)(nmarks_all + nm)) || !grow(out->text, (size_t)(ntext_all + ntx)))
                    return TFIDF_E_NOMEM;
                if (nm) {
                    HIPCHK(hipMemcpyAsync(out->mark_byte + nmarks_all, df, nm * 8, hipMemcpyDeviceToHost, s));
                    HIPCHK(hipMemcpyAsync(out->mark_len + nmarks_all, df + f_len, nm * 4, hipMemcpyDeviceToHost, s));
                    HIPCHK(hipMemcpyAsync(out->mark_slot + nmarks_all, df + f_slot, nm * 4, hipMemcpyDeviceToHost, s));
                }
                if (ntx) HIPCHK(hipMemcpyAsync(out->text + ntext_all, df + f_text, ntx, hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                si.ms_emit += ev_ms(ctx->ev_sn[8], ctx->ev_sn[9]);
                nmarks_all += nm;
                ntext_all += ntx;
            }
            c0 = c1;
        }
        b0 = b1;
    }
    out->mark_off[njobs] = nmarks_all;
    out->text_off[njobs] = ntext_all;
    si.ms_total = wall_ms(wall0);
    ctx->sninfo = si;
    guard.s = nullptr;
    return TFIDF_OK;
}

extern "C" int tfidf_last_snippet_info(const tfidf_ctx* ctx, tfidf_snippet_info* info) {
    return ctx ? copy_info(info, ctx->sninfo) : TFIDF_E_INVAL;
}
