/*
 * engine_text.cpp — tfidf_analyze and tfidf_ngrams (analyze.hip, ngram.hip), and what they share
 * with tfidf_transform: the intake of a tfidf_corpus and a slice's token bounds.
 * The context and the helpers every engine file shares: engine_ctx.h.
 */
#include "engine_ctx.h"
#include "analyze_tab.h"

/* ------------------------------------------------------------ corpus intake ----
 * What tfidf_transform, tfidf_analyze and tfidf_ngrams do with the tfidf_corpus they are given
 * (declared and described in engine_ctx.h). */

int corpus_offsets(tfidf_ctx* ctx, const tfidf_corpus& in, std::vector<uint64_t>& copy, const uint64_t** off_out) {
    const uint32_t N = in.ndocs;
    if (N && !in.doc_off) return TFIDF_E_INVAL;
    const uint64_t* off = in.doc_off;
    if ((in.flags & TFIDF_CORPUS_DEVICE) && N) {
        copy.resize((size_t)N + 1);
        HIPCHK(hipMemcpyAsync(copy.data(), in.doc_off, ((size_t)N + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        off = copy.data();
    }
    for (uint32_t d = 0; d < N; ++d)
        if (off[d] > off[d + 1]) return TFIDF_E_INVAL;
    if (N && off[N] > in.nbytes) return TFIDF_E_INVAL;
    *off_out = off;
    return TFIDF_OK;
}

int stage_window(tfidf_ctx* ctx, const tfidf_corpus& in, const uint64_t* off, DevBuf& bytes, DevBuf& offs,
                 const uint8_t** d_bytes, const uint64_t** d_off) {
    const uint32_t N = in.ndocs;
    *d_bytes = in.bytes;
    *d_off = in.doc_off;
    if ((in.flags & TFIDF_CORPUS_DEVICE) || !N) return TFIDF_OK;
    ENSURE(bytes, in.nbytes + 64);
    ENSURE(offs, ((size_t)N + 1) * 8);
    if (off[N] > off[0])
        HIPCHK(hipMemcpyAsync(bytes.as<uint8_t>() + off[0], in.bytes + off[0], off[N] - off[0], hipMemcpyHostToDevice,
                              ctx->stream));
    HIPCHK(hipMemcpyAsync(offs.p, off, ((size_t)N + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    *d_bytes = bytes.as<uint8_t>();
    *d_off = offs.as<uint64_t>();
    return TFIDF_OK;
}

void corpus_out(tfidf_corpus* out, const tfidf_corpus& in, const uint8_t* bytes, uint64_t nbytes, const uint64_t* doc_off,
                const DevBuf& ids) {
    out->bytes = bytes;
    out->nbytes = nbytes;
    out->doc_off = doc_off;
    out->doc_ids = (in.doc_ids && in.ndocs) ? ids.as<uint32_t>() : nullptr;
    out->ndocs = in.ndocs;
    out->flags = TFIDF_CORPUS_DEVICE;
    out->ndocs_total = in.ndocs_total;
}

/* ------------------------------------------------------------- token bounds ----
 * transform.hip's boundary kernels over one slice of a device corpus, for tfidf_transform (per
 * slice) and tfidf_ngrams (the whole window as one slice). */

int token_scratch(tfidf_ctx* ctx, TrSlice& sl, DevBuf& scratch, size_t head, size_t* a_end) {
    sl.p0 = (long long)sl.b0 - (long long)(((uintptr_t)sl.bytes + sl.b0) & 15u);
    sl.ntiles = (uint64_t)((long long)sl.b1 - sl.p0 + (TR_TILE - 1)) / TR_TILE;
    const size_t a_cs = al256(head + (size_t)(sl.ntiles * (TR_TILE / 32u) + 1u) * 4);
    const size_t a_ce = al256(a_cs + (size_t)(sl.ntiles + 1) * 8);
    *a_end = al256(a_ce + (size_t)(sl.ntiles + 1) * 8);
    ENSURE(scratch, *a_end);
    uint8_t* A = scratch.as<uint8_t>();
    sl.status = (uint32_t*)A;
    sl.dstart = (uint32_t*)(A + head);
    sl.cnt_s = (uint64_t*)(A + a_cs);
    sl.cnt_e = (uint64_t*)(A + a_ce);
    return TFIDF_OK;
}

int token_bounds(tfidf_ctx* ctx, const TrSlice& sl, const char* who, uint64_t* T) {
    hipStream_t s = ctx->stream;
    ctx->arena.used = 0;   /* as format_prepare: nothing of a run's result lives in the arena */
    LAUNCH(launch_tr_docstarts(sl, s) || launch_tr_count(sl, s));
    LAUNCH(scan_excl_u64(sl.cnt_s, sl.cnt_s, sl.ntiles, ctx->arena, s) ||
           scan_excl_u64(sl.cnt_e, sl.cnt_e, sl.ntiles, ctx->arena, s));
    uint64_t tot[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&tot[0], sl.cnt_s + sl.ntiles, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&tot[1], sl.cnt_e + sl.ntiles, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (tot[1] != tot[0] || tot[0] > tr_max_tokens(sl.b1 - sl.b0, (uint64_t)sl.d1 - sl.d0)) {
        fprintf(stderr, "tfidf: %s: %llu token starts, %llu ends in %llu bytes\n", who, (unsigned long long)tot[0],
                (unsigned long long)tot[1], (unsigned long long)(sl.b1 - sl.b0));
        return TFIDF_E_STATE;
    }
    if (tot[0] > 0xFFFFFFFEull) return TFIDF_E_CAPACITY;
    *T = tot[0];
    return TFIDF_OK;
}

int token_write(tfidf_ctx* ctx, TrSlice& sl, uint64_t* tok_start, uint64_t* tok_end, uint64_t T, size_t arena_want) {
    if (arena_scratch(ctx, arena_want)) return TFIDF_E_NOMEM;
    sl.tok_start = tok_start;
    sl.tok_end = tok_end;
    sl.tok_cap = T;
    LAUNCH(launch_tr_write(sl, ctx->stream));
    return TFIDF_OK;
}

/* ---------------------------------------------------------------- analyzer ----
 * include/tfidf.h, section "analyzer"; analyze.hip.  The check, the table build and the host
 * definition are analyze_host.c.  The call stands beside a run: it reads and writes buffers of
 * its own and none of the run's state. */
extern "C" int tfidf_analyze(tfidf_ctx* ctx, const tfidf_analyzer* an, const tfidf_corpus* in_, uint32_t slot,
                             tfidf_corpus* out) {
    if (!ctx || !an || !in_ || !out || slot > 1u) return TFIDF_E_INVAL;
    const int arc = tfidf_analyzer_check(an);
    if (arc) return arc;
    const tfidf_corpus in = *in_;   /* out may be the same struct */
    const uint32_t N = in.ndocs;
    if (in.nbytes && !in.bytes) return TFIDF_E_INVAL;   /* every byte is copied, also outside the window */
    const bool dev = (in.flags & TFIDF_CORPUS_DEVICE) != 0;
    DevBuf& ob = ctx->an_bytes[slot];
    if (dev && ob.p && in.bytes >= ob.as<uint8_t>() && in.bytes < ob.as<uint8_t>() + ob.cap) return TFIDF_E_INVAL;
    const auto wall0 = std::chrono::steady_clock::now();
    if (const int rc = call_begin(ctx, ctx->ev_an)) return rc;
    hipStream_t s = ctx->stream;
    std::vector<uint64_t> off_copy;
    const uint64_t* off = nullptr;
    if (const int rc = corpus_offsets(ctx, in, off_copy, &off)) return rc;
    const hipMemcpyKind up = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    ENSURE(ctx->an_bytes[slot], in.nbytes + 64);
    ENSURE(ctx->an_off[slot], ((size_t)N + 1) * 8);
    if (in.doc_off) HIPCHK(hipMemcpyAsync(ctx->an_off[slot].p, in.doc_off, ((size_t)N + 1) * 8, up, s));
    else HIPCHK(hipMemsetAsync(ctx->an_off[slot].p, 0, 8, s));
    if (in.doc_ids && N) {
        ENSURE(ctx->an_ids[slot], (size_t)N * 4);
        HIPCHK(hipMemcpyAsync(ctx->an_ids[slot].p, in.doc_ids, (size_t)N * 4, up, s));
    }
    const uint8_t* d_in = in.bytes;
    if (!dev && in.nbytes) {   /* the whole buffer: the bytes outside the window pass through */
        ENSURE(ctx->an_in, in.nbytes + 64);
        HIPCHK(hipMemcpyAsync(ctx->an_in.p, in.bytes, in.nbytes, hipMemcpyHostToDevice, s));
        d_in = ctx->an_in.as<uint8_t>();
    }
    std::vector<uint32_t> blob(tfidf_an_table_bytes(an) / 4u);
    const uint32_t tab_bytes = tfidf_an_table_build(an, blob.data());
    ENSURE(ctx->an_tab, tab_bytes);
    ENSURE(ctx->an_cnt, 256);
    HIPCHK(hipMemcpyAsync(ctx->an_tab.p, blob.data(), tab_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(ctx->an_cnt.p, 0, 24, s));

    AnArgs a{};
    a.in = d_in;
    a.out = ctx->an_bytes[slot].as<uint8_t>();
    a.nbytes = in.nbytes;
    a.lo = N ? off[0] : 0;
    a.hi = N ? off[N] : 0;
    a.doc_off = ctx->an_off[slot].as<uint64_t>();
    a.ndocs = N;
    a.flags = an->flags;
    if (!(a.flags & (TFIDF_AN_LOWER | TFIDF_AN_PUNCT))) a.flags &= ~TFIDF_AN_UTF8;   /* alone it changes nothing */
    a.min_len = an->min_len;
    a.tab = ctx->an_tab.as<uint32_t>();
    a.tab_bytes = tab_bytes;
    a.blanked = ctx->an_cnt.as<unsigned long long>();
    a.stemmer = an->stemmer;
    const uint32_t lds = an_lds_bytes(a, an->nstop);
    const bool need_dstart = lds || (a.flags & TFIDF_AN_UTF8);   /* a document boundary cuts a sequence */
    if (need_dstart) {
        ENSURE(ctx->an_dstart, (size_t)(in.nbytes / 32u + 2u) * 4u);
        a.dstart = ctx->an_dstart.as<uint32_t>();
    }
    HIPCHK(hipEventRecord(ctx->ev_an[0], s));
    uint32_t grid = 0;
    LAUNCH((need_dstart && launch_an_docstarts(a, s)) || launch_analyze(a, an->nstop, ctx->ncu, ctx->an_grid, &grid, s));
    HIPCHK(hipEventRecord(ctx->ev_an[1], s));
    unsigned long long counts[3] = {0, 0, 0};   /* tokens blanked, tokens stemmed, sequences changed */
    HIPCHK(hipMemcpyAsync(counts, ctx->an_cnt.p, 24, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));

    corpus_out(out, in, a.out, in.nbytes, a.doc_off, ctx->an_ids[slot]);

    tfidf_analyze_info ai{};
    ai.nbytes = in.nbytes;
    ai.ndocs = N;
    ai.nstop = an->nstop;
    ai.table_slots = blob[0];
    ai.lds_bytes = lds;
    ai.tile_bytes = AN_TILE;
    ai.grid = grid;
    ai.blanked_tokens = counts[0];
    ai.stemmed_tokens = counts[1];
    ai.utf8_changed = counts[2];
    ai.ms_kernel = ev_ms(ctx->ev_an[0], ctx->ev_an[1]);
    ai.ms_total = wall_ms(wall0);
    ctx->aninfo = ai;
    return TFIDF_OK;
}

extern "C" int tfidf_last_analyze_info(const tfidf_ctx* ctx, tfidf_analyze_info* info) {
    return ctx ? copy_info(info, ctx->aninfo) : TFIDF_E_INVAL;
}

/* ----------------------------------------------------------------- n-grams ----
 * include/tfidf.h, section "n-grams"; ngram.hip.  The check and the host definition are
 * ngram_host.c.  Like the analyzer the call stands beside a run: it reads and writes buffers of
 * its own and none of the run's state (the arena is scratch between runs, as for
 * tfidf_transform).  Two host round trips size the buffers: the tokens, then the output's bytes. */
extern "C" int tfidf_ngrams(tfidf_ctx* ctx, const tfidf_ngram_params* params, const tfidf_corpus* in_, uint32_t slot,
                            tfidf_corpus* out) {
    if (!ctx || !params || !in_ || !out || slot > 1u) return TFIDF_E_INVAL;
    const int prc = tfidf_ngram_check(params);
    if (prc) return prc;
    const tfidf_corpus in = *in_;   /* out may be the same struct */
    const uint32_t N = in.ndocs;
    if (in.nbytes && !in.bytes) return TFIDF_E_INVAL;
    const bool dev = (in.flags & TFIDF_CORPUS_DEVICE) != 0;
    DevBuf& ob = ctx->ng_bytes[slot];
    if (dev && ob.p && in.bytes >= ob.as<uint8_t>() && in.bytes < ob.as<uint8_t>() + ob.cap) return TFIDF_E_INVAL;
    const auto wall0 = std::chrono::steady_clock::now();
    if (const int rc = call_begin(ctx, ctx->ev_ng)) return rc;
    hipStream_t s = ctx->stream;
    std::vector<uint64_t> off_copy;
    const uint64_t* off = nullptr;
    if (const int rc = corpus_offsets(ctx, in, off_copy, &off)) return rc;
    const uint64_t b0 = N ? off[0] : 0, b1 = N ? off[N] : 0;
    const uint8_t* d_bytes = nullptr;
    const uint64_t* d_off = nullptr;
    if (const int rc = stage_window(ctx, in, off, ctx->ng_in, ctx->ng_inoff, &d_bytes, &d_off)) return rc;
    ENSURE(ctx->ng_off[slot], ((size_t)N + 1) * 8);
    if (in.doc_ids && N) {
        ENSURE(ctx->ng_ids[slot], (size_t)N * 4);
        HIPCHK(hipMemcpyAsync(ctx->ng_ids[slot].p, in.doc_ids, (size_t)N * 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    }

    tfidf_ngram_info ni{};
    ni.nbytes_in = in.nbytes;
    ni.ndocs = N;
    ni.tile_bytes = NG_TILE;
    uint64_t T = 0, nbytes_out = 0;
    unsigned long long ngrams = 0;
    HIPCHK(hipEventRecord(ctx->ev_ng[0], s));
    /* ---- token bounds: transform.hip's kernels over the whole window as one slice ---- */
    TrSlice sl{};
    size_t a_end = 0;
    if (b1 > b0) {
        sl.bytes = d_bytes;
        sl.nbytes = in.nbytes;
        sl.doc_off = d_off;
        sl.d0 = 0;
        sl.d1 = N;
        sl.b0 = b0;
        sl.b1 = b1;
        /* ng_a: status and the gram counter; behind them the bitmap and the per-tile counts */
        if (const int rc = token_scratch(ctx, sl, ctx->ng_a, 256, &a_end)) return rc;
        HIPCHK(hipMemsetAsync(ctx->ng_a.p, 0, 256, s));   /* status, gram counter */
        if (const int rc = token_bounds(ctx, sl, "ngrams", &T)) return rc;
    }
    NgArgs na{};
    if (T) {
        /* ng_b: 24 bytes per token */
        const size_t b_ts = 0, b_te = al256(b_ts + (size_t)T * 8), b_so = al256(b_te + (size_t)T * 8);
        const size_t b_end = al256(b_so + ((size_t)T + 1) * 8);
        ENSURE(ctx->ng_b, b_end);
        uint8_t* B = ctx->ng_b.as<uint8_t>();
        /* the arena: the scans' block sums */
        if (const int rc = token_write(ctx, sl, (uint64_t*)(B + b_ts), (uint64_t*)(B + b_te), T, (size_t)(T / 32) + (1u << 20)))
            return rc;
        HIPCHK(hipEventRecord(ctx->ev_ng[1], s));
        /* ---- segment sizes, their scan, the output's size ---- */
        na.bytes = d_bytes;
        na.nbytes = in.nbytes;
        na.doc_off = d_off;
        na.ndocs = N;
        na.dstart = sl.dstart;
        na.p0 = sl.p0;
        na.min_n = params->min_n;
        na.max_n = params->max_n;
        na.joiner = params->joiner ? params->joiner : 0x5Fu;
        na.tok_start = sl.tok_start;
        na.tok_end = sl.tok_end;
        na.ntok = T;
        na.seg_off = (uint64_t*)(B + b_so);
        na.ngrams = (unsigned long long*)(ctx->ng_a.as<uint8_t>() + 8);
        LAUNCH(launch_ng_sizes(na, s) || scan_excl_u64(na.seg_off, na.seg_off, T, ctx->arena, s));
        uint32_t status = 0;
        HIPCHK(hipMemcpyAsync(&nbytes_out, na.seg_off + T, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&ngrams, na.ngrams, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&status, sl.status, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (status) {
            fprintf(stderr, "tfidf: ngrams: status 0x%x\n", status);
            return TFIDF_E_STATE;
        }
        ni.scratch_bytes = a_end + b_end;
    } else {
        HIPCHK(hipEventRecord(ctx->ev_ng[1], s));
    }
    ENSURE(ctx->ng_bytes[slot], nbytes_out + 64);
    if (nbytes_out) {
        na.out_off = ctx->ng_off[slot].as<uint64_t>();
        na.out = ctx->ng_bytes[slot].as<uint8_t>();
        na.nbytes_out = nbytes_out;
        na.ntiles = (nbytes_out + NG_TILE - 1) / NG_TILE;
        ENSURE(ctx->ng_tseg, (size_t)(na.ntiles + 1) * 4);
        na.tile_seg = ctx->ng_tseg.as<uint32_t>();
        ni.scratch_bytes += (size_t)(na.ntiles + 1) * 4;
        LAUNCH(launch_ng_offsets(na, s));
        HIPCHK(hipEventRecord(ctx->ev_ng[2], s));
        LAUNCH(launch_ng_write(na, s));
        ni.grid = (uint32_t)na.ntiles;
    } else {   /* no gram: every document is empty */
        HIPCHK(hipMemsetAsync(ctx->ng_off[slot].p, 0, ((size_t)N + 1) * 8, s));
        HIPCHK(hipEventRecord(ctx->ev_ng[2], s));
    }
    HIPCHK(hipEventRecord(ctx->ev_ng[3], s));
    HIPCHK(hipStreamSynchronize(s));

    corpus_out(out, in, ctx->ng_bytes[slot].as<uint8_t>(), nbytes_out, ctx->ng_off[slot].as<uint64_t>(), ctx->ng_ids[slot]);

    ni.nbytes_out = nbytes_out;
    ni.ntokens = T;
    ni.ngrams = ngrams;
    ni.ms_bounds = ev_ms(ctx->ev_ng[0], ctx->ev_ng[1]);
    ni.ms_sizes = ev_ms(ctx->ev_ng[1], ctx->ev_ng[2]);
    ni.ms_write = ev_ms(ctx->ev_ng[2], ctx->ev_ng[3]);
    ni.ms_total = wall_ms(wall0);
    ctx->nginfo = ni;
    return TFIDF_OK;
}

extern "C" int tfidf_last_ngram_info(const tfidf_ctx* ctx, tfidf_ngram_info* info) {
    return ctx ? copy_info(info, ctx->nginfo) : TFIDF_E_INVAL;
}
