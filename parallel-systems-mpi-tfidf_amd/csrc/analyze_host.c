/*
 * analyze_host.c — the analyzer on the host (include/tfidf.h, section "analyzer"): the check
 * of a tfidf_analyzer, the build of its stop-word table (analyze_tab.h: the blob the device
 * kernel copies into LDS) and tfidf_analyze_host, the definition in plain C.  No HIP here: the
 * file also links into a stand-alone test program.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"
#include "analyze_tab.h"

int tfidf_analyzer_check(const tfidf_analyzer* an) {
    if (!an || an->size < sizeof(tfidf_analyzer)) return TFIDF_E_INVAL;
    if (an->flags & ~(TFIDF_AN_LOWER | TFIDF_AN_PUNCT)) return TFIDF_E_INVAL;
    if (an->min_len > TFIDF_AN_MAX_WORD) return TFIDF_E_INVAL;
    if (an->nstop > TFIDF_AN_MAX_STOP) return TFIDF_E_INVAL;
    if (!an->nstop) return TFIDF_OK;
    if (!an->stop_bytes || !an->stop_off) return TFIDF_E_INVAL;
    const uint64_t base = an->stop_off[0];
    for (uint32_t i = 0; i < an->nstop; ++i) {
        const uint64_t b = an->stop_off[i], e = an->stop_off[i + 1];
        if (e < b) return TFIDF_E_INVAL;
        if (e == b || e - b > TFIDF_AN_MAX_WORD) return TFIDF_E_INVAL;
        if (e - base > TFIDF_AN_MAX_STOP_BYTES) return TFIDF_E_INVAL;
        for (uint64_t k = b; k < e; ++k)
            if (an->stop_bytes[k] == 0 || an_is_sep(an->stop_bytes[k])) return TFIDF_E_INVAL;
    }
    return TFIDF_OK;
}

static uint32_t an_slots(uint32_t nstop) {
    uint32_t s = 0;
    if (nstop)
        for (s = 16; s < 2u * nstop; s <<= 1) {
        }
    return s;
}

/* the len bytes at p as zero-padded little-endian chunks: aw of an_chunk with shift 0 */
static void an_pack(const uint8_t* p, uint32_t len, uint32_t* aw) {
    memset(aw, 0, ((len + 3u) / 4u) * 4u);
    for (uint32_t k = 0; k < len; ++k) aw[k >> 2] |= (uint32_t)p[k] << (8u * (k & 3u));
}

uint32_t tfidf_an_table_bytes(const tfidf_analyzer* an) {
    uint32_t chunks = 0;
    for (uint32_t i = 0; i < an->nstop; ++i) chunks += ((uint32_t)(an->stop_off[i + 1] - an->stop_off[i]) + 3u) / 4u;
    return AN_HDR_WORDS * 4u + an_slots(an->nstop) * 4u + ((chunks * 4u + 15u) & ~15u);
}

uint32_t tfidf_an_table_build(const tfidf_analyzer* an, uint32_t* blob) {
    const uint32_t nslots = an_slots(an->nstop);
    memset(blob, 0, tfidf_an_table_bytes(an));
    uint32_t* slots = blob + AN_HDR_WORDS;
    uint32_t* words = slots + nslots;
    uint32_t nwords = 0, nchunks = 0;
    for (uint32_t i = 0; i < an->nstop; ++i) {
        const uint32_t len = (uint32_t)(an->stop_off[i + 1] - an->stop_off[i]);
        uint32_t* aw = words + nchunks;   /* packed in place; a duplicate is overwritten by the next word */
        an_pack(an->stop_bytes + an->stop_off[i], len, aw);
        const uint32_t h = an_hash(aw, 0u, len);
        if (an_tab_find(slots, nslots, words, aw, 0u, len, h)) {
            memset(aw, 0, ((len + 3u) / 4u) * 4u);
            continue;
        }
        uint32_t s = h & (nslots - 1u);
        while (slots[s]) s = (s + 1u) & (nslots - 1u);
        slots[s] = an_entry(nchunks, len, h);
        nchunks += (len + 3u) / 4u;
        ++nwords;
    }
    const uint32_t total = (AN_HDR_WORDS + nslots) * 4u + ((nchunks * 4u + 15u) & ~15u);
    blob[0] = nslots;
    blob[1] = nwords;
    blob[2] = (AN_HDR_WORDS + nslots) * 4u;
    blob[3] = total;
    return total;
}

int tfidf_analyze_host(const tfidf_analyzer* an, const uint8_t* bytes, uint64_t nbytes, const uint64_t* off, uint32_t n,
                       uint8_t* out) {
    const int rc = tfidf_analyzer_check(an);
    if (rc) return rc;
    if (nbytes && (!bytes || !out)) return TFIDF_E_INVAL;
    if (n && !off) return TFIDF_E_INVAL;
    for (uint32_t d = 0; d < n; ++d)
        if (off[d] > off[d + 1]) return TFIDF_E_INVAL;
    if (n && off[n] > nbytes) return TFIDF_E_INVAL;

    uint8_t map[256];
    for (uint32_t c = 0; c < 256u; ++c) {
        uint32_t m = c;
        if (c < 0x80u) {
            const int upper = c >= 0x41u && c <= 0x5Au, lower = c >= 0x61u && c <= 0x7Au, digit = c >= 0x30u && c <= 0x39u;
            if ((an->flags & TFIDF_AN_PUNCT) && !upper && !lower && !digit && !an_is_sep(c)) m = 0x20u;
            if ((an->flags & TFIDF_AN_LOWER) && upper) m = c + 0x20u;
        }
        map[c] = (uint8_t)m;
    }
    uint32_t* blob = NULL;
    if (an->nstop) {
        blob = (uint32_t*)malloc(tfidf_an_table_bytes(an));
        if (!blob) return TFIDF_E_NOMEM;
        tfidf_an_table_build(an, blob);
    }
    const uint32_t nslots = blob ? blob[0] : 0u;
    const uint32_t* slots = blob ? blob + AN_HDR_WORDS : NULL;
    const uint32_t* words = blob ? blob + blob[2] / 4u : NULL;
    uint32_t aw[TFIDF_AN_MAX_WORD / 4u + 1u];

    if (out != bytes && nbytes) memmove(out, bytes, (size_t)nbytes);
    for (uint32_t d = 0; d < n; ++d) {
        const uint64_t b = off[d], e = off[d + 1];
        for (uint64_t i = b; i < e; ++i) out[i] = map[out[i]];
        for (uint64_t i = b; i < e;) {
            if (an_is_sep(out[i])) { ++i; continue; }
            uint64_t j = i;
            while (j < e && !an_is_sep(out[j])) ++j;
            const uint64_t len = j - i;
            if (len <= TFIDF_AN_MAX_WORD) {
                int blank = len < an->min_len;
                if (!blank && nslots) {
                    an_pack(out + i, (uint32_t)len, aw);
                    blank = an_tab_find(slots, nslots, words, aw, 0u, (uint32_t)len, an_hash(aw, 0u, (uint32_t)len));
                }
                if (blank) memset(out + i, 0x20, (size_t)len);
            }
            i = j;
        }
    }
    free(blob);
    return TFIDF_OK;
}
