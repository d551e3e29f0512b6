/*
 * ngram_host.c — word n-grams on the host (include/tfidf.h, section "n-grams"): the check of a
 * tfidf_ngram_params and tfidf_ngrams_host, the definition in plain C.  Two passes over the
 * documents with the same walk: the first sizes the output, the second writes it.  No HIP here:
 * the file also links into a stand-alone test program.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"

static int ng_is_sep(uint32_t c) { return c == 0x20u || (c - 0x09u) <= 4u; }

int tfidf_ngram_check(const tfidf_ngram_params* p) {
    if (!p || p->size < sizeof(tfidf_ngram_params)) return TFIDF_E_INVAL;
    if (p->min_n == 0u || p->max_n < p->min_n || p->max_n > TFIDF_NGRAM_MAX_N) return TFIDF_E_INVAL;
    if (ng_is_sep(p->joiner)) return TFIDF_E_INVAL;
    for (uint32_t i = 0; i < sizeof(p->reserved); ++i)
        if (p->reserved[i]) return TFIDF_E_INVAL;
    return TFIDF_OK;
}

/* One document: its grams appended at `out` (NULL: only counted).  Returns the bytes of the
 * output document.  The last TFIDF_NGRAM_MAX_N token bounds are kept in a ring: when token q
 * has been read, every gram that ends at q is complete, but the order is by first token, so the
 * grams of position p are written once token p + max_n - 1 (or the document's end) is known. */
static uint64_t ng_doc(const uint8_t* doc, uint64_t len, uint32_t min_n, uint32_t max_n, uint8_t joiner, uint8_t* out,
                       uint64_t* ntokens, uint64_t* ngrams) {
    uint64_t ts[TFIDF_NGRAM_MAX_N], te[TFIDF_NGRAM_MAX_N];   /* token q lives at q % MAX_N */
    uint64_t m = 0, done = 0, o = 0, i = 0;
    for (;;) {
        while (i < len && ng_is_sep(doc[i])) ++i;
        const int end = i >= len;
        if (!end) {
            const uint64_t b = i;
            while (i < len && !ng_is_sep(doc[i])) ++i;
            ts[m % TFIDF_NGRAM_MAX_N] = b;
            te[m % TFIDF_NGRAM_MAX_N] = i;
            ++m;
        }
        /* positions whose longest gram is known: all of them at the end, else p + max_n <= m */
        while (done < m && (end || done + max_n <= m)) {
            for (uint32_t n = min_n; n <= max_n && done + n <= m; ++n) {
                for (uint32_t k = 0; k < n; ++k) {
                    const uint64_t q = (done + k) % TFIDF_NGRAM_MAX_N, l = te[q] - ts[q];
                    if (out) {
                        memcpy(out + o, doc + ts[q], (size_t)l);
                        out[o + l] = k + 1u < n ? joiner : 0x20u;
                    }
                    o += l + 1u;
                }
                ++*ngrams;
            }
            ++done;
        }
        if (end) break;
    }
    *ntokens += m;
    return o;
}

int tfidf_ngrams_host(const tfidf_ngram_params* params, const uint8_t* bytes, uint64_t nbytes, const uint64_t* off,
                      uint32_t n, uint8_t** out_bytes, uint64_t* out_nbytes, uint64_t** out_off) {
    if (out_bytes) *out_bytes = NULL;
    if (out_nbytes) *out_nbytes = 0;
    if (out_off) *out_off = NULL;
    if (!out_bytes || !out_nbytes || !out_off) return TFIDF_E_INVAL;
    const int rc = tfidf_ngram_check(params);
    if (rc) return rc;
    if (nbytes && !bytes) return TFIDF_E_INVAL;
    if (n && !off) return TFIDF_E_INVAL;
    for (uint32_t d = 0; d < n; ++d)
        if (off[d] > off[d + 1]) return TFIDF_E_INVAL;
    if (n && off[n] > nbytes) return TFIDF_E_INVAL;

    const uint8_t joiner = params->joiner ? params->joiner : 0x5Fu;
    uint64_t* oo = (uint64_t*)malloc(((size_t)n + 1u) * sizeof(uint64_t));
    if (!oo) return TFIDF_E_NOMEM;
    uint64_t ntok = 0, ngr = 0;
    oo[0] = 0;
    for (uint32_t d = 0; d < n; ++d)
        oo[d + 1] = oo[d] + ng_doc(bytes ? bytes + off[d] : NULL, off[d + 1] - off[d], params->min_n, params->max_n, joiner, NULL, &ntok, &ngr);
    uint8_t* ob = (uint8_t*)malloc((size_t)oo[n] + 1u);
    if (!ob) {
        free(oo);
        return TFIDF_E_NOMEM;
    }
    for (uint32_t d = 0; d < n; ++d)
        (void)ng_doc(bytes ? bytes + off[d] : NULL, off[d + 1] - off[d], params->min_n, params->max_n, joiner, ob + oo[d], &ntok, &ngr);
    *out_bytes = ob;
    *out_nbytes = oo[n];
    *out_off = oo;
    return TFIDF_OK;
}
