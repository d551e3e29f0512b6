/*
 * query_ops.h — the operators of `tfidf --query FILE --query-ops`: every line of the query file
 * is sorted, token by token, into the three texts of a tfidf_clauses query.
 *
 * Tokens are the maximal runs of bytes outside {0x20, 0x09..0x0D}, as everywhere else.  A token
 * of >= 2 bytes that starts with '+' goes to the must text without the '+', one of >= 2 bytes
 * that starts with '-' goes to the must_not text without the '-', every other token (a lone '+'
 * or '-' too) goes to the should text, or with all_must to the must text.  Only the first byte is
 * an operator: "++x" requires "+x" and "-+x" excludes "+x".  A token's other bytes are copied as
 * they are, a NUL included (the term ends there later, as for any query).  Each text is its
 * tokens in their order, joined by one blank.  With ops == 0 no byte is an operator.
 *
 * This runs before the analyzer and the n-grams, which then see three ordinary batches.
 */
#ifndef TFIDF_QUERY_OPS_H
#define TFIDF_QUERY_OPS_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { QOPS_MUST = 0, QOPS_SHOULD = 1, QOPS_MUST_NOT = 2 };

static inline int qops_is_ws(uint8_t c) { return c == 0x20u || (c >= 0x09u && c <= 0x0Du); }

/* the class of the token [t, t + n), n >= 1, and in *skip the operator bytes to drop */
static inline int qops_classify(const uint8_t* t, size_t n, int ops, int all_must, size_t* skip) {
    *skip = 0;
    if (ops && n >= 2 && (t[0] == '+' || t[0] == '-')) {
        *skip = 1;
        return t[0] == '+' ? QOPS_MUST : QOPS_MUST_NOT;
    }
    return all_must ? QOPS_MUST : QOPS_SHOULD;
}

/* One line.  out[c] has room for len bytes (a text is never longer than its line); out_n[c]
 * receives the bytes written. */
static inline void qops_split_line(const uint8_t* line, size_t len, int ops, int all_must, uint8_t* const out[3],
                                   size_t out_n[3]) {
    out_n[0] = out_n[1] = out_n[2] = 0;
    for (size_t i = 0; i < len;) {
        while (i < len && qops_is_ws(line[i])) ++i;
        if (i >= len) break;
        const size_t t0 = i;
        while (i < len && !qops_is_ws(line[i])) ++i;
        size_t skip = 0;
        const int c = qops_classify(line + t0, i - t0, ops, all_must, &skip);
        if (out_n[c]) out[c][out_n[c]++] = ' ';
        memcpy(out[c] + out_n[c], line + t0 + skip, i - t0 - skip);
        out_n[c] += i - t0 - skip;
    }
}

/* A batch of nq lines (line q = bytes[off[q], off[q + 1])) into three batches over the same
 * queries.  The arrays come from malloc: bytes_out[c] (never NULL on success), nbytes_out[c],
 * off_out[c] with nq + 1 entries.  Returns 0, or -1 when memory runs out (nothing is kept). */
static inline int qops_split_batch(const uint8_t* bytes, const uint64_t* off, uint32_t nq, int ops, int all_must,
                                   uint8_t* bytes_out[3], uint64_t nbytes_out[3], uint64_t* off_out[3]) {
    const uint64_t total = nq ? off[nq] - off[0] : 0;
    for (int c = 0; c < 3; ++c) {
        bytes_out[c] = (uint8_t*)malloc((size_t)total + 1);
        off_out[c] = (uint64_t*)malloc(((size_t)nq + 1) * sizeof(uint64_t));
    }
    for (int c = 0; c < 3; ++c)
        if (!bytes_out[c] || !off_out[c]) {
            for (int d = 0; d < 3; ++d) { free(bytes_out[d]); free(off_out[d]); bytes_out[d] = NULL; off_out[d] = NULL; }
            return -1;
        }
    uint64_t at[3] = {0, 0, 0};
    for (uint32_t q = 0; q < nq; ++q) {
        uint8_t* const out[3] = {bytes_out[0] + at[0], bytes_out[1] + at[1], bytes_out[2] + at[2]};
        size_t n[3];
        qops_split_line(bytes + off[q], (size_t)(off[q + 1] - off[q]), ops, all_must, out, n);
        for (int c = 0; c < 3; ++c) { off_out[c][q] = at[c]; at[c] += n[c]; }
    }
    for (int c = 0; c < 3; ++c) { off_out[c][nq] = at[c]; nbytes_out[c] = at[c]; }
    return 0;
}

#endif
