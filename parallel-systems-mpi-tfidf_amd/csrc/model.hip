/*
 * model.hip — the device side of the portable model (include/tfidf.h: tfidf_model_import,
 * tfidf_model_export).  The reference has one pass over one corpus (TFIDF.c:130-247) and keeps
 * nothing; here a model's term list becomes the frozen table a run leaves behind, so that
 * transform.hip probes it unchanged.
 *
 *   build   one lane per term t (its rank: the list is in term-table order): the identity key
 *           from the term's bytes (dev_common.h: the key a token of these bytes gets in K1 and
 *           in k_tr_resolve), find-or-insert with K1's own vocab_insert_s at home alignment ~1
 *           (dev_vocab.h: rep published before the key, agent-scope claim and publish), the
 *           uploaded term bytes in the corpus's place: a long term's rep is
 *           len << 40 | offset into the blob, and two distinct long terms with one 120-bit key
 *           are compared byte by byte and reported (ST_LONG_COLLIDE), never merged.  Then
 *           rank_of_slot[slot] = t by an exchange: the table was cleared to QUERY_NO_TERM, so a
 *           rank already there means the key was present (ST_MODEL_DUP: the host check
 *           excludes it; reported, no fault).
 *   lens    the export's identity selection and u64 lengths for terms.hip's word gather.
 */
#include "kernels.h"
#include "dev_common.h"
#include "dev_vocab.h"

namespace {

constexpr int NT = 256;
inline unsigned grid_for(uint64_t n) { return n ? (unsigned)((n + NT - 1) / NT) : 1u; }
int ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

constexpr uint64_t TERM_MAX = 1ull << 24;   /* the 24 length bits of a long term's rep */

__global__ __launch_bounds__(NT) void k_model_build(const ModelBuild a) {
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (t >= a.nterms) return;
    const uint64_t o = a.term_off[t], e = a.term_off[t + 1];
    if (!(o <= e && e <= a.blob_bytes)) { atomicOr(a.status, ST_BOUNDS); return; }
    const uint64_t n = e - o;
    if (n >= TERM_MAX) { atomicOr(a.status, ST_TERM_LONG); return; }
    const uint8_t* p = a.blob + o;
    uint64_t klo = 0, khi = 0, rep = 0;
    if (n < 16u) {
        uint64_t l8 = 0, h8 = 0;
        for (uint32_t b = 0; b < (uint32_t)n; ++b) {
            const uint64_t c = p[b];
            if (b < 8u) l8 |= c << (8u * b);
            else h8 |= c << (8u * (b - 8u));
        }
        /* a NUL inside the term would shorten the key: not the term the list names */
        if (make_short_key(l8, h8, (uint32_t)n, &klo, &khi) != (uint32_t)n) { atomicOr(a.status, ST_BOUNDS); return; }
    } else {
        make_long_key(p, n, &klo, &khi);
        rep = (n << 40) | o;
    }
    const uint32_t slot = vocab_insert_s<~1ull>(a.keys, a.rep, a.mask, klo, khi, rep, a.status, a.blob);
    if (slot == INVALID_SLOT) return;   /* the insert has set its status bit */
    if ((uint64_t)slot > a.mask) { atomicOr(a.status, ST_BOUNDS); return; }
    if (atomicExch(&a.rank_of_slot[slot], (uint32_t)t) != QUERY_NO_TERM) atomicOr(a.status, ST_MODEL_DUP);
}

__global__ __launch_bounds__(NT) void k_model_lens(const uint32_t* __restrict__ tlen, uint32_t n,
                                                   uint32_t* __restrict__ term, uint64_t* __restrict__ wlen) {
    const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (i > n) return;
    wlen[i] = i < n ? (uint64_t)tlen[i] : 0ull;
    if (i < n) term[i] = (uint32_t)i;
}

}  // namespace

int launch_model_build(const ModelBuild& a, hipStream_t s) {
    if (!a.nterms) return 0;
    k_model_build<<<grid_for(a.nterms), NT, 0, s>>>(a);
    return ok();
}

int launch_model_lens(const uint32_t* tlen, uint32_t n, uint32_t* term, uint64_t* wlen, hipStream_t s) {
    k_model_lens<<<grid_for((uint64_t)n + 1u), NT, 0, s>>>(tlen, n, term, wlen);
    return ok();
}
