/*
 * launch_util.h — the host helpers every launch function of the query-side files uses.
 */
#ifndef TFIDF_LAUNCH_UTIL_H
#define TFIDF_LAUNCH_UTIL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

/* workgroups of nt threads that cover n items (at least one) */
inline unsigned grid_for(uint64_t n, int nt = 256) { return n ? (unsigned)((n + nt - 1) / nt) : 1u; }
/* 0 when the launch before went through, else -1 */
inline int ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }
/* workgroups of a launch that strides over `want` items with at most per_cu workgroups per CU */
inline unsigned cu_grid(uint64_t want, uint32_t ncu, uint32_t per_cu) {
    const uint64_t cap = (uint64_t)(ncu ? ncu : 256u) * per_cu;
    return (unsigned)(want < cap ? want : cap);
}
/* ... and of the launch behind it that takes a workgroup per big document: min(want, BIG_WG_MAX,
 * ncu * BIG_WG_PER_CU), which is min(want, BIG_WG_MAX) from 64 CUs on */
inline unsigned big_grid(uint32_t want, uint32_t ncu) {
    return cu_grid(want < BIG_WG_MAX ? want : BIG_WG_MAX, ncu, BIG_WG_PER_CU);
}

#endif
