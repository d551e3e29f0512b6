/*
 * launch_util.h — the two host helpers every launch function of the query-side files uses.
 */
#ifndef TFIDF_LAUNCH_UTIL_H
#define TFIDF_LAUNCH_UTIL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/* workgroups of nt threads that cover n items (at least one) */
inline unsigned grid_for(uint64_t n, int nt = 256) { return n ? (unsigned)((n + nt - 1) / nt) : 1u; }
/* 0 when the launch before went through, else -1 */
inline int ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

#endif
