/*
 * knobs.h — the numeric range knobs tfidf_open reads from the environment: one table, one parse
 * function.  Plain C++ with no HIP dependency (tests/native/knobs_test.cpp builds it alone).
 * The string and flag knobs (TFIDF_K1, TFIDF_XCHG, TFIDF_XAGG, TFIDF_STAMPS, TFIDF_DF_SPLIT,
 * TFIDF_REC_PACK, the
 * two TFIDF_TEST_*_RANK hooks) stay in tfidf_open.
 */
#ifndef TFIDF_KNOBS_H
#define TFIDF_KNOBS_H

#include <stdint.h>
#include <stdlib.h>

enum KnobKind {
    KNOB_PLAIN,   /* the value itself */
    KNOB_MB,      /* megabytes: the accepted value shifted left by 20 */
    KNOB_POW2,    /* a power of two (hi unused) */
    KNOB_LOW32,   /* the value's low 32 bits are what is checked and taken: the two load limits */
};
struct Knob {
    const char* name;
    uint64_t lo, hi;   /* the accepted range, both ends included, before KNOB_MB's shift */
    KnobKind kind;
};
/* in the table's order */
enum KnobId {
    KNOB_SL_MAXCAP, KNOB_QUERY_ACC_MB, KNOB_TERMS_MB, KNOB_TRANSFORM_MB, KNOB_DEDUP_MB, KNOB_NB_MB, KNOB_KMEANS_MB,
    KNOB_KMEANS_SPLIT, KNOB_AN_GRID, KNOB_GRID_CUS, KNOB_VCAP, KNOB_VLOAD_BIG, KNOB_VLOAD, KNOB_COUNT
};
static const Knob kKnobs[KNOB_COUNT] = {
    {"TFIDF_SL_MAXCAP", 1024, 1ull << 25, KNOB_PLAIN},   /* hi: K1_SL_MAX_CAP (asserted in engine.cpp) */
    {"TFIDF_QUERY_ACC_MB", 1, 1ull << 20, KNOB_MB},
    {"TFIDF_TERMS_MB", 1, 1ull << 20, KNOB_MB},
    {"TFIDF_TRANSFORM_MB", 1, 1ull << 20, KNOB_MB},
    {"TFIDF_DEDUP_MB", 1, 1ull << 20, KNOB_MB},
    {"TFIDF_NB_MB", 1, 1ull << 20, KNOB_MB},
    {"TFIDF_KMEANS_MB", 1, 1ull << 20, KNOB_MB},
    {"TFIDF_KMEANS_SPLIT", 1, 1024, KNOB_PLAIN},
    {"TFIDF_AN_GRID", 1, 65536, KNOB_PLAIN},
    {"TFIDF_GRID_CUS", 1, 4096, KNOB_PLAIN},
    /* diagnostics: initial vocabulary capacity (power of two) and the loads it may reach before the
     * run is repeated with a larger table (TFIDF_VLOAD percent below 16M slots, default 12;
     * TFIDF_VLOAD_BIG from 16M slots on, default 45) */
    {"TFIDF_VCAP", 1024, ~0ull, KNOB_POW2},
    {"TFIDF_VLOAD_BIG", 10, 90, KNOB_LOW32},
    {"TFIDF_VLOAD", 10, 90, KNOB_LOW32},
};

/* `text` (getenv's answer; null: unset) as knob k's value.  false: unset or rejected, *out is not
 * written and the default stays.  The number is strtoull's with base 0 (decimal, 0x.., 0..);
 * characters behind it are ignored, and no digits at all read as 0. */
static inline bool knob_parse(const Knob& k, const char* text, uint64_t* out) {
    if (!text) return false;
    uint64_t v = strtoull(text, nullptr, 0);
    if (k.kind == KNOB_LOW32) v = (uint32_t)v;
    if (v < k.lo || v > k.hi) return false;
    if (k.kind == KNOB_POW2 && (v & (v - 1)) != 0) return false;
    *out = k.kind == KNOB_MB ? v << 20 : v;
    return true;
}

#endif
