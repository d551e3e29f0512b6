/*
 * knobs_test.cpp — csrc/knobs.h against the values tfidf_open accepted before the knobs had a
 * table: every expectation below was written by hand from those stanzas (strtoull with base 0,
 * the bounds of each knob, the shift of the _MB ones, the power of two of TFIDF_VCAP, the 32-bit
 * reading of the two load limits), none by calling the code under test.  Stand-alone: built with
 * AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_knobs_native.py.
 */
#include <stdio.h>
#include <string.h>

#include "knobs.h"

namespace {

constexpr uint64_t REJ = ~0ull;   /* the expectation "rejected": no knob accepts this value */

struct Case {
    const char* name;
    const char* text;   /* null: unset */
    uint64_t want;      /* the value tfidf_open stored, or REJ: the default stayed */
};

#define MB(x) ((uint64_t)(x) << 20)
/* the six budgets: 1 .. 2^20 megabytes, stored as bytes */
#define MB_CASES(n)                                                                             \
    {n, nullptr, REJ}, {n, "", REJ}, {n, "0", REJ}, {n, "1", 1048576ull}, {n, "1048576", 1099511627776ull}, \
    {n, "1048577", REJ}, {n, "0x10", MB(16)}, {n, "64MB", MB(64)}, {n, "010", MB(8)}, {n, "-1", REJ},       \
    {n, "MB", REJ}, {n, "99999999999999999999999", REJ}
/* the two load limits: 10 .. 90 percent, read through a 32-bit cast */
#define PCT_CASES(n)                                                                            \
    {n, nullptr, REJ}, {n, "", REJ}, {n, "9", REJ}, {n, "10", 10}, {n, "90", 90}, {n, "91", REJ},           \
    {n, "0x20", 32}, {n, "50%", 50}, {n, "010", REJ}, {n, "-1", REJ}, {n, "4294967316", 20},                \
    {n, "4294967295", REJ}

const Case kCases[] = {
    /* TFIDF_SL_MAXCAP: 1024 .. 2^25 slots */
    {"TFIDF_SL_MAXCAP", nullptr, REJ}, {"TFIDF_SL_MAXCAP", "", REJ}, {"TFIDF_SL_MAXCAP", "1023", REJ},
    {"TFIDF_SL_MAXCAP", "1024", 1024}, {"TFIDF_SL_MAXCAP", "33554432", 33554432}, {"TFIDF_SL_MAXCAP", "33554433", REJ},
    {"TFIDF_SL_MAXCAP", "0x800", 2048}, {"TFIDF_SL_MAXCAP", "4096abc", 4096}, {"TFIDF_SL_MAXCAP", "-1", REJ},
    {"TFIDF_SL_MAXCAP", "3000", 3000},   /* no power of two is asked of this one */
    MB_CASES("TFIDF_QUERY_ACC_MB"), MB_CASES("TFIDF_TERMS_MB"), MB_CASES("TFIDF_TRANSFORM_MB"),
    MB_CASES("TFIDF_DEDUP_MB"), MB_CASES("TFIDF_NB_MB"), MB_CASES("TFIDF_KMEANS_MB"),
    /* TFIDF_KMEANS_SPLIT: 1 .. 1024 */
    {"TFIDF_KMEANS_SPLIT", nullptr, REJ}, {"TFIDF_KMEANS_SPLIT", "", REJ}, {"TFIDF_KMEANS_SPLIT", "0", REJ},
    {"TFIDF_KMEANS_SPLIT", "1", 1}, {"TFIDF_KMEANS_SPLIT", "1024", 1024}, {"TFIDF_KMEANS_SPLIT", "1025", REJ},
    {"TFIDF_KMEANS_SPLIT", "0x10", 16}, {"TFIDF_KMEANS_SPLIT", "8x", 8}, {"TFIDF_KMEANS_SPLIT", "010", 8},
    {"TFIDF_KMEANS_SPLIT", "-1", REJ}, {"TFIDF_KMEANS_SPLIT", "4294967297", REJ},   /* no 32-bit reading here */
    /* TFIDF_AN_GRID: 1 .. 65536 */
    {"TFIDF_AN_GRID", nullptr, REJ}, {"TFIDF_AN_GRID", "", REJ}, {"TFIDF_AN_GRID", "0", REJ}, {"TFIDF_AN_GRID", "1", 1},
    {"TFIDF_AN_GRID", "65536", 65536}, {"TFIDF_AN_GRID", "65537", REJ}, {"TFIDF_AN_GRID", "0x100", 256},
    {"TFIDF_AN_GRID", "12 groups", 12}, {"TFIDF_AN_GRID", "-1", REJ},
    /* TFIDF_GRID_CUS: 1 .. 4096 */
    {"TFIDF_GRID_CUS", nullptr, REJ}, {"TFIDF_GRID_CUS", "", REJ}, {"TFIDF_GRID_CUS", "0", REJ}, {"TFIDF_GRID_CUS", "1", 1},
    {"TFIDF_GRID_CUS", "4096", 4096}, {"TFIDF_GRID_CUS", "4097", REJ}, {"TFIDF_GRID_CUS", "0x20", 32},
    {"TFIDF_GRID_CUS", "64cu", 64}, {"TFIDF_GRID_CUS", "-1", REJ},
    /* TFIDF_VCAP: a power of two from 1024 on; no upper bound was ever checked */
    {"TFIDF_VCAP", nullptr, REJ}, {"TFIDF_VCAP", "", REJ}, {"TFIDF_VCAP", "1023", REJ}, {"TFIDF_VCAP", "512", REJ},
    {"TFIDF_VCAP", "1024", 1024}, {"TFIDF_VCAP", "9223372036854775808", 9223372036854775808ull},
    {"TFIDF_VCAP", "9223372036854775809", REJ}, {"TFIDF_VCAP", "18446744073709551616", REJ},
    {"TFIDF_VCAP", "0x100000", 1048576}, {"TFIDF_VCAP", "2048k", 2048}, {"TFIDF_VCAP", "3000", REJ},
    {"TFIDF_VCAP", "1536", REJ}, {"TFIDF_VCAP", "-1", REJ},
    PCT_CASES("TFIDF_VLOAD_BIG"), PCT_CASES("TFIDF_VLOAD"),
};

/* every knob of the table is one tfidf_open read, by name, and no other */
const char* const kNames[] = {"TFIDF_SL_MAXCAP", "TFIDF_QUERY_ACC_MB", "TFIDF_TERMS_MB", "TFIDF_TRANSFORM_MB",
                              "TFIDF_DEDUP_MB", "TFIDF_NB_MB", "TFIDF_KMEANS_MB", "TFIDF_KMEANS_SPLIT", "TFIDF_AN_GRID",
                              "TFIDF_GRID_CUS", "TFIDF_VCAP", "TFIDF_VLOAD_BIG", "TFIDF_VLOAD"};

const Knob* find(const char* name) {
    for (const Knob& k : kKnobs)
        if (!strcmp(k.name, name)) return &k;
    return nullptr;
}

}  // namespace

int main() {
    int bad = 0;
    const size_t nnames = sizeof kNames / sizeof kNames[0];
    if ((size_t)KNOB_COUNT != nnames) { printf("the table has %d entries, want %zu\n", (int)KNOB_COUNT, nnames); ++bad; }
    for (const char* n : kNames) {
        int seen = 0, cases = 0;
        for (const Knob& k : kKnobs) seen += !strcmp(k.name, n);
        for (const Case& c : kCases) cases += !strcmp(c.name, n);
        if (seen != 1 || cases < 9) { printf("%s: %d table entries, %d cases\n", n, seen, cases); ++bad; }
    }
    for (const Case& c : kCases) {
        const Knob* k = find(c.name);
        if (!k) { printf("%s: not in the table\n", c.name); ++bad; continue; }
        const uint64_t untouched = 0x5EED5EED5EED5EEDull;
        uint64_t v = untouched;
        const bool ok = knob_parse(*k, c.text, &v);
        const bool want_ok = c.want != REJ;
        if (ok != want_ok || (ok && v != c.want) || (!ok && v != untouched)) {
            printf("%s=%s: accepted %d value %llu, want accepted %d value %llu\n", c.name, c.text ? c.text : "(unset)", (int)ok,
                   (unsigned long long)v, (int)want_ok, (unsigned long long)c.want);
            ++bad;
        }
    }
    if (bad) { printf("%d FAILED\n", bad); return 1; }
    printf("%zu cases ok\n", sizeof kCases / sizeof kCases[0]);
    return 0;
}
