/*
 * utf8_host_test.c — the kernel's form of the UTF-8 sequence map (csrc/analyze_utf8.h, plain C
 * as well) against the byte-wise one of tfidf_analyze_host (csrc/analyze_host.c), as a
 * stand-alone program: built with -fsanitize=address,undefined by tests/test_utf8_native.py.
 * Links only analyze_host.c.  Every buffer is a heap block of its exact size, so a read outside
 * in[0, nbytes) is a report.  Exit status 0: every case passed.
 *
 * The buffers: every two-byte pattern C0..DF x 80..BF and every three-byte pattern E0..EF x
 * 80..BF x 80..BF, each followed by a blank, and F0 x 90..9F x 80..BF x 80..BF likewise; whole
 * and cut short inside their last sequence; as one document, and as documents of 1001 bytes
 * inside a window, whose boundaries fall inside sequences; the input at every byte shift 0..15.
 * They hold no ASCII byte but the blank, so the byte map of the ASCII bytes is the identity.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"
#include "../../parallel-systems-mpi-tfidf_amd/csrc/analyze_utf8.h"

static int g_fail = 0;
static unsigned long g_groups = 0, g_changed = 0;

/* what k_an_docstarts leaves: bit i = a document starts at byte i, lo < i < hi */
static uint32_t* doc_starts(const uint64_t* off, uint32_t n, uint64_t nbytes) {
    uint32_t* ds = (uint32_t*)calloc((size_t)(nbytes / 32u + 2u), 4);
    for (uint32_t d = 1; d < n; ++d) {
        const uint64_t pos = off[d];
        if (pos <= off[0] || pos >= off[n] || pos >= nbytes) continue;
        ds[pos >> 5] |= 1u << (pos & 31u);
    }
    return ds;
}

/* what the kernels do with a group, for every group of in[0, nbytes) */
static uint64_t group_map(const uint8_t* in, uint64_t nbytes, const uint64_t* off, uint32_t n, uint32_t flags, uint8_t* out) {
    const uint64_t lo = n ? off[0] : 0, hi = n ? off[n] : 0;
    uint32_t* ds = doc_starts(off, n, nbytes);
    uint64_t changed = 0;
    for (uint64_t p = 0; p < nbytes; p += 16u) {
        uint32_t c[6], g[4];
        for (int k = 0; k < 6; ++k) c[k] = an_u8_ld4(in, nbytes, (long long)p - 4 + 4 * k);
        memcpy(g, c + 1, 16);
        const int inside = p + 16u > lo && p < hi;   /* range16 != 0 */
        if (inside && an_u8_any(c + 1))
            changed += an_u8_group(c, an_u8_range24((long long)p, lo, hi), an_u8_cut24(ds, (long long)p, lo, hi), flags, g);
        const uint64_t m = nbytes - p < 16u ? nbytes - p : 16u;
        memcpy(out + p, g, (size_t)m);
        ++g_groups;
    }
    free(ds);
    return changed;
}

static uint8_t* exhaustive_23(uint64_t* nbytes) {
    uint8_t* b = (uint8_t*)malloc(32u * 64u * 3u + 16u * 64u * 64u * 4u);
    uint64_t n = 0;
    for (uint32_t a = 0xC0u; a < 0xE0u; ++a)
        for (uint32_t x = 0x80u; x < 0xC0u; ++x) { b[n++] = (uint8_t)a; b[n++] = (uint8_t)x; b[n++] = 0x20u; }
    for (uint32_t a = 0xE0u; a < 0xF0u; ++a)
        for (uint32_t x = 0x80u; x < 0xC0u; ++x)
            for (uint32_t y = 0x80u; y < 0xC0u; ++y) { b[n++] = (uint8_t)a; b[n++] = (uint8_t)x; b[n++] = (uint8_t)y; b[n++] = 0x20u; }
    *nbytes = n;
    return b;
}

static uint8_t* exhaustive_4(uint64_t* nbytes) {
    uint8_t* b = (uint8_t*)malloc(16u * 64u * 64u * 5u);
    uint64_t n = 0;
    for (uint32_t x = 0x90u; x < 0xA0u; ++x)
        for (uint32_t y = 0x80u; y < 0xC0u; ++y)
            for (uint32_t z = 0x80u; z < 0xC0u; ++z) {
                b[n++] = 0xF0u; b[n++] = (uint8_t)x; b[n++] = (uint8_t)y; b[n++] = (uint8_t)z; b[n++] = 0x20u;
            }
    *nbytes = n;
    return b;
}

/* the first nbytes of src as documents (split: 1001 bytes each inside a window, else one) under
 * flags: the byte-wise host map once, the group map at every shift of the input */
static void cross(const char* name, const uint8_t* src, uint64_t nbytes, int split, uint32_t flags) {
    uint32_t n = 1;
    uint64_t* off;
    if (split) {
        const uint64_t lead = 37, trail = 21, step = 1001;
        n = (uint32_t)((nbytes - lead - trail + step - 1u) / step);
        off = (uint64_t*)malloc(((size_t)n + 3u) * 8u);
        for (uint32_t d = 0; d < n; ++d) off[d] = lead + d * step;
        off[n] = nbytes - trail;
        off[n + 1u] = off[n];          /* and an empty document at the end */
        ++n;
    } else {
        off = (uint64_t*)malloc(2u * 8u);
        off[0] = 0;
        off[1] = nbytes;
    }
    tfidf_analyzer an;
    memset(&an, 0, sizeof(an));
    an.size = sizeof(an);
    an.flags = flags | TFIDF_AN_UTF8;
    uint8_t* exact = (uint8_t*)malloc((size_t)nbytes);
    uint8_t* want = (uint8_t*)malloc((size_t)nbytes);
    uint8_t* got = (uint8_t*)malloc((size_t)nbytes);
    memcpy(exact, src, (size_t)nbytes);
    if (tfidf_analyze_host(&an, exact, nbytes, off, n, want) != TFIDF_OK) { printf("FAIL %s: host rc\n", name); ++g_fail; }
    uint64_t first = 0;
    for (uint32_t shift = 0; shift < 16u; ++shift) {
        uint8_t* base = (uint8_t*)malloc((size_t)nbytes + shift);   /* 16-byte aligned: in's low address bits are shift */
        memset(base, 0xE2, shift);                                  /* a lead in front of in[0]: reading it shows */
        memcpy(base + shift, src, (size_t)nbytes);
        memset(got, 0xEE, (size_t)nbytes);
        const uint64_t changed = group_map(base + shift, nbytes, off, n, flags, got);
        if (shift == 0u) first = changed;
        if (memcmp(got, want, (size_t)nbytes) != 0 || changed != first) {
            uint64_t at = 0;
            while (at < nbytes && got[at] == want[at]) ++at;
            if (g_fail < 20)
                printf("FAIL %s: nbytes %llu split %d flags %u shift %u at %llu (changed %llu, %llu)\n", name, (unsigned long long)nbytes,
                       split, flags, shift, (unsigned long long)at, (unsigned long long)changed, (unsigned long long)first);
            ++g_fail;
        }
        free(base);
    }
    if (!first && nbytes > 1000u) { printf("FAIL %s: nothing changed\n", name); ++g_fail; }
    g_changed += first;
    free(exact);
    free(want);
    free(got);
    free(off);
}

int main(void) {
    uint64_t n23 = 0, n4 = 0;
    uint8_t* b23 = exhaustive_23(&n23);
    uint8_t* b4 = exhaustive_4(&n4);
    for (uint32_t flags = 1; flags <= 3u; ++flags)
        for (int split = 0; split < 2; ++split) {
            cross("two and three bytes", b23, n23, split, flags);
            cross("four bytes", b4, n4, split, flags);
        }
    /* the buffer ends inside its last sequence, and the window does */
    for (uint64_t k = 2; k <= 4u; ++k)
        for (int split = 0; split < 2; ++split) {
            if (k <= 3u) cross("three bytes cut", b23, n23 - k, split, 3u);
            cross("four bytes cut", b4, n4 - k, split, 3u);
        }
    /* short buffers: fewer bytes than a group, and a sequence across the first group edge */
    static const uint8_t small[] = {0xC3, 0x89, 0x20, 0xE2, 0x80, 0x9C, 0x20, 0xF0, 0x9F, 0x98, 0x80, 0x20, 0xD0, 0x96,
                                    0xF0, 0x90, 0x90, 0x80, 0xE1, 0xB8, 0x80};
    for (uint64_t k = 1; k <= sizeof(small); ++k) cross("short", small, k, 0, 3u);
    free(b23);
    free(b4);
    if (g_fail) { printf("%d failures\n", g_fail); return 1; }
    printf("%lu groups, %lu sequences changed\nok\n", g_groups, g_changed);
    return 0;
}
