/*
 * analyze_tab.h — the analyzer's stop-word table (include/tfidf.h, section "analyzer"): one
 * layout and one hash for the host function (analyze_host.c) and the device kernel
 * (analyze.hip), so the CPU tests of tfidf_analyze_host cover the table's collisions too.
 *
 * A token is hashed and compared four bytes at a time: chunk k = its bytes 4k..4k+3 as a
 * little-endian word, the last one zero-padded.  Both sides read the chunks from aligned 32-bit
 * words and a byte shift (an_chunk): the kernel from the tile in LDS, where a token starts at any
 * byte; the host from a zero-padded copy of the token.
 *
 * The table is one blob of 32-bit words, built on the host once per call:
 *   word 0  nslots      a power of two >= 2 x the list's words (0: no list)
 *   word 1  nwords      distinct words inserted
 *   word 2  words_off   byte offset of the word chunks inside the blob (16-byte aligned)
 *   word 3  blob_bytes  the whole blob, a multiple of 16
 *   word 4..            nslots entries, open addressing with linear probing; 0 = empty, else
 *                         bits  0..14  index of the word's first chunk
 *                         bits 15..21  its length in bytes, 1..64
 *                         bits 22..31  the hash's top 10 bits (a mismatch skips the compare)
 *   words_off..         every distinct word as its chunks (each word padded to whole chunks)
 * Load is at most 1/2, so a probe run ends at an empty slot.
 */
#ifndef TFIDF_ANALYZE_TAB_H
#define TFIDF_ANALYZE_TAB_H

#include <stdint.h>

#ifdef __HIPCC__
#define AN_FN __host__ __device__ static inline
#else
#define AN_FN static inline
#endif

#define AN_HDR_WORDS 4u
#define AN_HASH_INIT 2166136261u

AN_FN int an_is_sep(uint32_t c) { return c == 0x20u || (c - 0x09u) <= 4u; }

/* chunk k of the len-byte token that starts `shift` bytes (0..3) into aw[0] */
AN_FN uint32_t an_chunk(const uint32_t* aw, uint32_t shift, uint32_t k, uint32_t len) {
    uint32_t c = shift ? (aw[k] >> (8u * shift)) | (aw[k + 1u] << (32u - 8u * shift)) : aw[k];
    const uint32_t rem = len - 4u * k;
    if (rem < 4u) c &= (1u << (8u * rem)) - 1u;
    return c;
}

/* FNV-1a's step on whole chunks, the length, then one xor-shift so the slot bits see the high bits */
AN_FN uint32_t an_hash(const uint32_t* aw, uint32_t shift, uint32_t len) {
    uint32_t h = AN_HASH_INIT;
    for (uint32_t k = 0; 4u * k < len; ++k) h = (h ^ an_chunk(aw, shift, k, len)) * 16777619u;
    h = (h ^ len) * 16777619u;
    return h ^ (h >> 15);
}

AN_FN uint32_t an_entry(uint32_t first, uint32_t len, uint32_t h) { return first | (len << 15) | ((h >> 22) << 22); }

/* 1 when the token (1 <= len <= 64, hash h) is a word of the table */
AN_FN int an_tab_find(const uint32_t* slots, uint32_t nslots, const uint32_t* words, const uint32_t* aw, uint32_t shift,
                      uint32_t len, uint32_t h) {
    const uint32_t want = an_entry(0u, len, h);
    for (uint32_t i = h & (nslots - 1u), n = 0; n < nslots; i = (i + 1u) & (nslots - 1u), ++n) {
        const uint32_t e = slots[i];
        if (!e) return 0;
        if ((e & ~0x7FFFu) != want) continue;
        const uint32_t* w = words + (e & 0x7FFFu);
        uint32_t k = 0;
        while (4u * k < len && w[k] == an_chunk(aw, shift, k, len)) ++k;
        if (4u * k >= len) return 1;
    }
    return 0;
}

#ifdef __cplusplus
extern "C" {
#endif
struct tfidf_analyzer;
/* an upper bound of the blob's bytes for a checked analyzer (a header of its own when the list is empty) */
uint32_t tfidf_an_table_bytes(const struct tfidf_analyzer* an);
/* fills blob (tfidf_an_table_bytes bytes, 4-byte aligned); returns the bytes used, a multiple of 16 */
uint32_t tfidf_an_table_build(const struct tfidf_analyzer* an, uint32_t* blob);
#ifdef __cplusplus
}
#endif

#endif
