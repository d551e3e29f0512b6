/*
 * analyze_host.c — the analyzer on the host (include/tfidf.h, section "analyzer"): the check
 * of a tfidf_analyzer, the build of its stop-word table (analyze_tab.h: the blob the device
 * kernel copies into LDS), tfidf_stem_porter, the Porter stemmer byte by byte, the UTF-8
 * sequence map of TFIDF_AN_UTF8 byte by byte, and tfidf_analyze_host, the definition in plain C.  No HIP here: the file also links into a
 * stand-alone test program.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/tfidf.h"
#include "analyze_tab.h"
#define AN_U8_NO_T2   /* the ranges alone: the direct table is the kernel's */
#include "analyze_utf8_tab.h"

int tfidf_analyzer_check(const tfidf_analyzer* an) {
    if (!an || an->size < sizeof(tfidf_analyzer)) return TFIDF_E_INVAL;
    if (an->flags & ~(TFIDF_AN_LOWER | TFIDF_AN_PUNCT | TFIDF_AN_UTF8)) return TFIDF_E_INVAL;
    if (an->min_len > TFIDF_AN_MAX_WORD) return TFIDF_E_INVAL;
    if (an->nstop > TFIDF_AN_MAX_STOP) return TFIDF_E_INVAL;
    if (an->stemmer > TFIDF_STEM_PORTER) return TFIDF_E_INVAL;
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

/* ------------------------------------------------------------ Porter 1980 ----
 * The paper's rules on a word b[0, n), one byte at a time: the second opinion on the kernel's
 * bit-mask form (analyze_stem.h).  A step works on (b, n) and returns the new n. */

/* b[i] is a consonant: a letter other than a, e, i, o, u and other than a y behind a consonant */
static int st_cons(const uint8_t* b, uint32_t i) {
    switch (b[i]) {
        case 'a': case 'e': case 'i': case 'o': case 'u': return 0;
        case 'y': return i == 0 || !st_cons(b, i - 1u);
        default: return 1;
    }
}

/* m of b[0, n) = [C](VC)^m[V] */
static uint32_t st_m(const uint8_t* b, uint32_t n) {
    uint32_t m = 0;
    for (uint32_t i = 1; i < n; ++i) m += st_cons(b, i) && !st_cons(b, i - 1u);
    return m;
}

/* *v*: b[0, n) contains a vowel */
static int st_vowel(const uint8_t* b, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i)
        if (!st_cons(b, i)) return 1;
    return 0;
}

/* *d: b[0, n) ends in a double consonant */
static int st_double(const uint8_t* b, uint32_t n) { return n >= 2u && b[n - 1u] == b[n - 2u] && st_cons(b, n - 1u); }

/* *o: b[0, n) ends consonant, vowel, consonant and the last is not w, x or y */
static int st_cvc(const uint8_t* b, uint32_t n) {
    if (n < 3u || !st_cons(b, n - 3u) || st_cons(b, n - 2u) || !st_cons(b, n - 1u)) return 0;
    return b[n - 1u] != 'w' && b[n - 1u] != 'x' && b[n - 1u] != 'y';
}

static int st_ends(const uint8_t* b, uint32_t n, const char* s) {
    const uint32_t k = (uint32_t)strlen(s);
    return k <= n && !memcmp(b + n - k, s, k);
}

/* b[0, stem) followed by r */
static uint32_t st_set(uint8_t* b, uint32_t stem, const char* r) {
    const uint32_t k = (uint32_t)strlen(r);
    memcpy(b + stem, r, k);
    return stem + k;
}

typedef struct { const char *suffix, *to; } st_rule;

/* the longest suffix of the list that b[0, n) ends in, or NULL */
static const st_rule* st_longest(const uint8_t* b, uint32_t n, const st_rule* rules, uint32_t nrules) {
    const st_rule* best = NULL;
    for (uint32_t i = 0; i < nrules; ++i)
        if (st_ends(b, n, rules[i].suffix) && (!best || strlen(rules[i].suffix) > strlen(best->suffix))) best = rules + i;
    return best;
}

static uint32_t st_step1a(uint8_t* b, uint32_t n) {
    if (st_ends(b, n, "sses") || st_ends(b, n, "ies")) return n - 2u;
    if (st_ends(b, n, "ss")) return n;
    return st_ends(b, n, "s") ? n - 1u : n;
}

static uint32_t st_step1b(uint8_t* b, uint32_t n) {
    if (st_ends(b, n, "eed")) return st_m(b, n - 3u) > 0 ? n - 1u : n;
    uint32_t stem;
    if (st_ends(b, n, "ed")) stem = n - 2u;
    else if (st_ends(b, n, "ing")) stem = n - 3u;
    else return n;
    if (!st_vowel(b, stem)) return n;
    if (st_ends(b, stem, "at") || st_ends(b, stem, "bl") || st_ends(b, stem, "iz")) return st_set(b, stem, "e");
    if (st_double(b, stem) && b[stem - 1u] != 'l' && b[stem - 1u] != 's' && b[stem - 1u] != 'z') return stem - 1u;
    if (st_m(b, stem) == 1u && st_cvc(b, stem)) return st_set(b, stem, "e");
    return stem;
}

static uint32_t st_step1c(uint8_t* b, uint32_t n) {
    if (st_ends(b, n, "y") && st_vowel(b, n - 1u)) b[n - 1u] = 'i';
    return n;
}

static const st_rule ST_STEP2[] = {
    {"ational", "ate"}, {"tional", "tion"}, {"enci", "ence"}, {"anci", "ance"}, {"izer", "ize"}, {"abli", "able"},
    {"alli", "al"}, {"entli", "ent"}, {"eli", "e"}, {"ousli", "ous"}, {"ization", "ize"}, {"ation", "ate"},
    {"ator", "ate"}, {"alism", "al"}, {"iveness", "ive"}, {"fulness", "ful"}, {"ousness", "ous"}, {"aliti", "al"},
    {"iviti", "ive"}, {"biliti", "ble"}};
static const st_rule ST_STEP3[] = {{"icate", "ic"}, {"ative", ""}, {"alize", "al"}, {"iciti", "ic"},
                                   {"ical", "ic"},  {"ful", ""},   {"ness", ""}};
static const st_rule ST_STEP4[] = {{"al", ""},  {"ance", ""}, {"ence", ""}, {"er", ""},  {"ic", ""},  {"able", ""}, {"ible", ""},
                                   {"ant", ""}, {"ement", ""}, {"ment", ""}, {"ent", ""}, {"ion", ""}, {"ou", ""},   {"ism", ""},
                                   {"ate", ""}, {"iti", ""},  {"ous", ""},  {"ive", ""}, {"ize", ""}};
#define ST_COUNT(a) ((uint32_t)(sizeof(a) / sizeof((a)[0])))

/* steps 2 to 4: the longest suffix of the list, replaced when m of the stem in front of it is > min_m */
static uint32_t st_replace(uint8_t* b, uint32_t n, const st_rule* rules, uint32_t nrules, uint32_t min_m) {
    const st_rule* r = st_longest(b, n, rules, nrules);
    if (!r) return n;
    const uint32_t stem = n - (uint32_t)strlen(r->suffix);
    if (st_m(b, stem) <= min_m) return n;
    if (!strcmp(r->suffix, "ion") && min_m == 1u && !(stem && (b[stem - 1u] == 's' || b[stem - 1u] == 't'))) return n;
    return st_set(b, stem, r->to);
}

static uint32_t st_step5a(uint8_t* b, uint32_t n) {
    if (!st_ends(b, n, "e")) return n;
    const uint32_t m = st_m(b, n - 1u);
    return (m > 1u || (m == 1u && !st_cvc(b, n - 1u))) ? n - 1u : n;
}

static uint32_t st_step5b(uint8_t* b, uint32_t n) {
    return (st_m(b, n) > 1u && st_double(b, n) && b[n - 1u] == 'l') ? n - 1u : n;
}

int tfidf_stem_porter(uint8_t* word, uint32_t len) {
    if (!word) return len ? TFIDF_E_INVAL : 0;
    if (len < 3u || len > TFIDF_AN_MAX_WORD) return (int)len;
    for (uint32_t i = 0; i < len; ++i)
        if (word[i] < 0x61u || word[i] > 0x7Au) return (int)len;
    uint8_t b[TFIDF_AN_MAX_WORD + 1u];   /* step 1b may append an e to a shortened word: never past len */
    memcpy(b, word, len);
    uint32_t n = len;
    n = st_step1a(b, n);
    n = st_step1b(b, n);
    n = st_step1c(b, n);
    n = st_replace(b, n, ST_STEP2, ST_COUNT(ST_STEP2), 0u);
    n = st_replace(b, n, ST_STEP3, ST_COUNT(ST_STEP3), 0u);
    n = st_replace(b, n, ST_STEP4, ST_COUNT(ST_STEP4), 1u);
    n = st_step5a(b, n);
    n = st_step5b(b, n);
    /* 1 <= n <= len by the rules: no replacement is longer than its suffix, 1b's e follows a
     * removal of two or more letters, and every removal leaves a vowel (1b), m > 0 (2 to 5) or,
     * in 1a with len >= 3, a letter.  The check guards the copy all the same. */
    if (n < 1u || n > len) return TFIDF_E_INVAL;
    memcpy(word, b, n);
    return (int)n;
}

/* --------------------------------------------------------- TFIDF_AN_UTF8 ----
 * The sequence map byte by byte, with the well-formed byte ranges of the Unicode standard's
 * table 3-7 and a linear walk over the tables: the second opinion on analyze_utf8.h. */

/* the length of the well-formed sequence at s[0, avail) and its code point, or 0 */
static uint32_t u8_seq(const uint8_t* s, uint64_t avail, uint32_t* cp) {
    const uint32_t b0 = s[0];
    uint32_t len, lo1 = 0x80u, hi1 = 0xBFu;
    if (b0 >= 0xC2u && b0 <= 0xDFu) len = 2u;
    else if (b0 >= 0xE0u && b0 <= 0xEFu) {
        len = 3u;
        if (b0 == 0xE0u) lo1 = 0xA0u;   /* no overlong form */
        if (b0 == 0xEDu) hi1 = 0x9Fu;   /* no surrogate */
    } else if (b0 >= 0xF0u && b0 <= 0xF4u) {
        len = 4u;
        if (b0 == 0xF0u) lo1 = 0x90u;
        if (b0 == 0xF4u) hi1 = 0x8Fu;   /* nothing above U+10FFFF */
    } else return 0u;
    if (avail < len || s[1] < lo1 || s[1] > hi1) return 0u;
    for (uint32_t k = 2; k < len; ++k)
        if (s[k] < 0x80u || s[k] > 0xBFu) return 0u;
    if (len == 2u) *cp = ((b0 & 0x1Fu) << 6) | (s[1] & 0x3Fu);
    else if (len == 3u) *cp = ((b0 & 0x0Fu) << 12) | ((uint32_t)(s[1] & 0x3Fu) << 6) | (s[2] & 0x3Fu);
    else *cp = ((b0 & 0x07u) << 18) | ((uint32_t)(s[1] & 0x3Fu) << 12) | ((uint32_t)(s[2] & 0x3Fu) << 6) | (s[3] & 0x3Fu);
    return len;
}

static int u8_is_blank(uint32_t cp) {
    for (uint32_t i = 0; i < AN_U8_NBLANK; ++i)
        if (cp >= AN_U8_BLANK[i].lo && cp <= AN_U8_BLANK[i].hi) return 1;
    return 0;
}

/* L(cp), or 0 for a code point outside FOLD */
static uint32_t u8_lower(uint32_t cp) {
    for (uint32_t i = 0; i < AN_U8_NFOLD; ++i) {
        const an_u8_fold* f = AN_U8_FOLD + i;
        if (cp >= f->lo && cp <= f->hi && (cp - f->lo) % f->stride == 0u) return (uint32_t)((int32_t)cp + f->delta);
    }
    return 0u;
}

/* the sequences that lie wholly inside the document s[0, n) */
static void u8_map_doc(uint8_t* s, uint64_t n, uint32_t flags) {
    for (uint64_t i = 0; i < n;) {
        uint32_t cp = 0;
        const uint32_t len = s[i] >= 0x80u ? u8_seq(s + i, n - i, &cp) : 0u;
        if (!len) { ++i; continue; }
        uint32_t lc;
        if ((flags & TFIDF_AN_PUNCT) && u8_is_blank(cp)) memset(s + i, 0x20, len);
        else if ((flags & TFIDF_AN_LOWER) && (lc = u8_lower(cp)) != 0u) {   /* the same length: FOLD's definition */
            if (len == 2u) {
                s[i] = (uint8_t)(0xC0u | (lc >> 6));
                s[i + 1] = (uint8_t)(0x80u | (lc & 0x3Fu));
            } else if (len == 3u) {
                s[i] = (uint8_t)(0xE0u | (lc >> 12));
                s[i + 1] = (uint8_t)(0x80u | ((lc >> 6) & 0x3Fu));
                s[i + 2] = (uint8_t)(0x80u | (lc & 0x3Fu));
            } else {
                s[i] = (uint8_t)(0xF0u | (lc >> 18));
                s[i + 1] = (uint8_t)(0x80u | ((lc >> 12) & 0x3Fu));
                s[i + 2] = (uint8_t)(0x80u | ((lc >> 6) & 0x3Fu));
                s[i + 3] = (uint8_t)(0x80u | (lc & 0x3Fu));
            }
        }
        i += len;
    }
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
        if ((an->flags & TFIDF_AN_UTF8) && (an->flags & (TFIDF_AN_LOWER | TFIDF_AN_PUNCT))) u8_map_doc(out + b, e - b, an->flags);
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
                else if (an->stemmer == TFIDF_STEM_PORTER) {
                    const int st = tfidf_stem_porter(out + i, (uint32_t)len);   /* ineligible: len, nothing written */
                    if (st < 0) { free(blob); return st; }
                    memset(out + i + st, 0x20, (size_t)(len - (uint64_t)st));
                }
            }
            i = j;
        }
    }
    free(blob);
    return TFIDF_OK;
}
