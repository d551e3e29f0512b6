/* kernels.h — parameter blocks and host launchers of the TF-IDF path kernels. */
#ifndef TFIDF_KERNELS_H
#define TFIDF_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prims.h"

/* chunking (K0/K1) */
#define K1_NT        256                 /* threads per tokenize+count workgroup */
#define K1_WIN       (K1_NT * 16)        /* bytes per window: one 16-byte group per thread */
#ifndef CHUNK_BYTES
#define CHUNK_BYTES  12288u              /* nominal chunk (work unit) size: tokcount_vs / general
                                            (c4: 16 -> 12 KiB snapped to document starts keeps more
                                            chunks under the LDS table's fill limit: 8.2 M -> fewer
                                            partial records, merge 0.92 -> 0.68 ms, K1 +0.04 ms) */
#endif
#ifndef CHUNK_BYTES_ST
#define CHUNK_BYTES_ST 24576u            /* ... and tokcount_sl/st's: their per-chunk set-up, flush and
                                            barrier wait over 1.5x the bytes (c2 K1 -3 %, c5 -5 %) */
#endif
#ifndef DENSE_DOC
#define DENSE_DOC    (4ull << 20)        /* documents longer than this: dense merge of their partial records */
#endif
#define BIG_LIST_CAP 4096u               /* dense-merge candidates K0 lists */
#define DENSE_REP    16u                 /* copies of each dense per-document array (spreads hot-term atomics) */
#ifndef BIG_DOC
#define BIG_DOC      49152u              /* documents longer than this are split across chunks */
#endif
#ifndef K5_MAX_PAIRS
#define K5_MAX_PAIRS 4096                /* largest complete (unmerged) document K5 sorts in LDS */
#endif
/* The thresholds at which the DF and score stages of finalize.hip switch form: here, not in
 * finalize.hip, so that tests/native/finalize_test.cpp builds its cases from them. */
constexpr uint32_t DFH_RECS = 65535;      /* records per workgroup up to which no u16 bin can wrap */
constexpr uint32_t DFH_MAXV = 65536;      /* the largest V the LDS histogram takes */
constexpr uint32_t DFS_NT = 1024;
constexpr uint32_t DFS_PER = 16;
constexpr uint64_t DFS_TILE = (uint64_t)DFS_NT * DFS_PER;   /* records per tile of the sliced form */
constexpr uint32_t DFS_SLICE = 32768;      /* u32 bins: 128 KB of LDS */
constexpr uint32_t DFS_MAXSL = 4096;       /* slice histogram: 16 KB of LDS (V <= 134 M) */
constexpr uint32_t K5_SMALL_DOC = 128; /* documents up to this many pairs: k_score_small */
constexpr uint32_t K5_PS_SPLIT = 4096; /* presorted documents over this many pairs: chunk tasks */
constexpr uint32_t K5_WAVE = 1024;    /* one wave, LDS radix sort of packed (rank, index) keys */
constexpr uint32_t K5_IDX_BITS = 11;  /* index bits of a packed key (n <= 2048) */
constexpr uint32_t K5_NB_BITS = 9;    /* bucket sort: 512 buckets by the rank's top bits */
constexpr uint32_t K5_GROUP_MAX = 48; /* larger buckets (skewed ranks): the radix path */
constexpr uint32_t K5L_GROUP_MAX = 32; /* k_score_large: larger buckets (skewed ranks) take the radix path */
constexpr int K5S_WG = 4;   /* k_score_small: waves per workgroup */
#ifndef K5S_OCC
#define K5S_OCC 6           /* k_score_small: workgroups per CU it is compiled for */
#endif

/* status bits (device word) */
#define ST_VOCAB_FULL  1u
#define ST_VOCAB_SPIN  2u
#define ST_REC_FULL    4u
#define ST_PART_FULL   8u
#define ST_BOUNDS      16u   /* internal consistency guard tripped (a bug, reported as an error) */
#define ST_HAS_LONG    64u   /* the vocabulary holds terms of >= 16 bytes (their order needs vocab_long_fixup) */
#define ST_TERM_LONG   32u   /* a term of >= 16 MiB: beyond the 24-bit length of a long key's rep */
#define ST_LONG_COLLIDE 128u /* two distinct terms of >= 16 bytes share their 120-bit key (dev_vocab.h) */

/* doc flags */
#define DF_PARTIAL     1u
#define DF_PRESORTED   2u

#define INVALID_SLOT   0xFFFFFFFFu

struct CorpusDev {
    const uint8_t* bytes;
    uint64_t nbytes;
    const uint64_t* doc_off;   /* ndocs + 1 */
    uint32_t ndocs;
    uint64_t lo, hi;           /* doc_off[0], doc_off[ndocs] (host-known) */
};

struct VocabDev {
    uint4* keys;               /* cap identity keys (see dev_common.h) */
    uint64_t* rep;             /* long terms: (len << 40) | byte offset */
    uint64_t mask;             /* cap - 1 */
};

struct K1Out {
    uint32_t* rec_slot;        /* complete documents' (term slot, count) records */
    uint32_t* rec_cnt;
    unsigned long long* rec_alloc;
    uint64_t rec_cap;
    uint32_t* part_doc;        /* records of documents split across flushes/chunks */
    uint32_t* part_slot;
    uint32_t* part_cnt;
    unsigned long long* part_alloc;
    uint64_t part_cap;
    uint64_t* doc_recoff;
    uint32_t* doc_npairs;
    uint32_t* doc_size;
    uint8_t* doc_flags;
    uint32_t* status;
    unsigned long long* ntokens;
    unsigned long long* chunk_ctr;   /* K1 dynamic chunk schedule (zeroed per run) */
    unsigned long long* chunk_shard; /* tokcount_st: 8 sharded chunk counters (zeroed per run) */
    unsigned long long* stamps;  /* diagnostic build only: K1_NSTAMP phase cycle sums, WG count,
                                    then K1_NCOUNT event counters */
};
#define K1_NSTAMP 17
#define K1_NCOUNT 4   /* segments, flushes, tokens taking the full probe, probe iterations */
#define K1_STAMP_WORDS (K1_NSTAMP + 1 + K1_NCOUNT)
#define K1_DEBUG_WORDS 16384   /* diagnostic builds: the stamps buffer's size in u64 words */

/* K0: chunk boundaries; chunk_start has nchunks+1 entries, chunk_doc nchunks */
int launch_plan_chunks(const CorpusDev& c, uint64_t nchunks, uint32_t chunk_bytes, uint64_t* chunk_start,
                       uint32_t* chunk_doc, uint32_t* big_list, unsigned long long* big_ctr, hipStream_t s);
/* K1: tokenize + per-document term counts for chunks [c0, c1) */
int launch_tokcount(const CorpusDev& c, const uint64_t* chunk_start, const uint32_t* chunk_doc,
                    uint64_t c0, uint64_t c1, const VocabDev& v, const K1Out& o, hipStream_t s);

/* The two persistent K1 kernels below launch min(chunks, ncu * 4) workgroups that claim chunks
 * from a global counter.  ncu: the context's CU count (ctx_ncu: the device's, or env
 * TFIDF_GRID_CUS), 0: the launcher asks the device; *grid (when not null) receives the
 * workgroups launched (0: none). */
/* K1 round-1 path (tokcount_vs.hip): 16-byte aligned corpus base; returns -3 when the
 * vocabulary capacity exceeds the LDS entry's slot field */
int launch_tokcount_vs(const CorpusDev& c, const uint64_t* chunk_start, const uint32_t* chunk_doc, uint64_t c0,
                       uint64_t c1, const VocabDev& v, const K1Out& o, hipStream_t s, uint32_t ncu = 0,
                       uint32_t* grid = nullptr);
#define K1_VS_MAX_CAP (1ull << 28)

#define K1_ST_MAX_CAP (1ull << 22)   /* tokcount_sl past this vocabulary capacity: half-size chunks */
#define K1_SL_MAX_CAP (1ull << 25)   /* the largest table tokcount_sl addresses (the default limit;
                                        TFIDF_SL_MAXCAP lowers it), tokcount_vs beyond */
/* K1 default (tokcount_sl.hip): one workgroup per chunk, straight-line rounds; the output
 * block is read from device memory (o_dev: a K1Out the engine copies there per run).
 * 16-byte aligned corpus base; -3 when the vocabulary exceeds K1_SL_MAX_CAP slots.
 * pack != 0 (tables up to K1_ST_MAX_CAP slots): a complete document's record leaves as one word
 * in rec_slot, count << sbits | slot (sbits = log2 of the capacity), and rec_cnt is not written
 * for it; a document with a count of 1 << (32 - sbits) or more leaves as partial records */
int launch_tokcount_sl(const CorpusDev& c, const uint64_t* chunk_start, const uint32_t* chunk_doc, uint64_t c0,
                       uint64_t c1, const VocabDev& v, const K1Out* o_dev, hipStream_t s, uint32_t ncu = 0,
                       uint32_t* grid = nullptr, uint32_t pack = 0);


/* vocabulary finalisation */
int launch_vocab_flags(const VocabDev& v, uint64_t cap, uint32_t* flags, hipStream_t s);
int launch_vocab_compact(const VocabDev& v, uint64_t cap, const uint32_t* dense_of_slot, const CorpusDev& c,
                         uint32_t* vslot, uint4* sortkey, uint32_t* seq, hipStream_t s);
/* large-V vocabulary sort as two u64 sorts: key halves (in seq order when seq != null) and
 * the sorted keys gathered back (long-term fix-up only) */
int launch_sortkey_half(const uint4* k, uint64_t n, const uint32_t* seq, int hi, uint64_t* out, hipStream_t s);
int launch_gather_u128(const uint4* k, const uint32_t* seq, uint64_t n, uint4* out, hipStream_t s);
/* several byte fills in one launch (a run's clears: one kernel instead of one per buffer);
 * each segment's base 16-byte aligned (device allocations are) */
constexpr int FILL_MAX = 8;
struct FillList {
    void* p[FILL_MAX];
    uint64_t bytes[FILL_MAX];
    uint32_t val[FILL_MAX];   /* the byte value, replicated */
    uint32_t n;
};
int launch_fill_multi(const FillList& l, hipStream_t s);
/* a few device words (4 or 8 bytes each) into pinned host memory in one launch (the run's
 * status reads: one small kernel instead of one copy per word) */
constexpr int WORDS_MAX = 16;
struct WordList {
    const void* src[WORDS_MAX];
    uint32_t bytes[WORDS_MAX];   /* 4 or 8 */
    uint32_t n;
    uint64_t token;              /* nonzero: written to dst[n] after the words (system-scope fence
                                    between): the host polls it instead of waiting on the stream */
};
int launch_words_to_host(const WordList& l, uint64_t* host_dst, hipStream_t s);
int launch_vocab_rank(const uint32_t* sorted_dense, const uint32_t* vslot, uint32_t V, uint32_t* rank_of_slot,
                      uint32_t* slot_of_rank, uint16_t* rank16, hipStream_t s);
/* long terms tied on their first 16 bytes: ordered by iterated segmented sorts (host loop,
 * one sync per 16 bytes of common prefix); -2 when the arena is too small */
/* the large-V sort's tie fix-up (finalize.hip): runs of equal first 8 bytes in the
 * prefix-sorted order re-ordered by the low halves (low_mask: their varying bytes) */
int launch_vocab_prefix_ties(const uint64_t* sorted_hi, uint32_t* sorted_dense, const uint4* skey, uint32_t V,
                             uint32_t low_mask, Arena& ar, hipStream_t s);
int launch_vocab_long_fixup(const uint4* sorted_keys, uint32_t* sorted_dense, const uint32_t* vslot,
                            const VocabDev& v, const CorpusDev& c, uint32_t V, Arena& ar, hipStream_t s);

/* partial documents: sort key (doc << 32 | rank) and merge */
int launch_part_keys(const uint32_t* part_doc, const uint32_t* part_slot, const uint32_t* rank_of_slot, uint64_t n,
                     uint64_t* keys, uint32_t* seq, hipStream_t s);
int launch_part_heads(const uint64_t* keys, uint64_t n, uint32_t* head, hipStream_t s);
int launch_part_merge(const uint64_t* keys, const uint32_t* seq, const uint32_t* part_cnt, const uint32_t* head_pos,
                      uint64_t n, const uint32_t* slot_of_rank, uint64_t rec_base, uint32_t* rec_slot,
                      uint32_t* rec_cnt, uint64_t* doc_recoff, uint32_t* doc_npairs, uint8_t* doc_flags,
                      hipStream_t s);
/* dense merge of the partial records of long documents (finalize.hip) */
int launch_part_dense(const uint32_t* part_doc, const uint32_t* part_slot, const uint32_t* part_cnt, uint64_t q,
                      const uint32_t* big_idx, const uint32_t* rank_of_slot, uint32_t V, uint32_t* dense,
                      uint64_t* keys, uint32_t* seq, uint32_t* cnt_out, uint32_t* nkeep, hipStream_t s);
int launch_set_big_idx(const uint32_t* big_list, uint32_t nb, uint32_t* big_idx, hipStream_t s);
int launch_dense_emit(const uint32_t* dense, uint32_t nb, uint32_t V, const uint32_t* big_list,
                      const uint32_t* slot_of_rank, uint64_t rec_base, uint32_t* merged_count, uint32_t* tile_cnt,
                      uint32_t* rec_slot, uint32_t* rec_cnt, uint64_t* doc_recoff, uint32_t* doc_npairs,
                      uint8_t* doc_flags, Arena& ar, hipStream_t s);

/* DF.  accumulate: add into df instead of overwriting it (the split DF of a run with
 * partial records, whose main records are counted beside the merge stage) */
/* bits of the largest term rank of V terms (K5Args.rank_bits) */
static inline uint32_t k5_rank_bits(uint32_t V) { return V > 1 ? 32u - (uint32_t)__builtin_clz(V - 1) : 1u; }
/* Packed records (K1's count << sbits | slot words, launch_tokcount_sl's pack) stay packed through
 * DF when the LDS histogram takes V and a rank fits the field the slot had: the count field then
 * keeps its 32 - sbits bits or more. */
static inline bool df_keeps_packed(uint32_t V, uint32_t sbits) {
    return V != 0 && V <= DFH_MAXV && sbits != 0 && sbits < 32 && k5_rank_bits(V) <= sbits;
}
/* pack_sbits != 0 (only where df_keeps_packed): records [0, nrec) are K1's packed words; each is
 * rewritten as rank << (32 - k5_rank_bits(V)) | count, the merged records after them as ever */
int launch_df_hist(uint32_t* rec_slot, uint64_t nrec, const uint32_t* nrec_extra, uint64_t nrec_max,
                   const uint32_t* rank_of_slot, const uint16_t* rank16, uint32_t V, uint64_t slot_cap,
                   uint32_t* status, uint32_t* df, Arena& ar, hipStream_t s, bool accumulate = false,
                   uint32_t pack_sbits = 0);
/* K1's packed records [0, n) of rec_slot (count << sbits | slot) back into two words: the slot in
 * rec_slot, the count in rec_cnt (runs whose DF pass or ranks do not take packed records) */
int launch_rec_unpack(uint32_t* rec_slot, uint32_t* rec_cnt, uint64_t n, uint32_t sbits, hipStream_t s);
/* device scratch launch_df_hist takes from its arena (an upper bound) */
size_t df_hist_scratch(uint64_t nrec_max, uint32_t V);
int launch_df_mark(const uint32_t* df, uint32_t V, uint32_t* present, hipStream_t s);
int launch_df_list(const uint32_t* present_scan, uint64_t nvals, uint32_t* vals, hipStream_t s);

/* documents: name order key and output */
int launch_doc_keys(const uint32_t* doc_ids, uint32_t ndocs, uint64_t* keys, uint32_t* seq, hipStream_t s);
int launch_gather_meta(const uint32_t* order, const uint32_t* doc_npairs, const uint64_t* doc_recoff,
                       const uint32_t* doc_size, const uint8_t* doc_flags, uint32_t ndocs, uint64_t* npairs_ord,
                       uint4* meta, hipStream_t s);
struct K5Args {
    const uint32_t* order;       /* docs in output order */
    const uint4* meta;           /* per output position: {recoff lo, hi, npairs | flags << 30, docSize} */
    const uint64_t* out_off;     /* per output position */
    const uint64_t* doc_recoff;
    const uint32_t* doc_npairs;
    const uint32_t* doc_size;
    const uint8_t* doc_flags;
    const uint32_t* rec_slot;
    const uint32_t* rec_cnt;
    const uint32_t* rank_of_slot;
    const uint32_t* df_of_rank;  /* global df */
    const uint32_t* idf_idx;     /* df value -> index into idf */
    const double* idf;
    double* idf_rank;            /* [nterms] scratch: idf of each term rank */
    uint32_t* large_list;        /* [ndocs] scratch: output positions left to k_score_large */
    uint32_t* large_count;
    uint32_t* cls_list;          /* [ndocs] scratch: output positions by kernel class — small documents
                                    (k_score_small), then the wave kernel's, then k_score_large's;
                                    null (wide ranks): the wave kernel takes every position */
    uint32_t* cls_off;           /* [3 * cls_nblk + 1] scratch: per-block class counts, scanned: the
                                    segments start at 0, [cls_nblk], [2 cls_nblk], end at [3 cls_nblk] */
    uint32_t cls_nblk;
    uint2* split_tasks;          /* (output position, chunk) of presorted documents over K5_PS_SPLIT pairs */
    uint32_t* split_count;       /*   null: k_score_large emits them whole */
    uint32_t split_cap;
    uint32_t ndocs;
    uint32_t nterms;
    uint32_t rank_bits;          /* bits of the largest term rank (radix passes) */
    uint32_t idf_by_df;          /* 1: the score kernels read idf[df_of_rank[r]] (large V with a full idf
                                    table: a 4-byte gather into V words + an L2-resident table instead of
                                    an 8-byte gather into V doubles; idf_rank is not built) */
    uint64_t rec_total;          /* bounds guard: records in rec_slot/rec_cnt */
    uint64_t slot_cap;           /* bounds guard: vocabulary capacity */
    uint32_t* status;            /* ST_BOUNDS set instead of faulting */
    uint32_t* out_term;          /* output order: term rank */
    uint32_t* out_cnt;           /*               wordCount */
    double* out_score;           /*               tf * idf */
    uint32_t rec_pack;           /* nonzero: a document's records are single words in rec_slot,
                                    rank << pack_cb | count (the packed DF pass wrote them), and rec_cnt
                                    is not read for them; presorted (merged) documents keep rank and
                                    count in rec_slot / rec_cnt.  0: two words throughout */
    uint32_t pack_cb;            /* the packed word's count bits: 32 - rank_bits */
};
/* ncu sizes the persistent score kernels (k_score_small, the wave kernel, the chunk tasks): the
 * context's CU count, 0: the launcher asks the device */
int launch_score_order(const K5Args& a, Arena& ar, hipStream_t s, hipStream_t s2, hipEvent_t ev_fork,
                       hipEvent_t ev_join, uint32_t ncu = 0);

/* multi-GPU vocabulary agreement */
int launch_keys_by_rank(const uint4* vkeys, const uint32_t* slot_of_rank, uint32_t V, uint4* out, hipStream_t s);
/* hash-owner DF exchange: partition this rank's terms by owner into 20-byte (key, df)
 * records (cnt[R] = terms per owner, cur[R] scratch); the send/receive segment offsets from
 * the all-gathered count matrix m (R rows of R counts + 1 status word); aggregate the
 * received records on the owner (table of tcap = 2^k >= 1.5 n slots; *used = distinct keys)
 * and reply per sender (segment + one trailer word = *used); write the returned global df at
 * the term ranks and global V (the trailers summed) to *vg */
/* where the partition reads this rank's term keys: the vocabulary sort's own keys in rank
 * order (skey[r] = the strcmp sort key of term rank r), not a gather through the slot table.
 * A short term's sort key is its identity key byte-swapped; a long term's identity key is
 * read from vkeys at its slot */
struct OwnerKeySrc {
    const uint4* skey;
    const uint32_t* slot_of_rank;   /* long terms */
    const uint4* vkeys;
};
int launch_owner_partition(const OwnerKeySrc& ks, const uint32_t* df, uint32_t V, uint32_t R, uint32_t* cnt, uint32_t* cur,
                           uint32_t* srec, uint32_t* sidx, hipStream_t s);
int launch_owner_offsets(const uint32_t* m, uint32_t R, uint32_t me, uint32_t* soff, uint32_t* roff, hipStream_t s);
int launch_owner_aggregate(const uint32_t* rrec, uint64_t n, const uint32_t* roff, uint32_t R, uint4* tkey, uint64_t tcap,
                           uint32_t* tdf, uint32_t* rslot, uint32_t* reply, unsigned long long* used, uint32_t* status,
                           hipStream_t s);
/* the same, bucketed: records grouped by key hash into buckets of <= 512 on average (a radix sort of
 * (bucket, record index) pairs), each bucket aggregated in LDS; scratch of
 * owner_bucket_scratch(n) bytes */
size_t owner_bucket_scratch(uint64_t n);
int launch_owner_aggregate_buckets(const uint32_t* rrec, uint64_t n, const uint32_t* roff, uint32_t R, void* scratch,
                                   size_t scratch_bytes, uint32_t* reply, unsigned long long* used, uint32_t* status,
                                   uint32_t stage_max, hipStream_t s);
int launch_owner_back(const uint32_t* back, const uint32_t* soff, uint32_t R, const uint32_t* sidx, uint32_t V,
                      uint32_t* df_global, uint32_t* vg, hipStream_t s);
/* out[i] = sum of rows[r * n + i] over r < nrows (the in-process transport's all-reduce) */
int launch_sum_rows_u32(const uint32_t* rows, uint32_t nrows, uint64_t n, uint32_t* out, hipStream_t s);
/* the in-process transport's collectives between contexts on one device, one launch each:
 * XCOPY_MAX segments of 4-byte words copied src[i] -> dst[i] (words[i] each) */
#define XCOPY_MAX 64
struct XCopyList {
    const uint32_t* src[XCOPY_MAX];
    uint32_t* dst[XCOPY_MAX];
    uint64_t off[XCOPY_MAX + 1];   /* prefix sums of the segments' word counts */
    uint32_t n;
};
int launch_xcopy(const XCopyList& l, hipStream_t s);
/* out[i] = sum over r < n of src[r][lo + i], i < len (a reduce-scatter slice) */
int launch_xsum_slice(const XCopyList& l, uint64_t lo, uint64_t len, uint32_t* out, hipStream_t s);
/* dense DF exchange (small vocabularies): gathered keys -> shared positions (tpos[slot] =
 * smallest gathered position of the key, *used = distinct keys), this rank's df scattered
 * over them (pos[r] = position of term rank r), and read back after the all-reduce */
int launch_dense_ids(const uint4* gkeys, uint64_t n, uint4* tkey, uint32_t* tpos, uint64_t tcap,
                     unsigned long long* used, uint32_t* status, hipStream_t s);
int launch_dense_scatter(const uint4* mine, const uint32_t* df, uint32_t V, const uint4* tkey, uint64_t tcap,
                         const uint32_t* tpos, uint32_t* pos, uint32_t* dense, uint32_t* status, hipStream_t s);
int launch_dense_gather(const uint32_t* dense, const uint32_t* pos, uint32_t V, uint32_t* df_global, hipStream_t s);
/* the same with merge numbering when no rank holds long terms (lists in term order, padded
 * with all-ones keys): pos = the keys below each term over all lists; lbm: R x V words;
 * dense[sumv] accumulates the keys first held by each rank (global V after the sum) */
int launch_dense_merge_ids(const uint4* gkeys, uint64_t maxv, uint32_t R, uint32_t me, uint32_t V, uint32_t* lbm,
                           const uint32_t* df, uint64_t sumv, uint32_t* pos, uint32_t* dense, hipStream_t s);

/* Cross-rank identity of terms of >= 16 bytes (engine.cpp exchange_long_check; TFIDF.c:229's
 * strcmp): a long term's identity key is a 120-bit hash, so the ranks all-gather their long
 * terms (key, length, bytes) and every rank checks each key two ranks share byte by byte. */
struct LongEnt {
    uint4 key;
    uint32_t len, pad;
    uint64_t boff;             /* its bytes in the rank's blob */
};
/* this rank's long terms: ents[0, cnt[0]) (blob offsets from an atomic byte counter cnt[1]),
 * src[e] = the corpus offset of one occurrence (the vocabulary's rep) */
int launch_long_list(const uint4* vkeys, const uint64_t* vrep, const uint32_t* slot_of_rank, uint32_t V, LongEnt* ents,
                     uint64_t* src, unsigned long long* cnt, hipStream_t s);
int launch_long_bytes(const LongEnt* ents, const uint64_t* src, uint32_t n, const uint8_t* bytes, uint8_t* blob,
                      hipStream_t s);
/* every gathered entry (R blocks of lcap, blobs of bcap bytes each; padding keys EMPTY)
 * compared with the first entry of its key: a different length or byte sets ST_LONG_COLLIDE */
int launch_long_verify(const LongEnt* g, uint64_t n, uint64_t lcap, const uint8_t* gblob, uint64_t bcap, uint4* tkey,
                       uint32_t* tpos, uint64_t tcap, uint32_t* status, hipStream_t s);

/* synthetic corpus generation on the device */
struct SynSpecDev;
int launch_synth_bytes(const void* spec, const uint32_t* doc_ids, const uint64_t* ntok, const uint64_t* blk_first,
                       uint64_t nblocks, uint32_t ndocs, uint64_t* blk_bytes, hipStream_t s);
int launch_synth_fill(const void* spec, const uint32_t* doc_ids, const uint64_t* ntok, const uint64_t* blk_first,
                      uint64_t nblocks, uint32_t ndocs, const uint64_t* blk_off, uint8_t* bytes, uint64_t* doc_off,
                      hipStream_t s);

/* ---- output emission (emit.hip) ---- */
struct EmitLaunch {
    const uint32_t* order;
    const uint32_t* doc_ids;
    const uint64_t* out_off;
    const uint32_t* term;
    const double* score;
    const uint4* tkey;
    const uint32_t* tlen;
    const uint8_t* corpus;
    uint32_t ndocs;
    uint32_t* status;
};
int launch_term_meta(const uint4* vkeys, const uint64_t* vrep, const uint32_t* slot_of_rank, uint32_t V,
                     uint4* tkey, uint32_t* tlen, hipStream_t s);
/* both take min(documents / 4, ncu * 8) workgroups of four waves, a wave per document, that
 * stride over the documents; ncu: the context's CU count, 0: the launcher asks the device */
int launch_emit_bytes(const EmitLaunch& e, uint64_t* doc_bytes, hipStream_t s, uint32_t ncu = 0);
/* formats the output positions [d0, d1) (default: all) */
int launch_emit_write(const EmitLaunch& e, const uint64_t* doc_text, uint8_t* text, hipStream_t s, uint32_t d0 = 0,
                      uint32_t d1 = 0xFFFFFFFFu, uint32_t ncu = 0);
int launch_format_f64(const double* v, uint64_t n, uint8_t* out, uint32_t* status, hipStream_t s);

/* ---- grids of the launches over the resident result ----
 * Each is min(work, ncu * its multiplier) workgroups that stride over the work; ncu is the
 * context's CU count (call_begin: the device's, or env TFIDF_GRID_CUS).  The launches that take
 * one workgroup per big document (over QS_BIG / RW_BIG pairs) are bounded by BIG_WG_MAX as well:
 * from BIG_WG_MAX / BIG_WG_PER_CU = 64 CUs on that bound alone holds.  tests/stride_corpus.py reads
 * these to size a corpus on which every such loop makes several trips.  The run's own persistent
 * kernels (launch_tokcount_sl / _vs, launch_score_order, launch_emit_bytes / _write) take the same
 * count as their ncu argument; tests/run_stride_corpus.py is their corpus. */
#define QS_WG_PER_CU       3u  /* k_doc_score (query, BM25): ~52 KiB of LDS each */
#define SM_WG_PER_CU       8u  /* k_sim_score: no LDS, the waves a CU holds */
#define KM_WG_PER_CU       8u  /* k_km_assign: as k_sim_score */
#define RW_WG_PER_CU       8u  /* k_rw_docs */
#define DD_WG_PER_CU       8u  /* k_dd_sig, k_dd_verify */
#define DD_BIG_WG_PER_CU   4u  /* k_dd_sig_big, k_dd_verify_big */
#define TM_LIST_WG_PER_CU  32u /* k_terms_select_list: one wave, the list in registers */
#define TM_W512_WG_PER_CU  24u /* k_terms_select<64, 512>: 6 KiB of LDS per one-wave workgroup */
#define TM_W2048_WG_PER_CU 6u  /* k_terms_select<64, 2048>: 24 KiB */
#define TM_BIG_WG_PER_CU   3u  /* k_terms_select<256, 4096, BIG> */
#define PR_WG_PER_CU       4u  /* k_pr_pairs (count and write) */
#define NB_WG_PER_CU       8u  /* k_nb_count, k_nb_sums, k_nb_predict: a wave per document or row, as k_km_assign */
#define NB_EL_WG_PER_CU    8u  /* k_nb_argmax, k_nb_list, k_nb_weights: a thread per matrix entry */
#define MT_WG_PER_CU       7u  /* k_mt_scan: ~21.5 KiB of LDS each (the lanes' term bytes and the group's patterns) */
#define SN_WG_PER_CU       8u  /* k_sn_scan: ~14 KiB of LDS each (the tile, its halo, the query's keys); k_sn_select, k_sn_emit, k_sn_fill */
#define BIG_WG_MAX         256u /* k_doc_score_big, k_sim_score_big, k_rw_docs_big: at most this many ... */
#define BIG_WG_PER_CU      4u  /* ... and this many per CU */

/* ---- top-k retrieval over the resident result (query.hip, tfidf_query) ---- */
#define QG_MAX        64u      /* queries per scoring pass: one accumulator per lane of the owner wave */
#define QS_BIG        4096u    /* documents over this many pairs: a workgroup each (K5_MAX_PAIRS's cut) */
#define QT_SLICE      4096u    /* candidates a top-k workgroup sorts in LDS (> TFIDF_QUERY_MAX_K) */
#define QTAB_WORDS    4096u    /* a group's table is staged in LDS when it has at most this many u32 words (16 KiB) */
#define QUERY_NO_TERM 0xFFFFFFFFu
/* distinct query terms -> term ranks (QUERY_NO_TERM: not in this shard's vocabulary) */
struct QLookupArgs {
    const uint8_t* tbytes;       /* term i = tbytes[toff[i], toff[i + 1]), NUL-free */
    const uint64_t* toff;
    uint32_t nterms;
    const uint4* vkeys;          /* the run's table, read only */
    const uint64_t* vrep;
    uint64_t mask;               /* capacity - 1 */
    uint64_t home;               /* home alignment of the run's inserts (dev_vocab.h): ~1 pairs, ~3 quads */
    const uint32_t* rank_of_slot;
    const uint8_t* corpus;       /* long terms' bytes */
    uint64_t corpus_bytes;
    uint32_t V;
    uint32_t* rank_out;
};
int launch_query_lookup(const QLookupArgs& a, hipStream_t s);
/* One scan of the resident pairs for a group of nq <= QG_MAX queries (docscan.h), the part every
 * ranking function shares: gterm = the group's sorted distinct term ranks, term i's postings
 * (query in the group, weight) at [post_off[i], post_off[i + 1]); acc / cnt are written for
 * every (query, output position): [nq][ndocs].  The table is one block from gterm on: gterm,
 * post_off, post_q as u32 words, with clauses post_inc (one u32 per posting), then the weights
 * in the ranking function's type (u32, or binary64 at an even word). */
struct DocScanArgs {
    const uint64_t* out_off;
    const uint32_t* out_term;
    uint32_t ndocs;
    uint64_t npairs;
    const uint32_t* gterm;
    uint32_t ngterm;
    const uint32_t* post_off;
    const uint32_t* post_q;
    const uint32_t* post_w;      /* the weights' first word */
    uint32_t tab_words;          /* u32 words of the whole block (0: do not stage it in LDS) */
    uint32_t nq;
    double* acc;
    uint32_t* cnt;
    uint32_t* big_list;          /* [ndocs] scratch: output positions of documents over QS_BIG pairs */
    uint32_t* big_count;
};
/* TF-IDF: u32 weights (the term's count in the query), a match reads the pair's score */
struct QScoreArgs : DocScanArgs {
    const double* out_score;
};
int launch_query_score(const QScoreArgs& a, uint32_t ncu, hipStream_t s);
/* Clauses (tfidf_query_clauses): a posting's increment of the count word, one field per clause
 * kind, and the word a document's count is tested against: 12 + 12 + 8 bits. */
#define CL_INC_SHOULD 1u
#define CL_INC_MUST   (1u << 12)
#define CL_INC_NOT    (1u << 24)
#define CL_FIELD      0xFFFu
/* the same pass where a match adds its posting's post_inc to cnt instead of 1: one u32 per
 * posting (the CL_INC_* of the term's clause kinds, summed), inside the table's block */
struct QClauseArgs : QScoreArgs {
    const uint32_t* post_inc;
};
int launch_query_score_clauses(const QClauseArgs& a, uint32_t ncu, hipStream_t s);
/* one top-k round: per (query, slice of QT_SLICE inputs) the best kk in order.  First round
 * (acc != null): the inputs are the output positions, hits where cnt != 0 (need == null) or
 * where cnt passes the clause test against need[q] = |M| << 12 | min_should, ids through
 * order / doc_ids (null: index + 1), nmatch[q] += the slice's hits.  Later rounds: in_slices
 * lists of kk (score bits, id) with in_n valid entries each.  out_*: [nq][out_slices][kk] */
struct QTopkArgs {
    const double* acc;
    const uint32_t* cnt;
    const uint32_t* need;        /* first round: per query of the group, or null */
    const uint32_t* order;
    const uint32_t* doc_ids;
    const uint64_t* in_s;
    const uint32_t* in_id;
    const uint32_t* in_n;
    uint32_t in_slices;
    uint64_t n_in;               /* inputs per query: ndocs, or in_slices * kk */
    uint32_t kk;
    uint64_t* out_s;
    uint32_t* out_id;
    uint32_t* out_n;
    uint32_t out_slices;         /* ceil(n_in / QT_SLICE) */
    unsigned long long* nmatch;
};
int launch_query_topk(const QTopkArgs& a, uint32_t nq, hipStream_t s);

/* ---- BM25 scoring over the resident result (bm25.hip, tfidf_query_bm25) ---- */
/* out[i] = df[rank[i]] (0 where rank[i] is QUERY_NO_TERM): the found terms' global df */
int launch_bm25_df(const uint32_t* rank, uint32_t n, const uint32_t* df, uint32_t V, uint32_t* out, hipStream_t s);
/* BM25: binary64 weights W(q,t).  A match reads the pair's count (out_cnt); the document's
 * normaliser comes from doc_size through order. */
struct BScoreArgs : DocScanArgs {
    const uint32_t* out_cnt;
    const uint32_t* order;       /* output position -> document index */
    const uint32_t* doc_size;    /* by document index */
    double k1, b, avgdl;         /* avgdl > 0 */
    double k1_plus_1;            /* fl(k1 + 1.0) */
    double one_minus_b;          /* fl(1.0 - b) */
};
int launch_bm25_score(const BScoreArgs& a, uint32_t ncu, hipStream_t s);
struct BClauseArgs : BScoreArgs {
    const uint32_t* post_inc;    /* as QClauseArgs */
};
int launch_bm25_score_clauses(const BClauseArgs& a, uint32_t ncu, hipStream_t s);

/* ---- per-document top-k terms over the resident result (terms.hip, tfidf_top_terms) ---- */
#define TERMS_NO_POS 0xFFFFFFFFu
/* requested global document ids -> output positions (TERMS_NO_POS: not in this shard): a binary
 * search of the id's document-name key (launch_doc_keys) over the output positions */
struct TLookupArgs {
    const uint32_t* ids;
    uint32_t nids;
    const uint32_t* order;       /* output position -> local document */
    const uint32_t* doc_ids;     /* local document -> global id (null: index + 1) */
    uint32_t ndocs;
    uint32_t* pos;
};
int launch_terms_lookup(const TLookupArgs& a, hipStream_t s);
/* one batch of rows: row i < nrows is the document at output position pos[row0 + i] (pos null:
 * row0 + i).  Its k best pairs under (score descending, pair position ascending) go to
 * score / pair / term / cnt / wlen at [i * k, i * k + rnterms[i]), the rest of the row is
 * zeroed; wlen = the term's byte length (tlen of launch_term_meta) */
struct TSelArgs {
    const uint64_t* out_off;
    const uint32_t* out_term;
    const uint32_t* out_cnt;
    const double* out_score;
    const uint32_t* order;
    const uint32_t* doc_ids;
    const uint32_t* tlen;
    uint32_t ndocs;
    uint32_t nterms;             /* V */
    uint64_t npairs;
    const uint32_t* pos;
    uint32_t row0, nrows, k;
    uint32_t* rdoc;              /* per row: global id (0: no such document) */
    uint64_t* rnpairs;
    uint32_t* rnterms;
    uint64_t* score;             /* the scores' bit patterns */
    uint64_t* pair;
    uint32_t* term;
    uint32_t* cnt;
    uint64_t* wlen;
    uint32_t* big_list;          /* [nrows] scratch: rows of documents over QS_BIG pairs */
    uint32_t* big_count;
};
int launch_terms_select(const TSelArgs& a, uint32_t ncu, hipStream_t s);
/* the selected words' bytes: entry i is bytes [woff[i], woff[i + 1]) of `bytes` (short terms
 * from their key, long terms from the corpus, as emit.hip's lines) */
struct TWordArgs {
    const uint32_t* term;
    const uint64_t* woff;        /* n + 1 */
    uint64_t n;
    const uint4* tkey;
    uint32_t nterms;
    const uint8_t* corpus;
    uint64_t corpus_bytes;
    uint8_t* bytes;
};
int launch_terms_words(const TWordArgs& a, hipStream_t s);

/* ---- top-k similar documents over the resident result (similar.hip, tfidf_similar) ---- */
#define SG_MAX 64u   /* rows per scoring pass: one accumulator per lane of the owner wave (= QG_MAX) */
/* sq[j] = the sequential sum of the squared scores of the document at output position j,
 * norm[j] = its correctly rounded square root */
int launch_sim_norms(const uint64_t* out_off, const double* out_score, uint32_t ndocs, uint64_t npairs, double* sq,
                     double* norm, hipStream_t s);
/* the rows of a call: row i is the document at output position pos[i] (pos null: i; no such
 * position: an empty row with norm 0 and id 0) */
struct SimRowArgs {
    const uint64_t* out_off;
    const uint32_t* order;
    const uint32_t* doc_ids;
    const double* sq;
    const double* norm;
    uint32_t ndocs;
    uint64_t npairs;
    const uint32_t* pos;
    uint32_t nrows;
    uint64_t* rb;                /* per row: its vector is entries [rb, re) of the pair arrays */
    uint64_t* re;
    double* rnorm;
    double* rsq;
    uint32_t* rpos;
    uint32_t* rid;
};
int launch_sim_rows(const SimRowArgs& a, hipStream_t s);
/* one group's term -> postings table over the shard's term ranks: row r < nrows <= SG_MAX holds
 * the entries [rb[r], re[r]) of (term, score); entries whose term is >= V (a word this shard's
 * vocabulary does not hold) are skipped.  mark sets bit r of mask[t] (V words, zeroed by the
 * caller) for every term t of row r and writes cnt[t] = popcount(mask[t]); after post_off = the
 * exclusive scan of cnt, fill writes row r's weight for t to
 * post_w[post_off[t] + popcount(mask[t] below bit r)] */
struct SimTabArgs {
    const uint32_t* term;
    const double* score;
    const uint64_t* rb;
    const uint64_t* re;
    uint64_t nentries;           /* bound of term / score */
    uint32_t nrows;
    uint32_t V;
    uint64_t* mask;
    uint32_t* cnt;
    const uint32_t* post_off;
    double* post_w;
    uint32_t post_cap;
};
int launch_sim_mark(const SimTabArgs& a, hipStream_t s);
int launch_sim_fill(const SimTabArgs& a, hipStream_t s);
/* one scan of the pairs for a group of nq <= SG_MAX rows: sim(row, document) and the number of
 * shared terms for every (row, output position), [nq][ndocs], the layout of QScoreArgs.  The
 * position rpos[row] (the row's own document) gets count 0. */
struct SimScoreArgs {
    const uint64_t* out_off;
    const uint32_t* out_term;
    const double* out_score;
    uint32_t ndocs;
    uint64_t npairs;
    uint32_t V;
    const uint64_t* mask;        /* V: the rows holding the term */
    const uint32_t* post_off;    /* V + 1 */
    const double* post_w;
    uint32_t post_cap;
    uint32_t nq;
    const double* rnorm;         /* the group's rows */
    const uint32_t* rpos;
    const double* dnorm;         /* by output position */
    double* acc;
    uint32_t* cnt;
    uint32_t* big_list;          /* [ndocs] scratch: output positions of documents over QS_BIG pairs */
    uint32_t* big_count;
};
int launch_sim_score(const SimScoreArgs& a, uint32_t ncu, hipStream_t s);
/* shared[e] = cnt[row][pos[e]] for the n_of_row[row] first entries of row = e / k, else 0 */
int launch_sim_shared(const uint32_t* cnt, const uint32_t* pos, const uint32_t* n_of_row, uint32_t nrows, uint32_t k,
                      uint32_t ndocs, uint32_t* shared, hipStream_t s);
/* a group of rows' vectors made contiguous: row r's entries [rb[r], re[r]) of the pair arrays
 * go to [eoff[r], ...) of term / score, wlen = the terms' byte lengths */
struct SimExportArgs {
    const uint32_t* out_term;
    const double* out_score;
    const uint32_t* tlen;
    uint32_t V;
    const uint64_t* rb;
    const uint64_t* re;
    const uint64_t* eoff;
    uint32_t nrows;
    uint32_t* term;
    double* score;
    uint64_t* wlen;
};
int launch_sim_export(const SimExportArgs& a, hipStream_t s);

/* ---- scoring unseen documents against the resident model (transform.hip, tfidf_transform) ---- */
/* The frozen vocabulary of a finished run, as its read-only consumers probe it
 * (vocab_find_rank, dev_vocab.h). */
struct VocabRO {
    const uint4* vkeys;          /* the run's table, read only */
    const uint64_t* vrep;
    uint64_t mask;               /* capacity - 1 */
    uint64_t home;               /* home alignment of the run's inserts: ~1 pairs, ~3 quads */
    const uint32_t* rank_of_slot;
    const uint8_t* corpus;       /* the run's corpus: long terms' bytes */
    uint64_t corpus_bytes;
    uint32_t V;
};
#define TR_TILE 4096u            /* bytes per boundary workgroup: 256 lanes x one 16-byte group */
/* One slice of a batch: the documents [d0, d1), bytes [b0, b1) of the batch buffer.  Tile t
 * covers the positions [p0 + t * TR_TILE, + TR_TILE); p0 = b0 minus the misalignment of
 * bytes + b0 (it may be negative), so every group that lies inside the window is one aligned
 * 16-byte load; groups that straddle a window edge take the byte path. */
struct TrSlice {
    const uint8_t* bytes;
    uint64_t nbytes;             /* bound of `bytes` */
    const uint64_t* doc_off;     /* the batch's ndocs + 1 offsets (device) */
    uint32_t d0, d1;
    uint64_t b0, b1;
    long long p0;
    uint64_t ntiles;
    uint32_t* dstart;            /* ntiles * (TR_TILE / 32) + 1 words: bit i = a document other than d0 starts at p0 + i */
    uint64_t* cnt_s;             /* ntiles + 1: token starts per tile, then their exclusive scan */
    uint64_t* cnt_e;             /* the same for token ends */
    uint64_t* tok_start;         /* tok_cap: token i = bytes [tok_start[i], tok_end[i]) */
    uint64_t* tok_end;
    uint64_t tok_cap;
    uint32_t* status;            /* ST_BOUNDS instead of a fault */
};
/* zeroes dstart and marks the starts of the documents (d0, d1) */
int launch_tr_docstarts(const TrSlice& a, hipStream_t s);
/* per-tile counts of token starts and ends -> cnt_s / cnt_e */
int launch_tr_count(const TrSlice& a, hipStream_t s);
/* after the scans of cnt_s / cnt_e: tok_start / tok_end (the i-th start pairs with the i-th end) */
int launch_tr_write(const TrSlice& a, hipStream_t s);
/* one lane per token: its row (upper_bound of the start in doc_off), its term (cut at the first
 * NUL), the term's rank in the frozen vocabulary.  key = row << 32 | rank, rank = V for a term
 * the vocabulary does not hold (it sorts behind the row's pairs); val = the token index. */
struct TrResolve {
    TrSlice sl;
    uint64_t ntok;
    VocabRO voc;
    uint64_t* key;
    uint32_t* val;
    uint32_t* tlen;              /* the term's length */
};
int launch_tr_resolve(const TrResolve& a, hipStream_t s);
/* over the sorted (key, val): flag = first record of a run of equal keys whose rank is < V;
 * after pos = the exclusive scan of flag (pos[ntok] = the slice's pairs), the pairs */
struct TrPairs {
    const uint64_t* key;         /* sorted */
    const uint32_t* val;
    uint64_t ntok;
    uint32_t d0, d1, V;
    const uint64_t* doc_off;
    const uint64_t* tok_start;   /* ascending */
    const uint32_t* tlen;
    uint32_t* flag;
    const uint32_t* pos;
    const uint32_t* df;          /* the run's global df by rank */
    const uint32_t* idf_idx;     /* df -> index into idf; null: idf is indexed by df */
    const double* idf;
    uint64_t Nt;
    uint32_t* doc_size;          /* d1 - d0, every token */
    uint32_t* doc_oov;           /* d1 - d0, zeroed by the caller */
    uint64_t* row_off;           /* d1 - d0 + 1, slice-local */
    uint32_t* p_row;             /* per pair */
    uint32_t* p_term;
    uint32_t* p_count;
    uint32_t* p_df;
    double* p_score;
    uint64_t* p_woff;
    uint32_t* p_wlen;
    uint32_t* status;
};
int launch_tr_flags(const TrPairs& a, hipStream_t s);
int launch_tr_pairs(const TrPairs& a, hipStream_t s);
/* the same under a weighting scheme other than the reference's (tfidf_reweight): an instantiation
 * of its own that reads no idf and writes no score; launch_rw_pairs scores the rows from p_count,
 * p_df and doc_size afterwards */
int launch_tr_pairs_w(const TrPairs& a, hipStream_t s);

/* ---- the portable model (model.hip, tfidf_model_import / tfidf_model_export) ---- */
#define ST_MODEL_DUP 256u   /* import: a term's key was in the table already (the host check excludes it) */
/* The frozen table a run leaves behind, built from a model's term list instead: term t =
 * blob[term_off[t], term_off[t + 1]) in term-table order, so t is the term's rank.  One lane
 * per term: the identity key from the bytes, vocab_insert_s at home alignment ~1 with the blob
 * in the corpus's place (a long term's rep = len << 40 | offset into the blob), then
 * rank_of_slot[slot] = t.  The caller has cleared keys to KEY_EMPTY_HI and rank_of_slot to
 * QUERY_NO_TERM: a lane that finds a rank already there sets ST_MODEL_DUP.  Every read of the
 * blob is guarded by blob_bytes (ST_BOUNDS), a term of >= 16 MiB sets ST_TERM_LONG. */
struct ModelBuild {
    const uint64_t* term_off;    /* nterms + 1 */
    const uint8_t* blob;
    uint64_t blob_bytes;
    uint32_t nterms;
    uint4* keys;
    uint64_t* rep;
    uint64_t mask;               /* capacity - 1 */
    uint32_t* rank_of_slot;
    uint32_t* status;
};
int launch_model_build(const ModelBuild& a, hipStream_t s);
/* export: term[t] = t and wlen[t] = tlen[t] for t < n, wlen[n] = 0: the identity selection and
 * the lengths (scanned by the caller) that launch_terms_words gathers the whole table with */
int launch_model_lens(const uint32_t* tlen, uint32_t n, uint32_t* term, uint64_t* wlen, hipStream_t s);

/* ---- spherical k-means over the resident result (kmeans.hip, tfidf_kmeans) ---- */
#define KM_MAX_K      256u          /* four accumulators per lane of the owner wave */
#define KM_MAX_TERMS  64u
#define KM_NO_CLUSTER 0xFFFFFFFFu
#define KM_TOP_SLICES 64u           /* term slices of a round of the top-term selection */
/* The centroid matrix C is dense, [V][K] (a term's K weights are one contiguous row), indexed
 * with 64-bit offsets.  norm is launch_sim_norms's, by output position. */
struct KmArgs {
    const uint64_t* out_off;
    const uint32_t* out_term;
    const double* out_score;
    const double* norm;
    uint32_t ndocs;
    uint64_t npairs;
    uint32_t V;
    uint32_t K;
    double* C;
    uint32_t* label;             /* [ndocs] this pass's labels (KM_NO_CLUSTER: norm 0) */
    const uint32_t* prev;        /* [ndocs] the pass before's (null: the first pass) */
    double* sim;                 /* [ndocs] similarity to the document's own centroid */
    uint32_t* changed;           /* documents whose label differs from prev */
    uint32_t* size;              /* [K] members per cluster */
    uint32_t* moff;              /* [K + 1] exclusive scan of size */
    uint32_t* members;           /* [ndocs] output positions by cluster, ascending inside a cluster */
    const uint32_t* seedpos;     /* [K] output positions of the seeds */
    double* cnorm;               /* [K] */
};
/* id[j] = the global id of the document at output position j */
int launch_km_docs(const uint32_t* order, const uint32_t* doc_ids, uint32_t ndocs, uint32_t* id, hipStream_t s);
/* C = 0, then column c = the unit vector of the document at seedpos[c] */
int launch_km_seed(const KmArgs& a, hipStream_t s);
/* one pass over the pairs: label, sim, size (zeroed here) and changed (zeroed here) */
int launch_km_assign(const KmArgs& a, uint32_t ncu, hipStream_t s);
/* the centroids of the clusters with members from label / size; `split` workgroups per cluster,
 * each owning a range of term ranks (the result does not depend on it) */
int launch_km_update(const KmArgs& a, uint32_t split, hipStream_t s);
/* the T best (weight descending, term rank ascending) non-zero entries of every column:
 * term / weight bits at [c * T, c * T + n[c]), the rest 0xFFFFFFFF / 0; wlen = the selected
 * terms' byte lengths (T * K + 1 words, the last 0).  part: K * KM_TOP_SLICES * 16 bytes, prev: K * 16 */
struct KmTopArgs {
    const double* C;
    uint32_t V, K, T;
    const uint32_t* tlen;
    uint64_t* part;
    uint64_t* prev;
    uint32_t* term;
    uint64_t* weight;
    uint32_t* n;
    uint64_t* wlen;
};
int launch_km_top(const KmTopArgs& a, hipStream_t s);

/* ---- the analyzer (analyze.hip, tfidf_analyze) ---- */
#define AN_TILE 4096u   /* bytes a workgroup owns per step: 256 lanes x 16 */
#define AN_HALO 80u     /* mapped bytes held on each side of the tile (a multiple of 16, > TFIDF_AN_MAX_WORD + 1) */
/* out[i] = the analyzed in[i] for i in [0, nbytes): the byte map inside [lo, hi) = the documents'
 * window, the token filter on the mapped bytes, everything else copied.  out is 16-byte
 * aligned, in has any alignment; no byte outside in[0, nbytes) is read and none outside
 * out[0, nbytes) written.  dstart: bit i = a document starts at byte i, lo < i < hi
 * (launch_an_docstarts), read by the filtering form and, with TFIDF_AN_UTF8 in flags, by the
 * byte map too (a document boundary cuts a UTF-8 sequence).  flags holds TFIDF_AN_UTF8 only
 * beside a map flag: alone it changes nothing and the caller clears it.  tab: the stop-word blob of
 * analyze_tab.h in device memory (a header alone when the list is empty). */
struct AnArgs {
    const uint8_t* in;
    uint8_t* out;
    uint64_t nbytes, lo, hi;
    const uint64_t* doc_off;
    uint32_t ndocs;
    uint32_t flags, min_len;
    uint32_t* dstart;            /* nbytes / 32 + 2 words */
    const uint32_t* tab;
    uint32_t tab_bytes;
    unsigned long long* blanked; /* three counters zeroed by the caller: tokens blanked, tokens stemmed,
                                    UTF-8 sequences changed */
    uint32_t stemmer;            /* TFIDF_STEM_*: != 0 selects the stemming instantiation of the tile kernel */
};
/* zeroes dstart and sets the documents' start bits */
int launch_an_docstarts(const AnArgs& a, hipStream_t s);
/* LDS of a workgroup of the filtering form; 0: the call is a pure byte map (never with a stemmer) */
uint32_t an_lds_bytes(const AnArgs& a, uint32_t nstop);
/* grid_cap: at most that many persistent workgroups of the tile kernel (0: the resident ones);
 * *grid receives the workgroups launched (0: the byte map, or no bytes) */
int launch_analyze(const AnArgs& a, uint32_t nstop, uint32_t ncu, uint32_t grid_cap, uint32_t* grid, hipStream_t s);

/* ---- word n-grams (ngram.hip, tfidf_ngrams) ---- */
#define NG_TILE 4096u   /* output bytes a workgroup of the write kernel owns: 256 lanes x one 16-byte store */
/* The tokens come from transform.hip's boundary kernels: token i = bytes [tok_start[i],
 * tok_end[i]), in order.  Segment i = the grams that start at token i, min_n first; seg_off holds
 * the segments' byte counts (launch_ng_sizes), then their exclusive scan (the caller's
 * scan_excl_u64 in place: seg_off[ntok] = the output's bytes). */
struct NgArgs {
    const uint8_t* bytes;        /* the input */
    uint64_t nbytes;             /* bound of `bytes` */
    const uint64_t* doc_off;     /* the input's ndocs + 1 offsets (device) */
    uint32_t ndocs;
    uint32_t min_n, max_n, joiner;
    const uint32_t* dstart;      /* TrSlice's bitmap of the same input: bit i = a document starts at p0 + i */
    long long p0;
    const uint64_t* tok_start;
    const uint64_t* tok_end;
    uint64_t ntok;               /* > 0 */
    uint64_t* seg_off;           /* ntok + 1 */
    unsigned long long* ngrams;  /* grams written, zeroed by the caller (one integer add per workgroup) */
    uint64_t* out_off;           /* ndocs + 1: the output's document offsets */
    uint32_t* tile_seg;          /* ntiles + 1: the segment that holds a tile's first byte */
    uint8_t* out;                /* 16-byte aligned, nbytes_out rounded up to 16 bytes writable */
    uint64_t nbytes_out;
    uint64_t ntiles;             /* ceil(nbytes_out / NG_TILE) */
};
/* one lane per token: the lengths of the next max_n - 1 tokens of the same row (no document
 * start between them) -> seg_off[i] = the segment's bytes */
int launch_ng_sizes(const NgArgs& a, hipStream_t s);
/* after the scan: out_off[d] = seg_off[lower_bound(tok_start, doc_off[d])], one lane per document;
 * tile_seg[t] = the last segment that starts at or before byte t * NG_TILE, one lane per tile */
int launch_ng_offsets(const NgArgs& a, hipStream_t s);
/* the output bytes: a workgroup per tile, the descriptors of the tile's segments in LDS, one
 * 16-byte store per lane */
int launch_ng_write(const NgArgs& a, hipStream_t s);

/* ---- vocabulary pruning by document frequency (prune.hip, tfidf_prune) ---- */
#define PR_TILE 1024u              /* pairs a workgroup owns per step: 256 lanes x four pairs (one 16-byte load of out_term) */
#define PR_LDS_TERMS (1u << 18)    /* the keep bitmap is staged in LDS up to this many terms (32 KiB: four
                                      workgroups of the pair pass per CU); beyond it is read through L2 */
#define PR_KEY_DEAD (1ull << 32)   /* sort key of a term that failed the range test (N - df < 2^32 sorts in front) */
/* one lane per term rank: flag[r] = 1 when df[r] passes the range test, else 0; with key != null
 * also key[r] = Nt - df[r] (PR_KEY_DEAD for a failed term) and val[r] = r for the max_features sort */
int launch_pr_range(const uint32_t* df, uint32_t V, uint64_t Nt, uint32_t min_df, uint32_t max_df, uint32_t* flag,
                    uint64_t* key, uint32_t* val, hipStream_t s);
/* after the stable sort of (key, val): flag[val[p]] = p < M && key[p] != PR_KEY_DEAD, one lane per position */
int launch_pr_take(const uint64_t* key, const uint32_t* val, uint32_t V, uint32_t M, uint32_t* flag, hipStream_t s);
/* bits: word w bit b = flag[32 w + b] != 0; 2 * ceil(V / 64) words are written (a wave's ballot each pair) */
int launch_pr_bitmap(const uint32_t* flag, uint32_t V, uint32_t* bits, hipStream_t s);
/* new_rank = the exclusive scan of flag (V + 1 entries, new_rank[V] = V').  One lane per old rank r:
 * a kept r scatters slot_of_rank and df to new_rank[r] */
struct PrTerms {
    const uint32_t* bits;
    const uint32_t* new_rank;
    uint32_t V;
    const uint32_t* slot_of_rank;
    const uint32_t* df;
    uint32_t* new_slot_of_rank;
    uint32_t* new_df;
};
int launch_pr_terms(const PrTerms& a, hipStream_t s);
/* the one step in place, run last: rank_of_slot[slot_of_rank[r]] = new_rank[r] for a kept r and
 * QUERY_NO_TERM for a pruned one (its key keeps its slot and stops resolving: vocab_find_rank);
 * a slot >= slot_cap is skipped */
int launch_pr_slots(const PrTerms& a, uint32_t* rank_of_slot, uint64_t slot_cap, hipStream_t s);
/* The pair pass over tiles of PR_TILE pairs, ntiles = npairs / PR_TILE + 1 (the tile that holds
 * index npairs exists, for the documents that end there).  count: tile_cnt[t] = kept pairs of
 * tile t; the caller scans tile_cnt in place (tile_cnt[ntiles] = P').  write: the kept pairs to
 * their compacted positions with new_rank[term], and new_off[j] = the kept pairs before
 * min(out_off[j], npairs) for the documents whose offset lies in the tile (tile_doc, from
 * launch_pr_tiledoc).  Persistent workgroups (grid <= ntiles) that own tiles t = block, block +
 * grid, ..: every tile's result is its own, so the outcome does not depend on the grid. */
struct PrPairs {
    const uint64_t* out_off;     /* ndocs + 1 */
    const uint32_t* out_term;
    const uint32_t* out_cnt;
    const double* out_score;
    uint64_t npairs;
    uint32_t ndocs, V;
    const uint32_t* bits;
    const uint32_t* new_rank;
    uint64_t ntiles;
    uint64_t* tile_cnt;          /* ntiles + 1 */
    uint32_t* tile_doc;          /* ntiles + 1: the first j with min(out_off[j], npairs) >= t * PR_TILE */
    uint32_t* new_term;
    uint32_t* new_cnt;
    double* new_score;
    uint64_t* new_off;           /* ndocs + 1 */
    uint32_t* emptied;           /* one word, zeroed by the caller: documents that lost their last pair */
};
int launch_pr_tiledoc(const PrPairs& a, hipStream_t s);
int launch_pr_count(const PrPairs& a, uint32_t ncu, hipStream_t s);
int launch_pr_write(const PrPairs& a, uint32_t ncu, hipStream_t s);
/* after the write pass: one lane per document, one integer add per workgroup into *emptied */
int launch_pr_emptied(const PrPairs& a, hipStream_t s);

/* ---- weighting schemes (reweight.hip, tfidf_reweight; tfidf_transform under a scheme) ---- */
#define RW_LUT_MAX (1u << 16)      /* sublinear tf: fl(1 + log c) is tabulated by the host for c = 1..min(Cmax, RW_LUT_MAX) */
#define RW_LIST_MAX (1u << 20)     /* pairs whose count is above RW_LUT_MAX are listed (4 bytes each) up to this many */
#define RW_BIG 4096u               /* documents over this many pairs: a workgroup each (QS_BIG's cut) */
#define RW_KEEP 256u               /* a wave keeps the w of a document of up to this many pairs in registers */
/* cmax[0] = max(count[0..n)), cmax[1] = the pairs with count > RW_LUT_MAX, whose counts are
 * appended to list (in no fixed order: the host sorts them) while they fit in list_cap.  n is
 * *n_dev when n_dev is not null (a transform slice's pair total, still on the device), clamped
 * to n.  cmax is zeroed by the caller.  Integer atomics only. */
int launch_rw_cmax(const uint32_t* count, uint64_t n, const uint32_t* n_dev, uint32_t* cmax, uint32_t* list,
                   uint32_t list_cap, hipStream_t s);
/* idf_rank[r] = idf[idf_idx ? idf_idx[df[r]] : df[r]], one lane per term rank */
int launch_rw_idf_rank(const uint32_t* df, uint32_t V, const double* idf, const uint32_t* idf_idx, uint64_t idf_n,
                       double* idf_rank, hipStream_t s);
/* The pair pass, document-major.  Document j = pairs [off[j], off[j + 1]) (clamped to npairs);
 * its docSize is doc_size[order ? order[j] : j].  Pair p: c = count[p], tf by tf_mode
 * (TFIDF_TF_LOG: tf_lut[c] for c <= lut_n, else listed_v[i] with listed_c[i] == c, sorted),
 * idf = 1.0 when idf is null, else idf[idf_idx ? idf_idx[key[p]] : key[p]] (key = term rank with
 * an idf by rank, or df with the table by df), w = fl(tf * idf); the norm as include/tfidf.h
 * defines it: one ordered sum per document, carried by every lane of the wave that owns the
 * document.  A wave keeps w in registers up to RW_KEEP pairs and reloads what it wrote beyond;
 * documents over RW_BIG pairs go to a second launch, one workgroup each, whose wave 0 adds each
 * tile's 256 rounded terms in pair order.  score may not alias an input. */
struct RwArgs {
    const uint64_t* off;         /* ndocs + 1 */
    uint64_t npairs;
    uint32_t ndocs;
    uint32_t tf_mode, norm;
    const uint32_t* order;       /* null: identity */
    const uint32_t* doc_size;
    const uint32_t* count;
    const uint32_t* key;
    uint64_t key_n;              /* keys at or above it read no table (idf 1.0; never with valid input) */
    const double* idf;
    const uint32_t* idf_idx;
    const double* tf_lut;
    uint32_t lut_n;
    uint32_t nlisted;
    const uint32_t* listed_c;
    const double* listed_v;
    double* score;
    uint32_t* big_list;          /* [ndocs] scratch */
    uint32_t* misc;              /* [0] big_count, [1] documents with pairs and a zero norm; zeroed by the launch */
};
int launch_rw_pairs(const RwArgs& a, uint32_t ncu, hipStream_t s);

/* ---- near duplicates (dedup.hip, tfidf_minhash / tfidf_near_dups) ---- */
#define DD_BIG_PAIRS 4096u         /* documents over this many pairs: a workgroup each in the signature pass, and
                                      candidates that hold one a workgroup each in the verification (QS_BIG's cut) */
#define DD_MAX_H 256u              /* TFIDF_MINHASH_MAX_H */
/* h0[r] = mix64(FNV-1a-64(term bytes)), one lane per term rank: the bytes of a short term from
 * tkey (tlen of them), of a long term from the corpus at the position tkey holds (launch_term_meta) */
int launch_dd_h0(const uint4* tkey, const uint32_t* tlen, uint32_t V, const uint8_t* corpus, uint64_t corpus_bytes,
                 uint64_t* h0, hipStream_t s);
/* The signature pass, document-major: sig[j * H + i] = min over the pairs p of document j (pairs
 * [off[j], off[j + 1]) clamped to npairs) of (u32)((fam_a[i] * h0[term[p]]) >> 32) + fam_b[i];
 * 0xFFFFFFFF for a document without pairs.  A wave per document whose lanes own the hash
 * functions (i = lane, lane + 64, ..); documents over DD_BIG_PAIRS pairs go to a second launch, a
 * workgroup each, whose waves combine their minima in LDS.  A minimum is order-free: the shape
 * changes no bit. */
struct DdSigArgs {
    const uint64_t* off;         /* ndocs + 1 */
    uint64_t npairs;
    uint32_t ndocs;
    uint32_t H;                  /* 1..DD_MAX_H */
    uint32_t V;                  /* terms at or above it are skipped (never with valid input) */
    const uint32_t* term;        /* per pair: term rank */
    const uint64_t* h0;          /* V */
    const uint64_t* fam_a;       /* DD_MAX_H */
    const uint32_t* fam_b;       /* DD_MAX_H */
    uint32_t* sig;               /* ndocs * H */
    uint32_t* big_list;          /* [ndocs] scratch */
    uint32_t* big_count;         /* one word, zeroed by the launch */
};
int launch_dd_sig(const DdSigArgs& a, uint32_t ncu, hipStream_t s);
/* Band keys in band-major order: entry x = j * M + m (band j, the m-th document with pairs,
 * position live[m]) gets key[x] = the band key of include/tfidf.h and val[x] = x. */
int launch_dd_bandkeys(const uint32_t* sig, const uint32_t* live, uint32_t M, uint32_t H, uint32_t rows, uint64_t* key,
                       uint32_t* val, hipStream_t s);
/* flag[x] = 1 when the sorted entries x - 1 and x hold equal keys of one band (val / M), else 0
 * (flag[0] = 0); n entries */
int launch_dd_runflag(const uint64_t* key, const uint32_t* val, uint64_t n, uint32_t M, uint32_t* flag, hipStream_t s);
/* the flagged entries' candidates (live[val[x - 1] % M] << 32 | live[val[x] % M]) at at[x]
 * (the flags' exclusive scan) */
int launch_dd_runwrite(const uint32_t* val, const uint32_t* at, uint64_t n, uint32_t M, const uint32_t* live,
                       uint64_t* cand, hipStream_t s);
/* flag[x] = 1 when the sorted candidate x differs from x - 1 (flag[0] = 1), and the write of the
 * flagged ones at at[x] */
int launch_dd_uniqflag(const uint64_t* cand, uint64_t n, uint32_t* flag, hipStream_t s);
int launch_dd_uniqwrite(const uint64_t* cand, const uint32_t* at, uint64_t n, uint64_t* out, hipStream_t s);
/* Verification: per candidate c = (a << 32 | b) shared[c] = the terms the two ascending lists
 * have in common (lanes take terms of the shorter list and binary-search the longer one) and
 * same[c] = the equal signature entries.  A wave per candidate; candidates with a document over
 * DD_BIG_PAIRS pairs go to a second launch, a workgroup each.  The wave or workgroup owns its
 * output words: no atomics on results. */
struct DdVerArgs {
    const uint64_t* cand;
    uint64_t ncand;
    const uint64_t* off;
    uint64_t npairs;
    uint32_t ndocs;
    uint32_t H;
    const uint32_t* term;
    const uint32_t* sig;
    uint32_t* shared;            /* ncand */
    uint32_t* same;              /* ncand */
    uint32_t* big_list;          /* [ncand] scratch (ncand < 2^32) */
    uint32_t* big_count;         /* one word, zeroed by the launch */
};
int launch_dd_verify(const DdVerArgs& a, uint32_t ncu, hipStream_t s);

/* ---- Naive Bayes classification (nb.hip, tfidf_nb_fit / tfidf_nb_predict) ---- */
#define NB_MAX_K    256u           /* TFIDF_NB_MAX_CLASSES: four accumulators per lane of the owner wave */
#define NB_NO_CLASS 0xFFFFFFFFu
#define NB_LUT_MAX  (1u << 16)     /* the host tabulates log(fl((double)m + alpha)) for m = 0..min(max, NB_LUT_MAX) */
/* The fit's device side.  The matrices are term-major: entry (t, c) at t * K + c (64-bit), so a
 * term's K values are one contiguous row.  An entry's log argument m is FC (multinomial) or
 * F[t] - FC (complement); its logarithm comes from lut[m] up to lut_n - 1 and beyond from the
 * sorted list (list_key ascending and distinct, list_val beside it). */
struct NbFitArgs {
    const uint64_t* off;         /* ndocs + 1: pairs of the document at an output position */
    const uint32_t* term;
    const uint32_t* cnt;
    uint64_t npairs;
    uint32_t ndocs;
    uint32_t V;
    uint32_t K;
    uint32_t complement, binary;
    const uint32_t* lab;         /* [ndocs] class by output position, NB_NO_CLASS: unlabelled */
    uint64_t* FC;                /* [V][K] */
    uint64_t* F;                 /* [V] */
    uint64_t* T;                 /* [K] */
    uint64_t* misc;              /* [0] the largest log argument, [1] arguments >= lut_n, [2] the list's cursor */
    uint64_t* list;              /* the arguments >= lut_n, unordered, with repeats (nb_list fills it) */
    uint64_t list_cap;
    const double* lut;
    uint64_t lut_n;
    const uint64_t* list_key;
    const double* list_val;
    uint64_t list_n;
    const double* lc;            /* [K] the class's own logarithm */
    double* W;                   /* [V][K] */
};
/* FC = 0, then the document-major pass: a wave per labelled document adds x into FC[t * K + label]
 * with 64-bit integer atomics (exact in any order) */
int launch_nb_count(const NbFitArgs& a, uint32_t ncu, hipStream_t s);
/* F[t] and T[c] (a wave per term row; the waves' column sums end in 64-bit integer atomics), then
 * misc[0] and misc[1] for the table of lut_n entries the host is about to build */
int launch_nb_sums(const NbFitArgs& a, uint32_t ncu, hipStream_t s);
int launch_nb_argmax(const NbFitArgs& a, uint32_t ncu, hipStream_t s);
/* the arguments >= lut_n into list (at most list_cap) */
int launch_nb_list(const NbFitArgs& a, uint32_t ncu, hipStream_t s);
/* W: one rounded subtraction per entry */
int launch_nb_weights(const NbFitArgs& a, uint32_t ncu, hipStream_t s);
/* Prediction, the shape of k_km_assign: a wave per row, lane l owns the scores of the classes
 * l + 64 * i.  Row r < nrows is the pairs [off[j], off[j + 1]) with j = pos ? pos[r] : r, clamped to
 * npairs; pos[r] >= ndocs (a document the context does not hold) gives NB_NO_CLASS and +0.0.
 * One kernel serves the resident pairs (off = out_off, ndocs = the context's) and uploaded rows
 * (pos null, ndocs = nrows). */
struct NbPredictArgs {
    const uint64_t* off;
    const uint32_t* term;
    const uint32_t* cnt;
    uint64_t npairs;
    uint32_t ndocs;
    const uint32_t* pos;         /* null: row r is position r */
    uint32_t nrows;
    uint32_t V, K;
    uint32_t binary;
    const double* W;             /* [V][K] */
    const double* prior;         /* [K] */
    uint32_t* label;             /* [nrows] */
    double* score;               /* [nrows] */
    double* all;                 /* [nrows][K] or null */
};
int launch_nb_predict(const NbPredictArgs& a, uint32_t ncu, hipStream_t s);

/* ---- fuzzy and prefix term matching over the resident term table (match.hip, tfidf_match_terms) ---- */
#define MT_NT       256u         /* threads per scan workgroup = terms per tile: one lane per term */
#define MT_GROUP    64u          /* patterns per scan: their bytes, lengths, kinds and budgets staged in LDS */
#define MT_PAT      64u          /* a pattern's slot in the pattern block (TFIDF_MATCH_MAX_PATTERN) */
#define MT_TERM_MAX 66u          /* bytes of a term a lane holds: no longer term matches a fuzzy pattern, and a
                                    prefix pattern reads at most MT_PAT of them */
#define MT_NO_MATCH 3u           /* a distance over every budget */
/* Where the scan reads term t's bytes.  From a run: t_key / t_len of launch_term_meta (a term under
 * 16 bytes is its key, a longer one lies in the corpus at the key's offset).  From an imported
 * model: m_off / m_blob, with tkey null. */
struct MtSrc {
    const uint4* tkey;           /* null: the model form */
    const uint32_t* tlen;
    const uint8_t* corpus;
    uint64_t corpus_bytes;       /* bound of corpus / blob */
    const uint64_t* moff;        /* nterms + 1 */
    const uint8_t* blob;
};
/* One scan of the table for the patterns [p0, p0 + np), np <= MT_GROUP, of the call's pattern
 * block: pat = MT_PAT bytes per pattern, plen / pkind / pbudget one byte each.  Every match adds 1
 * to nmatch[p] (u64 atomics: exact in any order) and takes the next record of the list from
 * *nrec; records beyond list_cap are counted and not written.  A record's key orders the list:
 * w = p - p0, z = dist, y = ~df, x = rank. */
struct MtScanArgs {
    MtSrc src;
    const uint32_t* df;          /* global df by rank */
    uint32_t V;
    const uint8_t* pat;
    const uint8_t* plen;
    const uint8_t* pkind;
    const uint8_t* pbudget;
    uint32_t p0, np;
    uint32_t fixed_prefix;
    uint32_t transpose;
    unsigned long long* nmatch;  /* by pattern of the call */
    unsigned long long* nrec;
    uint4* key;
    uint32_t* val;               /* the rank again: the sorts carry a value */
    uint64_t list_cap;
};
int launch_match_scan(const MtScanArgs& a, uint32_t ncu, hipStream_t s);
/* The cut over the sorted list: pattern i < np of the batch owns the records [seg[i], seg[i + 1]);
 * entry i * k + j takes record seg[i] + j for j < min(k, its records): term, dist, df and wlen =
 * the term's byte length; the rest of the row is term 0, wlen 0.  wlen[np * k] = 0. */
struct MtCutArgs {
    const uint4* key;
    const uint32_t* seg;         /* np + 1 */
    uint32_t np, k;
    MtSrc src;
    uint32_t V;
    uint32_t* term;
    uint8_t* dist;
    uint32_t* df;
    uint64_t* wlen;
};
int launch_match_cut(const MtCutArgs& a, hipStream_t s);
/* launch_terms_words for the model form: entry i is bytes [woff[i], woff[i + 1]) of `bytes` */
int launch_match_words_model(const uint32_t* term, const uint64_t* woff, uint64_t n, const MtSrc& src, uint32_t V,
                             uint8_t* bytes, hipStream_t s);

/* ---- snippets over the resident corpus (snippets.hip, tfidf_snippet) ---- */
#define SN_NT          256u      /* threads per workgroup: one lane per 16-byte group of a tile */
#define SN_TILE        4096u     /* bytes of a job's document one workgroup trip scans */
#define SN_HALO        64u       /* bytes behind the tile staged in LDS with it: a token that starts in the tile
                                    reads on from LDS up to there, beyond from HBM */
#define SN_TAB_MAX     512u      /* slots of a query's term table: 2 x TFIDF_SNIP_MAX_TERMS */
#define SN_SLICE       1024u     /* candidate starts one select workgroup trip takes (four per lane) */
#define SN_MAX_TILES   (1u << 20)   /* tiles of one batch: its token ordinals stay under 2^32 (2048 per tile) */
/* an entry of a query's term table (open addressing by sn_hash, linear probing, built on the host from
 * the keys the lookup returned; found terms only).  khi == SN_ENT_EMPTY: an empty slot */
#define SN_ENT_EMPTY 0xEEEEEEEEEEEEEEEEull
struct SnEnt {
    uint64_t klo, khi;           /* the term's identity key (dev_common.h) */
    uint64_t boff;               /* its bytes in the call's term blob: a term of >= 16 bytes is compared with them */
    uint32_t len, slot;
};
static inline __host__ __device__ uint32_t sn_hash(uint64_t klo, uint64_t khi) {
    return (uint32_t)(((klo ^ (khi * 0x9E3779B97F4A7C15ull)) * 0xD6E8FEB86659FD93ull) >> 32);
}
struct SnQuery {
    uint32_t tab_off;            /* the query's table: tab[tab_off, tab_off + tab_size) */
    uint32_t tab_size;           /* a power of two <= SN_TAB_MAX; 0: the query has no found term */
    uint32_t lmax;               /* its longest found term: a longer token cannot match */
    uint32_t pad;
};
struct SnJob {
    uint64_t base, len;          /* the document's bytes in the corpus */
    uint32_t query;
    uint32_t flags;              /* TFIDF_SNIP_NO_DOC */
    uint32_t pad[2];
};
/* a job's result as the emit kernel leaves it */
struct SnOut {
    uint32_t flags, ntokens, nmatch, nterms_matched, win_tok[2], cover, hits;
    uint64_t win_byte[2];
    uint32_t nmarks, pad;
    uint64_t mlo;                /* the first mark's record in the sub-batch's list */
    uint64_t text_len;
};
/* the call's distinct-per-query terms -> their keys and whether the vocabulary holds them */
struct SnLookupArgs {
    const uint8_t* tbytes;       /* term i = tbytes[toff[i], toff[i + 1]), NUL-free */
    const uint64_t* toff;
    uint32_t nterms;
    VocabRO voc;
    uint64_t* key;               /* 2 * nterms: klo, khi */
    uint32_t* found;
};
int launch_sn_lookup(const SnLookupArgs& a, hipStream_t s);
/* jobs -> their documents: pos[j] is the document's output position (TERMS_NO_POS: not held) */
int launch_sn_jobs(const uint32_t* pos, const uint32_t* job_query, uint32_t njobs, const uint32_t* order,
                   const uint64_t* doc_off, SnJob* jobs, hipStream_t s);
/* One pass over the tiles [t0, t1) of a batch of jobs.  Tile t belongs to the job j with
 * tile_first[j] <= t < tile_first[j + 1] and is its tile t - tile_first[j]: the bytes
 * [p0 + k * SN_TILE, + SN_TILE) of the document, p0 = its first byte minus the misalignment of its
 * address, so every group inside the document is one aligned 16-byte load.  A token belongs to the
 * tile that holds its first byte.  Count pass (rec null): tile_tok[t], tile_match[t].  Write pass:
 * both arrays hold their exclusive scans, and the tile's matches go to rec[tile_match[t] - rec0 + ..]
 * in position order as (byte offset lo, hi, token ordinal in the document, len << 8 | slot). */
struct SnScanArgs {
    const uint8_t* corpus;
    const SnJob* jobs;           /* of the batch */
    const uint32_t* tile_first;  /* njobs + 1 */
    uint32_t njobs;
    uint32_t t0, t1;
    const SnQuery* queries;
    const SnEnt* tab;
    const uint8_t* tbytes;
    uint32_t* tile_tok;
    uint32_t* tile_match;
    uint4* rec;
    uint32_t rec0;
};
int launch_sn_scan(const SnScanArgs& a, uint32_t ncu, hipStream_t s);
/* per job of the batch: tot[2 j] = its tokens, tot[2 j + 1] = its matches, from the scanned tile arrays */
int launch_sn_totals(const uint32_t* tile_first, uint32_t njobs, const uint32_t* tile_tok, const uint32_t* tile_match,
                     uint32_t* tot, hipStream_t s);
/* The jobs [j0, j1) of a batch whose match lists lie in rec from rec0 = tile_match[tile_first[j0]] on.
 * Select: slice x of SN_SLICE candidates belongs to the job jj with slice_first[jj] <= x <
 * slice_first[jj + 1] (jj relative to j0); best[jj] takes the maximum of cover << 44 | hits << 32 |
 * ~position over the job's candidates (a total key: the maximum is unique), mask[4 jj ..] the OR of
 * the document's slots.  Both zeroed by the caller. */
struct SnSelArgs {
    const SnJob* jobs;
    const uint32_t* tile_first;
    const uint32_t* tile_tok;
    const uint32_t* tile_match;
    uint32_t j0, j1;
    const uint4* rec;
    const uint32_t* slice_first; /* j1 - j0 + 1 */
    uint32_t nslices;            /* slice_first[j1 - j0] */
    unsigned long long* best;
    unsigned long long* mask;
    uint32_t window, max_marks, want_text;
    const uint8_t* corpus;
    SnOut* out;                  /* j1 - j0 */
};
int launch_sn_select(const SnSelArgs& a, uint32_t ncu, hipStream_t s);
/* centring, the recount, the window's byte bounds: one workgroup per job, striding */
int launch_sn_emit(const SnSelArgs& a, uint32_t ncu, hipStream_t s);
/* the marks and the window's bytes of every job to mark_*[mark_off[jj] ..] and text[text_off[jj] ..] */
struct SnFillArgs {
    const SnJob* jobs;
    uint32_t j0, j1;
    const uint4* rec;
    const SnOut* out;
    const uint64_t* mark_off;    /* j1 - j0 + 1, relative to the sub-batch */
    const uint64_t* text_off;
    const uint8_t* corpus;
    uint64_t* mark_byte;
    uint32_t* mark_len;
    uint32_t* mark_slot;
    uint8_t* text;
};
int launch_sn_fill(const SnFillArgs& a, uint32_t ncu, hipStream_t s);

#endif
