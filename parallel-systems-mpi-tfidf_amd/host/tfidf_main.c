/*
 * tfidf_main.c — `tfidf`, the drop-in for the reference program's process contract.
 *
 * Run with no arguments in a directory holding input/doc1..docN: writes ./output.txt with
 * one "docN@word\t%.16f" line per (document, word) in strcmp order, exactly as
 * `mpirun -np P ./TFIDF` does (TFIDF.c:52-287).  Messages and exit codes follow the
 * reference: "Directory failed to open" -> 1 (TFIDF.c:100-103), "Error Opening File: ..."
 * -> 0 (TFIDF.c:134-138, 274-278), an empty input/ -> "More workers than input files!
 * Exiting." (TFIDF.c:120-123, as with -np 2).  --debug-jobs prints the TF Job / IDF Job
 * blocks (TFIDF.c:199-205, 236-239), one pair of blocks per shard (the reference prints
 * one per rank); --stats prints one JSON line of ingest / run / output times to stderr.
 *
 * Parallelism (the reference's `mpirun -np P`, TFIDF.c:82-92,125-130):
 *   --gpus N     GPUs to use (default 1; capped at the visible GPUs), one shard each;
 *   --shards K   shards (default: N), dealt to the GPUs round-robin — more shards than
 *                GPUs run through the in-process transport (tests on one GPU).
 * Shards are byte-balanced contiguous ranges of the "docN@" order (tfidf_plan_dir), never
 * more than N documents; their outputs are concatenated in shard order.  One shard
 * streams input/ straight into HBM (tfidf_ingest_dir_device).  The work runs on the GPU
 * through libtfidf_hip.so; there is no CPU path.
 *
 * Retrieval (beyond the reference, which ends at output.txt):
 *   --query FILE  every line of FILE (split at '\n' only) is one query, tokenised like a
 *                 document; after output.txt is written, the best documents of each query go
 *                 to the hits file as "q<i>\tdoc<N>\t%.16f" lines (i 1-based, score
 *                 descending, then document id ascending; a query without hits writes nothing);
 *   --top K       hits per query (default 10, at most TFIDF_QUERY_MAX_K);
 *   --hits FILE   the hits file (default hits.txt);
 *   --bm25        rank by Okapi BM25 (tfidf_query_bm25) instead of the summed TF-IDF scores:
 *                 the same hits file and line format, the scores are BM25's;
 *   --bm25-k1 X   its term-frequency saturation (default 1.2, X >= 0);
 *   --bm25-b Y    its length normalisation (default 0.75, 0 <= Y <= 1); the average document
 *                 length is the corpus's own.  Either parameter implies --bm25; any of the
 *                 three without --query is a usage error (exit 2).
 *   --query-ops   clauses (tfidf_query_clauses; host/query_ops.h): a token "+word" of a line must
 *                 occur in a hit, a token "-word" must not, every other token scores as before.
 *                 The operators are read before the analyzer and the n-grams, which then see
 *                 the three texts: --strip-punct never sees them ("+Fox," under --lower
 *                 --strip-punct requires "fox"), and under --ngrams 2 "+new +york" requires the
 *                 phrase new_york (and both words);
 *   --query-all   every token must occur; with --query-ops, every token without an operator;
 *   --min-match M at least M (0..4095) of a line's plain tokens' distinct terms must occur.
 *                 Each of the three implies the clause call, works with --bm25 and keeps the
 *                 hits file's format; without --query each is a usage error (exit 2).
 * With several shards the ranks' hits are merged (tfidf_group_query / tfidf_group_query_bm25 /
 * tfidf_group_query_clauses).
 *   --fuzzy D|auto  term expansion (tfidf_match_terms; host/query_expand.h): every token of a
 *                 line, as the lookup would see it (behind the analyzer and the n-grams), of at most
 *                 64 bytes is matched against the dictionary within D = 0..2 byte edits (auto: 0 up
 *                 to 2 bytes, 1 up to 5, else 2) and the line is rewritten as the words its tokens
 *                 matched, which then goes to the same call as before; --fuzzy-no-transpose counts
 *                 an adjacent transposition as two edits, --fuzzy-prefix P (default 0) requires the
 *                 first P bytes to match, --max-expansions E (default 50, at most 1024) words stand
 *                 in for a token, the best by distance, then df;
 *   --prefix-ops  a token of >= 2 bytes that ends in '*' (read before the analyzer) is a prefix:
 *                 every word that starts with it, the best E by df.  Works with --bm25 and
 *                 --shards; the hits file keeps its format.  Not with --query-ops, --query-all or
 *                 --min-match (exit 2).
 *   --suggest FILE  instead of ranking, the matches of every distinct token of every line of FILE
 *                 go to suggest.txt (--suggest-file FILE) as q<i>\t<token>\t<word>\t<dist>\t<df>;
 *                 needs --fuzzy or --prefix-ops (exit 2); also as `tfidf --model FILE --suggest
 *                 FILE`, without input/ or output.txt.
 *   --snippets W  after the hits file, the best passage of W tokens (1..1024) of every hit
 *                 (tfidf_snippet / tfidf_group_snippet) goes to snippets.txt (--snippets-file FILE),
 *                 one line per hit: q<i>\tdoc<N>\t<first token>\t<cover>/<query terms>\t<text>,
 *                 every marked term in [ ] (at most --snippet-marks M, default 32), bytes below
 *                 0x20 as blanks, trailing blanks trimmed.  The query text is what went to the
 *                 ranking call: behind the analyzer, under --fuzzy / --prefix-ops the rewritten
 *                 line, with --query-ops / --query-all / --min-match the must and should texts
 *                 joined (must-not words are not highlighted).  Works with --bm25 and --shards;
 *                 needs --query; not with --ngrams or --model (exit 2).  The text is the corpus as
 *                 the counter saw it (behind the analyzer).
 *
 * Keywords (the k best-scoring words of every document, tfidf_top_terms):
 *   --keywords K          after output.txt (and after the hits file of --query), one line
 *                         "doc<N>\t<word>\t%.16f" per returned word: documents in "docN@"
 *                         order, a document's words by score descending, then in the order
 *                         of its output.txt lines; K is 1..TFIDF_TERMS_MAX_K;
 *   --keywords-file FILE  the keywords file (default keywords.txt).
 * With several shards the ranks' rows are written in rank order (tfidf_group_top_terms).
 *
 * Similar documents (nearest neighbours under the cosine similarity of the TF-IDF vectors,
 * tfidf_similar):
 *   --similar K           after output.txt (and the files of --query and --keywords), one line
 *                         "doc<N>\tdoc<M>\t%.16f" per returned neighbour: documents in "docN@"
 *                         order, a document's neighbours by similarity descending, then document
 *                         id ascending; K is 1..TFIDF_SIMILAR_MAX_K.  Every document is a row:
 *                         ceil(N / group) scans of the scored pairs, group <= 64;
 *   --similar-docs FILE   rows for the document ids of FILE only (one id per line), in FILE's
 *                         order;
 *   --similar-file FILE   the neighbours file (default similar.txt).
 * With several shards the result is the single-shard one (tfidf_group_similar).
 *
 * Clusters (spherical k-means over the TF-IDF vectors, tfidf_kmeans):
 *   --clusters K           after output.txt (and the files of --query, --keywords and --similar),
 *                          K clusters, 1..TFIDF_KMEANS_MAX_K.  First one line per cluster,
 *                          "c<i>\t<size>\t<word>:%.16f <word>:%.16f ..", its best terms by weight
 *                          descending; then one line per document in "docN@" order,
 *                          "doc<N>\tc<i>\t%.16f" (the similarity to its centroid), or
 *                          "doc<N>\t-\t0.0000000000000000" for a document whose every score is 0;
 *   --clusters-iter I      at most I passes (default 20);
 *   --clusters-seeds FILE  the K seed document ids (one per line) instead of the default seeds;
 *   --clusters-terms T     terms per cluster line, 0..TFIDF_KMEANS_MAX_TERMS (default 10);
 *   --clusters-file FILE   the clusters file (default clusters.txt).
 * One shard only: with --gpus or --shards above 1 the option is refused (the shards' term tables
 * differ, so they share no centroid matrix).
 *
 * Near duplicates (MinHash signatures, LSH bands, exact Jaccard: tfidf_near_dups):
 *   --near-dups T              after output.txt and the other files, and after the pruning and
 *                              weighting options: the pairs of documents whose exact Jaccard over
 *                              their resident terms is at least T (0..1; 0.8 is the usual choice).
 *                              First one line per group of two or more,
 *                              "g<i>\t<size>\tdoc<a> doc<b> ..", members in "docN@" order, groups by
 *                              their first member; then one line per kept pair,
 *                              "doc<A>\tdoc<B>\t<shared>\t<union>\t%.16f";
 *   --near-dups-hashes H       hash functions, 1..TFIDF_MINHASH_MAX_H (default 128);
 *   --near-dups-rows R         rows per band, a divisor of H (default 4);
 *   --near-dups-seed S         the hash family's seed (default 1);
 *   --near-dups-file FILE      the file (default dups.txt).
 * With --ngrams the sets are shingle sets.  One shard only and not under --model (exit 2), like
 * --clusters.
 *
 * Transform (documents the run has not seen, scored with the run's vocabulary, df, N and idf,
 * tfidf_transform):
 *   --transform DIR        after output.txt (and the other files), DIR/doc1..docM are read under
 *                          the input contract (TFIDF.c:98-110,130-147) and written as
 *                          "docM@word\t%.16f" lines, documents in "docN@" order, a document's
 *                          words in output.txt's order; words the run's vocabulary does not hold
 *                          give no line (they still count in docSize).  `--transform input`
 *                          reproduces output.txt byte for byte;
 *   --transform-file FILE  the file (default transform.txt).
 * With several shards the ranks' rows are merged by word (tfidf_group_transform).
 *
 * Classification (Naive Bayes fitted on the documents a file labels: tfidf_nb_fit and
 * tfidf_nb_predict / tfidf_nb_predict_rows):
 *   --labels FILE          lines "doc<N>\t<name>": document N of input/ belongs to class <name>.  The
 *                          classes are the distinct names in byte order (host/labels_file.h).  The fit
 *                          runs after output.txt and the other files, on the pairs the pruning
 *                          options left; the weighting options play no part (counts only).
 *                          With it exactly one of:
 *   --classify DIR         DIR/doc1..docM go through the analyzer and n-gram options like the
 *                          documents of --transform DIR, then tfidf_transform, and are classified;
 *   --classify-unlabelled  the documents of input/ that FILE does not label are classified;
 *   --classify-file FILE   the file (default classes.txt): a line "doc<M>\t<name>\t%.16f" per
 *                          classified document, the class and its score, documents in "docN@" order;
 *   --nb-alpha X           the smoothing, finite and > 0 (default 1);
 *   --nb-complement        complement NB in place of multinomial NB;
 *   --nb-binary            a word counts once per document;
 *   --nb-uniform-prior     no class prior (the complement never has one).
 * One shard only and not under --model (exit 2), like --clusters.
 *
 * Model (the term table, the global df and N as a file: fit once, serve from the file):
 *   --save-model FILE      after output.txt and the other files, the run's model is written to
 *                          FILE (tfidf_model_export + tfidf_model_save; with several shards
 *                          tfidf_group_model_export: the same bytes as with one);
 *   --model FILE           no run: input/ is not read and output.txt is not written; FILE is
 *                          imported (tfidf_model_load + tfidf_model_import) and --transform DIR,
 *                          which must be given, is scored against it on one GPU.  With an option
 *                          that needs the run's pairs (--query, --keywords, --similar,
 *                          --save-model, --debug-jobs) it is a usage error (exit 2).
 *
 * Analyzer (case folding, punctuation, short tokens and stop words, applied to the bytes before
 * they are counted: tfidf_analyze on the GPU for input/, tfidf_analyze_host for the rest):
 *   --lower                0x41..0x5A become lower case;
 *   --strip-punct          every ASCII byte that is no letter, digit or separator becomes a blank;
 *   --min-token N          tokens shorter than N bytes are blanked, N is 0..TFIDF_AN_MAX_WORD;
 *   --stopwords FILE       the words of FILE (split at separators, passed through the same
 *                          --lower / --strip-punct first, so "The" in the file works with
 *                          --lower) are blanked; at most TFIDF_AN_MAX_STOP words.
 *   --stem                 the tokens that are left, when they are 3..64 lower-case ASCII
 *                          letters, are replaced by their Porter stems (TFIDF_STEM_PORTER).  It
 *                          does not imply --lower: "Running" stays without it.  The words of
 *                          --stopwords FILE are not stemmed: they are compared with the
 *                          unstemmed tokens.
 *   --utf8                 TFIDF_AN_UTF8: --lower also folds the UTF-8 sequences of cased
 *                          letters whose lowercase has the same length, and --strip-punct also
 *                          blanks the sequences of punctuation, symbols and separators (NBSP,
 *                          typographic quotes and dashes, emoji).  Alone it changes nothing.  The
 *                          words of --stopwords FILE pass through the same map.
 * With any of the six, input/ is analyzed in HBM between ingest and run (every shard on its own
 * GPU), and the lines of --query FILE and the documents of --transform DIR pass through the same
 * analyzer on the host, also under --model FILE.  The model file does not record the analyzer:
 * whoever serves from it passes the same flags again.  Without any of them nothing new is
 * called and every byte of every output is as before.
 *
 * Word n-grams (tfidf_ngrams on the GPU for input/, tfidf_ngrams_host for the rest), behind the
 * analyzer:
 *   --ngrams SPEC          SPEC is N (= 1-N) or A-B with 1 <= A <= B <= TFIDF_NGRAM_MAX_N: the
 *                          terms are the grams of A..B consecutive tokens of a document, joined
 *                          by '_'.  A bad SPEC ("0", "3-2", "9", "1-") is a usage error (exit 2).
 *   --ngram-joiner C       the byte C instead of '_' (no separator); needs --ngrams.
 * input/ is shingled in HBM after the analyzer (every shard on its own GPU), the lines of
 * --query FILE and the documents of --transform DIR on the host, also under --model FILE.  The
 * model file does not record the option.  Without --ngrams nothing new is called.
 *
 * Vocabulary pruning by document frequency (tfidf_prune / tfidf_group_prune after the run,
 * tfidf_model_prune under --model FILE), before output.txt and every other file:
 *   --min-df X             drop the words in fewer than X documents;
 *   --max-df X             drop the words in more than X documents.  X is a count, or with a '.'
 *                          a fraction of N in (0, 1]: ceil(X * N) for --min-df, floor(X * N) for
 *                          --max-df;
 *   --max-features M       of the words that pass, keep the M in the most documents (ties by word
 *                          order).  One shard only: with --gpus or --shards above 1 it is refused
 *                          (exit 2), like --clusters.
 * Scores, counts and docSize are the run's: nothing is recomputed, so --transform input against
 * the pruned result reproduces the pruned output.txt.  A model saved after pruning holds the
 * kept words only and needs no option when it is served.  Without the options nothing new is
 * called and every byte of every output is as before.
 *
 * Weighting schemes (tfidf_reweight / tfidf_group_reweight after the run and after the pruning
 * options, before output.txt and every other file; under --model FILE after the import):
 *   --tf ratio|raw|log|binary     the term frequency: count / docSize (the reference's), the count,
 *                                 1 + ln(count), or 1.  --sublinear-tf is a synonym of --tf log.
 *   --idf ref|smooth|plus1|none   ln(N / df) (the reference's), ln((N + 1) / (df + 1)) + 1,
 *                                 ln(N / df) + 1, or 1.
 *   --norm none|l1|l2             every document's scores divided by their sum or by the root of the
 *                                 sum of their squares.
 * --tf raw needs a norm.  --query, --keywords, --similar, --clusters and --transform follow the
 * scheme (BM25 does not read the scores); --transform input reproduces output.txt.  The model
 * file does not record the scheme: pass the options again with --model FILE.  With --debug-jobs
 * the options are refused (exit 2): those blocks are the reference's.  Without the options
 * nothing new is called and every byte of every output is as before.
 */
#include <dirent.h>
#include <math.h>
#include <pthread.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "../../include/tfidf.h"
#include "labels_file.h"
#include "query_ops.h"
#include "query_expand.h"

static double wall_ms(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec / 1e6;
}

static int fail(int rc) {
    fprintf(stderr, "tfidf: %s\n", tfidf_strerror(rc));
    return 3;
}

/* TFIDF.c:134-138 */
static int missing_doc(const char* indir, uint32_t bad, uint32_t ndocs) {
    printf("Error Opening File: %s/doc%u, rank = %d, i=%u, numDocs= %u\n", indir, bad, 1, bad, ndocs);
    return 0;
}

/* --debug-jobs: the TF Job / IDF Job blocks of one shard (TFIDF.c:199-205,236-239) */
static int debug_jobs(tfidf_ctx* ctx) {
    tfidf_result r;
    int rc = tfidf_fetch(ctx, &r);
    if (rc) return rc;
    tfidf_print_jobs(&r);
    tfidf_result_free(&r);
    return TFIDF_OK;
}

/* --------------------------------------------------------------- analyzer -- */

static struct {
    int on;             /* 0: none of the analyzer's options, behaviour and bytes as without them */
    const char* stopfile;
    tfidf_analyzer an;
} g_an;

/* --stopwords: FILE through the analyzer's own byte map, split at separators.  A word longer than
 * TFIDF_AN_MAX_WORD bytes or one that holds a NUL equals no token that can be blanked: dropped. */
static int load_stopwords(void) {
    g_an.an.size = sizeof(g_an.an);
    if (!g_an.stopfile) return TFIDF_OK;
    FILE* f = fopen(g_an.stopfile, "rb");
    if (!f) { fprintf(stderr, "tfidf: --stopwords: cannot open %s\n", g_an.stopfile); return TFIDF_E_INVAL; }
    size_t cap = 1 << 16, n = 0;
    uint8_t* b = (uint8_t*)malloc(cap);
    for (;;) {
        if (!b) { fclose(f); return TFIDF_E_NOMEM; }
        const size_t got = fread(b + n, 1, cap - n, f);
        n += got;
        if (got == 0) break;
        if (n == cap) { cap *= 2; b = (uint8_t*)realloc(b, cap); }
    }
    fclose(f);
    tfidf_analyzer map = g_an.an;   /* the same flags, no list, every token kept, no stemmer */
    map.min_len = 0;
    map.stemmer = TFIDF_STEM_NONE;
    const uint64_t whole[2] = {0, n};
    int rc = tfidf_analyze_host(&map, b, n, whole, 1, b);
    uint64_t* off = (uint64_t*)malloc(((size_t)TFIDF_AN_MAX_STOP + 1) * sizeof(uint64_t));
    if (!rc && !off) rc = TFIDF_E_NOMEM;
    uint32_t nw = 0;
    size_t w = 0;   /* the kept words, packed at the buffer's front */
    if (off) off[0] = 0;
    for (size_t i = 0; !rc && i < n;) {
        const uint8_t c = b[i];
        if (c == 0x20 || (c >= 0x09 && c <= 0x0D)) { ++i; continue; }
        size_t j = i;
        int nul = 0;
        while (j < n && !(b[j] == 0x20 || (b[j] >= 0x09 && b[j] <= 0x0D))) nul |= b[j++] == 0;
        if (!nul && j - i <= TFIDF_AN_MAX_WORD) {
            if (nw == TFIDF_AN_MAX_STOP || w + (j - i) > TFIDF_AN_MAX_STOP_BYTES) {
                fprintf(stderr, "tfidf: --stopwords takes at most %u words and %u bytes\n", TFIDF_AN_MAX_STOP,
                        TFIDF_AN_MAX_STOP_BYTES);
                rc = TFIDF_E_INVAL;
                break;
            }
            memmove(b + w, b + i, j - i);
            w += j - i;
            off[++nw] = w;
        }
        i = j;
    }
    if (rc) { free(b); free(off); return rc; }
    g_an.an.stop_bytes = b;
    g_an.an.stop_off = off;
    g_an.an.nstop = nw;
    return TFIDF_OK;
}

/* the analyzer on host bytes in place (query lines, transform batches); a no-op without its options */
static int analyze_host_batch(uint8_t* bytes, uint64_t nbytes, const uint64_t* off, uint32_t n) {
    return g_an.on ? tfidf_analyze_host(&g_an.an, bytes, nbytes, off, n, bytes) : TFIDF_OK;
}

/* ---------------------------------------------------------------- n-grams -- */

static struct {
    int on;             /* 0: no --ngrams, behaviour and bytes as without the option */
    tfidf_ngram_params p;
} g_ng;

/* --ngrams SPEC: N (= 1-N) or A-B, decimal digits only */
static int parse_ngram_spec(const char* spec) {
    char* end = NULL;
    if (spec[0] < '0' || spec[0] > '9') return TFIDF_E_INVAL;
    const unsigned long a = strtoul(spec, &end, 10);
    unsigned long b = a, lo = 1;
    if (*end == '-') {
        const char* q = end + 1;
        if (q[0] < '0' || q[0] > '9') return TFIDF_E_INVAL;
        b = strtoul(q, &end, 10);
        lo = a;
    }
    if (*end || lo < 1 || b < lo || b > TFIDF_NGRAM_MAX_N) return TFIDF_E_INVAL;
    memset(&g_ng.p, 0, offsetof(tfidf_ngram_params, joiner));   /* --ngram-joiner may have come first */
    g_ng.p.size = sizeof(g_ng.p);
    g_ng.p.min_n = (uint32_t)lo;
    g_ng.p.max_n = (uint32_t)b;
    g_ng.on = 1;
    return TFIDF_OK;
}

/* the shingled batch in place of a host batch (query lines, transform batches), behind the
 * analyzer; the old arrays are freed.  A no-op without --ngrams */
static int ngram_host_batch(uint8_t** bytes, uint64_t* nbytes, uint64_t** off, uint32_t n) {
    if (!g_ng.on) return TFIDF_OK;
    uint8_t* ob = NULL;
    uint64_t on = 0, *oo = NULL;
    const int rc = tfidf_ngrams_host(&g_ng.p, *bytes, *nbytes, *off, n, &ob, &on, &oo);
    if (rc) return rc;
    tfidf_free(*bytes);
    tfidf_free(*off);
    *bytes = ob;
    *nbytes = on;
    *off = oo;
    return TFIDF_OK;
}

/* ---------------------------------------------------------------- queries -- */

static struct {
    const char* file;   /* NULL: no retrieval, behaviour and bytes as without the option */
    const char* hits;
    uint32_t top;
    int bm25;           /* 0: the summed TF-IDF scores, bytes as without the option */
    double k1, b;
    int ops, all;       /* --query-ops, --query-all */
    long min_match;     /* --min-match, -1: not given.  None of the three: the calls and bytes as without them */
} g_query = {NULL, "hits.txt", 10, 0, TFIDF_BM25_DEFAULT_K1, TFIDF_BM25_DEFAULT_B, 0, 0, -1};

/* the query file's lines as one batch (tfidf_queries): q_off at the line starts */
static int load_queries(const char* path, uint8_t** bytes, uint64_t* nbytes, uint64_t** off, uint32_t* nq) {
    FILE* f = fopen(path, "rb");
    if (!f) return TFIDF_E_NOINPUT;
    size_t cap = 1 << 16, n = 0;
    uint8_t* b = (uint8_t*)malloc(cap);
    for (;;) {
        if (!b) { fclose(f); return TFIDF_E_NOMEM; }
        const size_t got = fread(b + n, 1, cap - n, f);
        n += got;
        if (got == 0) break;
        if (n == cap) { cap *= 2; b = (uint8_t*)realloc(b, cap); }
    }
    fclose(f);
    size_t lines = 0;
    for (size_t i = 0; i < n; ++i) lines += b[i] == '\n';
    if (n && b[n - 1] != '\n') ++lines;   /* a last line without its newline */
    if (lines > TFIDF_QUERY_MAX_QUERIES) { free(b); return TFIDF_E_INVAL; }
    uint64_t* o = (uint64_t*)malloc((lines + 1) * sizeof(uint64_t));
    if (!o) { free(b); return TFIDF_E_NOMEM; }
    size_t q = 0;
    o[0] = 0;
    for (size_t i = 0; i < n; ++i)
        if (b[i] == '\n') o[++q] = i + 1;   /* the newline stays in its query: whitespace */
    if (q < lines) o[++q] = n;
    *bytes = b;
    *nbytes = n;
    *off = o;
    *nq = (uint32_t)lines;
    return TFIDF_OK;
}

/* ---- term expansion (--fuzzy, --prefix-ops, --suggest; query_expand.h) ---- */
static struct {
    int fuzzy;              /* QEXP_OFF: no --fuzzy; 0..2 or QEXP_AUTO */
    int prefix_ops;
    int no_transpose;
    int opts;               /* --fuzzy-no-transpose, --fuzzy-prefix or --max-expansions given */
    uint32_t fixed_prefix, max_expansions;
    const char* suggest;    /* NULL: no suggestions.  None of these: the calls and bytes as without them */
    const char* suggest_file;
} g_expand = {QEXP_OFF, 0, 0, 0, 0, 50, NULL, "suggest.txt"};

/* a file's lines as the call sees them: the plain and the prefix text behind the analyzer and the
 * n-grams, their tokens and patterns, and the patterns' matches in ctx's or the group's dictionary */
typedef struct {
    uint8_t* tb[2];
    uint64_t tn[2], *to[2];
    uint32_t nq;
    qexp_plan plan;
    tfidf_term_matches m;
} expansion;

static void expansion_free(expansion* x) {
    for (int c = 0; c < 2; ++c) { free(x->tb[c]); free(x->to[c]); }
    qexp_plan_free(&x->plan);
    tfidf_term_matches_free(&x->m);
    memset(x, 0, sizeof(*x));
}

static int expansion_load(tfidf_ctx* ctx, tfidf_group* g, const char* path, expansion* x) {
    memset(x, 0, sizeof(*x));
    int rc = load_queries(path, &x->tb[0], &x->tn[0], &x->to[0], &x->nq);
    if (rc) return rc;
    if (g_expand.prefix_ops) {
        uint8_t* sb[2];
        uint64_t sn[2], *so[2];
        if (qexp_split_batch(x->tb[0], x->to[0], x->nq, sb, sn, so)) rc = TFIDF_E_NOMEM;
        if (!rc) {
            free(x->tb[0]);
            free(x->to[0]);
            for (int c = 0; c < 2; ++c) { x->tb[c] = sb[c]; x->tn[c] = sn[c]; x->to[c] = so[c]; }
        }
    }
    for (int c = 0; c < 2 && !rc; ++c) {
        if (!x->tb[c]) continue;
        rc = analyze_host_batch(x->tb[c], x->tn[c], x->to[c], x->nq);
        if (!rc) rc = ngram_host_batch(&x->tb[c], &x->tn[c], &x->to[c], x->nq);
    }
    if (!rc) {
        const uint8_t* const text[2] = {x->tb[0], x->tb[1]};
        const uint64_t* const off[2] = {x->to[0], x->to[1]};
        const int q = qexp_plan_build(text, off, x->nq, g_expand.fuzzy, &x->plan);
        if (q == QEXP_E_PATTERNS) fprintf(stderr, "tfidf: %s holds more than %u distinct patterns\n", path, TFIDF_MATCH_MAX_PATTERNS);
        rc = q == QEXP_E_NOMEM ? TFIDF_E_NOMEM : q ? TFIDF_E_INVAL : TFIDF_OK;
    }
    if (!rc) {
        tfidf_match_params mp;
        memset(&mp, 0, sizeof(mp));
        mp.size = sizeof(mp);
        mp.max_expansions = g_expand.max_expansions;
        mp.flags = g_expand.no_transpose ? 0u : TFIDF_MATCH_TRANSPOSE;
        mp.fixed_prefix = g_expand.fixed_prefix;
        rc = g ? tfidf_group_match_terms(g, &x->plan.patterns, &mp, &x->m) : tfidf_match_terms(ctx, &x->plan.patterns, &mp, &x->m);
    }
    if (rc) expansion_free(x);
    return rc;
}

/* --suggest: the matches of every token of FILE's lines, from ctx's dictionary or every rank's of g */
static int run_suggest(tfidf_ctx* ctx, tfidf_group* g) {
    if (!g_expand.suggest) return TFIDF_OK;
    expansion x;
    int rc = expansion_load(ctx, g, g_expand.suggest, &x);
    if (rc == TFIDF_E_NOINPUT) { printf("Error Opening File: %s\n", g_expand.suggest); return TFIDF_OK; }
    if (rc) return rc;
    FILE* f = fopen(g_expand.suggest_file, "w");
    if (!f) printf("Error Opening File: %s\n", g_expand.suggest_file);
    if (f) {
        qexp_suggest(&x.plan, x.nq, &x.m, f);
        if (fclose(f) != 0) rc = TFIDF_E_OUTPUT;
    }
    expansion_free(&x);
    return rc;
}

static void write_hits(const tfidf_hits* h, int* rc) {
    FILE* f = fopen(g_query.hits, "w");
    if (!f) printf("Error Opening File: %s\n", g_query.hits);
    for (uint32_t q = 0; f && q < h->nqueries; ++q)
        for (uint32_t i = 0; i < h->nhits[q]; ++i)
            fprintf(f, "q%u\tdoc%u\t%.16f\n", q + 1, h->doc[(size_t)q * h->k + i], h->score[(size_t)q * h->k + i]);
    if (f && fclose(f) != 0) *rc = TFIDF_E_OUTPUT;
}

/* ---- --snippets: the best passage of every hit (tfidf_snippet / tfidf_group_snippet) ---- */
static struct {
    int window;         /* 0: no snippets, calls and bytes as without the option */
    int marks;
    const char* file;
} g_snip = {0, 32, "snippets.txt"};

/* After the hits file: the hits are the jobs, `qs` the text that went to the ranking call.  One line
 * per hit: q<i>\tdoc<N>\t<s'>\t<cover>/<|U|>\t<text>, every marked term in [ ], bytes below 0x20
 * as blanks, trailing blanks trimmed. */
static int write_snippets(tfidf_ctx* ctx, tfidf_group* g, const tfidf_queries* qs, const tfidf_hits* h) {
    if (!g_snip.window) return TFIDF_OK;
    size_t nj = 0;
    for (uint32_t q = 0; q < h->nqueries; ++q) nj += h->nhits[q];
    uint32_t* jq = (uint32_t*)malloc((nj + 1) * sizeof(uint32_t));
    uint32_t* jd = (uint32_t*)malloc((nj + 1) * sizeof(uint32_t));
    if (!jq || !jd) { free(jq); free(jd); return TFIDF_E_NOMEM; }
    nj = 0;
    for (uint32_t q = 0; q < h->nqueries; ++q)
        for (uint32_t i = 0; i < h->nhits[q]; ++i) {
            jq[nj] = q;
            jd[nj++] = h->doc[(size_t)q * h->k + i];
        }
    tfidf_snippet_params pr;
    memset(&pr, 0, sizeof(pr));
    pr.size = sizeof(pr);
    pr.window = (uint32_t)g_snip.window;
    pr.max_marks = (uint32_t)g_snip.marks;
    pr.flags = TFIDF_SNIP_TEXT;
    tfidf_snippets s;
    int rc = g ? tfidf_group_snippet(g, qs, jq, jd, (uint32_t)nj, &pr, &s) : tfidf_snippet(ctx, qs, jq, jd, (uint32_t)nj, &pr, &s);
    if (!rc) {
        FILE* f = fopen(g_snip.file, "w");
        if (!f) printf("Error Opening File: %s\n", g_snip.file);
        for (size_t j = 0; f && j < nj; ++j) {
            const uint8_t* t = s.text + s.text_off[j];
            const uint64_t n = s.text_off[j + 1] - s.text_off[j], base = s.win_byte[2 * j];
            const uint64_t m0 = s.mark_off[j], m1 = s.mark_off[j + 1];
            uint8_t* line = (uint8_t*)malloc((size_t)(n + 2 * (m1 - m0) + 1));
            if (!line) { rc = TFIDF_E_NOMEM; break; }
            uint64_t len = 0, at = 0;
            for (uint64_t m = m0; m < m1; ++m) {   /* the marks lie inside the text, in position order */
                const uint64_t b = s.mark_byte[m] - base, e = b + s.mark_len[m];
                memcpy(line + len, t + at, (size_t)(b - at));
                len += b - at;
                line[len++] = '[';
                memcpy(line + len, t + b, (size_t)(e - b));
                len += e - b;
                line[len++] = ']';
                at = e;
            }
            memcpy(line + len, t + at, (size_t)(n - at));
            len += n - at;
            for (uint64_t i = 0; i < len; ++i)
                if (line[i] < 0x20u) line[i] = ' ';
            while (len && line[len - 1] == ' ') --len;
            fprintf(f, "q%u\tdoc%u\t%u\t%u/%llu\t", jq[j] + 1, jd[j], s.win_tok[2 * j], s.cover[j],
                    (unsigned long long)(s.qterm_off[jq[j] + 1] - s.qterm_off[jq[j]]));
            fwrite(line, 1, (size_t)len, f);
            free(line);
            fputc('\n', f);
        }
        if (f && fclose(f) != 0) rc = TFIDF_E_OUTPUT;
        tfidf_snippets_free(&s);
    }
    free(jq);
    free(jd);
    return rc;
}

/* --query with --query-ops, --query-all or --min-match: the lines' tokens sorted into the three
 * texts (query_ops.h), each text through the analyzer and the n-grams like the lines themselves */
static int run_clause_queries(tfidf_ctx* ctx, tfidf_group* g) {
    uint64_t* off = NULL;
    uint8_t* bytes = NULL;
    uint64_t nbytes = 0;
    uint32_t nq = 0;
    int rc = load_queries(g_query.file, &bytes, &nbytes, &off, &nq);
    if (rc == TFIDF_E_NOINPUT) { printf("Error Opening File: %s\n", g_query.file); return TFIDF_OK; }
    if (rc) return rc;
    uint8_t* tb[3] = {NULL, NULL, NULL};
    uint64_t tn[3] = {0, 0, 0}, *to[3] = {NULL, NULL, NULL};
    if (qops_split_batch(bytes, off, nq, g_query.ops, g_query.all, tb, tn, to)) rc = TFIDF_E_NOMEM;
    free(bytes);
    free(off);
    tfidf_queries text[3];
    memset(text, 0, sizeof(text));
    for (int c = 0; c < 3 && !rc; ++c) {
        rc = analyze_host_batch(tb[c], tn[c], to[c], nq);
        if (!rc) rc = ngram_host_batch(&tb[c], &tn[c], &to[c], nq);
        text[c].bytes = tb[c];
        text[c].nbytes = tn[c];
        text[c].q_off = to[c];
        text[c].nqueries = nq;
    }
    uint32_t* mm = NULL;
    if (!rc && g_query.min_match > 0) {
        mm = (uint32_t*)malloc(((size_t)nq + 1) * sizeof(uint32_t));
        if (!mm) rc = TFIDF_E_NOMEM;
        for (uint32_t q = 0; mm && q < nq; ++q) mm[q] = (uint32_t)g_query.min_match;
    }
    tfidf_hits h;
    memset(&h, 0, sizeof(h));
    if (!rc) {
        tfidf_bm25_params bp;
        memset(&bp, 0, sizeof(bp));
        bp.size = sizeof(bp);
        bp.k1 = g_query.k1;
        bp.b = g_query.b;
        tfidf_clauses cl;
        memset(&cl, 0, sizeof(cl));
        cl.size = sizeof(cl);
        cl.nqueries = nq;
        cl.ranking = g_query.bm25 ? TFIDF_RANK_BM25 : TFIDF_RANK_TFIDF;
        cl.must = &text[QOPS_MUST];
        cl.should = &text[QOPS_SHOULD];
        cl.must_not = &text[QOPS_MUST_NOT];
        cl.min_should = mm;
        cl.bm25 = g_query.bm25 ? &bp : NULL;
        rc = g ? tfidf_group_query_clauses(g, &cl, g_query.top, &h) : tfidf_query_clauses(ctx, &cl, g_query.top, &h);
    }
    if (!rc) write_hits(&h, &rc);
    if (!rc && g_snip.window) {   /* the must and should texts joined; must-not words are not highlighted */
        tfidf_queries joined;
        memset(&joined, 0, sizeof(joined));
        uint64_t* jo = (uint64_t*)malloc(((size_t)nq + 1) * sizeof(uint64_t));
        uint8_t* jb = (uint8_t*)malloc((size_t)(tn[QOPS_MUST] + tn[QOPS_SHOULD] + nq + 1));
        if (!jo || !jb) rc = TFIDF_E_NOMEM;
        uint64_t at = 0;
        for (uint32_t q = 0; !rc && q < nq; ++q) {
            jo[q] = at;
            for (int c = 0; c < 2; ++c) {
                const int x = c ? QOPS_SHOULD : QOPS_MUST;
                const uint64_t n = to[x][q + 1] - to[x][q];
                memcpy(jb + at, tb[x] + to[x][q], (size_t)n);
                at += n;
                if (!c) jb[at++] = ' ';
            }
        }
        if (!rc) {
            jo[nq] = at;
            joined.bytes = jb;
            joined.nbytes = at;
            joined.q_off = jo;
            joined.nqueries = nq;
            rc = write_snippets(ctx, g, &joined, &h);
        }
        free(jo);
        free(jb);
    }
    tfidf_hits_free(&h);
    free(mm);
    for (int c = 0; c < 3; ++c) { free(tb[c]); free(to[c]); }
    return rc;
}

/* --query: ranks the resident result of ctx (one shard) or of every rank of g */
static int run_queries(tfidf_ctx* ctx, tfidf_group* g) {
    if (!g_query.file) return TFIDF_OK;
    if (g_query.ops || g_query.all || g_query.min_match >= 0) return run_clause_queries(ctx, g);
    tfidf_queries qs;
    uint64_t* off = NULL;
    uint8_t* bytes = NULL;
    memset(&qs, 0, sizeof(qs));
    int rc;
    if (g_expand.fuzzy != QEXP_OFF || g_expand.prefix_ops) {   /* the lines' tokens stand for the words they match */
        expansion x;
        rc = expansion_load(ctx, g, g_query.file, &x);
        if (rc == TFIDF_E_NOINPUT) { printf("Error Opening File: %s\n", g_query.file); return TFIDF_OK; }
        if (!rc) {
            const uint8_t* const text[2] = {x.tb[0], x.tb[1]};
            qs.nqueries = x.nq;
            if (qexp_rewrite(&x.plan, text, x.nq, &x.m, &bytes, &qs.nbytes, &off)) rc = TFIDF_E_NOMEM;
            expansion_free(&x);
        }
    } else {
        rc = load_queries(g_query.file, &bytes, &qs.nbytes, &off, &qs.nqueries);
        if (rc == TFIDF_E_NOINPUT) { printf("Error Opening File: %s\n", g_query.file); return TFIDF_OK; }
        if (!rc) rc = analyze_host_batch(bytes, qs.nbytes, off, qs.nqueries);
        if (!rc) rc = ngram_host_batch(&bytes, &qs.nbytes, &off, qs.nqueries);
    }
    if (rc) { free(bytes); free(off); return rc; }
    qs.bytes = bytes;
    qs.q_off = off;
    tfidf_hits h;
    memset(&h, 0, sizeof(h));
    if (g_query.bm25) {
        tfidf_bm25_params bp;
        memset(&bp, 0, sizeof(bp));
        bp.size = sizeof(bp);
        bp.k1 = g_query.k1;
        bp.b = g_query.b;
        rc = g ? tfidf_group_query_bm25(g, &qs, g_query.top, &bp, &h) : tfidf_query_bm25(ctx, &qs, g_query.top, &bp, &h);
    } else {
        rc = g ? tfidf_group_query(g, &qs, g_query.top, &h) : tfidf_query(ctx, &qs, g_query.top, &h);
    }
    if (!rc) write_hits(&h, &rc);
    if (!rc) rc = write_snippets(ctx, g, &qs, &h);
    tfidf_hits_free(&h);
    free(bytes);
    free(off);
    return rc;
}

/* --------------------------------------------------------------- keywords -- */

static struct {
    uint32_t k;         /* 0: no keywords, behaviour and bytes as without the option */
    const char* file;
} g_keywords = {0, "keywords.txt"};

/* --keywords: the best words of every document of ctx (one shard) or of every rank of g */
static int run_keywords(tfidf_ctx* ctx, tfidf_group* g) {
    if (!g_keywords.k) return TFIDF_OK;
    tfidf_doc_terms t;
    memset(&t, 0, sizeof(t));
    int rc = g ? tfidf_group_top_terms(g, NULL, 0, g_keywords.k, &t) : tfidf_top_terms(ctx, NULL, 0, g_keywords.k, &t);
    if (rc) return rc;
    FILE* f = fopen(g_keywords.file, "w");
    if (!f) printf("Error Opening File: %s\n", g_keywords.file);
    for (uint32_t r = 0; f && r < t.ndocs; ++r)
        for (uint32_t j = 0; j < t.nterms[r]; ++j) {
            const size_t e = (size_t)r * t.k + j;
            fprintf(f, "doc%u\t", t.doc[r]);
            fwrite(t.word_bytes + t.word_off[e], 1, (size_t)(t.word_off[e + 1] - t.word_off[e]), f);
            fprintf(f, "\t%.16f\n", t.score[e]);
        }
    if (f && fclose(f) != 0) rc = TFIDF_E_OUTPUT;
    tfidf_doc_terms_free(&t);
    return rc;
}

/* ---------------------------------------------------------------- similar -- */

static struct {
    uint32_t k;         /* 0: no search, behaviour and bytes as without the option */
    const char* docs;   /* NULL: every document */
    const char* file;
} g_similar = {0, NULL, "similar.txt"};

/* --similar: the nearest neighbours of the documents of ctx (one shard) or of every rank of g */
static int run_similar(tfidf_ctx* ctx, tfidf_group* g) {
    if (!g_similar.k) return TFIDF_OK;
    uint32_t* ids = NULL;
    uint32_t nids = 0;
    if (g_similar.docs) {
        FILE* f = fopen(g_similar.docs, "r");
        if (!f) { printf("Error Opening File: %s\n", g_similar.docs); return TFIDF_OK; }
        size_t cap = 1024;
        ids = (uint32_t*)malloc(cap * sizeof(uint32_t));
        unsigned long long v;
        while (ids && fscanf(f, "%llu", &v) == 1) {
            if (nids == cap) { cap *= 2; ids = (uint32_t*)realloc(ids, cap * sizeof(uint32_t)); }
            if (ids) ids[nids++] = v > 0xFFFFFFFFull ? 0u : (uint32_t)v;   /* no document has id 0 */
        }
        fclose(f);
        if (!ids) return TFIDF_E_NOMEM;
    }
    tfidf_neighbors n;
    memset(&n, 0, sizeof(n));
    int rc = g ? tfidf_group_similar(g, ids, nids, g_similar.k, &n) : tfidf_similar(ctx, ids, nids, g_similar.k, &n);
    free(ids);
    if (rc) return rc;
    FILE* f = fopen(g_similar.file, "w");
    if (!f) printf("Error Opening File: %s\n", g_similar.file);
    for (uint32_t r = 0; f && r < n.ndocs; ++r)
        for (uint32_t j = 0; j < n.nnb[r]; ++j) {
            const size_t e = (size_t)r * n.k + j;
            fprintf(f, "doc%u\tdoc%u\t%.16f\n", n.doc[r], n.nb_doc[e], n.nb_score[e]);
        }
    if (f && fclose(f) != 0) rc = TFIDF_E_OUTPUT;
    tfidf_neighbors_free(&n);
    return rc;
}

/* --------------------------------------------------------------- clusters -- */

static struct {
    uint32_t k;         /* 0: no clustering, behaviour and bytes as without the option */
    uint32_t iter, terms;
    const char* seeds;  /* NULL: the default seeds */
    const char* file;
} g_clusters = {0, 0, 10, NULL, "clusters.txt"};

/* --clusters: k-means over the documents of ctx */
static int run_clusters(tfidf_ctx* ctx) {
    if (!g_clusters.k) return TFIDF_OK;
    uint32_t* ids = NULL;
    uint32_t nids = 0;
    if (g_clusters.seeds) {
        FILE* f = fopen(g_clusters.seeds, "r");
        if (!f) { printf("Error Opening File: %s\n", g_clusters.seeds); return TFIDF_OK; }
        size_t cap = 256;
        ids = (uint32_t*)malloc(cap * sizeof(uint32_t));
        unsigned long long v;
        while (ids && fscanf(f, "%llu", &v) == 1) {
            if (nids == cap) { cap *= 2; ids = (uint32_t*)realloc(ids, cap * sizeof(uint32_t)); }
            if (ids) ids[nids++] = v > 0xFFFFFFFFull ? 0u : (uint32_t)v;   /* no document has id 0 */
        }
        fclose(f);
        if (!ids) return TFIDF_E_NOMEM;
    }
    tfidf_kmeans_params p;
    memset(&p, 0, sizeof(p));
    p.size = sizeof(p);
    p.k = g_clusters.k;
    p.max_iter = g_clusters.iter;
    p.nterms = g_clusters.terms;
    p.seeds = ids;
    p.nseeds = nids;
    tfidf_clusters c;
    memset(&c, 0, sizeof(c));
    int rc = tfidf_kmeans(ctx, &p, &c);
    free(ids);
    if (rc == TFIDF_E_INVAL)
        fprintf(stderr, "tfidf: --clusters: K exceeds the documents with a non-zero vector, or a bad seed list\n");
    if (rc) return rc;
    FILE* f = fopen(g_clusters.file, "w");
    if (!f) printf("Error Opening File: %s\n", g_clusters.file);
    for (uint32_t i = 0; f && i < c.k; ++i) {
        fprintf(f, "c%u\t%u\t", i, c.size[i]);
        for (uint32_t j = 0; j < c.nterms[i]; ++j) {
            const size_t e = (size_t)i * c.t + j;
            if (j) fputc(' ', f);
            fwrite(c.word_bytes + c.word_off[e], 1, (size_t)(c.word_off[e + 1] - c.word_off[e]), f);
            fprintf(f, ":%.16f", c.weight[e]);
        }
        fputc('\n', f);
    }
    for (uint32_t j = 0; f && j < c.ndocs; ++j) {
        if (c.label[j] == TFIDF_NO_CLUSTER) fprintf(f, "doc%u\t-\t%.16f\n", c.doc[j], 0.0);
        else fprintf(f, "doc%u\tc%u\t%.16f\n", c.doc[j], c.label[j], c.sim[j]);
    }
    if (f && fclose(f) != 0) rc = TFIDF_E_OUTPUT;
    tfidf_clusters_free(&c);
    return rc;
}

/* -------------------------------------------------------- near duplicates -- */

static struct {
    int on;             /* 0: no pass, behaviour and bytes as without the option */
    double threshold;
    uint32_t hashes, rows;
    uint64_t seed;
    const char* file;
} g_dups = {0, 0.8, TFIDF_DEDUP_DEFAULT_H, TFIDF_DEDUP_DEFAULT_ROWS, TFIDF_DEDUP_DEFAULT_SEED, "dups.txt"};

/* --near-dups: near-duplicate pairs and groups of the documents of ctx */
static int run_dups(tfidf_ctx* ctx) {
    if (!g_dups.on) return TFIDF_OK;
    tfidf_dedup_params p;
    memset(&p, 0, sizeof(p));
    p.size = sizeof(p);
    p.nhashes = g_dups.hashes;
    p.rows = g_dups.rows;
    p.seed = g_dups.seed;
    p.threshold = g_dups.threshold;
    tfidf_dups d;
    memset(&d, 0, sizeof(d));
    int rc = tfidf_near_dups(ctx, &p, &d);
    if (rc == TFIDF_E_CAPACITY)
        fprintf(stderr, "tfidf: --near-dups: the signatures and candidates exceed TFIDF_DEDUP_MB\n");
    if (rc) return rc;
    FILE* f = fopen(g_dups.file, "w");
    if (!f) printf("Error Opening File: %s\n", g_dups.file);
    /* the members of a group follow its first member in position order: count, then print */
    uint32_t* size = (uint32_t*)calloc((size_t)d.ndocs + 1, sizeof(uint32_t));
    if (!size) { if (f) fclose(f); tfidf_dups_free(&d); return TFIDF_E_NOMEM; }
    for (uint32_t j = 0; j < d.ndocs; ++j) ++size[d.group[j]];
    uint32_t g = 0;
    for (uint32_t j = 0; f && j < d.ndocs; ++j) {
        if (d.group[j] != j || size[j] < 2) continue;
        fprintf(f, "g%u\t%u\t", g++, size[j]);
        int first = 1;
        for (uint32_t m = j; m < d.ndocs; ++m) {
            if (d.group[m] != j) continue;
            fprintf(f, first ? "doc%u" : " doc%u", d.doc[m]);
            first = 0;
        }
        fputc('\n', f);
    }
    free(size);
    for (uint64_t e = 0; f && e < d.nedges; ++e)
        fprintf(f, "doc%u\tdoc%u\t%u\t%u\t%.16f\n", d.a_doc[e], d.b_doc[e], d.shared[e], d.uni[e], d.jaccard[e]);
    if (f && fclose(f) != 0) rc = TFIDF_E_OUTPUT;
    tfidf_dups_free(&d);
    return rc;
}

/* -------------------------------------------------------------- transform -- */

static struct {
    const char* dir;    /* NULL: no transform, behaviour and bytes as without the option */
    const char* file;
} g_transform = {NULL, "transform.txt"};

/* --transform: DIR's documents against the model of ctx (one shard) or of every rank of g */
static int run_transform(tfidf_ctx* ctx, tfidf_group* g) {
    if (!g_transform.dir) return TFIDF_OK;
    tfidf_corpus b;
    memset(&b, 0, sizeof(b));
    uint8_t* bytes = NULL;
    uint64_t* off = NULL;
    uint32_t bad = 0;
    int rc = tfidf_ingest_dir(g_transform.dir, &bytes, &b.nbytes, &off, &b.ndocs, &bad);
    if (rc == TFIDF_E_NOINPUT) { printf("Directory failed to open\n"); return TFIDF_OK; }
    if (rc == TFIDF_E_NODOC) { (void)missing_doc(g_transform.dir, bad, b.ndocs); return TFIDF_OK; }
    if (!rc) rc = analyze_host_batch(bytes, b.nbytes, off, b.ndocs);
    if (!rc) rc = ngram_host_batch(&bytes, &b.nbytes, &off, b.ndocs);   /* kept until the rows are written: word_off points into it */
    if (rc) { tfidf_free(bytes); tfidf_free(off); return rc; }
    b.bytes = bytes;
    b.doc_off = off;
    tfidf_rows t;
    memset(&t, 0, sizeof(t));
    uint32_t* ids = (uint32_t*)malloc(((size_t)b.ndocs + 1) * sizeof(uint32_t));
    rc = ids ? tfidf_doc_name_order(b.ndocs, ids) : TFIDF_E_NOMEM;
    if (!rc) rc = g ? tfidf_group_transform(g, &b, &t) : tfidf_transform(ctx, &b, &t);
    if (!rc) {
        FILE* f = fopen(g_transform.file, "w");
        if (!f) printf("Error Opening File: %s\n", g_transform.file);
        for (uint32_t i = 0; f && i < t.ndocs; ++i) {   /* rows in "docN@" order (TFIDF.c:273) */
            const uint32_t r = ids[i] - 1;
            for (uint64_t x = t.row_off[r]; x < t.row_off[r + 1]; ++x) {
                fprintf(f, "doc%u@", ids[i]);
                fwrite(bytes + t.word_off[x], 1, t.word_len[x], f);
                fprintf(f, "\t%.16f\n", t.score[x]);
            }
        }
        if (f && fclose(f) != 0) rc = TFIDF_E_OUTPUT;
    }
    tfidf_rows_free(&t);
    free(ids);
    tfidf_free(bytes);
    tfidf_free(off);
    return rc;
}

/* --------------------------------------------------------------- classify -- */

static struct {
    const char* labels;   /* NULL: no classification, behaviour and bytes as without the options */
    const char* dir;
    int unlabelled;
    int opts;             /* an --nb-* option was given */
    const char* file;
    tfidf_nb_params p;
    labels_file lf;       /* parsed before anything touches the GPU */
} g_nb = {NULL, NULL, 0, 0, "classes.txt", {sizeof(tfidf_nb_params), 0, TFIDF_NB_MULTINOMIAL, TFIDF_NB_COUNT, 0, 0.0, 0, NULL, NULL},
          {0, 0, NULL, NULL, NULL}};

/* --labels FILE: 0, or 2 after a line on stderr */
static int load_labels(void) {
    FILE* f = fopen(g_nb.labels, "rb");
    if (!f) { fprintf(stderr, "tfidf: --labels: cannot open %s\n", g_nb.labels); return 2; }
    size_t cap = 1 << 16, n = 0;
    uint8_t* b = (uint8_t*)malloc(cap);
    for (;;) {
        if (!b) { fclose(f); return fail(TFIDF_E_NOMEM); }
        const size_t got = fread(b + n, 1, cap - n, f);
        n += got;
        if (got == 0) break;
        if (n == cap) { cap *= 2; b = (uint8_t*)realloc(b, cap); }
    }
    fclose(f);
    size_t bad = 0;
    const int rc = labels_parse(b, n, &g_nb.lf, &bad);
    free(b);
    if (rc) {
        if (bad) fprintf(stderr, "tfidf: --labels: %s line %zu is not \"doc<N>\\t<name>\"\n", g_nb.labels, bad);
        else fprintf(stderr, "tfidf: --labels: %s holds no line, or more than %u classes\n", g_nb.labels, LABELS_MAX_CLASSES);
        return 2;
    }
    g_nb.p.nclasses = g_nb.lf.k;
    g_nb.p.nlabelled = g_nb.lf.n;
    g_nb.p.doc = g_nb.lf.doc;
    g_nb.p.label = g_nb.lf.label;
    if (tfidf_nb_check(&g_nb.p) != TFIDF_OK) {
        fprintf(stderr, "tfidf: --labels: %s names a document twice, or --nb-alpha is not finite and > 0\n", g_nb.labels);
        return 2;
    }
    return 0;
}

static int u32_cmp(const void* a, const void* b) {
    const uint32_t x = *(const uint32_t*)a, y = *(const uint32_t*)b;
    return x < y ? -1 : (x > y ? 1 : 0);
}

/* --labels: the fit on ctx's documents, then the labels of --classify DIR or of the unlabelled */
static int run_classify(tfidf_ctx* ctx) {
    if (!g_nb.labels) return TFIDF_OK;
    int rc = tfidf_nb_fit(ctx, &g_nb.p);
    if (rc == TFIDF_E_INVAL) fprintf(stderr, "tfidf: --labels: %s names a document that input/ does not hold\n", g_nb.labels);
    if (rc == TFIDF_E_CAPACITY) fprintf(stderr, "tfidf: --labels: the classifier's matrices exceed TFIDF_NB_MB\n");
    if (rc) return rc;
    tfidf_nb_labels out;
    memset(&out, 0, sizeof(out));
    uint32_t* ids = NULL;       /* --classify: the batch's documents in "docN@" order */
    uint32_t* sorted = NULL;    /* --classify-unlabelled: the labelled ids, ascending */
    if (g_nb.dir) {
        tfidf_corpus b;
        memset(&b, 0, sizeof(b));
        uint8_t* bytes = NULL;
        uint64_t* off = NULL;
        uint32_t bad = 0;
        rc = tfidf_ingest_dir(g_nb.dir, &bytes, &b.nbytes, &off, &b.ndocs, &bad);
        if (rc == TFIDF_E_NOINPUT) { printf("Directory failed to open\n"); return TFIDF_OK; }
        if (rc == TFIDF_E_NODOC) { (void)missing_doc(g_nb.dir, bad, b.ndocs); return TFIDF_OK; }
        if (!rc) rc = analyze_host_batch(bytes, b.nbytes, off, b.ndocs);
        if (!rc) rc = ngram_host_batch(&bytes, &b.nbytes, &off, b.ndocs);
        b.bytes = bytes;
        b.doc_off = off;
        tfidf_rows t;
        memset(&t, 0, sizeof(t));
        ids = (uint32_t*)malloc(((size_t)b.ndocs + 1) * sizeof(uint32_t));
        if (!rc) rc = ids ? tfidf_doc_name_order(b.ndocs, ids) : TFIDF_E_NOMEM;
        if (!rc) rc = tfidf_transform(ctx, &b, &t);
        if (!rc) rc = tfidf_nb_predict_rows(ctx, &t, 0, &out);
        tfidf_rows_free(&t);
        tfidf_free(bytes);
        tfidf_free(off);
    } else {
        rc = tfidf_nb_predict(ctx, NULL, 0, 0, &out);
        sorted = (uint32_t*)malloc(((size_t)g_nb.lf.n + 1) * sizeof(uint32_t));
        if (!rc && !sorted) rc = TFIDF_E_NOMEM;
        if (!rc) {
            memcpy(sorted, g_nb.lf.doc, (size_t)g_nb.lf.n * sizeof(uint32_t));
            qsort(sorted, g_nb.lf.n, sizeof(uint32_t), u32_cmp);
        }
    }
    if (!rc) {
        FILE* f = fopen(g_nb.file, "w");
        if (!f) printf("Error Opening File: %s\n", g_nb.file);
        for (uint32_t i = 0; f && i < out.ndocs; ++i) {
            const uint32_t r = ids ? ids[i] - 1 : i;                  /* rows are in batch order, resident ones in "docN@" order */
            const uint32_t id = ids ? ids[i] : out.doc[i];
            if (sorted && bsearch(&id, sorted, g_nb.lf.n, sizeof(uint32_t), u32_cmp)) continue;
            if (out.label[r] >= g_nb.lf.k) continue;
            fprintf(f, "doc%u\t%s\t%.16f\n", id, g_nb.lf.name[out.label[r]], out.score[r]);
        }
        if (f && fclose(f) != 0) rc = TFIDF_E_OUTPUT;
    }
    tfidf_nb_labels_free(&out);
    free(ids);
    free(sorted);
    return rc;
}

/* ------------------------------------------------------------------ model -- */

static struct {
    const char* save;   /* NULL: no model file, behaviour and bytes as without the option */
    const char* load;
} g_model = {NULL, NULL};

/* --save-model: the model of ctx (one shard) or of every rank of g */
static int save_model(tfidf_ctx* ctx, tfidf_group* g) {
    if (!g_model.save) return TFIDF_OK;
    tfidf_model m;
    memset(&m, 0, sizeof(m));
    int rc = g ? tfidf_group_model_export(g, &m) : tfidf_model_export(ctx, &m);
    if (rc) return rc;
    rc = tfidf_model_save(&m, g_model.save);
    tfidf_model_free(&m);
    if (rc == TFIDF_E_OUTPUT) { printf("Error Opening File: %s\n", g_model.save); return TFIDF_OK; }
    return rc;
}

/* ------------------------------------------------------------------ prune -- */

/* --min-df X, --max-df X, --max-features M: the vocabulary is pruned after the run (after every
 * shard's run) and before output.txt and every other file, so all of them see the pruned
 * result.  X is a count, or with a '.' a fraction of N in (0, 1]: ceil(X * N) for --min-df,
 * floor(X * N) for --max-df, in binary64.  Without the options nothing is called. */
static struct {
    int on;
    int min_frac, max_frac;
    double min_x, max_x;
    uint32_t min_df, max_df, max_features;
} g_prune = {0, 0, 0, 0.0, 0.0, 0, 0, 0};

/* X of --min-df / --max-df: 0 on success */
static int parse_df(const char* a, int* frac, double* x, uint32_t* n) {
    char* end = NULL;
    if (strchr(a, '.')) {
        const double v = strtod(a, &end);
        if (end == a || *end || !(v > 0.0) || !(v <= 1.0)) return -1;
        *frac = 1;
        *x = v;
        return 0;
    }
    if (a[0] < '0' || a[0] > '9') return -1;
    const unsigned long long v = strtoull(a, &end, 10);
    if (end == a || *end || v > 0xFFFFFFFFull) return -1;
    *frac = 0;
    *n = (uint32_t)v;
    return 0;
}

/* the parameters for a corpus of N documents; TFIDF_E_INVAL when the fractions give min > max */
static int prune_params_for(uint64_t N, tfidf_prune_params* p) {
    memset(p, 0, sizeof(*p));
    p->size = sizeof(*p);
    p->min_df = g_prune.min_frac ? (uint32_t)ceil(g_prune.min_x * (double)N) : g_prune.min_df;
    p->max_df = g_prune.max_frac ? (uint32_t)floor(g_prune.max_x * (double)N) : g_prune.max_df;
    p->max_features = g_prune.max_features;
    if (g_prune.max_frac && p->max_df == 0) {   /* no df is <= 0: nothing survives (max_df = 0 would mean no bound) */
        p->min_df = 0xFFFFFFFFu;
        return TFIDF_OK;
    }
    return tfidf_prune_check(p);
}

static int prune_bad_range(void) {
    fprintf(stderr, "tfidf: --min-df is above --max-df\n");
    return 2;
}

/* -------------------------------------------------------------- weighting -- */

/* --tf, --idf, --norm, --sublinear-tf: the scores are computed again by the scheme after the run
 * (after every shard's run) and after the pruning options, before output.txt and every other
 * file; under --model after the import, for --transform */
static struct {
    int on;
    tfidf_weighting w;
} g_weight = {0, {sizeof(tfidf_weighting), TFIDF_TF_RATIO, TFIDF_IDF_REF, TFIDF_NORM_NONE, 0}};

/* the index of `s` among n names, or -1 */
static int name_index(const char* s, const char* const* names, int n) {
    for (int i = 0; i < n; ++i)
        if (!strcmp(s, names[i])) return i;
    return -1;
}

/* --model: no run; the file's model is pruned on the host (with the prune options), imported and
 * --transform scored against it */
static int run_model(int device) {
    tfidf_model m;
    int rc = tfidf_model_load(g_model.load, &m);
    if (rc) { fprintf(stderr, "tfidf: %s: %s\n", g_model.load, tfidf_strerror(rc)); return 3; }
    if (g_prune.on) {
        tfidf_prune_params pp;
        tfidf_model pruned;
        if (prune_params_for(m.ndocs_total, &pp) != TFIDF_OK) { tfidf_model_free(&m); return prune_bad_range(); }
        rc = tfidf_model_prune(&m, &pp, &pruned);
        tfidf_model_free(&m);
        if (rc) return fail(rc);
        m = pruned;
    }
    tfidf_ctx* ctx = NULL;
    rc = tfidf_open(device, &ctx);
    if (!rc) rc = tfidf_model_import(ctx, &m);
    tfidf_model_free(&m);   /* the context owns what it needs */
    if (!rc && g_weight.on) rc = tfidf_reweight(ctx, &g_weight.w);   /* the file records no scheme */
    if (!rc) rc = run_transform(ctx, NULL);
    if (!rc) rc = run_suggest(ctx, NULL);   /* the dictionary is all it needs */
    tfidf_close(ctx);
    return rc ? fail(rc) : 0;
}

/* ------------------------------------------------------------- one shard -- */

static int run_single(int device, const char* indir, const char* outpath, int debug, int stats) {
    tfidf_ctx* ctx = NULL;
    int rc = tfidf_open(device, &ctx);
    if (rc) return fail(rc);
    /* input/doc1..N streamed into HBM through pinned segments (TFIDF.c:98-110,130-147) */
    tfidf_corpus c;
    tfidf_ingest_info ii;
    uint32_t bad = 0;
    rc = tfidf_ingest_dir_device(ctx, indir, 0, &c, &bad, &ii);
    if (rc == TFIDF_E_NOINPUT) { printf("Directory failed to open\n"); tfidf_close(ctx); return 1; }
    if (rc == TFIDF_E_NODOC) { tfidf_close(ctx); return missing_doc(indir, bad, c.ndocs); }
    if (rc) { tfidf_close(ctx); return fail(rc); }
    if (c.ndocs == 0) { printf("More workers than input files! Exiting.\n"); tfidf_close(ctx); return 0; }
    if (g_an.on) rc = tfidf_analyze(ctx, &g_an.an, &c, TFIDF_AN_SLOT_CORPUS, &c);   /* in HBM, where the ingest left it */
    if (!rc && g_ng.on) rc = tfidf_ngrams(ctx, &g_ng.p, &c, TFIDF_NG_SLOT_CORPUS, &c);
    if (!rc) rc = tfidf_run(ctx, &c);
    if (!rc && debug) rc = debug_jobs(ctx);
    if (!rc && g_prune.on) {
        tfidf_prune_params pp;
        if (prune_params_for(c.ndocs_total ? c.ndocs_total : c.ndocs, &pp) != TFIDF_OK) { tfidf_close(ctx); return prune_bad_range(); }
        rc = tfidf_prune(ctx, &pp);
    }
    if (!rc && g_weight.on) rc = tfidf_reweight(ctx, &g_weight.w);   /* over the pairs the pruning left */
    if (rc) { tfidf_close(ctx); return fail(rc); }
    tfidf_run_info ri;
    ri.size = sizeof(ri);
    double t_out = 0;
    if (stats) { tfidf_last_run_info(ctx, &ri); t_out = wall_ms(); }
    /* lines formatted on the GPU, copied out through pinned buffers (TFIDF.c:245,274-282) */
    rc = tfidf_write_output_gpu(ctx, outpath, 0);
    if (rc == TFIDF_E_OUTPUT) printf("Error Opening File: %s\n", outpath);
    else if (rc) { tfidf_close(ctx); return fail(rc); }
    if (stats) {
        const double out_ms = wall_ms() - t_out;
        tfidf_output_info oi;
        memset(&oi, 0, sizeof(oi));
        oi.size = sizeof(oi);
        (void)tfidf_last_output_info(ctx, &oi);
        fprintf(stderr,
                "{\"docs\": %u, \"corpus_bytes\": %llu, \"shards\": 1, \"ingest_threads\": %u, \"ingest_scan_ms\": %.3f, "
                "\"ingest_read_h2d_ms\": %.3f, \"ingest_GBps\": %.3f, \"run_device_ms\": %.3f, \"pairs\": %llu, "
                "\"output_ms\": %.3f, \"output_bytes\": %llu, \"output_format_prepare_ms\": %.3f, "
                "\"output_d2h_busy_ms\": %.3f, \"output_write_thread_ms\": %.3f, \"output_writers\": %u}\n",
                ii.ndocs, (unsigned long long)ii.nbytes, ii.threads, ii.ms_scan, ii.ms_read,
                ii.ms_total > 0 ? ii.nbytes / ii.ms_total / 1e6 : 0.0, ri.ms_total, (unsigned long long)ri.npairs,
                out_ms, (unsigned long long)oi.text_bytes, oi.ms_prepare, oi.ms_d2h_busy, oi.ms_write, oi.writers);
    }
    rc = run_queries(ctx, NULL);
    if (!rc) rc = run_suggest(ctx, NULL);
    if (!rc) rc = run_keywords(ctx, NULL);
    if (!rc) rc = run_similar(ctx, NULL);
    if (!rc) rc = run_clusters(ctx);
    if (!rc) rc = run_dups(ctx);
    if (!rc) rc = run_transform(ctx, NULL);
    if (!rc) rc = run_classify(ctx);
    if (!rc) rc = save_model(ctx, NULL);
    tfidf_close(ctx);
    if (rc) return fail(rc);
    return 0;
}

/* ------------------------------------------------------------ K shards -- */

struct shard_job {
    tfidf_group* g;
    const tfidf_dir_plan* plan;
    const char* indir;
    uint32_t shard;
    tfidf_corpus corpus;
    uint32_t bad;
    int rc;
};

static void* ingest_job(void* arg) {
    struct shard_job* j = (struct shard_job*)arg;
    j->bad = 0;
    /* each rank's reader pool gets a share of the host threads */
    const int threads = 4;
    j->rc = tfidf_ingest_shard_device(tfidf_group_ctx(j->g, (int)j->shard), j->indir, j->plan, j->shard, threads,
                                      &j->corpus, &j->bad, NULL);
    if (!j->rc && g_an.on)
        j->rc = tfidf_analyze(tfidf_group_ctx(j->g, (int)j->shard), &g_an.an, &j->corpus, TFIDF_AN_SLOT_CORPUS, &j->corpus);
    if (!j->rc && g_ng.on)
        j->rc = tfidf_ngrams(tfidf_group_ctx(j->g, (int)j->shard), &g_ng.p, &j->corpus, TFIDF_NG_SLOT_CORPUS, &j->corpus);
    return NULL;
}

static int run_sharded(int ngpus, int nshards, const char* indir, const char* outpath, int debug, int stats) {
    const double t0 = wall_ms();
    tfidf_dir_plan plan;
    uint32_t bad = 0;
    int rc = tfidf_plan_dir(indir, (uint32_t)nshards, 0, &plan, &bad);
    if (rc == TFIDF_E_NOINPUT) { printf("Directory failed to open\n"); return 1; }
    if (rc == TFIDF_E_NODOC) return missing_doc(indir, bad, plan.ndocs);
    if (rc) return fail(rc);
    if (plan.ndocs == 0) { printf("More workers than input files! Exiting.\n"); tfidf_plan_free(&plan); return 0; }
    if (plan.ndocs < (uint32_t)nshards) {   /* idle GPUs are simply not used */
        nshards = (int)plan.ndocs;
        tfidf_plan_free(&plan);
        rc = tfidf_plan_dir(indir, (uint32_t)nshards, 0, &plan, &bad);
        if (rc == TFIDF_E_NODOC) return missing_doc(indir, bad, plan.ndocs);
        if (rc) return fail(rc);
    }
    int* dev = (int*)malloc(sizeof(int) * (size_t)nshards);
    struct shard_job* jobs = (struct shard_job*)calloc((size_t)nshards, sizeof(struct shard_job));
    pthread_t* th = (pthread_t*)malloc(sizeof(pthread_t) * (size_t)nshards);
    tfidf_corpus* cs = (tfidf_corpus*)calloc((size_t)nshards, sizeof(tfidf_corpus));
    if (!dev || !jobs || !th || !cs) { tfidf_plan_free(&plan); return fail(TFIDF_E_NOMEM); }
    for (int r = 0; r < nshards; ++r) dev[r] = r % ngpus;
    tfidf_group* g = NULL;
    rc = tfidf_group_open(nshards, dev, 0, &g);
    if (rc) { tfidf_plan_free(&plan); return fail(rc); }
    const double t_open = wall_ms();
    /* every shard streams its documents into its GPU at once */
    for (int r = 0; r < nshards; ++r) {
        jobs[r].g = g;
        jobs[r].plan = &plan;
        jobs[r].indir = indir;
        jobs[r].shard = (uint32_t)r;
        pthread_create(&th[r], NULL, ingest_job, &jobs[r]);
    }
    for (int r = 0; r < nshards; ++r) pthread_join(th[r], NULL);
    uint32_t worst_bad = 0;
    for (int r = 0; r < nshards; ++r) {
        if (jobs[r].rc == TFIDF_E_NODOC && (worst_bad == 0 || jobs[r].bad < worst_bad)) worst_bad = jobs[r].bad;
        else if (jobs[r].rc && !rc) rc = jobs[r].rc;
        cs[r] = jobs[r].corpus;
    }
    if (worst_bad) {
        const uint32_t n = plan.ndocs;
        tfidf_group_close(g);
        tfidf_plan_free(&plan);
        return missing_doc(indir, worst_bad, n);
    }
    const double t_ingest = wall_ms();
    if (!rc) rc = tfidf_group_run(g, cs);
    for (int r = 0; r < nshards && !rc && debug; ++r) rc = debug_jobs(tfidf_group_ctx(g, r));
    if (!rc && g_prune.on) {
        tfidf_prune_params pp;
        if (prune_params_for(plan.ndocs, &pp) != TFIDF_OK) { tfidf_group_close(g); tfidf_plan_free(&plan); return prune_bad_range(); }
        rc = tfidf_group_prune(g, &pp);
    }
    if (!rc && g_weight.on) rc = tfidf_group_reweight(g, &g_weight.w);
    if (rc) { tfidf_group_close(g); tfidf_plan_free(&plan); return fail(rc); }
    const double t_run = wall_ms();
    /* each GPU formats its shard; the texts are written in shard order (TFIDF.c:253-282) */
    rc = tfidf_group_write_output(g, outpath);
    if (rc == TFIDF_E_OUTPUT) printf("Error Opening File: %s\n", outpath);
    else if (rc) { tfidf_group_close(g); tfidf_plan_free(&plan); return fail(rc); }
    if (stats) {
        uint64_t pairs = 0, bytes = 0;
        for (int r = 0; r < nshards; ++r) {
            tfidf_run_info ri;
            ri.size = sizeof(ri);
            if (tfidf_last_run_info(tfidf_group_ctx(g, r), &ri) == 0) pairs += ri.npairs;
            bytes += plan.shard_bytes[r];
        }
        fprintf(stderr,
                "{\"docs\": %u, \"corpus_bytes\": %llu, \"shards\": %d, \"gpus\": %d, \"plan_open_ms\": %.3f, "
                "\"ingest_ms\": %.3f, \"run_ms\": %.3f, \"pairs\": %llu, \"output_ms\": %.3f}\n",
                plan.ndocs, (unsigned long long)bytes, nshards, ngpus, t_open - t0, t_ingest - t_open, t_run - t_ingest,
                (unsigned long long)pairs, wall_ms() - t_run);
    }
    rc = run_queries(NULL, g);
    if (!rc) rc = run_suggest(NULL, g);
    if (!rc) rc = run_keywords(NULL, g);
    if (!rc) rc = run_similar(NULL, g);
    if (!rc) rc = run_transform(NULL, g);
    if (!rc) rc = save_model(NULL, g);
    tfidf_group_close(g);
    tfidf_plan_free(&plan);
    if (rc) return fail(rc);
    free(dev);
    free(jobs);
    free(th);
    free(cs);
    return 0;
}

static int usage(void) {
    fprintf(stderr, "usage: tfidf [--debug-jobs] [--stats] [--gpus N] [--shards K] [--device D] "
                    "[--input DIR] [--output FILE] [--query FILE [--top K] [--hits FILE] [--bm25 [--bm25-k1 X] [--bm25-b Y]] [--query-ops] [--query-all] [--min-match M] "
                    "[--fuzzy D|auto] [--prefix-ops] [--fuzzy-no-transpose] [--fuzzy-prefix P] [--max-expansions E]] "
                    "[--suggest FILE [--suggest-file FILE]] "
                    "[--snippets W [--snippet-marks M] [--snippets-file FILE]] "
                    "[--keywords K [--keywords-file FILE]] "
                    "[--similar K [--similar-docs FILE] [--similar-file FILE]] "
                    "[--clusters K [--clusters-iter I] [--clusters-seeds FILE] [--clusters-terms T] [--clusters-file FILE]] "
                    "[--near-dups T [--near-dups-hashes H] [--near-dups-rows R] [--near-dups-seed S] [--near-dups-file FILE]] "
                    "[--transform DIR [--transform-file FILE]] [--save-model FILE] "
                    "[--labels FILE (--classify DIR | --classify-unlabelled) [--classify-file FILE] [--nb-alpha X] "
                    "[--nb-complement] [--nb-binary] [--nb-uniform-prior]] "
                    "[--min-df X] [--max-df X] [--max-features M] "
                    "[--tf ratio|raw|log|binary] [--sublinear-tf] [--idf ref|smooth|plus1|none] [--norm none|l1|l2] "
                    "[--lower] [--strip-punct] [--min-token N] [--stopwords FILE] [--stem] [--utf8] [--ngrams SPEC [--ngram-joiner C]]\n"
                    "       tfidf --model FILE --suggest FILE (--fuzzy D|auto | --prefix-ops) [--suggest-file FILE] [--device D]\n"
                    "       tfidf --model FILE --transform DIR [--transform-file FILE] [--device D] [--min-df X] [--max-df X] [--max-features M] "
                    "[--tf T] [--sublinear-tf] [--idf I] [--norm L] "
                    "[--lower] [--strip-punct] [--min-token N] [--stopwords FILE] [--stem] [--utf8] [--ngrams SPEC [--ngram-joiner C]]\n"
                    "  --similar K without --similar-docs searches for every document: "
                    "ceil(N / group) scans of the scored pairs, group <= 64\n"
                    "  --save-model FILE writes the run's term table, df and N; --model FILE scores "
                    "--transform DIR against such a file without input/ or output.txt\n"
                    "  --lower, --strip-punct, --min-token N, --stopwords FILE and --stem analyze input/, the "
                    "query lines and the --transform documents before they are counted; the model file does "
                    "not record them\n"
                    "  --stem replaces tokens of 3..64 lower-case ASCII letters by their Porter stems; it does "
                    "not imply --lower, and the words of --stopwords FILE are not stemmed\n"
                    "  --utf8 extends --lower and --strip-punct to UTF-8 sequences: cased letters whose lowercase "
                    "has the same length are folded, punctuation, symbols and separators are blanked\n"
                    "  --min-df X and --max-df X drop the words in fewer than / more than X documents before anything "
                    "is written (X with a '.': a fraction of N in (0, 1]); --max-features M keeps the M words in the most "
                    "documents (ties by word order; one shard only); scores and docSize are unchanged, and a model "
                    "saved after pruning needs no option when it is served\n"
                    "  --tf, --idf and --norm replace the reference's count / docSize * ln(N / df) after the run and the "
                    "pruning: --tf log (= --sublinear-tf) is 1 + ln(count), --idf smooth is ln((N + 1) / (df + 1)) + 1, "
                    "--idf plus1 is ln(N / df) + 1, --norm l1|l2 divides a document's scores by their sum or by the root of "
                    "the sum of their squares; --tf raw needs a norm; the model file does not record them; not with "
                    "--debug-jobs\n"
                    "  --fuzzy D|auto replaces every token of a --query line by the words of the dictionary within D byte edits "
                    "(auto: 0 up to 2 bytes, 1 up to 5, else 2; an adjacent transposition is one edit unless --fuzzy-no-transpose; "
                    "--fuzzy-prefix P bytes must match exactly), the best --max-expansions E (default 50) by distance, then df; "
                    "--prefix-ops reads a token ending in '*' as a prefix; --suggest FILE writes the matches of FILE's tokens "
                    "instead of ranking with them, also from --model FILE\n"
                    "  --snippets W writes the best passage of W tokens of every hit of --query to snippets.txt, the matched words "
                    "in [ ] (at most --snippet-marks M); not with --ngrams or --model\n"
                    "  --ngrams SPEC adds word n-grams behind the analyzer: SPEC is N (= 1-N) or A-B with 1 <= A <= B <= 8; "
                    "the words of a gram are joined by '_' or by the byte of --ngram-joiner C\n");
    return 2;
}

int main(int argc, char** argv) {
    int debug = 0, stats = 0, device = -1, ngpus = 0, nshards = 0;
    const char* indir = "input";
    const char* outpath = "output.txt";
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--debug-jobs")) debug = 1;
        else if (!strcmp(argv[i], "--stats")) stats = 1;
        else if (!strcmp(argv[i], "--device") && i + 1 < argc) device = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--gpus") && i + 1 < argc) ngpus = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--shards") && i + 1 < argc) nshards = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--input") && i + 1 < argc) indir = argv[++i];
        else if (!strcmp(argv[i], "--output") && i + 1 < argc) outpath = argv[++i];
        else if (!strcmp(argv[i], "--query") && i + 1 < argc) g_query.file = argv[++i];
        else if (!strcmp(argv[i], "--hits") && i + 1 < argc) g_query.hits = argv[++i];
        else if (!strcmp(argv[i], "--top") && i + 1 < argc) {
            const long k = atol(argv[++i]);
            if (k < 1 || k > (long)TFIDF_QUERY_MAX_K) { fprintf(stderr, "tfidf: --top takes 1..%u\n", TFIDF_QUERY_MAX_K); return 2; }
            g_query.top = (uint32_t)k;
        }
        else if (!strcmp(argv[i], "--bm25")) g_query.bm25 = 1;
        else if (!strcmp(argv[i], "--query-ops")) g_query.ops = 1;
        else if (!strcmp(argv[i], "--fuzzy") && i + 1 < argc) {
            const char* v = argv[++i];
            if (!strcmp(v, "auto")) g_expand.fuzzy = QEXP_AUTO;
            else if (v[0] >= '0' && v[0] <= '2' && !v[1]) g_expand.fuzzy = v[0] - '0';
            else { fprintf(stderr, "tfidf: --fuzzy takes 0..%u or auto\n", TFIDF_MATCH_MAX_EDITS); return 2; }
        }
        else if (!strcmp(argv[i], "--prefix-ops")) g_expand.prefix_ops = 1;
        else if (!strcmp(argv[i], "--fuzzy-no-transpose")) { g_expand.no_transpose = 1; g_expand.opts = 1; }
        else if (!strcmp(argv[i], "--fuzzy-prefix") && i + 1 < argc) {
            const long v = atol(argv[++i]);
            if (v < 0 || v > (long)TFIDF_MATCH_MAX_PATTERN) { fprintf(stderr, "tfidf: --fuzzy-prefix takes 0..%u\n", TFIDF_MATCH_MAX_PATTERN); return 2; }
            g_expand.fixed_prefix = (uint32_t)v;
            g_expand.opts = 1;
        }
        else if (!strcmp(argv[i], "--max-expansions") && i + 1 < argc) {
            const long v = atol(argv[++i]);
            if (v < 1 || v > (long)TFIDF_MATCH_MAX_EXPANSIONS) { fprintf(stderr, "tfidf: --max-expansions takes 1..%u\n", TFIDF_MATCH_MAX_EXPANSIONS); return 2; }
            g_expand.max_expansions = (uint32_t)v;
            g_expand.opts = 1;
        }
        else if (!strcmp(argv[i], "--suggest") && i + 1 < argc) g_expand.suggest = argv[++i];
        else if (!strcmp(argv[i], "--suggest-file") && i + 1 < argc) g_expand.suggest_file = argv[++i];
        else if (!strcmp(argv[i], "--query-all")) g_query.all = 1;
        else if (!strcmp(argv[i], "--snippets") && i + 1 < argc) {
            g_snip.window = atoi(argv[++i]);
            if (g_snip.window < 1 || g_snip.window > (int)TFIDF_SNIP_MAX_WINDOW) return usage();
        } else if (!strcmp(argv[i], "--snippet-marks") && i + 1 < argc) {
            g_snip.marks = atoi(argv[i + 1]);
            if (g_snip.marks < 0 || g_snip.marks > (int)TFIDF_SNIP_MAX_MARKS || (g_snip.marks == 0 && strcmp(argv[i + 1], "0"))) return usage();
            ++i;
        } else if (!strcmp(argv[i], "--snippets-file") && i + 1 < argc) g_snip.file = argv[++i];
        else if (!strcmp(argv[i], "--min-match") && i + 1 < argc) {
            char* end = NULL;
            const char* a = argv[++i];
            const long m = strtol(a, &end, 10);
            if (a[0] < '0' || a[0] > '9' || *end || m > (long)TFIDF_CLAUSE_MAX_TERMS) {
                fprintf(stderr, "tfidf: --min-match takes 0..%u\n", TFIDF_CLAUSE_MAX_TERMS);
                return 2;
            }
            g_query.min_match = m;
        }
        else if ((!strcmp(argv[i], "--bm25-k1") || !strcmp(argv[i], "--bm25-b")) && i + 1 < argc) {
            const int is_b = !strcmp(argv[i], "--bm25-b");
            char* end = NULL;
            const double v = strtod(argv[++i], &end);
            if (end == argv[i] || *end || !(v >= 0.0) || !(is_b ? v <= 1.0 : v <= TFIDF_BM25_MAX_K1)) {
                fprintf(stderr, "tfidf: --bm25-k1 takes a number >= 0, --bm25-b one in 0..1\n");
                return 2;
            }
            if (is_b) g_query.b = v; else g_query.k1 = v;
            g_query.bm25 = 1;   /* a BM25 parameter asks for BM25 */
        }
        else if (!strcmp(argv[i], "--keywords-file") && i + 1 < argc) g_keywords.file = argv[++i];
        else if (!strcmp(argv[i], "--keywords") && i + 1 < argc) {
            const long k = atol(argv[++i]);
            if (k < 1 || k > (long)TFIDF_TERMS_MAX_K) { fprintf(stderr, "tfidf: --keywords takes 1..%u\n", TFIDF_TERMS_MAX_K); return 2; }
            g_keywords.k = (uint32_t)k;
        }
        else if (!strcmp(argv[i], "--lower")) { g_an.an.flags |= TFIDF_AN_LOWER; g_an.on = 1; }
        else if (!strcmp(argv[i], "--strip-punct")) { g_an.an.flags |= TFIDF_AN_PUNCT; g_an.on = 1; }
        else if (!strcmp(argv[i], "--stem")) { g_an.an.stemmer = TFIDF_STEM_PORTER; g_an.on = 1; }
        else if (!strcmp(argv[i], "--utf8")) { g_an.an.flags |= TFIDF_AN_UTF8; g_an.on = 1; }
        else if (!strcmp(argv[i], "--stopwords") && i + 1 < argc) { g_an.stopfile = argv[++i]; g_an.on = 1; }
        else if (!strcmp(argv[i], "--min-token") && i + 1 < argc) {
            const long v = atol(argv[++i]);
            if (v < 0 || v > (long)TFIDF_AN_MAX_WORD) { fprintf(stderr, "tfidf: --min-token takes 0..%u\n", TFIDF_AN_MAX_WORD); return 2; }
            g_an.an.min_len = (uint32_t)v;
            g_an.on = 1;
        }
        else if (!strcmp(argv[i], "--ngrams") && i + 1 < argc) {
            if (parse_ngram_spec(argv[++i]) != TFIDF_OK) return usage();
        }
        else if (!strcmp(argv[i], "--ngram-joiner") && i + 1 < argc) {
            const char* c = argv[++i];
            if (strlen(c) != 1) return usage();
            g_ng.p.joiner = (uint8_t)c[0];
        }
        else if (!strcmp(argv[i], "--transform-file") && i + 1 < argc) g_transform.file = argv[++i];
        else if (!strcmp(argv[i], "--transform") && i + 1 < argc) g_transform.dir = argv[++i];
        else if (!strcmp(argv[i], "--save-model") && i + 1 < argc) g_model.save = argv[++i];
        else if (!strcmp(argv[i], "--model") && i + 1 < argc) g_model.load = argv[++i];
        else if (!strcmp(argv[i], "--labels") && i + 1 < argc) g_nb.labels = argv[++i];
        else if (!strcmp(argv[i], "--classify-file") && i + 1 < argc) g_nb.file = argv[++i];
        else if (!strcmp(argv[i], "--classify-unlabelled")) g_nb.unlabelled = 1;
        else if (!strcmp(argv[i], "--classify") && i + 1 < argc) g_nb.dir = argv[++i];
        else if (!strcmp(argv[i], "--nb-complement")) { g_nb.p.variant = TFIDF_NB_COMPLEMENT; g_nb.opts = 1; }
        else if (!strcmp(argv[i], "--nb-binary")) { g_nb.p.feature = TFIDF_NB_BINARY; g_nb.opts = 1; }
        else if (!strcmp(argv[i], "--nb-uniform-prior")) { g_nb.p.uniform_prior = 1; g_nb.opts = 1; }
        else if (!strcmp(argv[i], "--nb-alpha") && i + 1 < argc) {
            char* end = NULL;
            const double v = strtod(argv[++i], &end);
            if (!end || *end || end == argv[i] || !(v > 0.0 && v <= TFIDF_NB_MAX_ALPHA)) { fprintf(stderr, "tfidf: --nb-alpha takes a finite number above 0\n"); return 2; }
            g_nb.p.alpha = v;
            g_nb.opts = 1;
        }
        else if (!strcmp(argv[i], "--near-dups-file") && i + 1 < argc) g_dups.file = argv[++i];
        else if (!strcmp(argv[i], "--near-dups-hashes") && i + 1 < argc) {
            char* end = NULL;
            const long v = strtol(argv[++i], &end, 10);
            if (!end || *end || v < 1 || v > (long)TFIDF_MINHASH_MAX_H) { fprintf(stderr, "tfidf: --near-dups-hashes takes 1..%u\n", TFIDF_MINHASH_MAX_H); return 2; }
            g_dups.hashes = (uint32_t)v;
        }
        else if (!strcmp(argv[i], "--near-dups-rows") && i + 1 < argc) {
            char* end = NULL;
            const long v = strtol(argv[++i], &end, 10);
            if (!end || *end || v < 1 || v > (long)TFIDF_MINHASH_MAX_H) { fprintf(stderr, "tfidf: --near-dups-rows takes 1..%u\n", TFIDF_MINHASH_MAX_H); return 2; }
            g_dups.rows = (uint32_t)v;
        }
        else if (!strcmp(argv[i], "--near-dups-seed") && i + 1 < argc) {
            char* end = NULL;
            g_dups.seed = strtoull(argv[++i], &end, 0);
            if (!end || *end) { fprintf(stderr, "tfidf: --near-dups-seed takes an unsigned integer\n"); return 2; }
        }
        else if (!strcmp(argv[i], "--near-dups") && i + 1 < argc) {
            char* end = NULL;
            const double v = strtod(argv[++i], &end);
            if (!end || *end || end == argv[i] || !(v >= 0.0 && v <= 1.0)) { fprintf(stderr, "tfidf: --near-dups takes a threshold in 0..1\n"); return 2; }
            g_dups.threshold = v;
            g_dups.on = 1;
        }
        else if (!strcmp(argv[i], "--clusters-seeds") && i + 1 < argc) g_clusters.seeds = argv[++i];
        else if (!strcmp(argv[i], "--clusters-file") && i + 1 < argc) g_clusters.file = argv[++i];
        else if (!strcmp(argv[i], "--clusters-iter") && i + 1 < argc) {
            const long v = atol(argv[++i]);
            if (v < 1 || v > 1000000L) { fprintf(stderr, "tfidf: --clusters-iter takes 1..1000000\n"); return 2; }
            g_clusters.iter = (uint32_t)v;
        }
        else if (!strcmp(argv[i], "--clusters-terms") && i + 1 < argc) {
            const long v = atol(argv[++i]);
            if (v < 0 || v > (long)TFIDF_KMEANS_MAX_TERMS) { fprintf(stderr, "tfidf: --clusters-terms takes 0..%u\n", TFIDF_KMEANS_MAX_TERMS); return 2; }
            g_clusters.terms = (uint32_t)v;
        }
        else if (!strcmp(argv[i], "--clusters") && i + 1 < argc) {
            const long k = atol(argv[++i]);
            if (k < 1 || k > (long)TFIDF_KMEANS_MAX_K) { fprintf(stderr, "tfidf: --clusters takes 1..%u\n", TFIDF_KMEANS_MAX_K); return 2; }
            g_clusters.k = (uint32_t)k;
        }
        else if ((!strcmp(argv[i], "--min-df") || !strcmp(argv[i], "--max-df")) && i + 1 < argc) {
            const int is_max = !strcmp(argv[i], "--max-df");
            if (parse_df(argv[++i], is_max ? &g_prune.max_frac : &g_prune.min_frac, is_max ? &g_prune.max_x : &g_prune.min_x,
                         is_max ? &g_prune.max_df : &g_prune.min_df) != 0) {
                fprintf(stderr, "tfidf: --min-df and --max-df take a count, or with a '.' a fraction of N in (0, 1]\n");
                return 2;
            }
            g_prune.on = 1;
        }
        else if (!strcmp(argv[i], "--max-features") && i + 1 < argc) {
            const long long v = atoll(argv[++i]);
            if (v < 1 || v > 0xFFFFFFFFll) { fprintf(stderr, "tfidf: --max-features takes 1..4294967295\n"); return 2; }
            g_prune.max_features = (uint32_t)v;
            g_prune.on = 1;
        }
        else if (!strcmp(argv[i], "--sublinear-tf")) { g_weight.w.tf = TFIDF_TF_LOG; g_weight.on = 1; }
        else if ((!strcmp(argv[i], "--tf") || !strcmp(argv[i], "--idf") || !strcmp(argv[i], "--norm")) && i + 1 < argc) {
            static const char* const tf_names[] = {"ratio", "raw", "log", "binary"};       /* TFIDF_TF_* */
            static const char* const idf_names[] = {"ref", "smooth", "plus1", "none"};     /* TFIDF_IDF_* */
            static const char* const norm_names[] = {"none", "l2", "l1"};                  /* TFIDF_NORM_* */
            const char* opt = argv[i];
            const int v = !strcmp(opt, "--tf") ? name_index(argv[++i], tf_names, 4)
                          : !strcmp(opt, "--idf") ? name_index(argv[++i], idf_names, 4) : name_index(argv[++i], norm_names, 3);
            if (v < 0) {
                fprintf(stderr, "tfidf: --tf takes ratio|raw|log|binary, --idf ref|smooth|plus1|none, --norm none|l1|l2\n");
                return 2;
            }
            if (!strcmp(opt, "--tf")) g_weight.w.tf = (uint32_t)v;
            else if (!strcmp(opt, "--idf")) g_weight.w.idf = (uint32_t)v;
            else g_weight.w.norm = (uint32_t)v;
            g_weight.on = 1;
        }
        else if (!strcmp(argv[i], "--similar-docs") && i + 1 < argc) g_similar.docs = argv[++i];
        else if (!strcmp(argv[i], "--similar-file") && i + 1 < argc) g_similar.file = argv[++i];
        else if (!strcmp(argv[i], "--similar") && i + 1 < argc) {
            const long k = atol(argv[++i]);
            if (k < 1 || k > (long)TFIDF_SIMILAR_MAX_K) { fprintf(stderr, "tfidf: --similar takes 1..%u\n", TFIDF_SIMILAR_MAX_K); return 2; }
            g_similar.k = (uint32_t)k;
        }
        else {
            return usage();
        }
    }
    if (g_an.on && load_stopwords() != TFIDF_OK) return 2;
    if (g_ng.on ? tfidf_ngram_check(&g_ng.p) != TFIDF_OK : g_ng.p.joiner != 0) return usage();   /* a separator as joiner; a joiner alone */
    if (g_prune.on && !g_prune.min_frac && !g_prune.max_frac && g_prune.max_df != 0 && g_prune.min_df > g_prune.max_df)
        return prune_bad_range();
    if (g_weight.on) {
        if (tfidf_weighting_check(&g_weight.w) != TFIDF_OK) {
            fprintf(stderr, "tfidf: --tf raw needs --norm l1 or --norm l2: a raw count times an idf has no bound\n");
            return 2;
        }
        if (debug) {
            fprintf(stderr, "tfidf: --tf, --idf, --norm and --sublinear-tf cannot be combined with --debug-jobs: its blocks are "
                            "the reference's\n");
            return 2;
        }
    }
    if (g_dups.on && g_dups.hashes % g_dups.rows != 0u) {
        fprintf(stderr, "tfidf: --near-dups-rows must divide --near-dups-hashes (%u)\n", g_dups.hashes);
        return 2;
    }
    if (!g_nb.labels ? (g_nb.dir || g_nb.unlabelled || g_nb.opts) : ((g_nb.dir != NULL) + g_nb.unlabelled != 1)) {
        fprintf(stderr, "tfidf: --labels FILE goes with exactly one of --classify DIR and --classify-unlabelled, and these and the "
                        "--nb-* options need --labels FILE\n");
        return 2;
    }
    /* asked of the options as given, before the device count: --gpus / --shards above 1 */
    if (g_nb.labels && (nshards > 1 || (nshards <= 0 && ngpus > 1 && device < 0))) {
        fprintf(stderr, "tfidf: --labels runs on one shard only: the shards' term tables differ, so they share no "
                        "weight matrix (drop --gpus / --shards)\n");
        return 2;
    }
    if (g_nb.labels && !g_model.load) {
        const int bad = load_labels();
        if (bad) return bad;
    }
    {   /* term expansion: what it needs and what it does not go with, before anything touches the GPU */
        const int expanding = g_expand.fuzzy != QEXP_OFF || g_expand.prefix_ops;
        if (g_expand.suggest && !expanding) {
            fprintf(stderr, "tfidf: --suggest FILE needs --fuzzy D|auto or --prefix-ops\n");
            return 2;
        }
        if (expanding && !g_query.file && !g_expand.suggest) {
            fprintf(stderr, "tfidf: --fuzzy and --prefix-ops need --query FILE or --suggest FILE\n");
            return 2;
        }
        if (g_expand.opts && !expanding) {
            fprintf(stderr, "tfidf: --fuzzy-no-transpose, --fuzzy-prefix and --max-expansions need --fuzzy D|auto or --prefix-ops\n");
            return 2;
        }
        if (expanding && (g_query.ops || g_query.all || g_query.min_match >= 0)) {
            fprintf(stderr, "tfidf: --fuzzy and --prefix-ops cannot be combined with --query-ops, --query-all or --min-match: a required "
                            "token with several expansions needs an any-of group in the clauses\n");
            return 2;
        }
    }
    if (g_model.load) {   /* a model holds no pairs: nothing to rank, list or print */
        if (g_snip.window) {
            fprintf(stderr, "tfidf: --snippets cannot be combined with --model: a model holds no corpus\n");
            return 2;
        }
        if (!g_transform.dir && !g_expand.suggest) {
            fprintf(stderr, "tfidf: --model needs --transform DIR\n");
            return 2;
        }
        if (g_query.file || g_keywords.k || g_similar.k || g_clusters.k || g_dups.on || g_nb.labels || g_model.save || debug) {
            fprintf(stderr, "tfidf: --model cannot be combined with --query, --keywords, --similar, --clusters, --near-dups, --labels, --save-model or "
                            "--debug-jobs: they need a run's pairs\n");
            return 2;
        }
        if (tfidf_device_count() <= 0) return fail(TFIDF_E_NODEV);
        return run_model(device >= 0 ? device : 0);
    }
    if (g_snip.window && (!g_query.file || g_ng.on)) {
        fprintf(stderr, g_ng.on ? "tfidf: --snippets cannot be combined with --ngrams: a gram is no passage of the text\n"
                                : "tfidf: --snippets W needs --query FILE\n");
        return 2;
    }
    if (g_query.bm25 && !g_query.file) {   /* nothing to rank: say so instead of ignoring the switch */
        fprintf(stderr, "tfidf: --bm25, --bm25-k1 and --bm25-b need --query FILE\n");
        return 2;
    }
    if ((g_query.ops || g_query.all || g_query.min_match >= 0) && !g_query.file) {
        fprintf(stderr, "tfidf: --query-ops, --query-all and --min-match need --query FILE\n");
        return 2;
    }
    /* TFIDF.c:100-103 before anything touches the GPU */
    DIR* d = opendir(indir);
    if (!d) { printf("Directory failed to open\n"); return 1; }
    closedir(d);
    const int visible = tfidf_device_count();
    if (visible <= 0) return fail(TFIDF_E_NODEV);
    if (device >= 0) ngpus = 1;                 /* --device D: one GPU, that one */
    /* default: ONE GPU.  Several GPUs (an RCCL clique over xGMI) only when asked for with
     * --gpus N: the multi-GPU path is validated on the driver's 8-GPU node, not here */
    if (ngpus <= 0) ngpus = 1;
    if (ngpus > visible) ngpus = visible;
    if (nshards <= 0) nshards = ngpus;
    if (g_clusters.k && nshards != 1) {
        fprintf(stderr, "tfidf: --clusters runs on one shard only: the shards' term tables differ, so they share no "
                        "centroid matrix (drop --gpus / --shards)\n");
        return 2;
    }
    if (g_dups.on && nshards != 1) {
        fprintf(stderr, "tfidf: --near-dups runs on one shard only: a document's candidates are sought among the shard's "
                        "own documents (drop --gpus / --shards)\n");
        return 2;
    }
    if (g_prune.max_features && nshards != 1) {
        fprintf(stderr, "tfidf: --max-features runs on one shard only: the shards' term tables differ, so they share no "
                        "ranking of the words (drop --gpus / --shards; --min-df and --max-df work on any number)\n");
        return 2;
    }
    if (nshards == 1) return run_single(device >= 0 ? device : 0, indir, outpath, debug, stats);
    if (device > 0) return fail(TFIDF_E_INVAL);   /* several shards use devices 0..N-1 */
    return run_sharded(ngpus, nshards, indir, outpath, debug, stats);
}
