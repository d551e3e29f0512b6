/*
 * prune.hip — vocabulary pruning by document frequency over the resident result of a run
 * (include/tfidf.h: tfidf_prune).  The reference keeps every word (TFIDF.c:152-188); here the
 * terms outside [min_df, max_df], or behind the max_features cut, leave the term table and
 * their pairs leave the output arrays, and every number that stays keeps its bits.  Integers
 * only, no floating-point operation (scores are moved as 8-byte words) and no atomic on a
 * result; every kernel follows the count -> scan -> write form of transform.hip's bounds.
 *
 *   select   one lane per term rank: the range test on the run's global df -> flag.  With
 *            max_features the caller sorts (Nt - df, rank) with the stable LSD radix sort, so
 *            equal df keep ascending rank, and the first M positions that passed the range test
 *            are flagged instead.  The flags become a bitmap (one ballot per wave) and, by an
 *            exclusive scan, the new ranks.
 *   terms    one lane per old rank: a kept rank scatters slot_of_rank and df to its new rank.
 *            rank_of_slot is rewritten in place by the last launch of the call (the new rank,
 *            or QUERY_NO_TERM: the key keeps its slot and stops resolving).
 *   pairs    tiles of PR_TILE pairs, one 16-byte load of out_term per lane.  The keep bits come
 *            from the bitmap, staged in LDS up to PR_LDS_TERMS terms and read through L2 beyond.
 *            count: kept pairs per tile; the caller scans them; write: a block scan of the
 *            lanes' counts gives every kept pair its compacted position, where new_rank[term],
 *            count and score go.  The lanes' prefixes and 4-bit masks stay in LDS for the
 *            documents whose offset lies in the tile: new_off[j] = the kept pairs before
 *            out_off[j], one lane per such document (found per tile by a binary search).
 *
 * Form kept: pair-major tiles, not the document-major waves of docscan.h.  A tile reads whole
 * aligned 16-byte groups whatever the documents' lengths, the per-tile counts make the result
 * independent of the grid, and the documents enter only through their offsets.  The
 * document-major form was not measured.
 */
#include "kernels.h"
#include "dev_common.h"

namespace {

constexpr int NT = 256;
static_assert(PR_TILE == NT * 4, "four pairs per lane");
static_assert(PR_LDS_TERMS % 32 == 0, "whole bitmap words");
inline unsigned grid_for(uint64_t n) { return n ? (unsigned)((n + NT - 1) / NT) : 1u; }
int ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

/* ------------------------------------------------------------------ select -- */

__global__ __launch_bounds__(NT) void k_pr_range(const uint32_t* __restrict__ df, uint32_t V, uint64_t Nt,
                                                 uint32_t min_df, uint32_t max_df, uint32_t* __restrict__ flag,
                                                 uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    const uint64_t r = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (r >= V) return;
    const uint32_t d = df[r];
    const bool in = (min_df <= 1u || d >= min_df) && (max_df == 0u || d <= max_df);
    flag[r] = in ? 1u : 0u;
    if (key) {
        key[r] = in && (uint64_t)d <= Nt ? Nt - (uint64_t)d : PR_KEY_DEAD;
        val[r] = (uint32_t)r;
    }
}

__global__ __launch_bounds__(NT) void k_pr_take(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                uint32_t V, uint32_t M, uint32_t* __restrict__ flag) {
    const uint64_t p = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (p >= V) return;
    const uint32_t r = val[p];
    if (r < V) flag[r] = (p < M && key[p] != PR_KEY_DEAD) ? 1u : 0u;
}

__global__ __launch_bounds__(NT) void k_pr_bitmap(const uint32_t* __restrict__ flag, uint32_t V,
                                                  uint32_t* __restrict__ bits) {
    const uint64_t r = (uint64_t)blockIdx.x * NT + threadIdx.x;   /* every wave is whole: the grid covers ceil(V / 64) * 64 */
    const bool f = r < V && flag[r] != 0u;
    const uint64_t b = __ballot(f);
    if ((threadIdx.x & 63u) == 0u && r < (((uint64_t)V + 63u) & ~63ull)) {
        bits[r >> 5] = (uint32_t)b;
        bits[(r >> 5) + 1u] = (uint32_t)(b >> 32);
    }
}

/* ------------------------------------------------------------------- terms -- */

__device__ __forceinline__ bool pr_bit(const uint32_t* bits, uint32_t t) { return (gload(bits + (t >> 5)) >> (t & 31u)) & 1u; }

__global__ __launch_bounds__(NT) void k_pr_terms(const PrTerms a) {
    const uint64_t r = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (r >= a.V || !pr_bit(a.bits, (uint32_t)r)) return;
    const uint32_t nr = a.new_rank[r];
    if (nr > r) return;   /* a new rank never exceeds the old one */
    a.new_slot_of_rank[nr] = a.slot_of_rank[r];
    a.new_df[nr] = a.df[r];
}

__global__ __launch_bounds__(NT) void k_pr_slots(const PrTerms a, uint32_t* __restrict__ rank_of_slot, uint64_t slot_cap) {
    const uint64_t r = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (r >= a.V) return;
    const uint32_t slot = a.slot_of_rank[r];
    if (slot >= slot_cap) return;
    rank_of_slot[slot] = pr_bit(a.bits, (uint32_t)r) ? a.new_rank[r] : QUERY_NO_TERM;
}

/* ------------------------------------------------------------------- pairs -- */

__global__ __launch_bounds__(NT) void k_pr_tiledoc(const PrPairs a) {
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (t > a.ntiles) return;
    const uint64_t target = t * PR_TILE;
    uint64_t lo = 0, hi = (uint64_t)a.ndocs + 1u;   /* the first j in [0, ndocs] whose offset is >= target */
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        uint64_t v = a.out_off[mid];
        if (v > a.npairs) v = a.npairs;
        if (v < target) lo = mid + 1u;
        else hi = mid;
    }
    a.tile_doc[t] = (uint32_t)lo;
}

template <bool WRITE, bool LDSMAP>
__global__ __launch_bounds__(NT) void k_pr_pairs(const PrPairs a) {
    __shared__ uint32_t s_bits[LDSMAP ? PR_LDS_TERMS / 32 : 1];
    __shared__ uint32_t s_pref[NT], s_mask[NT];
    __shared__ uint32_t wsum[NT / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t P = a.npairs;
    if (LDSMAP) {
        const uint32_t words = (a.V + 31u) >> 5;   /* <= PR_LDS_TERMS / 32: the launcher's choice */
        for (uint32_t w = tid; w < words; w += NT) s_bits[w] = gload(a.bits + w);
        __syncthreads();
    }
    for (uint64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const uint64_t i = tile * PR_TILE + (uint64_t)tid * 4u;
        uint32_t t[4] = {QUERY_NO_TERM, QUERY_NO_TERM, QUERY_NO_TERM, QUERY_NO_TERM};
        const bool whole = i + 4u <= P;
        if (whole) {
            const uint4 v = gload((const uint4*)(a.out_term + i));   /* i is a multiple of 4: aligned */
            t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k)
                if (i + k < P) t[k] = gload(a.out_term + i + k);
        }
        uint32_t m = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            bool keep = false;
            if (t[k] < a.V) keep = LDSMAP ? ((s_bits[t[k] >> 5] >> (t[k] & 31u)) & 1u) != 0u : pr_bit(a.bits, t[k]);
            m |= (keep ? 1u : 0u) << k;
        }
        uint32_t tot = 0;
        const uint32_t at = block_excl_scan<NT>(__popc(m), wsum, &tot);
        if (!WRITE) {
            if (tid == 0) a.tile_cnt[tile] = tot;
            continue;
        }
        const uint64_t tbase = a.tile_cnt[tile];   /* scanned: kept pairs in front of the tile */
        if (m) {
            uint32_t c[4];
            uint64_t sc[4];
            if (whole) {
                const uint4 cv = gload((const uint4*)(a.out_cnt + i));
                const uint4 s0 = gload((const uint4*)(a.out_score + i)), s1 = gload((const uint4*)(a.out_score + i + 2u));
                c[0] = cv.x; c[1] = cv.y; c[2] = cv.z; c[3] = cv.w;
                sc[0] = ((uint64_t)s0.y << 32) | s0.x; sc[1] = ((uint64_t)s0.w << 32) | s0.z;
                sc[2] = ((uint64_t)s1.y << 32) | s1.x; sc[3] = ((uint64_t)s1.w << 32) | s1.z;
            } else {
                const uint64_t* sb = (const uint64_t*)a.out_score;
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) {
                    c[k] = i + k < P ? gload(a.out_cnt + i + k) : 0u;
                    sc[k] = i + k < P ? gload(sb + i + k) : 0ull;
                }
            }
            uint64_t o = tbase + at;
            uint64_t* so = (uint64_t*)a.new_score;
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                if (!((m >> k) & 1u)) continue;
                if (o < P) {   /* kept pairs never outnumber the pairs */
                    gstore(a.new_term + o, gload(a.new_rank + t[k]));
                    gstore(a.new_cnt + o, c[k]);
                    gstore(so + o, sc[k]);
                }
                ++o;
            }
        }
        /* the documents whose offset lies in this tile */
        s_pref[tid] = at;
        s_mask[tid] = m;
        __syncthreads();
        const uint32_t j0 = a.tile_doc[tile], j1 = a.tile_doc[tile + 1u];
        for (uint64_t j = (uint64_t)j0 + tid; j < j1 && j <= a.ndocs; j += NT) {
            uint64_t v = a.out_off[j];
            if (v > P) v = P;
            const uint64_t r = v - tile * PR_TILE;
            if (r < PR_TILE) {
                const uint32_t l = (uint32_t)(r >> 2);
                a.new_off[j] = tbase + s_pref[l] + __popc(s_mask[l] & ((1u << (r & 3u)) - 1u));
            }
        }
        __syncthreads();   /* the next tile rewrites s_pref / s_mask */
    }
}

__global__ __launch_bounds__(NT) void k_pr_emptied(const PrPairs a) {
    __shared__ uint32_t wcnt[NT / 64];
    const uint64_t j = (uint64_t)blockIdx.x * NT + threadIdx.x;
    bool e = false;
    if (j < a.ndocs) {
        uint64_t b = a.out_off[j], en = a.out_off[j + 1u];
        if (en > a.npairs) en = a.npairs;
        if (b > en) b = en;
        e = en > b && a.new_off[j + 1u] == a.new_off[j];
    }
    const uint32_t c = (uint32_t)__popcll(__ballot(e));
    if ((threadIdx.x & 63u) == 0u) wcnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < NT / 64; ++w) sum += wcnt[w];
        if (sum) atomicAdd(a.emptied, sum);   /* a counter for the info struct, not a result */
    }
}

unsigned pairs_grid(const PrPairs& a, uint32_t ncu) {
    const uint64_t cap = (uint64_t)(ncu ? ncu : 256u) * PR_WG_PER_CU;
    return (unsigned)(a.ntiles < cap ? a.ntiles : cap);
}

}  // namespace

int launch_pr_range(const uint32_t* df, uint32_t V, uint64_t Nt, uint32_t min_df, uint32_t max_df, uint32_t* flag,
                    uint64_t* key, uint32_t* val, hipStream_t s) {
    if (!V) return 0;
    k_pr_range<<<grid_for(V), NT, 0, s>>>(df, V, Nt, min_df, max_df, flag, key, val);
    return ok();
}

int launch_pr_take(const uint64_t* key, const uint32_t* val, uint32_t V, uint32_t M, uint32_t* flag, hipStream_t s) {
    if (!V) return 0;
    k_pr_take<<<grid_for(V), NT, 0, s>>>(key, val, V, M, flag);
    return ok();
}

int launch_pr_bitmap(const uint32_t* flag, uint32_t V, uint32_t* bits, hipStream_t s) {
    if (!V) return 0;
    k_pr_bitmap<<<grid_for(V), NT, 0, s>>>(flag, V, bits);
    return ok();
}

int launch_pr_terms(const PrTerms& a, hipStream_t s) {
    if (!a.V) return 0;
    k_pr_terms<<<grid_for(a.V), NT, 0, s>>>(a);
    return ok();
}

int launch_pr_slots(const PrTerms& a, uint32_t* rank_of_slot, uint64_t slot_cap, hipStream_t s) {
    if (!a.V) return 0;
    k_pr_slots<<<grid_for(a.V), NT, 0, s>>>(a, rank_of_slot, slot_cap);
    return ok();
}

int launch_pr_tiledoc(const PrPairs& a, hipStream_t s) {
    k_pr_tiledoc<<<grid_for(a.ntiles + 1u), NT, 0, s>>>(a);
    return ok();
}

int launch_pr_count(const PrPairs& a, uint32_t ncu, hipStream_t s) {
    if (a.V <= PR_LDS_TERMS) k_pr_pairs<false, true><<<pairs_grid(a, ncu), NT, 0, s>>>(a);
    else k_pr_pairs<false, false><<<pairs_grid(a, ncu), NT, 0, s>>>(a);
    return ok();
}

int launch_pr_write(const PrPairs& a, uint32_t ncu, hipStream_t s) {
    if (a.V <= PR_LDS_TERMS) k_pr_pairs<true, true><<<pairs_grid(a, ncu), NT, 0, s>>>(a);
    else k_pr_pairs<true, false><<<pairs_grid(a, ncu), NT, 0, s>>>(a);
    return ok();
}

int launch_pr_emptied(const PrPairs& a, hipStream_t s) {
    if (!a.ndocs) return 0;
    k_pr_emptied<<<grid_for(a.ndocs), NT, 0, s>>>(a);
    return ok();
}
