// scan_maxsim.h — launch interface of the multi-vector search's kernels (scan_maxsim.hip; maxsim.hip is the host side) and its
// scratch plan, a pure function (DESIGN.md §3 "Multi-vector search", §5 "M0 / M1 — multi-vector search").
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "mvf_common.h"
#include "scan_gather.h"

namespace mvf {

constexpr uint32_t kMaxsimRows = 128;        // positions of the key-ordered list one block of M0 covers
constexpr uint32_t kMaxsimChunkMax = 32;     // tokens of a chunk at most: kMaxsimChunkMax x kMaxsimRows minima of LDS (16 KiB)
constexpr uint32_t kMaxsimTokenGroup = 4;    // tokens that meet a row's vectors together (the gathered-row kernel's four queries)
constexpr uint32_t kMaxsimRegSteps = 4;      // rows of up to this many 16-byte steps per lane (J) stay in registers over a chunk
constexpr uint32_t kMaxsimWindow = 1024;     // query sets per window at most
constexpr uint32_t kMaxsimKeyBytes = 20;     // scratch per key and query set beside the minima: S (4), the two sort buffers (8 + 8)

// The plan of a call: tokens per chunk and query sets per window, so that chunk x n_keys x 4 + n_keys x kMaxsimKeyBytes bytes per
// query set of a window stay inside budget_bytes.  A chunk holds at most kMaxsimChunkMax tokens and at most as many as LDS takes
// (kCandQueryLdsMax bytes of padded tokens; a token beyond that is read through the cache and does not count), and at least one
// token group -- all tokens where there are fewer -- whatever the budget: one group's scratch may exceed it.
struct MaxsimPlan {
    uint32_t chunk, window;
};
inline MaxsimPlan maxsim_plan(uint64_t n_keys, uint32_t n_tokens, uint32_t nq, uint64_t token_bytes, uint64_t budget_bytes) {
    const uint64_t in_lds = token_bytes == 0 || token_bytes > kCandQueryLdsMax ? kMaxsimChunkMax : kCandQueryLdsMax / token_bytes;
    const uint64_t cap = std::min<uint64_t>({n_tokens, kMaxsimChunkMax, in_lds});
    const uint64_t least = std::min<uint64_t>(cap, kMaxsimTokenGroup);
    const uint64_t per_key = budget_bytes / (n_keys ? n_keys : 1);
    const uint64_t fit = per_key > kMaxsimKeyBytes ? (per_key - kMaxsimKeyBytes) / 4 : 0;
    MaxsimPlan pl;
    pl.chunk = (uint32_t)std::min(std::max(fit, least), cap);
    const uint64_t per_set = (n_keys ? n_keys : 1) * ((uint64_t)pl.chunk * 4 + kMaxsimKeyBytes);
    pl.window = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({budget_bytes / per_set, nq, kMaxsimWindow}));
    return pl;
}

// The form of M0 that scores rows of J steps per lane of a G-lane group, a pure function: the bytes of a padded token
// (cand_query_bytes); qlds: the tokens live in LDS -- Int8 / UInt8 always, float tokens up to kCandQueryLdsMax bytes, beyond that
// they are read through the cache --; reg: the rows stay in registers over a chunk (J <= kMaxsimRegSteps), else they are read
// again per token group.  score_launch picks its instantiation from it and mvfgpu_selftest_maxsim_form reports it.
struct MaxsimForm {
    uint32_t token_bytes;
    bool qlds, reg;
};
inline MaxsimForm maxsim_form(uint8_t dtype, int G, uint32_t J) {
    MaxsimForm f;
    f.token_bytes = cand_query_bytes(dtype, G, J);
    f.qlds = is_int_dtype(dtype) || f.token_bytes <= kCandQueryLdsMax;
    f.reg = f.qlds && J <= kMaxsimRegSteps;
    return f;
}

// ord[i] = the ordinal, in the key table, of the key whose segment holds position i of the key-ordered list, from the table's
// offsets [n_keys + 1]; once per call
hipError_t maxsim_ordinals_launch(const uint64_t* offsets, uint64_t n_keys, uint32_t live, uint32_t* ord, hipStream_t s);

// M0.  Grid (blocks of kMaxsimRows list positions, query sets).  best[set][t][n_keys], all 0xFFFFFFFF on entry, receives the
// smallest order key of tokens [t0, t0 + tc) of every query set over each key's rows.
struct MaxsimScoreParams {
    const unsigned char* rows;
    const void* queries;   // device [sets][n_tokens][dim]: f32, or the space's int type
    const uint32_t* list;  // the key-ordered list [m]
    const uint32_t* ord;   // [m] key ordinals
    uint32_t* best;
    uint32_t m, n_keys, sets, n_tokens, t0, tc, dim, pitch, V, J;
    const struct MaxsimCandBlock* blocks;  // the candidate form's block table; not read by the full search's form
    uint64_t* best64;                      // M0-arg's minima (scan_maxsim_align.hip); not read by M0
};
hipError_t maxsim_score_launch(uint8_t dtype, int metric, int G, const MaxsimScoreParams& p, hipStream_t s);

// ---- the candidate form (mvfgpu_search_maxsim_candidates; DESIGN.md §3 "Candidate keys", §5 "E0")
// The plan of a query set, made on the host: its distinct held candidates in ascending key value are the segments
// [seg0, seg0 + count) of the call's segment arrays -- the slot ordinal of a candidate is its rank among them --, `rows` the rows
// they hold, list0 the set's first position of its window's concatenated list, a multiple of kMaxsimRows.
struct MaxsimCandSet {
    uint32_t seg0, count, list0, rows;
};
// a candidate's segment of rows_by_key and the rows the set's candidates in front of it hold
struct MaxsimCandSeg {
    uint32_t offset, before;
};
// the kMaxsimRows list positions of a block: its query set of the window and the positions that hold a row (1 .. kMaxsimRows);
// no block spans two sets
struct MaxsimCandBlock {
    uint32_t set, nr;
};
// list positions a set of `rows` candidate rows takes: padded to whole blocks
inline uint64_t maxsim_cand_positions(uint64_t rows) { return (rows + kMaxsimRows - 1) / kMaxsimRows * kMaxsimRows; }

// E0.  One thread per list position of the window's n_blocks blocks: list[pos] = the local row and ord[pos] = the slot ordinal
// of the position's candidate row, from a binary search of the set's `before` values; a position behind the set's rows is dead
// (row 0, the set's last ordinal), which no block of M0 reads.
struct MaxsimExpandParams {
    const uint32_t* rows_by_key;
    const MaxsimCandSet* sets;      // the window's
    const MaxsimCandSeg* segs;      // the call's
    const MaxsimCandBlock* blocks;  // the window's
    uint32_t n_blocks;
    uint32_t *list, *ord;           // [n_blocks * kMaxsimRows]
};
hipError_t maxsim_expand_launch(const MaxsimExpandParams& p, hipStream_t s);

// M0 over the concatenated list: grid (p.m / kMaxsimRows blocks, 1); a block takes its set, and with it its tokens and its
// best[set][t][n_keys], from p.blocks, and scores the block's first nr positions.  p.n_keys is the window's largest candidate
// count, p.ord the slot ordinals.  The arithmetic is maxsim_score_launch's.
hipError_t maxsim_score_candidates_launch(uint8_t dtype, int metric, int G, const MaxsimScoreParams& p, hipStream_t s);

// M1.  sum[set][g] (f32; not read when `first`) advances by the chunk's tc reconstructed scores in token order; `last`: the
// rank entry (key_from_score(S), ordinal g) goes to rank[set][g].
struct MaxsimSumParams {
    const uint32_t* best;
    float* sum;
    uint64_t* rank;
    uint32_t n_keys, sets, tc;
    uint8_t metric, dtype;
    bool first, last;
    const MaxsimCandSet* cand;  // nullable; the candidate form: ordinals from cand[set].count on are no keys -- dead rank entries
};
hipError_t maxsim_sum_launch(const MaxsimSumParams& p, hipStream_t s);

// The result rows of `sets` query sets from their sorted rank entries sorted[set][n_keys]: the first min(k, n_keys) ordinals'
// sums and key values (keys[n_keys], the index's key table), padding beyond, counts[set] (nullable) = min(k, n_keys).
// The candidate form (cand not NULL): cand[set].count takes n_keys' place in both minima -- sorted and sum keep the stride
// n_keys --, and ordinal g's key value is keys[cand[set].seg0 + g], the plan's key array.
struct MaxsimWriteParams {
    const uint64_t* sorted;
    const float* sum;
    const uint64_t* keys;
    float* out_scores;
    uint64_t* out_keys;
    uint32_t* out_counts;
    uint32_t n_keys, sets, k;
    uint8_t metric;
    const MaxsimCandSet* cand;  // nullable
};
hipError_t maxsim_write_launch(const MaxsimWriteParams& p, hipStream_t s);

// ---- alignments (mvfgpu_maxsim_align; scan_maxsim_align.hip; DESIGN.md §3 "Alignments", §5 "M0-arg and the alignment writer")
// The plan of an alignment call: maxsim_plan's chunk rules -- at most kMaxsimChunkMax tokens, at most what kCandQueryLdsMax bytes
// of padded tokens take, at least one token group whatever the budget -- with chunk x n_keys x 8 bytes of minima per query set of
// a window inside budget_bytes: M0-arg keeps a u64 per (token, key) and there are no sums and no sort buffers.  The caller takes
// the window's concatenated list (8 bytes per position) and the slot map (4 bytes per list entry) off the budget first.  One set
// whatever the budget.
inline MaxsimPlan maxsim_align_plan(uint64_t n_keys, uint32_t n_tokens, uint32_t nq, uint64_t token_bytes, uint64_t budget_bytes) {
    const uint64_t in_lds = token_bytes == 0 || token_bytes > kCandQueryLdsMax ? kMaxsimChunkMax : kCandQueryLdsMax / token_bytes;
    const uint64_t cap = std::min<uint64_t>({n_tokens, kMaxsimChunkMax, in_lds});
    const uint64_t least = std::min<uint64_t>(cap, kMaxsimTokenGroup);
    const uint64_t nk = n_keys ? n_keys : 1, fit = budget_bytes / nk / 8;
    MaxsimPlan pl;
    pl.chunk = (uint32_t)std::min(std::max(fit, least), cap);
    pl.window = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>({budget_bytes / (nk * pl.chunk * 8), nq, kMaxsimWindow}));
    return pl;
}

// M0-arg: maxsim_score_candidates_launch with the argument kept.  p.best64[set][t][n_keys], all-ones on entry, receives the
// smallest (order key << 32 | local row) of tokens [t0, t0 + tc) of every query set over each candidate's rows: the first row in
// mvfgpu_search's order.  p.best is not read.  The scoring is M0's, line for line.
hipError_t maxsim_score_arg_launch(uint8_t dtype, int metric, int G, const MaxsimScoreParams& p, hipStream_t s);

// The alignment writer.  One thread per (entry i of a set's list, token t of the chunk): slot = slots[set][i], the entry's slot
// ordinal (UINT32_MAX: skipped; a repeat carries its first occurrence's), and element (set, i, t0 + t) of the three outputs
// [sets][m][n_tokens] is the score, the reported row (ids[row] or index_base + row) and the exact integer (out_raw nullable) of
// best64[set][t][slot], or mvfgpu_search's padding for a skipped entry.  best64 NULL: every element is padding.
struct MaxsimAlignWriteParams {
    const uint64_t* best64;
    const uint32_t* slots;  // [sets][m]
    const uint64_t* ids;    // nullable
    uint64_t index_base;
    float* out_scores;
    uint64_t* out_rows;
    int32_t* out_raw;
    uint32_t sets, m, n_keys, n_tokens, t0, tc;
    uint8_t metric, dtype;
};
hipError_t maxsim_align_write_launch(const MaxsimAlignWriteParams& p, hipStream_t s);

// ---- the MFMA selection route (scan_maxsim_mfma.hip; DESIGN.md §3 "Multi-vector search: the MFMA route", §5 "A0 / P0")
// The route of a full multi-vector search, a pure function (mvfgpu_selftest_maxsim_route; the launch calls it): 1 = the one-pass
// route (M0 over every row), 2 = select on MFMA scores inside a proven bound, then M0 over the candidates' blocks.  forced:
// mvfgpu_set_maxsim_route / MVF_MAXSIM_ROUTE (0 = automatic).  Eligible: Float32 / Float16 rows under InnerProduct / Cosine;
// everything else takes route 1 whatever is forced.  Automatic takes route 2 where it is eligible, k <= n_keys / 2 (beyond that
// most keys are candidates), the call fills a tile of A0 (nq x n_tokens >= 32 query rows: A0 costs whole tiles) and held rows x
// n_tokens reaches the crossover of profiles/r18_maxsim_mfma.txt: 2M rows x 32 tokens is the smallest measured shape where
// route 2 wins on both README shapes with one query set (0.52 and 0.63 of route 1; at 500k x 32 the Float16 shape still loses).
constexpr uint64_t kMaxsimMfmaCrossover = 64000000ull;  // held rows x n_tokens
constexpr uint32_t kMaxsimMfmaTile = 32;                // query rows of an accumulator of A0
inline bool maxsim_mfma_eligible(uint8_t dtype, uint8_t metric) {
    return (dtype == MVF_DTYPE_FLOAT32 || dtype == MVF_DTYPE_FLOAT16) && (metric == MVF_METRIC_INNER_PRODUCT || metric == MVF_METRIC_COSINE);
}
inline uint32_t maxsim_route(uint64_t held_rows, uint64_t n_keys, uint32_t dim, uint8_t dtype, uint8_t metric, uint32_t nq,
                             uint32_t n_tokens, uint32_t k, int forced) {
    (void)dim;
    if (forced == 1 || !maxsim_mfma_eligible(dtype, metric)) return 1u;
    if (forced == 2) return 2u;
    const bool pays = (uint64_t)k <= n_keys / 2 && (uint64_t)nq * n_tokens >= kMaxsimMfmaTile &&
                      held_rows >= (kMaxsimMfmaCrossover + n_tokens - 1) / (n_tokens ? n_tokens : 1);  // no overflow
    return pays ? 2u : 1u;
}

// The bound of |S~ - S| of a query set, S~ the sum of the per-token bests of A0's scores, S the exact route's: as the device
// computes it (P0) and as mvfgpu_selftest_maxsim_margin states it.  eps is the batched search's own: (max(dim, 64) + 16) 2^-23 for
// the f32 accumulation and the norms, plus 2^-11 1.001 on Float16 rows for the query's rounding to f16; in units u_t = 1 (Cosine)
// or |q_t| sqrt(xxmax) (InnerProduct).  Delta = 1.001 (eps + (T - 1) 2^-23) sum u_t: the second term is the two f32 sums' own
// rounding, |b| <= u_t.  A unit that is NaN, or neither 0 nor in [1e-24, 1e37), leaves the premises (partial sums that overflow
// in one order and not in another; products the matrix unit may flush): Delta is +inf and every key a candidate.
MVF_HD double maxsim_margin(uint8_t dtype, uint8_t metric, uint32_t dim, const float* token_norms, uint32_t n_tokens, float xxmax) {
    double eps = (double)((dim > 64u ? dim : 64u) + 16u) * 1.1920928955078125e-7;
    if (dtype == MVF_DTYPE_FLOAT16) eps += 4.8828125e-4 * 1.001;
    const double xm = sqrt((double)xxmax), inf = (double)bits_f32(0x7F800000u);
    double sum = 0.0;
    for (uint32_t t = 0; t < n_tokens; t++) {
        const double u = metric == MVF_METRIC_COSINE ? 1.0 : (double)token_norms[t] * xm;
        if (!(u == 0.0 || (u >= 1e-24 && u < 1e37))) return inf;
        sum += u;
    }
    if (!(sum < 1e37)) return inf;
    return 1.001 * (eps + (double)(n_tokens - 1u) * 1.1920928955078125e-7) * sum;
}

// The plan of route 2: maxsim_plan's chunk for M0 over the candidates, a chunk of its own for A0 -- A0 keeps no tokens in LDS,
// so only kMaxsimChunkMax and the budget bound it: whole tiles of 32 query rows and fewer passes over the rows where M0's
// tokens are large --, and a window that also holds what the route adds per query set inside the budget: the prepared tokens
// (n_tokens rows of kp_bytes, two floats each), one flag byte per key and one MaxsimCandBlock per block of the list.  One set
// whatever the budget.
struct MaxsimMfmaPlan {
    uint32_t chunk, achunk, window;
};
inline MaxsimMfmaPlan maxsim_mfma_plan(uint64_t n_keys, uint64_t held_rows, uint32_t n_tokens, uint32_t nq, uint64_t token_bytes,
                                       uint64_t kp_bytes, uint64_t budget_bytes) {
    const MaxsimPlan m0 = maxsim_plan(n_keys, n_tokens, nq, token_bytes, budget_bytes), a0 = maxsim_plan(n_keys, n_tokens, nq, 0, budget_bytes);
    const uint64_t nk = n_keys ? n_keys : 1, blocks = (held_rows + kMaxsimRows - 1) / kMaxsimRows;
    const uint64_t per_set = nk * ((uint64_t)std::max(m0.chunk, a0.chunk) * 4 + kMaxsimKeyBytes + 1) + (uint64_t)n_tokens * (kp_bytes + 8) + blocks * 8;
    MaxsimMfmaPlan pl;
    pl.chunk = m0.chunk, pl.achunk = a0.chunk;
    pl.window = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min(m0.window, a0.window), budget_bytes / per_set));
    return pl;
}

// A0.  Grid (blocks of kMaxsimRows list positions), block 256: wave w scores positions 32 w .. 32 w + 31 of its block against
// the window's (set, token of the chunk) query rows, 32 per accumulator, and ends as M0 does: best[set][t][n_keys] receives the
// smallest order key of the APPROXIMATE score; force[set][n_keys] (bytes, zero on entry) is raised for a key where the bound's
// premises fail.
struct MaxsimMfmaParams {
    const unsigned char* rows;
    const unsigned char* qprep;  // [sets * n_tokens][kp_bytes]: f32 rows: the zero-padded f32 tokens; f16 rows: the plane f16(q 2^e)
    const float* undo;           // [sets * n_tokens] f16 rows: 2^-e; NULL on f32 rows
    const float* qnorm;          // [sets * n_tokens] |q|
    const float* xnorm;          // [n] |x| per local row
    const uint32_t* list;        // the key-ordered list [m]
    const uint32_t* ord;         // [m] key ordinals
    uint32_t* best;
    unsigned char* force;
    uint32_t m, n_keys, sets, n_tokens, t0, tc, pitch, V, kp_bytes;
};
hipError_t maxsim_mfma_score_launch(uint8_t dtype, int metric, const MaxsimMfmaParams& p, hipStream_t s);

// rank[set][g] = the live NaN entry where flag[set][g] != 0 or (also_nonfinite and sum[set][g] is not finite) -- behind every
// finite sum, in front of the dead entries --; dead: the dead entry where flag[set][g] == 0 instead (the keys that are no
// candidates of the set).
struct MaxsimMaskParams {
    uint64_t* rank;
    const float* sum;
    const unsigned char* flag;
    uint32_t n_keys, sets;
    bool dead;
};
hipError_t maxsim_mask_launch(const MaxsimMaskParams& p, hipStream_t s);

// P0.  flag[set][g] (A0's force on entry) becomes "g is a candidate of the set": forced, or S~(g), theta or Delta not finite, or
// S~(g) >= theta - 2 Delta (in double, rounded down), theta the score of the kth entry of sorted[set][n_keys] (kth < n_keys)
// and Delta = maxsim_margin of the set's token norms.  Then blocks[set][n_blocks] = {set, the block's positions where it holds a
// row of a candidate, else 0}.  stats (nullable): [2][sets] candidates and flagged blocks per set, zero on entry.
struct MaxsimPickParams {
    const uint64_t* sorted;
    const float* sum;
    const float* qnorm;   // [sets * n_tokens]
    const float* xxmax;   // [1]
    const uint32_t* ord;  // [m]
    unsigned char* flag;
    MaxsimCandBlock* blocks;
    uint32_t* stats;
    double* delta;        // [sets] scratch: the sets' bounds
    uint32_t m, n_keys, sets, n_tokens, kth, dim;
    uint8_t metric, dtype;
};
hipError_t maxsim_pick_launch(const MaxsimPickParams& p, hipStream_t s);

}  // namespace mvf
