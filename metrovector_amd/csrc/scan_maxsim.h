// scan_maxsim.h — launch interface of the multi-vector search's kernels (scan_maxsim.hip; maxsim.hip is the host side) and its
// scratch plan, a pure function (DESIGN.md §3 "Multi-vector search", §5 "M0 / M1 — multi-vector search").
#pragma once

#include <hip/hip_runtime.h>
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

}  // namespace mvf
