// scan_candidates.h — launch interface of the candidate search kernels (scan_candidates.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mvf {

constexpr uint32_t kCandLdsSort = 8192;  // C0 sorts a list of up to this many entries in one block's LDS (64 KiB)
constexpr uint32_t kCandChunk = 1024;    // C1: distinct rows per block (a chunk of one query's list)

// C0: one query's list (global positions) -> its distinct live local rows, ascending.  An entry is skipped when it is
// UINT64_MAX, outside [index_base, index_base + n) or a deleted row.
struct CandPrepParams {
    const uint64_t* cand;    // [nq][m] global positions
    uint32_t m;
    uint64_t index_base, n;
    const uint32_t* tomb;    // deletion bitmap over local rows; NULL = none
    uint64_t* ent;           // long lists (m > kCandLdsSort): [nq][m] rank entries (entry << 32 | local row, dead = 0xFFFFFFFF)
    uint32_t* rows;          // out: [nq][m] distinct local rows, ascending; the first counts[q] valid
    uint32_t* counts;        // out: [nq]
    uint64_t* out_counts;    // out (nullable): [nq] the same counts as u64 (the caller's)
};

// C1: grid (chunks of kCandChunk list entries, nq).  The G-lane group of K1's one-query shape scores one row with K1's
// arithmetic (k1_rowscore.h); composites (key << 32 | local row).  lists != NULL: each block writes its chunk's best
// min(kcap, rows) composites, sorted, ~0-padded, to lists[q][chunk][kcap] (the input of K3, select_final_kernel).
// dump != NULL: the rank entry of every list position i < m goes to dump[q][i] (positions past the count dead), for the
// whole-list sort of k > MVFGPU_K_PER_PASS.
struct CandScoreParams {
    const unsigned char* rows;
    const void* queries;     // device [nq][dim]: f32, or the space's int type
    const uint32_t* cand_rows;   // C0's lists [nq][m]
    const uint32_t* counts;      // [nq]
    uint32_t m, dim, pitch, V, J;
    uint64_t* lists;
    uint32_t kcap;
    uint64_t* dump;
};

// the query lives in LDS when its padded copy takes at most this many bytes, beyond that the rows read it through the cache
constexpr uint32_t kCandQueryLdsMax = 40u * 1024u;
inline uint32_t cand_query_bytes(uint8_t dtype, int G, uint32_t J) { return (uint32_t)G * J * (dtype == 1 ? 32u : 16u); }

hipError_t cand_prep_launch(const CandPrepParams& p, uint32_t nq, hipStream_t s);          // m <= kCandLdsSort: C0 in LDS
hipError_t cand_map_launch(const CandPrepParams& p, uint32_t nq, hipStream_t s);           // m > kCandLdsSort: entries to p.ent ..
hipError_t cand_compact_launch(const CandPrepParams& p, const uint64_t* sorted, uint32_t nq, hipStream_t s);  // .. sorted: C0's lists
hipError_t cand_score_launch(uint8_t dtype, int metric, int G, const CandScoreParams& p, uint32_t nq, hipStream_t s);

}  // namespace mvf
