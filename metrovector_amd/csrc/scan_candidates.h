// scan_candidates.h — launch interface of the candidate search's own kernels (scan_candidates.hip); its scoring kernel is
// the gathered-row kernel (scan_gather.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_gather.h"

namespace mvf {

constexpr uint32_t kCandLdsSort = 8192;  // C0 sorts a list of up to this many entries in one block's LDS (64 KiB)

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

hipError_t cand_prep_launch(const CandPrepParams& p, uint32_t nq, hipStream_t s);          // m <= kCandLdsSort: C0 in LDS
hipError_t cand_map_launch(const CandPrepParams& p, uint32_t nq, hipStream_t s);           // m > kCandLdsSort: entries to p.ent ..
hipError_t cand_compact_launch(const CandPrepParams& p, const uint64_t* sorted, uint32_t nq, hipStream_t s);  // .. sorted: C0's lists

}  // namespace mvf
