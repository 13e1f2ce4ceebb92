// scan_mmr.h — launch interface of D0, the greedy walk of the diversified re-ranking (scan_mmr.hip; mmr.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_gather.h"

namespace mvf {

constexpr uint32_t kMmrMaxCandidates = 1024;  // list entries per query: one block keeps their state in LDS

// D0.  One block per query walks its candidates: rank entries dump[q][i] (position << 32 | key', mvf_common.h) of the
// counts[q] distinct live rows of C0, in ascending row -- the gathered-row kernel's dump.  The block writes the first
// min(k, counts[q]) entries of the query's result row; the rest keeps what the caller filled it with (padding).
struct MmrWalkParams {
    const unsigned char* rows;
    const uint64_t* dump;    // [nq][m]
    const uint32_t* counts;  // [nq]
    float* qscratch;         // [nq][dim] f32: the picked row of a query whose padded copy exceeds kCandQueryLdsMax; else unused
    uint32_t m, nq, dim, pitch, V, J, k;
    float a, b;              // lambda, 1 - lambda
    uint64_t index_base;
    const uint64_t* ids;     // vector ids per local row, or NULL
    float* out_scores;       // [nq][k]
    uint64_t* out_indices;
    int32_t* out_raw;        // nullable
    float* out_objective;    // nullable
};

// The form of D0 that walks rows of J steps per lane of a G-lane group, a pure function: the bytes of the picked row padded as
// a query (cand_query_bytes); qlds: that copy is staged in LDS -- Int8 / UInt8 always, float rows up to kCandQueryLdsMax bytes,
// beyond that it goes to the query's f32 scratch row and is read back through the cache.  mmr_walk_launch picks its
// instantiation from it, mmr_core sizes the scratch row by it and mvfgpu_selftest_mmr_form reports it.
struct MmrForm {
    uint32_t qbytes;
    bool qlds;
};
inline MmrForm mmr_form(uint8_t dtype, int G, uint32_t J) {
    MmrForm f;
    f.qbytes = cand_query_bytes(dtype, G, J);
    f.qlds = is_int_dtype(dtype) || f.qbytes <= kCandQueryLdsMax;
    return f;
}

// G: the lane group of one_query_group (K1's one-query shape)
hipError_t mmr_walk_launch(uint8_t dtype, int metric, int G, const MmrWalkParams& p, hipStream_t s);

}  // namespace mvf
