// scan_columns.h — launch interface of P0, the predicate kernel of the column filters (scan_columns.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mvf {

constexpr uint32_t kWhereMaxClauses = 8;      // MVFGPU_WHERE_MAX_CLAUSES
constexpr uint32_t kWhereMaxSetValues = 4096; // MVFGPU_WHERE_MAX_SET_VALUES: 32 KiB of LDS
constexpr uint32_t kWhereStepRows = 256;      // rows a wave covers per step: four consecutive rows per lane, eight words

// One clause after the host's normalisation: a range test lo <= v <= hi or the membership of v in a sorted set, possibly
// negated.  A UInt32 column's range is clamped to 32 bits (an empty range is lo = 1, hi = 0).
struct WhereClause {
    const void* values;   // the column's values over local rows: u32 or u64, aligned to 16 bytes
    uint64_t lo, hi;      // range clauses
    uint32_t set_first;   // set clauses: their values are sets[set_first .. set_first + set_count), ascending, distinct
    uint32_t set_count;
    uint8_t is_u64, is_set, negate, pad;
    uint32_t pad2;
};

// P0: all clauses and the base filter -> the ALLOW words over local rows (ceil(n / 32) u32 words, bit r & 31 of word r >> 5,
// zero at and beyond n): the device form's layout, which F0 takes with shift 0.
struct WhereParams {
    WhereClause clause[kWhereMaxClauses];
    uint32_t n_clauses;
    uint32_t any;               // 0: every clause holds, 1: at least one
    uint64_t n;                 // rows; no column is read past n values
    const uint64_t* sets;       // [n_sets] the set clauses' values, or NULL
    uint32_t n_sets;            // <= kWhereMaxSetValues
    const uint32_t* base_deny;  // the base filter's deny mask (tombstone layout), or NULL
    uint32_t* allow;            // out: ceil(n / 32) words
};
hipError_t where_launch(const WhereParams& p, int num_cus, hipStream_t s);

}  // namespace mvf
