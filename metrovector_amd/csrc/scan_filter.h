// scan_filter.h — launch interface of the filtered search's kernels (scan_filter.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mvf {

constexpr uint32_t kFilterBlockRows = 32768;  // rows one block of F0 / F1 covers: 1024 threads, one 32-row word each
constexpr uint32_t kFilterGroup = 4;          // F2: queries a block scores against each row it loads, at most

// F0: the caller's allow bits -> the effective deny mask of a filtered search, in the tombstone buffer's layout
// (ceil(n / 32) + 1 words, zero at and beyond n), and the admitted rows of every block of kFilterBlockRows rows.
struct FilterMaskParams {
    const uint32_t* allow;   // words; bit (shift + r) counts for local row r.  Readable up to word (shift + n - 1) / 32 + 1
    uint32_t shift;          // 0 .. 31
    uint64_t n;
    const uint32_t* tomb;    // the handle's deletion bitmap; NULL = none
    uint32_t* deny;          // out: ceil(n / 32) + 1 words
    uint32_t* block_cnt;     // out: [ceil((ceil(n / 32) + 1) / 1024)] admitted rows per block
};
hipError_t filter_mask_launch(const FilterMaskParams& p, hipStream_t s);
inline uint32_t filter_blocks(uint64_t n) { return (uint32_t)(((n + 31) / 32 + 1 + 1023) / 1024); }

// F1: the exclusive scan of F0's block counts (block_off[nb], *total), then the admitted rows, ascending, as u32.
hipError_t filter_scan_launch(const uint32_t* block_cnt, uint32_t nb, uint64_t* block_off, uint64_t* total, hipStream_t s);
hipError_t filter_compact_launch(const uint32_t* deny, uint64_t n, const uint64_t* block_off, uint32_t* list, hipStream_t s);

// F2 is the gathered-row kernel (scan_gather.h) on F1's list.  Queries per group for a space whose padded query takes `qbytes`
// (cand_query_bytes): 4 where four fit the query's LDS budget (kCandQueryLdsMax), else 1
uint32_t filter_group_queries(uint32_t qbytes);

}  // namespace mvf
