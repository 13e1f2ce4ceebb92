// scan_filter.h — launch interface of the filtered search's kernels (scan_filter.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mvf {

constexpr uint32_t kFilterBlockRows = 32768;  // rows one block of F0 / F1 covers: 1024 threads, one 32-row word each
constexpr uint32_t kFilterChunk = 1024;       // F2: list rows per block
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

// F2: grid (chunks of kFilterChunk list rows, groups of queries).  The G-lane group of K1's one-query shape loads a row's
// 16-byte vectors once and scores it against every query of the block's group with K1's arithmetic (k1_rowscore.h);
// composites (key << 32 | local row).  lists != NULL: per query, the chunk's best min(kcap, rows) composites, sorted,
// ~0-padded, to lists[q][chunk][kcap] (the input of K3, select_final_kernel).  dump != NULL: the rank entry of every list
// position i < m goes to dump[q][i], for the whole-list sort.
struct FilterScoreParams {
    const unsigned char* rows;
    const void* queries;     // device [nq][dim]: f32, or the space's int type
    const uint32_t* list;    // [m] admitted local rows, ascending
    uint32_t m, nq, dim, pitch, V, J;
    uint64_t* lists;
    uint32_t kcap;
    uint64_t* dump;
};
// queries per group for a space whose padded query takes `qbytes` (cand_query_bytes): 4 where four fit the LDS budget of the
// candidate search (kCandQueryLdsMax), else 1
uint32_t filter_group_queries(uint32_t qbytes);
hipError_t filter_score_launch(uint8_t dtype, int metric, int G, const FilterScoreParams& p, hipStream_t s);

}  // namespace mvf
