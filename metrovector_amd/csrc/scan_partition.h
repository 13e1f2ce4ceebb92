// scan_partition.h — launch interface of the partition index's build kernels and of the partitioned search's kernels
// (scan_partition.hip; partition.hip is the host side).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mvf {

constexpr uint32_t kPartBlockRows = 8192;  // rows (or sorted entries) one 1024-thread block of the build kernels covers
constexpr int kPartSortTile = 2048;        // pairs per block tile of the pair sort (radix_pass.h: kRsTile)
inline uint32_t part_blocks(uint64_t n) { return (uint32_t)((n + kPartBlockRows - 1) / kPartBlockRows); }
inline uint32_t part_sort_tiles(uint64_t m) { return (uint32_t)((m + kPartSortTile - 1) / kPartSortTile); }

// ---- the build (DESIGN.md §5 "B0 .. B3 / S1 — partitioned search")
// B0, count: block_cnt[b] = live rows of block b's kPartBlockRows rows; bits[0] |= every live key, bits[1] &= every live key
// (the caller sets them to 0 / ~0): the keys differ exactly in the bits of bits[0] ^ bits[1].
hipError_t part_count_launch(const void* values, bool is_u64, uint64_t n, const uint32_t* tomb, uint32_t* block_cnt, uint64_t* bits,
                             hipStream_t s);
// B0, compact: the live rows' (key zero-extended to u64, local row) in ascending position; block_off from filter_scan_launch
hipError_t part_compact_launch(const void* values, bool is_u64, uint64_t n, const uint32_t* tomb, const uint64_t* block_off, uint64_t* keys,
                               uint32_t* rows, hipStream_t s);
// B1: one stable pass of the LSD radix sort of m (key, row) pairs on the 8 bits at `shift`.  bh: 256 * part_sort_tiles(m)
// words, tot: 256 words.
hipError_t part_sort_pass_launch(const uint64_t* keys_in, const uint32_t* rows_in, uint64_t* keys_out, uint32_t* rows_out, uint64_t m, int shift,
                                 uint32_t* bh, uint32_t* tot, hipStream_t s);
// B2, count: block_cnt[b] = entries of block b whose key differs from the one in front (entry 0 counts)
hipError_t part_heads_count_launch(const uint64_t* keys, uint64_t m, uint32_t* block_cnt, hipStream_t s);
// B2, write: table_keys[j] = the j-th distinct key, table_off[j] = its first entry, table_off[n_keys] = m
hipError_t part_heads_write_launch(const uint64_t* keys, uint64_t m, const uint64_t* block_off, uint64_t* table_keys, uint64_t* table_off,
                                   hipStream_t s);

// ---- the search
// one planned query: where it lies in the caller's buffers and which segment of rows_by_key it is answered from
struct PartQuery {
    uint32_t query, offset, count;
};

// S1: K1's scores of one segment of at most kGatherChunk rows per block -- the gathered-row kernel (scan_gather.hip) for one
// query and one chunk, the list base, the count and the query taken from plan[blockIdx.x].  lists[i][kcap]: the segment's best
// min(kcap, count) composites, sorted, ~0-padded (K3's input).
struct SegmentScoreParams {
    const unsigned char* rows;
    const void* queries;          // the caller's [nq][dim]
    const uint32_t* rows_by_key;
    const PartQuery* plan;        // [n] small-tier queries of this launch
    uint32_t n, dim, pitch, V, J;
    uint64_t* lists;
    uint32_t kcap;
};
hipError_t segment_score_launch(uint8_t dtype, int metric, int G, const SegmentScoreParams& p, hipStream_t s);

// the large tier's queries made contiguous: dst[i] = queries[plan[i].query], qrow bytes each (a multiple of 4, or any for
// the byte types)
hipError_t part_gather_queries_launch(const void* queries, const PartQuery* plan, uint32_t n, uint32_t qrow, void* dst, hipStream_t s);

// The call's result rows put where the caller's queries are: row plan[i].query of the outputs = row i of the compact results
// for i < n_scored, padding for n_scored <= i < nq.
struct PartScatterParams {
    const PartQuery* plan;  // [nq]: scored queries in compact order, then the padding queries
    uint32_t nq, n_scored, k;
    uint8_t metric;
    const float* c_scores;
    const uint64_t* c_indices;
    const int32_t* c_raw;   // NULL with out_raw
    float* out_scores;
    uint64_t* out_indices;
    int32_t* out_raw;       // nullable
};
hipError_t part_scatter_launch(const PartScatterParams& p, hipStream_t s);

}  // namespace mvf
