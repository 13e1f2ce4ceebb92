/*
 * mvf_gpu_hamming_radius.h — C ABI of libmvf_gpu.so, continued: radius search under Hamming distance, every bit-packed row
 * within r bits of each query.  The functions are additions to ABI version 3.
 */
#ifndef MVF_GPU_HAMMING_RADIUS_H
#define MVF_GPU_HAMMING_RADIUS_H

#include "mvf_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Hamming radius search ("Hamming radius search", section 5 "HR2 / HRP"): near-duplicate detection,
 * SimHash / MinHash dedupe, perceptual-hash lookup -- "every row within r bits of this code, and how many are there".  Handle
 * and queries are mvfgpu_search_hamming's: a UInt8 corpus whose `dimension` is the number of packed BYTES of a row, here
 * 1 .. 512, and UInt8 queries [nq][dimension], contiguous.  radii is a host array [nq]: row x matches query q iff it is not
 * deleted and d(q, x) <= radii[q] (inclusive), d the Hamming search's exact i32.  A radius of 8 x dimension or more matches
 * every live row.
 *   out_counts[q] = the exact number of matches, also beyond max_per_query.
 *   out_scores, out_indices, out_raw (nullable): [nq][max_per_query].  The first min(count, max_per_query) entries of a query
 *   are its best matches: ascending d, ties by ascending row POSITION; score (float)d (exact), raw d, index index_base + row,
 *   or the row's vector id where ids are attached.  The rest is the Hamming search's padding: index UINT64_MAX, score +inf,
 *   raw 0.
 * max_per_query is 0 .. MVFGPU_K_PER_PASS; 0 asks for the counts only, and the three entry buffers may then be NULL.
 *
 * The recipe this call replaces: the entries of query q are those of mvfgpu_search_hamming with k = max_per_query, cut off
 * behind the last entry with d <= radii[q]; the count is the number of live rows with d <= radii[q].  A top-k with a guessed k
 * gives neither the cut nor the count.
 *
 * The answer never depends on the bytes behind `dimension` in a row's pitch.  The call builds no norms or shadows, reads or
 * posts no repair feedback, keeps no state in the handle and changes nothing a later call on the handle does.
 *
 * Refused before any device call, in this order: mvfgpu_search_radius' checks that need no handle, with its codes and messages
 * (nq = 0; NULL queries, radii or out_counts; NULL out_scores / out_indices when max_per_query > 0); max_per_query above
 * MVFGPU_K_PER_PASS with MVF_ERR_INVALID_ARGUMENT ("max_per_query above 1024 is not built for Hamming radius search"); a NULL
 * corpus; a handle that is not UInt8 with MVF_ERR_BUILD; `dimension` above 512 with MVF_ERR_INVALID_ARGUMENT ("rows above 512
 * packed bytes are not built for Hamming radius search"); a query type other than UInt8 (MVF_ERR_BUILD);
 * query_dim != dimension (MVF_ERR_DIMENSION_MISMATCH).
 *
 * The call blocks, like mvfgpu_search_radius, and stages its queries, radii and results in windows with mvfgpu_search_device's
 * stream discipline.  Three launches per 1024 queries.  A query with more than MVFGPU_RADIUS_LIST_CAP matches that wants
 * entries is completed with one mvfgpu_search_hamming over all such queries (its entries are its top-max_per_query).
 *
 * Not built: a device-resident asynchronous call; rows above 512 packed bytes; max_per_query above 1024; shard sets; filters
 * and partitions; a VALU form.  The self-join ("all duplicate pairs") is mvfgpu_hamming_pairs (mvf_gpu_hamming_pairs.h).
 */
int mvfgpu_search_hamming_radius(const mvfgpu_corpus* corpus, const void* queries, uint8_t query_dtype, uint32_t query_dim,
                                 uint32_t nq, const uint32_t* radii, uint64_t max_per_query, uint64_t* out_counts,
                                 float* out_scores, uint64_t* out_indices, int32_t* out_raw);
/*
 * Self-test of the search's form (no GPU, no handle): the decision the launch itself takes for rows of `dimension` packed bytes,
 * nq queries in a window (1 .. ; a window holds 1024 at most) and `rows` rows on a part of num_cus compute units (0: 256).
 * *out_query_tile = queries a scan block holds in LDS: the smallest of 16, 32, 64, 128 that holds the window's, at most 128 for
 * rows of up to 256 bytes, 64 up to 512; *out_blocks_per_cu = blocks the slice rule gives a compute unit: what the tile's LDS
 * admits of 160 KiB, 8 at most; *out_row_slices = row ranges the scan is split into: blocks per CU x CUs over the query tiles,
 * slices of 1024 rows at least, no other cap (0 for no rows); *out_chunks = 64-byte chunks of a row; *out_lds_bytes = LDS of a
 * scan block; *out_scratch_bytes = a window's device scratch where entries are asked for.  Any output may be NULL.  Refused
 * with MVF_ERR_INVALID_ARGUMENT: dimension 0 or above 512, nq = 0, rows above 2^32 - 65536.
 */
int mvfgpu_selftest_hamming_radius_form(uint32_t dimension, uint32_t nq, uint64_t rows, uint32_t num_cus, uint32_t* out_query_tile,
                                        uint32_t* out_row_slices, uint32_t* out_blocks_per_cu, uint32_t* out_chunks,
                                        uint32_t* out_lds_bytes, uint64_t* out_scratch_bytes);
/*
 * Stage timer (scripts/probe_hamming_radius.py): the search's device work on resident queries, radii (u32 [nq]) and outputs,
 * with events around its launches, on hip_stream; waits for the stream and completes no overflowed query.
 * out_ms[0..2] = prepare (HQ), scan (HR2), pack (HRP), each summed over the call's windows.  Refused beside the search's own
 * refusals: a NULL out_ms.
 */
int mvfgpu_selftest_hamming_radius_stage_ms(const mvfgpu_corpus* corpus, const void* d_queries, uint8_t query_dtype, uint32_t query_dim,
                                            uint32_t nq, const uint32_t* d_radii, uint64_t max_per_query, uint64_t* d_counts,
                                            float* d_scores, uint64_t* d_indices, int32_t* d_raw, void* hip_stream, float* out_ms);

#ifdef __cplusplus
}
#endif
#endif
