/*
 * mvf_gpu_hamming_pairs.h — C ABI of libmvf_gpu.so, continued: the Hamming pair join, every two rows of one bit-packed corpus
 * within r bits of each other.  The functions are additions to ABI version 3.
 */
#ifndef MVF_GPU_HAMMING_PAIRS_H
#define MVF_GPU_HAMMING_PAIRS_H

#include "mvf_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MVFGPU_HAMMING_PAIRS_MAX (1ull << 24) /* listed pairs of one call at most */

/*
 * Hamming pair join ("Hamming pair join", section 5 "HJ / HJP"): the deduplication workload of SimHash /
 * MinHash / perceptual-hash codes -- "all near-duplicate pairs of this corpus" -- in one call on the resident rows.  The handle
 * is mvfgpu_search_hamming_radius': a UInt8 corpus whose `dimension` is the number of packed BYTES of a row, here 1 .. 512.
 *
 * A pair is two live (not tombstoned) rows at positions i < j with d(x_i, x_j) <= radius (inclusive), d the Hamming search's
 * exact i32.  A radius of 8 x dimension or more pairs every two live rows.  A row is never paired with itself; exact copies at
 * different positions are pairs with d = 0.  The answer never depends on the bytes behind `dimension` in a row's pitch.
 *   *out_total (required) = the exact number of pairs, whatever max_pairs is.
 *   out_degrees (nullable): u32 [rows] by row position: for a live row the number of OTHER live rows within the radius, 0 for
 *   a deleted row; the degrees sum to 2 x total.
 *   out_first, out_second (u64 [max_pairs]), out_raw (i32 [max_pairs], nullable), *out_listed (required): if
 *   total <= max_pairs the three arrays hold every pair, ascending by (i, j) POSITION, each row reported as every search reports
 *   it -- index_base + position, or its vector id where ids are attached --, out_raw = d, and *out_listed = total.  Otherwise
 *   *out_listed = 0 and the arrays are not written: the caller knows the total and calls again with room (the size-query
 *   idiom).  max_pairs = 0 asks for the total and the degrees only, and the three arrays may then be NULL.  max_pairs is
 *   MVFGPU_HAMMING_PAIRS_MAX at most.
 *
 * The recipe this call replaces: the packed rows read back and fed to mvfgpu_search_hamming_radius as queries, 1024 at a time.
 * That scores every pair twice, finds every row at distance 0 from itself, stages queries and results per window and completes
 * a query with more than 8192 matches by a top-k search.  Here both operands are resident, only the upper triangle is scored
 * and the answer is one list.  degrees[i] = that search's count for row i, minus the row itself.
 *
 * Refused before any device call, in this order: a NULL out_total or out_listed (MVF_ERR_INVALID_ARGUMENT, "NULL buffer"); a
 * NULL out_first or out_second with max_pairs > 0 (MVF_ERR_INVALID_ARGUMENT); max_pairs above MVFGPU_HAMMING_PAIRS_MAX
 * (MVF_ERR_INVALID_ARGUMENT, "max_pairs above 2^24 is not built for the Hamming pair join"); a NULL corpus; a handle that is
 * not UInt8 (MVF_ERR_BUILD); `dimension` above 512 (MVF_ERR_INVALID_ARGUMENT, "rows above 512 packed bytes are not built for
 * the Hamming pair join").
 *
 * The call blocks, like mvfgpu_search_hamming_radius, on the handle's host-call stream with mvfgpu_search_device's stream
 * discipline; it waits once for the total before it orders the list.  It builds no norms or shadows, reads or posts no repair
 * feedback, keeps no state in the handle and changes nothing a later call on the handle does.  All scratch is per call.
 *
 * Not built: rows above 512 packed bytes; more than 2^24 listed pairs; a join of two handles; shard sets; filters; an
 * asynchronous device call; Tanimoto pairs.
 */
int mvfgpu_hamming_pairs(const mvfgpu_corpus* corpus, uint32_t radius, uint64_t max_pairs, uint64_t* out_total,
                         uint32_t* out_degrees, uint64_t* out_first, uint64_t* out_second, int32_t* out_raw,
                         uint64_t* out_listed);
/*
 * Self-test of the join's form (no GPU, no handle): the decisions the launch itself takes for `rows` rows of `dimension` packed
 * bytes on a part of num_cus compute units (0: 256).  The corpus is cut into column tiles of *out_query_tile consecutive rows,
 * which a scan block expands into LDS (the smallest of 16, 32, 64, 128 that holds the rows, at most 128 for rows of up to 256
 * bytes, 64 up to 512), and into spans of *out_span_rows rows (a multiple of 256, 1024 .. 8192), which it streams against the
 * tile; one block per (tile, span) whose span holds a row position above the tile's first.  *out_chunks = 64-byte chunks of a
 * row; *out_tiles, *out_spans = the number of column tiles and of spans; *out_blocks = launched (tile, span) pairs;
 * *out_lds_bytes = LDS of a scan block; *out_scratch_bytes = the call's device scratch where max_pairs pairs are asked for and
 * found; *out_block_tile, *out_block_span = the (tile, span) of block `block_index` of the 1-D grid, through the function the
 * kernel decodes its own index with.  Any output may be NULL.  Refused with MVF_ERR_INVALID_ARGUMENT: dimension 0 or above 512,
 * rows above 2^32 - 65536, max_pairs above MVFGPU_HAMMING_PAIRS_MAX, and a block's place asked for with block_index >=
 * *out_blocks.
 */
int mvfgpu_selftest_hamming_pairs_form(uint32_t dimension, uint64_t rows, uint32_t num_cus, uint64_t max_pairs, uint64_t block_index,
                                       uint32_t* out_query_tile, uint32_t* out_chunks, uint32_t* out_span_rows, uint64_t* out_tiles,
                                       uint64_t* out_spans, uint64_t* out_blocks, uint32_t* out_lds_bytes, uint64_t* out_scratch_bytes,
                                       uint64_t* out_block_tile, uint64_t* out_block_span);
/*
 * Stage timer (scripts/probe_hamming_pairs.py): the join with its degrees and its list written to DEVICE buffers (d_degrees,
 * d_raw nullable; d_first / d_second required when max_pairs > 0), events around its stages, on hip_stream; out_total and
 * out_listed are host words.  Waits for the stream.  out_ms[0..1] = scan (the counters' clear and HJ), order (HJP: the radix
 * passes and the writer; 0 where nothing is listed).  Refused beside the join's own refusals: a NULL out_ms.
 */
int mvfgpu_selftest_hamming_pairs_stage_ms(const mvfgpu_corpus* corpus, uint32_t radius, uint64_t max_pairs, uint64_t* out_total,
                                           uint32_t* d_degrees, uint64_t* d_first, uint64_t* d_second, int32_t* d_raw,
                                           uint64_t* out_listed, void* hip_stream, float* out_ms);

#ifdef __cplusplus
}
#endif
#endif
