/*
 * mvf_gpu_hamming.h — C ABI of libmvf_gpu.so, continued: exact top-k by Hamming distance over bit-packed rows.  The functions
 * are additions to ABI version 3.  Their stream classes ("Stream discipline") are listed in
 * tests/_hamming.py.
 */
#ifndef MVF_GPU_HAMMING_H
#define MVF_GPU_HAMMING_H

#include "mvf_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Hamming search ("Hamming search", section 5 "H0 / H1"): binary embeddings, 1 bit per dimension, are
 * the rows of an ordinary UInt8 corpus whose `dimension` is the number of packed BYTES of a row, 1 .. MVFGPU_MAX_INT_DIM; a row
 * holds 8 x dimension bits, and the order of the bits inside a byte does not matter.  Queries are UInt8, [nq][dimension],
 * contiguous.
 *   d(q, x) = sum over the bytes i of popcount(q[i] ^ x[i]), an exact i32 of at most 264 200.
 * The k rows of smallest d per query, ties by ascending row POSITION, deleted rows never: out_raw (nullable) = d,
 * out_scores = (float)d (exact), out_indices = index_base + row, or the row's vector id where ids are attached.  k beyond the
 * live rows pads as an L2 mvfgpu_search on the handle does: index UINT64_MAX, score +inf, raw 0.
 * The answer does not depend on the bytes of a row's pitch padding, and the metric enum of mvf_gpu.h has no Hamming entry: this
 * call is the route.
 *
 * Refused before any device call, in this order: mvfgpu_search's checks that need no handle, with its codes and messages
 * (nq = 0, k outside 1 .. MVFGPU_MAX_K, a NULL buffer); k above MVFGPU_K_PER_PASS with MVF_ERR_INVALID_ARGUMENT ("k above 1024
 * is not built for Hamming search"); a NULL corpus; a handle that is not UInt8 with MVF_ERR_BUILD; then mvfgpu_search's checks
 * of the query: a type other than UInt8 (MVF_ERR_BUILD), query_dim != dimension (MVF_ERR_DIMENSION_MISMATCH).
 *
 * The host call blocks and stages its queries and results in windows (as mvfgpu_search_candidates does); the device call takes
 * resident queries and outputs, is asynchronous on hip_stream and makes no host wait.  Both keep mvfgpu_search_device's stream
 * discipline.  Neither builds norms or shadows, reads or posts the repair feedback, or changes what a later call on the handle
 * does.  Two launches per 1024 queries, whatever k.
 *
 * Not built: k above 1024; shard sets; partitions and candidate lists taking this metric; Int8 handles; a binary
 * shadow for the float routes.  (Filters: mvf_gpu_hamming_filtered.h; radius search under Hamming: mvf_gpu_hamming_radius.h;
 * Jaccard / Tanimoto: mvf_gpu_tanimoto.h.)
 */
int mvfgpu_search_hamming(const mvfgpu_corpus* corpus, const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                          uint32_t k, float* out_scores, uint64_t* out_indices, int32_t* out_raw);
int mvfgpu_search_hamming_device(const mvfgpu_corpus* corpus, const void* d_queries, uint8_t query_dtype, uint32_t query_dim,
                                 uint32_t nq, uint32_t k, float* d_scores, uint64_t* d_indices, int32_t* d_raw, void* hip_stream);
/*
 * Self-test of the search's form (no GPU, no handle): the decision the launch itself takes for rows of `dimension` packed bytes,
 * nq queries in a window (1 .. ; a window holds 1024 at most), k and `rows` rows on a part of num_cus compute units (0: 256).
 * *out_form = 0 register form (pitch up to 256 bytes: a lane keeps its 16-byte step of the row in registers), 1 streaming form;
 * *out_lanes_per_row = lanes of a row's group; *out_query_tile = queries a block holds in LDS; *out_row_slices = row ranges the
 * scan is split into (0 for no rows); *out_lds_bytes = LDS of a scan block; *out_merge_entries = list entries H1 merges per
 * query at most (row slices x next_pow2(k) stays inside it).  Any output may be NULL.  Refused with MVF_ERR_INVALID_ARGUMENT:
 * dimension 0 or above MVFGPU_MAX_INT_DIM, nq = 0, k outside 1 .. MVFGPU_K_PER_PASS, rows above 2^32 - 65536.
 */
int mvfgpu_selftest_hamming_form(uint32_t dimension, uint32_t nq, uint32_t k, uint64_t rows, uint32_t num_cus, uint32_t* out_form,
                                 uint32_t* out_lanes_per_row, uint32_t* out_query_tile, uint32_t* out_row_slices,
                                 uint32_t* out_lds_bytes, uint32_t* out_merge_entries);
/*
 * Stage timer (scripts/probe_hamming.py): mvfgpu_search_hamming_device with events around its launches; waits for the stream.
 * out_ms[0..1] = H0, H1, each summed over the call's windows.  Refused beside the search's own refusals: a NULL out_ms.
 */
int mvfgpu_selftest_hamming_stage_ms(const mvfgpu_corpus* corpus, const void* d_queries, uint8_t query_dtype, uint32_t query_dim,
                                     uint32_t nq, uint32_t k, float* d_scores, uint64_t* d_indices, int32_t* d_raw,
                                     void* hip_stream, float* out_ms);

#ifdef __cplusplus
}
#endif
#endif
