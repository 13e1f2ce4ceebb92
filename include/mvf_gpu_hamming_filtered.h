/*
 * mvf_gpu_hamming_filtered.h — C ABI of libmvf_gpu.so, continued: the exact Hamming top-k among the bit-packed rows a filter
 * admits.  The functions are additions to ABI version 3.
 */
#ifndef MVF_GPU_HAMMING_FILTERED_H
#define MVF_GPU_HAMMING_FILTERED_H

#include "mvf_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Filtered Hamming search ("Filtered Hamming search", section 5 "HG"): mvfgpu_search_hamming
 * (mvf_gpu_hamming.h) restricted to the rows `filter` admits -- a filter of this handle from mvfgpu_filter_create,
 * mvfgpu_filter_create_device or mvfgpu_filter_create_where.  The answer is exactly mvfgpu_search_hamming's on a twin handle
 * whose tombstones are `deleted | ~allow`: d = sum of popcount(q ^ x), an exact i32, out_scores = (float)d, out_raw (nullable)
 * = d, the k smallest, ties by ascending row POSITION, indices index_base + row or the row's vector id; k beyond the admitted
 * live rows pads with index UINT64_MAX, score +inf, raw 0 (a filter that admits nothing, or an empty corpus: all padding).  The
 * answer never depends on the bytes of a row's pitch padding.
 *
 * Two routes, the same bytes:
 *   mask  the Hamming search's own scan -- H0, or HQ / H2 where the handle's Hamming route says so -- with the filter's deny mask
 *         in the tombstones' place: every row is read;
 *   list  HG: H2's arithmetic over the filter's ascending row list, so that only admitted rows are read.  Eligible: rows of up to
 *         512 packed bytes, a filter that holds its row list (mvfgpu_filter_info.has_row_list), at least one admitted row.
 * The filter's forced route (MVF_FILTER_ROUTE when the handle read its tuning) decides where the list route is eligible;
 * otherwise the rule of mvfgpu_selftest_hamming_filtered_form does.
 *
 * Refused before any device call, in this order: mvfgpu_search's checks that need no handle, with its codes and messages
 * (nq = 0, k outside 1 .. MVFGPU_MAX_K, a NULL buffer); k above MVFGPU_K_PER_PASS with MVF_ERR_INVALID_ARGUMENT ("k above 1024
 * is not built for filtered Hamming search"); a NULL filter ("filter is NULL"); a NULL corpus; a handle that is not UInt8 with
 * MVF_ERR_BUILD; mvfgpu_search's checks of the query: a type other than UInt8 (MVF_ERR_BUILD), query_dim != dimension
 * (MVF_ERR_DIMENSION_MISMATCH); a filter created for another handle, then a stale filter, with mvfgpu_search_filtered's messages.
 *
 * The host call blocks and stages its queries and results in windows; the device call takes resident queries and outputs, is
 * asynchronous on hip_stream and makes no host wait.  Both keep mvfgpu_search_device's stream discipline.  Nothing is kept in
 * the handle or the filter, no norms or shadows are built and no repair feedback is read or posted.  Per 1024 queries: the
 * mask route's launches are the Hamming search's, the list route's are three.
 *
 * Not built: k above 1024; shard sets; filters for the sign-bit, Tanimoto, Hamming radius and binary MaxSim searches;
 * partitions and candidate lists under Hamming; the list route for rows above 512 bytes.
 */
int mvfgpu_search_hamming_filtered(const mvfgpu_corpus* corpus, const mvfgpu_filter* filter, const void* queries, uint8_t query_dtype,
                                   uint32_t query_dim, uint32_t nq, uint32_t k, float* out_scores, uint64_t* out_indices,
                                   int32_t* out_raw);
int mvfgpu_search_hamming_filtered_device(const mvfgpu_corpus* corpus, const mvfgpu_filter* filter, const void* d_queries,
                                          uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t k, float* d_scores,
                                          uint64_t* d_indices, int32_t* d_raw, void* hip_stream);
/*
 * Self-test of the route and of the list route's form (no GPU, no handle): the decisions the launch itself takes for one window
 * of nq queries (a window holds 1024 at most) over `rows` rows of `dimension` packed bytes under a filter that admits `admitted`
 * of them and holds its row list or not (has_row_list 0 / 1), with forced_route 0 (automatic), 1 (mask) or 2 (list), on a part
 * of num_cus compute units (0: 256).  *out_route = 1 mask, 2 list.  Automatic: the list only in the shapes in which it was
 * measured ahead -- from 10M rows of at least 64 bytes on, k up to 128, a filter that admits a tenth of the rows at most.
 * On route 2 the rest describes HG: *out_query_tile = queries a block holds in LDS (the smallest of 16, 32, 64, 128 that
 * holds the window's, at most 128 up to a 256-byte pitch and 64 beyond), *out_chunks = 64-byte chunks of a row,
 * *out_list_slices = ranges the list is split into, *out_slice_entries = list entries of a slice (1024 at least),
 * *out_lds_bytes = LDS of a scan block, *out_scratch_bytes = the candidate buffers.  On route 1 they are all 0: mvfgpu_selftest_hamming_form and mvfgpu_selftest_hamming_mfma_form describe the mask route.  Any
 * output may be NULL.  Refused with MVF_ERR_INVALID_ARGUMENT: dimension 0 or above MVFGPU_MAX_INT_DIM, nq = 0, k outside
 * 1 .. MVFGPU_K_PER_PASS, rows above 2^32 - 65536, admitted above rows, has_row_list above 1, forced_route outside 0 .. 2.
 */
int mvfgpu_selftest_hamming_filtered_form(uint32_t dimension, uint32_t nq, uint32_t k, uint64_t rows, uint64_t admitted,
                                          uint32_t has_row_list, int forced_route, uint32_t num_cus, uint32_t* out_route,
                                          uint32_t* out_query_tile, uint32_t* out_chunks, uint32_t* out_list_slices,
                                          uint64_t* out_slice_entries, uint32_t* out_lds_bytes, uint64_t* out_scratch_bytes);
/*
 * Stage timer (scripts/probe_hamming_filtered.py): mvfgpu_search_hamming_filtered_device with events around its launches;
 * waits for the stream.  out_ms[0..2] = prepare, scan, merge, each summed over the call's windows: HQ, HG, H1 on the list
 * route; 0, H0 (or HQ + H2), H1 on the mask route.  Refused beside the search's own refusals: a NULL out_ms.
 */
int mvfgpu_selftest_hamming_filtered_stage_ms(const mvfgpu_corpus* corpus, const mvfgpu_filter* filter, const void* d_queries,
                                              uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t k, float* d_scores,
                                              uint64_t* d_indices, int32_t* d_raw, void* hip_stream, float* out_ms);

#ifdef __cplusplus
}
#endif
#endif
