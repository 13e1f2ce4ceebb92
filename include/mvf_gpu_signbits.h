/*
 * mvf_gpu_signbits.h — C ABI of libmvf_gpu.so, continued: sign-bit search, the exact top-k of Int8 queries against bit-packed
 * rows.  The functions are additions to ABI version 3.
 */
#ifndef MVF_GPU_SIGNBITS_H
#define MVF_GPU_SIGNBITS_H

#include "mvf_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Sign-bit search ("Sign-bit search", section 5 "SQ / S2"): the asymmetric use of a binary-quantised corpus.
 * The rows are those of an ordinary UInt8 corpus whose `dimension` is the number of packed BYTES of a row, 1 .. 512 -- the
 * handles mvfgpu_search_hamming takes, so one upload serves both calls.  Element e = 8 i + b of a row is bit b of its byte i
 * (pack_sign_bits' order; unlike under Hamming the order matters).  Queries are Int8, [nq][8 x dimension], contiguous; an
 * embedding whose length is no multiple of 8 is padded with zero elements by the caller, and a zero element scores 0 whatever
 * the bit.
 *   s(q, x) = sum over the elements e of q[e] * (bit e of x ? +1 : -1), an exact i32 with |s| <= 128 x 4096 = 524288 < 2^24.
 * The k rows of LARGEST s per query, ties by ascending row POSITION, deleted rows never: out_raw (nullable) = s,
 * out_scores = (float)s (exact), out_indices = index_base + row, or the row's vector id where ids are attached.  k beyond the
 * live rows pads as an InnerProduct mvfgpu_search does: index UINT64_MAX, score -inf, raw 0.
 *
 * The recipe this call replaces: the answer has the indices and raw values of an InnerProduct mvfgpu_search with the same Int8
 * queries over an Int8 handle holding the rows unpacked to +1 / -1, at an eighth of that handle's bytes.
 *
 * The answer never depends on the bytes behind `dimension` in a row's pitch.  The call builds no norms or shadows, reads or
 * posts no repair feedback, keeps no state in the handle and changes nothing a later call on the handle does.
 *
 * Refused before any device call, in this order: mvfgpu_search's checks that need no handle, with its codes and messages
 * (nq = 0, k outside 1 .. MVFGPU_MAX_K, a NULL buffer); k above MVFGPU_K_PER_PASS with MVF_ERR_INVALID_ARGUMENT ("k above 1024
 * is not built for sign-bit search"); a NULL corpus; a handle that is not UInt8 with MVF_ERR_BUILD; `dimension` above 512 with
 * MVF_ERR_INVALID_ARGUMENT ("rows above 512 packed bytes are not built for sign-bit search"); a query type other than Int8
 * (MVF_ERR_BUILD); query_dim != 8 x dimension (MVF_ERR_DIMENSION_MISMATCH).
 *
 * The host call blocks and stages its queries and results in windows (as mvfgpu_search_hamming does); the device call takes
 * resident queries and outputs, is asynchronous on hip_stream and makes no host wait.  Both keep mvfgpu_search_device's stream
 * discipline.  Three launches per 1024 queries, whatever k.
 *
 * Not built: rows above 512 packed bytes; k above 1024; Float32 queries on the device (quantise on the host:
 * quantize_queries_int8); shard sets; filters, partitions and candidate lists taking this score; a VALU form for long rows; an
 * automatic two-stage call (this search, then a re-ranking of its hits on the float rows).
 */
int mvfgpu_search_signbits(const mvfgpu_corpus* corpus, const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                           uint32_t k, float* out_scores, uint64_t* out_indices, int32_t* out_raw);
int mvfgpu_search_signbits_device(const mvfgpu_corpus* corpus, const void* d_queries, uint8_t query_dtype, uint32_t query_dim,
                                  uint32_t nq, uint32_t k, float* d_scores, uint64_t* d_indices, int32_t* d_raw, void* hip_stream);
/*
 * Self-test of the search's form (no GPU, no handle): the decision the launch itself takes for rows of `dimension` packed bytes,
 * nq queries in a window (1 .. ; a window holds 1024 at most), k and `rows` rows on a part of num_cus compute units (0: 256).
 * *out_query_tile = queries a scan block holds in LDS: the smallest of 16, 32, 64, 128 that holds the window's, at most 128 for
 * rows of up to 128 bytes, 64 up to 256, 32 up to 512; *out_row_slices = row ranges the scan is split into (0 for no rows);
 * *out_chunks = 64-byte chunks of a row; *out_lds_bytes = LDS of a scan block; *out_scratch_bytes = the candidate buffers.  Any
 * output may be NULL.  Refused with MVF_ERR_INVALID_ARGUMENT: dimension 0 or above 512, nq = 0, k outside
 * 1 .. MVFGPU_K_PER_PASS, rows above 2^32 - 65536.
 */
int mvfgpu_selftest_signbits_form(uint32_t dimension, uint32_t nq, uint32_t k, uint64_t rows, uint32_t num_cus, uint32_t* out_query_tile,
                                  uint32_t* out_row_slices, uint32_t* out_chunks, uint32_t* out_lds_bytes, uint64_t* out_scratch_bytes);
/*
 * Stage timer (scripts/probe_signbits.py): mvfgpu_search_signbits_device with events around its launches; waits for the stream.
 * out_ms[0..2] = prepare (SQ), scan (S2), merge (H1), each summed over the call's windows.  Refused beside the search's own
 * refusals: a NULL out_ms.
 */
int mvfgpu_selftest_signbits_stage_ms(const mvfgpu_corpus* corpus, const void* d_queries, uint8_t query_dtype, uint32_t query_dim,
                                      uint32_t nq, uint32_t k, float* d_scores, uint64_t* d_indices, int32_t* d_raw,
                                      void* hip_stream, float* out_ms);

#ifdef __cplusplus
}
#endif
#endif
