/*
 * mvf_gpu_hamming_maxsim.h — C ABI of libmvf_gpu.so, continued: binary MaxSim, the multi-vector search over bit-packed rows by
 * summed per-token best Hamming distance.  The functions are additions to ABI version 3.
 */
#ifndef MVF_GPU_HAMMING_MAXSIM_H
#define MVF_GPU_HAMMING_MAXSIM_H

#include "mvf_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Binary MaxSim ("Binary MaxSim", section 5 "B0"): late interaction over binarised token embeddings -- a
 * ColBERT or ColPali token of 128 dimensions is 16 bytes, a page of about 1000 patches 16 KB.  The handle is the Hamming
 * search's, a UInt8 corpus whose `dimension` is the number of packed BYTES of a row, 1 .. 512, and the partition index is the
 * multi-vector search's: a key is a document, its rows the document's tokens.  Queries are UInt8, [nq][n_tokens][dimension],
 * contiguous; n_tokens is 1 .. MVFGPU_MAXSIM_MAX_TOKENS and the same for every set.  With
 *   d(t, x) = mvfgpu_search_hamming's exact distance of token t and row x (the first `dimension` bytes; never the pitch behind),
 *   b(t, g) = the minimum of d(t, x) over the rows the partition holds for key g,
 *   S(g)    = the sum of b(t, g) over the set's tokens, an exact integer <= 1024 x 4096 = 2^22,
 * a result row is the k keys of SMALLEST S, ties by ascending key value (the order of mvfgpu_partition_keys):
 * out_scores = (float)S, exact; out_keys = the column value zero-extended to 64 bits; entries from min(k, n_keys) on are padding,
 * key UINT64_MAX and score +inf; out_counts[q] (nullable) = min(k, n_keys).  k is 1 .. MVFGPU_MAX_K.  No rows, no held rows or no
 * keys: rows of padding and counts of 0.
 *
 * The arithmetic runs on v_mfma_scale_f32_16x16x128_f8f6f4 with exact 0 / +1 / -1 FP4 factors and is integer-exact throughout:
 * there is no bound, no repair path and no second pass, and a result does not depend on the window or chunk sizes.  The call
 * keeps nothing in the handle and reads or posts no repair feedback.  Its scratch per window of query sets stays inside the
 * handle's MVF_MAXSIM_SCRATCH_BYTES: per set n_keys x (4 x tokens of a chunk + 20) bytes and the set's prepared tokens
 * (n_tokens x (256 x chunks of a row + 4) bytes); one token group and one set whatever the budget.  Launches: the ordinals and
 * one clear per call; one preparation and the tail per window; the scan and the sums per chunk of tokens.
 *
 * Refused before any device call, in this order: mvfgpu_search_maxsim's nq, k and NULL-buffer checks with its codes and messages;
 * n_tokens out of range (its message); a NULL partition, then a NULL corpus; a handle that is not UInt8 (MVF_ERR_BUILD);
 * `dimension` above 512 with MVF_ERR_INVALID_ARGUMENT ("rows above 512 packed bytes are not built for binary MaxSim"); a query
 * type other than UInt8 (MVF_ERR_BUILD); query_dim != dimension (MVF_ERR_DIMENSION_MISMATCH); a partition of another handle or of
 * an older tombstone generation, with the partitioned search's messages.
 *
 * The host call blocks and stages its query sets and results in windows; the device call takes resident queries and outputs, is
 * asynchronous on hip_stream and makes no host wait.  Both keep mvfgpu_search_device's stream discipline.
 *
 * Not built: rows above 512 packed bytes; a VALU form; candidate-key re-ranking and alignments for binary rows; asymmetric
 * (int8-token) MaxSim; ragged token counts; shard sets; an automatic route inside mvfgpu_search_maxsim.
 */
int mvfgpu_search_hamming_maxsim(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, const void* queries, uint8_t query_dtype,
                                 uint32_t query_dim, uint32_t nq, uint32_t n_tokens, uint32_t k, float* out_scores, uint64_t* out_keys,
                                 uint32_t* out_counts);
int mvfgpu_search_hamming_maxsim_device(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, const void* d_queries,
                                        uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t n_tokens, uint32_t k,
                                        float* d_scores, uint64_t* d_keys, uint32_t* d_counts, void* hip_stream);
/*
 * Self-test of the search's form (no GPU, no handle): the decisions the launch itself takes for rows of `dimension` packed bytes,
 * nq query sets of n_tokens tokens, n_keys keys over held_rows rows and a scratch budget of budget_bytes (the handle's
 * MVF_MAXSIM_SCRATCH_BYTES); num_cus is not read (the scan's grid follows the list, not the part).
 * *out_query_tile = query rows one pass of the scan scores against a block's rows; *out_chunks = 64-byte chunks of a row;
 * *out_rows_in_registers = 1 where a lane's words of its rows stay in registers over every pass of a launch (a pitch of up to 64
 * bytes), 0 where they are loaded again per pass; *out_chunk_tokens = tokens per chunk; *out_window_sets = query sets per window;
 * *out_lds_bytes = LDS of a scan block; *out_scratch_bytes = what the budget holds (above).  Any output may be NULL.  Refused
 * with MVF_ERR_INVALID_ARGUMENT: dimension 0 or above 512, nq = 0, n_tokens out of range, held_rows above 2^32 - 65536,
 * n_keys above held_rows.
 */
int mvfgpu_selftest_hamming_maxsim_form(uint32_t dimension, uint32_t nq, uint32_t n_tokens, uint64_t n_keys, uint64_t held_rows,
                                        uint64_t budget_bytes, uint32_t num_cus, uint32_t* out_query_tile, uint32_t* out_chunks,
                                        uint32_t* out_rows_in_registers, uint32_t* out_chunk_tokens, uint32_t* out_window_sets,
                                        uint32_t* out_lds_bytes, uint64_t* out_scratch_bytes);
/*
 * Stage timer (scripts/probe_hamming_maxsim.py): mvfgpu_search_hamming_maxsim_device with events around its launches; waits for
 * the stream.  out_ms[0..3] = prepare (the ordinals, the clear, HQ), scan (B0), sum, tail, each summed over the call's chunks and
 * windows.  Refused beside the search's own refusals: a NULL out_ms; a handle or partition without held rows.
 */
int mvfgpu_selftest_hamming_maxsim_stage_ms(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, const void* d_queries,
                                            uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t n_tokens, uint32_t k,
                                            float* d_scores, uint64_t* d_keys, uint32_t* d_counts, void* hip_stream, float* out_ms);

#ifdef __cplusplus
}
#endif
#endif
