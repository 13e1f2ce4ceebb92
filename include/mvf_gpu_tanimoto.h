/*
 * mvf_gpu_tanimoto.h — C ABI of libmvf_gpu.so, continued: Tanimoto search, the exact top-k by Jaccard / Tanimoto similarity over
 * bit-packed rows.  The functions are additions to ABI version 3.
 */
#ifndef MVF_GPU_TANIMOTO_H
#define MVF_GPU_TANIMOTO_H

#include "mvf_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Tanimoto search ("Tanimoto search", section 5 "TQ / T2"): the metric of molecular fingerprints, MinHash
 * bitmaps and set-valued features.  The rows are those of an ordinary UInt8 corpus whose `dimension` is the number of packed
 * BYTES of a row, 1 .. 512 -- the handles mvfgpu_search_hamming takes, so one upload serves both calls.  Queries are UInt8,
 * [nq][dimension], contiguous.  With a = popcount(q), b = popcount(x), c = popcount(q & x) and u = a + b - c = popcount(q | x):
 *   T(q, x) = c / u  for u > 0,   T = 0  for u = 0
 * -- an empty query against an empty row matches nothing (chemfp's convention).  The k live rows of LARGEST T per query, ties by
 * ascending row POSITION, deleted rows never: out_scores = T, out_indices = index_base + row, or the row's vector id where ids
 * are attached.  k beyond the live rows pads with index UINT64_MAX and score -inf.  There is no out_raw.
 *
 * The score and the order key are one IEEE float, T = the correctly rounded f32 quotient (float)c / (float)u:
 *   - u <= 8 x dimension <= 4096, so two distinct values c1/u1 != c2/u2 differ by at least 1 / (u1 u2) > 2^-24, while a
 *     correctly rounded quotient in (0, 1] is within 2^-25 of its rational: the rounding is strictly monotone and injective on
 *     the exact rationals, and equal fractions (1/2 and 2/4) give equal floats;
 *   - the bits of a non-negative float are monotone as u32, so key = 0x3F800000 - bits(T), 0 for T = 1, orders as T does with
 *     smaller better, and fits the Hamming search's composite key << 32 | row;
 *   - the Hamming search's exact selection rule "below the k-th composite" therefore carries "largest T first, ties by position";
 *   - the float written to out_scores is that T: what is returned is what was ordered by.
 *
 * The answer never depends on the bytes behind `dimension` in a row's pitch or on the bit order inside a byte.  The call builds
 * no per-handle state (no row popcounts, no norms or shadows), reads or posts no repair feedback and changes nothing a later
 * call on the handle does; row writes, tombstones and ids need nothing from it.
 *
 * Refused before any device call, in the sign-bit search's order: mvfgpu_search's checks that need no handle, with its codes and
 * messages (nq = 0, k outside 1 .. MVFGPU_MAX_K, a NULL buffer); k above MVFGPU_K_PER_PASS with MVF_ERR_INVALID_ARGUMENT ("k
 * above 1024 is not built for Tanimoto search"); a NULL corpus; a handle that is not UInt8 with MVF_ERR_BUILD; `dimension` above
 * 512 with MVF_ERR_INVALID_ARGUMENT ("rows above 512 packed bytes are not built for Tanimoto search"); a query type other than
 * UInt8 (MVF_ERR_BUILD); query_dim != dimension (MVF_ERR_DIMENSION_MISMATCH).
 *
 * The host call blocks and stages its queries and results in windows (as mvfgpu_search_hamming does); the device call takes
 * resident queries and outputs, is asynchronous on hip_stream and makes no host wait.  Both keep mvfgpu_search_device's stream
 * discipline.  Three launches per 1024 queries, whatever k.
 *
 * Not built: rows above 512 packed bytes; k above 1024; a similarity threshold / radius form; Tversky and Dice; shard sets;
 * filters, partitions and candidate lists taking this metric; returning c and u.
 */
int mvfgpu_search_tanimoto(const mvfgpu_corpus* corpus, const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                           uint32_t k, float* out_scores, uint64_t* out_indices);
int mvfgpu_search_tanimoto_device(const mvfgpu_corpus* corpus, const void* d_queries, uint8_t query_dtype, uint32_t query_dim,
                                  uint32_t nq, uint32_t k, float* d_scores, uint64_t* d_indices, void* hip_stream);
/*
 * Self-test of the search's form (no GPU, no handle): the decision the launch itself takes for rows of `dimension` packed bytes,
 * nq queries in a window (1 .. ; a window holds 1024 at most), k and `rows` rows on a part of num_cus compute units (0: 256).
 * *out_query_tile = queries a scan block holds in LDS: the smallest of 16, 32, 64, 128 that holds the window's, at most 128 for
 * rows of up to 256 bytes and 64 beyond; *out_chunks = 64-byte chunks of a row; *out_row_slices = row ranges the scan is split
 * into (0 for no rows); *out_slice_rows = rows of a range; *out_lds_bytes = LDS of a scan block; *out_scratch_bytes = the
 * candidate buffers.  Any output may be NULL.  Refused with MVF_ERR_INVALID_ARGUMENT: dimension 0 or above 512, nq = 0, k outside
 * 1 .. MVFGPU_K_PER_PASS, rows above 2^32 - 65536.
 */
int mvfgpu_selftest_tanimoto_form(uint32_t dimension, uint32_t nq, uint32_t k, uint64_t rows, uint32_t num_cus, uint32_t* out_query_tile,
                                  uint32_t* out_chunks, uint32_t* out_row_slices, uint64_t* out_slice_rows, uint32_t* out_lds_bytes,
                                  uint64_t* out_scratch_bytes);
/*
 * Stage timer (scripts/probe_tanimoto.py): mvfgpu_search_tanimoto_device with events around its launches; waits for the stream.
 * out_ms[0..2] = prepare (TQ), scan (T2), merge (H1), each summed over the call's windows.  Refused beside the search's own
 * refusals: a NULL out_ms.
 */
int mvfgpu_selftest_tanimoto_stage_ms(const mvfgpu_corpus* corpus, const void* d_queries, uint8_t query_dtype, uint32_t query_dim,
                                      uint32_t nq, uint32_t k, float* d_scores, uint64_t* d_indices, void* hip_stream, float* out_ms);

#ifdef __cplusplus
}
#endif
#endif
