/*
 * mvf_gpu_hamming_route.h — C ABI of libmvf_gpu.so, continued: the MFMA route of the Hamming search (mvfgpu_search_hamming /
 * mvfgpu_search_hamming_device of include/mvf_gpu_hamming.h).  The functions are additions to ABI version 3.  Their stream
 * classes ("Stream discipline") are listed in tests/test_hamming_route_cpu.py.
 */
#ifndef MVF_GPU_HAMMING_ROUTE_H
#define MVF_GPU_HAMMING_ROUTE_H

#include "mvf_gpu_hamming.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The MFMA route of mvfgpu_search_hamming / _device ("Hamming search", section 5 "HQ / H2").  Route 1 is H0 + H1:
 * xor and popcount on the vector unit.  Route 2 computes the same distances on the matrix unit -- with a row as 0/1 values and a
 * query as +1 / -1, d = popcount(q) + sum of x q', FP4 tiles, f32 accumulators that hold every partial sum exactly -- and selects
 * by H0's rule; H1 is shared.  The result is route 1's byte for byte for every input; signature, checks, refusal order, padding
 * and the absence of a host wait are unchanged.  Three launches per 1024 queries instead of two.
 * Eligible: rows of up to 512 packed bytes (4096 bits; the pitch is what counts) and k up to 1024.  Everything else takes route 1
 * whatever is asked for.
 *   route 0: automatic -- route 2 where it is eligible, the window holds 1024 queries, the handle at least 10 000 000 rows of at
 *            least 64 bytes' pitch and k is at most 128: the shapes from which it was measured to win by more than the spread between
 *            boxes (profiles/r25_hamming_mfma.txt; DESIGN.md section 5, "HQ / H2"); else route 1;
 *         1: always route 1;  2: route 2 where eligible.  Any other value: MVF_ERR_INVALID_ARGUMENT, as is a NULL corpus.
 * MVF_HAMMING_ROUTE in the environment takes the same values (read when the handle is created, re-read by
 * mvfgpu_corpus_reload_tuning); a route set here other than 0 wins over it.  Do not call beside searches of the handle.
 * Scratch of route 2 per window, beside the slices' lists: the prepared queries, 4 bytes per byte of a query's pitch rounded up to
 * 64 plus 4 per query, 2 MiB and 4 KiB at most; and the candidate buffers, row slices x queries rounded up to the tile x
 * max(2 next_pow2(k), 512) x 8 bytes, which the slice count keeps within 512 MiB.
 *
 * Not built: rows of more than 512 packed bytes on route 2 (they need the queries staged in chunks of the row); the int8
 * 16x16x64 form of the same kernel; a tile of fewer than 64 queries (a short window pays for idle query columns).
 */
int mvfgpu_set_hamming_route(mvfgpu_corpus* corpus, int route);
/* The route one window of a Hamming search takes, a pure function (no GPU, no handle); the launch itself calls it.  dimension = packed
 * bytes of a row, nq_in_window = queries of the window (1 .. ; a window holds 1024 at most), forced: 0, 1 or 2 as above.  Refused with
 * MVF_ERR_INVALID_ARGUMENT: a NULL output, any other forced, and what mvfgpu_selftest_hamming_form refuses. */
int mvfgpu_selftest_hamming_route(uint32_t dimension, uint32_t nq_in_window, uint32_t k, uint64_t rows, int forced, uint32_t* out_route);
/*
 * Self-test of route 2's form (no GPU, no handle): the decision the launch itself takes for rows of `dimension` packed bytes, nq
 * queries in a window, k and `rows` rows on a part of num_cus compute units (0: 256).  *out_query_tile = queries whose prepared bits
 * a block holds in LDS (128 up to a pitch of 256 bytes, 64 beyond); *out_rows_per_wave, *out_threads = rows a wave owns per
 * iteration and threads of a block; *out_row_slices, *out_slice_rows = row ranges the scan is split into (0 for no rows) and the
 * rows of one; *out_lds_bytes = LDS of a scan block; *out_prepared_bytes, *out_scratch_bytes = the two scratch areas above.  Any
 * output may be NULL.  Refused with MVF_ERR_INVALID_ARGUMENT: what mvfgpu_selftest_hamming_form refuses, and a dimension above 512.
 */
int mvfgpu_selftest_hamming_mfma_form(uint32_t dimension, uint32_t nq, uint32_t k, uint64_t rows, uint32_t num_cus, uint32_t* out_query_tile,
                                      uint32_t* out_rows_per_wave, uint32_t* out_threads, uint32_t* out_row_slices, uint64_t* out_slice_rows,
                                      uint32_t* out_lds_bytes, uint64_t* out_prepared_bytes, uint64_t* out_scratch_bytes);

#ifdef __cplusplus
}
#endif
#endif
