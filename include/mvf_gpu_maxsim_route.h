/*
 * mvf_gpu_maxsim_route.h — C ABI of libmvf_gpu.so, continued: the MFMA selection route of the multi-vector search
 * (mvfgpu_search_maxsim / mvfgpu_search_maxsim_device of include/mvf_gpu.h).  The functions are additions to ABI version 3.
 * Their stream classes ("Stream discipline") are listed in tests/_maxsim_mfma.py.
 */
#ifndef MVF_GPU_MAXSIM_ROUTE_H
#define MVF_GPU_MAXSIM_ROUTE_H

#include "mvf_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The MFMA selection route of mvfgpu_search_maxsim / _device ("Multi-vector search: the MFMA route", section 5
 * "A0 / P0").  Route 1 scores every held row with the one-query arithmetic.  Route 2 first scores every row on the matrix unit --
 * another order of the f32 sum, the tokens rounded to f16 on Float16 rows --, sums the per-token bests as route 1 does, takes the
 * min(k, n_keys)-th best approximate sum theta and keeps as CANDIDATES of a set the keys whose approximate sum is at least
 * theta - 2 Delta (Delta: mvfgpu_selftest_maxsim_margin), the keys where a value left the bound's premises (not finite, too large,
 * too small) and every key where theta or Delta is not finite; then route 1's kernel scores the 128-row blocks of the key-ordered list
 * that hold a candidate's row and the answer is ranked among the candidates.  The result is route 1's byte for byte -- score bits,
 * keys, counts -- for every input; signature, checks, refusal order, padding and the absence of a host wait are unchanged.  The cost
 * follows the candidates: where everything ties every key is one and route 2 costs route 1 plus its selection.
 * Eligible: Float32 / Float16 rows under InnerProduct / Cosine.  L2 and Int8 / UInt8 rows take route 1 whatever is asked for.
 *   route 0: automatic -- route 2 where it is eligible, k <= n_keys / 2, nq x n_tokens >= 32 and held rows x n_tokens >=
 *            64 000 000, the crossover measured in profiles/r18_maxsim_mfma.txt ("A0 / P0"); else route 1;
 *         1: always route 1;  2: route 2 where eligible.  Any other value: MVF_ERR_INVALID_ARGUMENT.
 * MVF_MAXSIM_ROUTE in the environment takes the same values (read when the handle is created, re-read by
 * mvfgpu_corpus_reload_tuning); a route set here other than 0 wins over it.  Do not call beside searches of the handle.
 * Scratch of route 2 per query set of a window, inside MVF_MAXSIM_SCRATCH_BYTES with route 1's: the prepared tokens, one byte per
 * key and 8 bytes per 128 held rows.
 */
int mvfgpu_set_maxsim_route(mvfgpu_corpus* corpus, int route);
/* The route a full multi-vector search takes, a pure function (no GPU, no handle); the launch itself calls it.  forced: 0, 1 or 2 as
 * above.  Refused with MVF_ERR_INVALID_ARGUMENT: a NULL output, an unknown data type or metric, dimension 0, n_tokens outside
 * 1 .. MVFGPU_MAXSIM_MAX_TOKENS, any other forced. */
int mvfgpu_selftest_maxsim_route(uint64_t held_rows, uint64_t n_keys, uint32_t dimension, uint8_t data_type, uint8_t metric,
                                 uint32_t nq, uint32_t n_tokens, uint32_t k, int forced, uint32_t* out_route);
/*
 * The bound Delta of |approximate sum - exact sum| of one query set as the device computes it (no GPU needed), in double:
 *   eps   = (max(dimension, 64) + 16) 2^-23, plus 2^-11 x 1.001 on Float16 rows;
 *   u_t   = 1 under Cosine, token_norms[t] x sqrt(xxmax) under InnerProduct (xxmax: the largest sum of squares of a stored row);
 *   Delta = 1.001 x (eps + (n_tokens - 1) 2^-23) x sum of u_t;
 *   +inf where a u_t is NaN or neither 0 nor inside [1e-24, 1e37), or the sum reaches 1e37: every key is a candidate then.
 * Refused with MVF_ERR_INVALID_ARGUMENT: NULL buffers, a data type or metric the route does not take, dimension 0, n_tokens outside
 * 1 .. MVFGPU_MAXSIM_MAX_TOKENS.
 */
int mvfgpu_selftest_maxsim_margin(uint8_t data_type, uint8_t metric, uint32_t dimension, const float* token_norms, uint32_t n_tokens,
                                  float xxmax, double* out_delta);
/*
 * Stage timer of route 2 (scripts/probe_maxsim_mfma.py): mvfgpu_search_maxsim_device without d_counts by route 2 whatever the handle's
 * route, with events between its stages; waits for the stream.  out_ms[0..5] = the preparation (row norms on first use, key ordinals,
 * prepared tokens), A0 (the MFMA scoring), the approximate sums with their kth best and P0, route 1's kernel over the candidates'
 * blocks, its sums and the mask, the tail; each summed over the call's chunks and windows.  out_candidates[nq] / out_blocks[nq]: per
 * set the candidate keys and the 128-row blocks scored again.  Refused with MVF_ERR_INVALID_ARGUMENT beside the search's own
 * refusals: a NULL output, no held rows, a handle or metric the route is not eligible for.  mvfgpu_selftest_maxsim_stage_ms times
 * route 1 whatever the handle's route.
 */
int mvfgpu_selftest_maxsim_mfma_stage_ms(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, uint8_t metric,
                                         const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                                         uint32_t n_tokens, uint32_t k, float* d_scores, uint64_t* d_keys, void* hip_stream,
                                         float* out_ms, uint32_t* out_candidates, uint32_t* out_blocks);
/*
 * Read-out of route 2's selection (tests/test_gpu_maxsim_mfma_bound.py): mvfgpu_search_maxsim_device without d_counts by route 2
 * whatever the handle's route, as the stage timer runs it; waits for the stream.  Beside the search's result it fills caller-owned
 * HOST arrays with what the selection held on the device, per query set of the call and per key in ascending key value (the order
 * of mvfgpu_partition_keys):
 *   out_sums[nq][n_keys]        the approximate sums as P0 read them;
 *   out_forced[nq][n_keys]      bytes: A0's forced keys, before P0;
 *   out_candidates[nq][n_keys]  bytes: the candidates, behind P0;
 *   out_delta[nq]               the bound Delta the device computed;
 *   out_theta[nq], out_theta_nan[nq] (bytes)  the min(k, n_keys)-th best approximate sum P0 compared with, and whether that entry
 *                               was the live NaN entry (fewer keys than that with a sum the bound covers; out_theta is NaN then);
 *   out_xxmax[1]                the largest sum of squares of a stored row, as P0 read it.
 * The production path enqueues nothing for it.  Refused with MVF_ERR_INVALID_ARGUMENT: what the stage timer refuses, and every
 * NULL output.
 */
int mvfgpu_selftest_maxsim_mfma_selection(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, uint8_t metric,
                                          const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                                          uint32_t n_tokens, uint32_t k, float* d_scores, uint64_t* d_keys, void* hip_stream,
                                          float* out_sums, uint8_t* out_forced, uint8_t* out_candidates, double* out_delta,
                                          float* out_theta, uint8_t* out_theta_nan, float* out_xxmax);

#ifdef __cplusplus
}
#endif
#endif
