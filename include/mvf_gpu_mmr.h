/*
 * mvf_gpu_mmr.h — C ABI of libmvf_gpu.so, continued: diversified re-ranking by maximal marginal relevance (MMR) over each
 * query's candidate rows.  The functions are additions to ABI version 3.  Their stream classes ("Stream
 * discipline") are listed in tests/_mmr.py.
 */
#ifndef MVF_GPU_MMR_H
#define MVF_GPU_MMR_H

#include "mvf_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* list entries per query of a diversified re-ranking */
#define MVFGPU_MMR_MAX_CANDIDATES 1024u

/*
 * Diversified re-ranking ("Diversified re-ranking", section 5 "D0"): of each query's candidate rows, k that
 * are relevant and not near-copies of each other.  The arguments are mvfgpu_search_candidates' -- corpus, metric, queries, [nq][m]
 * lists (positions, or vector ids where attached; UINT64_MAX pads), k -- plus one lambda for the call.
 *
 * C, the candidates of a query, are its distinct, live, in-shard list entries in ascending position, as the candidate search keeps
 * them.  v(x) = x under InnerProduct and Cosine, -x under L2.  rel(d) = v(the score mvfgpu_search_candidates reports for (q, d));
 * sim(d, s) = v(the score of the same call with the STORED ROW s as the query): Float32 as stored, Float16 widened exactly,
 * Int8 / UInt8 as stored.  a = lambda, b = 1.0f - lambda.
 *   pick 0:      the first row of C in mvfgpu_search's order (best first, NaN last, ties by ascending position);
 *   after pick s: red(d) = fmaxf(red(d), sim(d, s)) for every row d not yet picked; red starts at -inf, a NaN is ignored, and of
 *                two equal values (-0.0 and +0.0) the one already held stays;
 *   pick j >= 1: the row that maximises obj(d) = (a rel(d)) - (b red(d)) -- two f32 multiplications and one f32 subtraction, each
 *                rounded to nearest, never an fma --, -0.0 equal to +0.0, NaN last, ties by ascending position;
 *   min(k, |C|) picks.
 * out_scores / out_indices / out_raw (nullable) [nq][k]: the picks in pick order, shaped as mvfgpu_search_candidates' results --
 * the score is the candidate search's score of (q, pick), not the objective --, mvfgpu_search's padding behind them.
 * out_objective [nq][k] (nullable): a rel for pick 0, obj for the later picks (a NaN as the quiet NaN 0x7FC00000, as a NaN score
 * is), the padding score behind them.
 * out_counts [nq] (nullable): |C|.
 * lambda = 1 on finite scores gives mvfgpu_search_candidates' first k (where distinct exact integers give distinct f32 scores);
 * permuting or repeating list entries changes nothing.
 *
 * Refused, before any device call: what mvfgpu_search_candidates refuses, in its order; then lambda NaN or outside [0, 1]; then
 * m > MVFGPU_MMR_MAX_CANDIDATES.  k = 1 .. MVFGPU_MAX_K (beyond |C|: padding); m = 0: padding, counts 0.
 * The host call stages through windows as mvfgpu_search_candidates does; the device call takes positions, is asynchronous on
 * hip_stream and makes no host wait.  Neither reads nor posts the repair feedback.
 *
 * Not built: more than 1024 candidates; a lambda per query; shard sets (the picks of two shards do not merge); a route that splits
 * one query over several workgroups; the candidates' rows cached in LDS; MMR over the keys of a partition.
 */
int mvfgpu_search_mmr(const mvfgpu_corpus* corpus, uint8_t metric, const void* queries, uint8_t query_dtype, uint32_t query_dim,
                      uint32_t nq, const uint64_t* candidates, uint32_t m, uint32_t k, float lambda, float* out_scores,
                      uint64_t* out_indices, int32_t* out_raw, float* out_objective, uint64_t* out_counts);
int mvfgpu_search_mmr_device(const mvfgpu_corpus* corpus, uint8_t metric, const void* d_queries, uint8_t query_dtype,
                             uint32_t query_dim, uint32_t nq, const uint64_t* d_candidates, uint32_t m, uint32_t k, float lambda,
                             float* d_scores, uint64_t* d_indices, int32_t* d_raw, float* d_objective, uint64_t* d_counts,
                             void* hip_stream);
/*
 * The walk alone, on the host (no GPU): m rows with scores rel_scores[m] and pairwise scores sim_scores[s][d] (row s as the query,
 * [m][m]), both in SCORE form (v is applied here), positions 0 .. m-1.  out_order[k]: the picks' positions, UINT32_MAX behind
 * them; out_objective[k] (nullable) as the search's.  Returns the number of picks, min(k, m), or -MVF_ERR_INVALID_ARGUMENT for a
 * NULL buffer (sim_scores may be NULL where m < 2 or k < 2), an unknown metric, lambda NaN or outside [0, 1],
 * m > MVFGPU_MMR_MAX_CANDIDATES or k = 0.
 */
int mvfgpu_selftest_mmr_walk(const float* rel_scores, const float* sim_scores, uint32_t m, uint8_t metric, float lambda, uint32_t k,
                             uint32_t* out_order, float* out_objective);
/*
 * Self-test of the walk kernel's form (no GPU, no handle): which instantiation of D0 ("D0") walks rows of
 * `dimension` elements of `data_type` -- the decision the launch itself takes.  forced_g = 0: the library's own lane-group rule;
 * 1, 4, 8, 16, 32 or 64: the width MVF_K1_G forces on a handle.  *out_g = lanes per row, *out_j = 16-byte steps per lane,
 * *out_qlds = 1 where the picked row is staged as a query in LDS (Int8 / UInt8 always; float rows whose padded f32 copy, g x j
 * vectors, takes at most 40 KiB), 0 where it goes to the query's f32 scratch row and is read back through the cache.  Refused with
 * MVF_ERR_INVALID_ARGUMENT: a NULL output, an unknown data type, dimension 0, an Int8 / UInt8 dimension above MVFGPU_MAX_INT_DIM,
 * a row above 1 GiB, any other forced_g.
 */
int mvfgpu_selftest_mmr_form(uint8_t data_type, uint32_t dimension, uint32_t forced_g, uint32_t* out_g, uint32_t* out_j,
                             uint32_t* out_qlds);
/*
 * Stage timer (scripts/probe_mmr.py): mvfgpu_search_mmr_device with events between its stages; waits for the stream.
 * out_ms[0..1] = C0 with the relevance scores, D0 (the walk); each summed over the call's windows.  Refused beside the search's
 * own refusals: a NULL out_ms.
 */
int mvfgpu_selftest_mmr_stage_ms(const mvfgpu_corpus* corpus, uint8_t metric, const void* d_queries, uint8_t query_dtype,
                                 uint32_t query_dim, uint32_t nq, const uint64_t* d_candidates, uint32_t m, uint32_t k, float lambda,
                                 float* d_scores, uint64_t* d_indices, int32_t* d_raw, float* d_objective, uint64_t* d_counts,
                                 void* hip_stream, float* out_ms);

#ifdef __cplusplus
}
#endif
#endif
