/*
 * mvf_gpu_maxsim_align.h — C ABI of libmvf_gpu.so, continued: MaxSim alignments, each listed document's best row per query token.
 * The functions are additions to ABI version 3 (MVFGPU_ABI_VERSION stays 3: functions are only added).
 */
#ifndef MVF_GPU_MAXSIM_ALIGN_H
#define MVF_GPU_MAXSIM_ALIGN_H

#include "mvf_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Alignments ("Alignments", section 5 "M0-arg and the alignment writer"): mvfgpu_search_maxsim and
 * mvfgpu_search_maxsim_candidates report one number per document, the sum over the query's tokens of each token's best score among
 * the document's rows; this call says WHICH row was the best for which token, for a list of keys per query set -- usually the keys
 * a multi-vector search just returned (the recipe for a full search: the search, then this call on its out_keys), or a first
 * stage's candidates.  A re-ranker highlights the passage tokens that carried the match, a page retriever draws its per-token
 * similarity map, a RAG service cuts the snippet around each returned document's best-matching passage.
 *   queries, n_tokens, metric, query_dtype, query_dim : mvfgpu_search_maxsim's, with its types, limits and dimension rules.
 *   keys     : [nq][m] column values, one list per query set; a HOST array in both calls, read before the call returns.
 *   outputs  : [nq][m][n_tokens], IN LIST ORDER: element (q, i, t) belongs to token t of set q and the key keys[q][i].
 * Element (q, i, t) is the first row in mvfgpu_search's order for token t -- best first, ties by ascending position, NaN last,
 * -0.0 == +0.0 -- among the rows the partition holds for that key:
 *   out_rows   : the row as every search reports it: index_base + row, or the vector id where ids are attached;
 *   out_scores : its score, reconstructed from the order key as every result is (+0.0 for +-0.0; the NaN every result carries);
 *   out_raw    : (nullable) the exact i32 on Int8 / UInt8 rows under L2 / InnerProduct, 0 otherwise.
 * Where the partition does not hold the key (an unknown key, every row deleted, the pad UINT64_MAX) the element is
 * mvfgpu_search's padding: row UINT64_MAX, score +inf (L2) or -inf, raw 0.  A key listed twice gets the same answer at both
 * entries.  m = 0 is allowed: nothing is written and keys may be NULL.  Every element of the three outputs is written by the call.
 * So, byte for byte (rows, score bits, raw), for every data type:
 *   1. element (q, i, t) is the single result of mvfgpu_search_partitioned for the one query "token t of set q" with the key
 *      keys[q][i] and k = 1 -- skipped and repeated entries included;
 *   2. ((s(q,i,0) + s(q,i,1)) + ...) in plain f32, in token order, is the score mvfgpu_search_maxsim_candidates reports for the
 *      key: the scores are the b(t, g) of mvfgpu_search_maxsim.
 * Refusals, all before any device call and leaving no device error: mvfgpu_search_maxsim_candidates', in its order and wording,
 * checked as with k = 1, with "NULL buffer (keys)" in the place of its candidate_keys message.
 * The device call is asynchronous on the caller's stream and waits on the host only for the previous call's plan to have left the
 * index's pinned buffer (the candidate search's rule); d_queries and the three outputs are device memory.  No repair feedback is
 * read or posted.
 * Cost: the listed keys' rows leave HBM once per chunk of tokens and query set; per window of query sets one expansion launch and
 * two launches per chunk, whatever nq, m and the lists.  Scratch per query set of a window: chunk x distinct held keys x 8 bytes,
 * 8 bytes per list position (each set's rows rounded up to a multiple of 128) and 4 bytes per list entry, inside
 * MVF_MAXSIM_SCRATCH_BYTES wherever one set with one group of four tokens fits.
 * Not built: alignments inside the full search or its MFMA route (the recipe above); keys in device memory; ragged token counts;
 * per-token weights; shard sets; the second-best row.
 */
int mvfgpu_maxsim_align(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, uint8_t metric, const void* queries,
                        uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t n_tokens, const uint64_t* keys, uint32_t m,
                        float* out_scores, uint64_t* out_rows, int32_t* out_raw);
int mvfgpu_maxsim_align_device(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, uint8_t metric, const void* d_queries,
                               uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t n_tokens, const uint64_t* keys,
                               uint32_t m, float* d_scores, uint64_t* d_rows, int32_t* d_raw, void* hip_stream);
/*
 * Self-test of the alignments' scratch plan (no GPU needed): mvfgpu_selftest_maxsim_plan's arguments, chunk rules and refusals,
 * with chunk x n_keys x 8 bytes per query set of a window inside budget_bytes -- a u64 per (token, key), no sums, no sort buffers.
 * budget_bytes is what the call's budget leaves beside the window's list (8 bytes per position) and slot map (4 bytes per entry).
 */
int mvfgpu_selftest_maxsim_align_plan(uint64_t n_keys, uint32_t n_tokens, uint32_t nq, uint64_t token_bytes, uint64_t budget_bytes,
                                      uint32_t* tokens_per_chunk, uint32_t* sets_per_window);
/*
 * Stage timer (scripts/probe_maxsim_align.py): mvfgpu_maxsim_align_device with events between its stages; waits for the stream.
 * out_ms[0..2] = the plan's upload and E0 (the expansion), M0-arg, the writer, each summed over the call's chunks and windows.
 * Refused beside the call's own refusals: a NULL out_ms.
 */
int mvfgpu_selftest_maxsim_align_stage_ms(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, uint8_t metric,
                                          const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                                          uint32_t n_tokens, const uint64_t* keys, uint32_t m, float* d_scores, uint64_t* d_rows,
                                          int32_t* d_raw, void* hip_stream, float* out_ms);

#ifdef __cplusplus
}
#endif
#endif
