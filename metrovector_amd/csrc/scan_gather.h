// scan_gather.h — the gathered-row scoring kernel of the candidate and filtered searches and the host tail both share
// (scan_gather.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>

#include "../../include/mvf_gpu.h"

#include "internal.h"
#include "scan_filter.h"

namespace mvf {

constexpr uint32_t kGatherChunk = 1024;  // listed rows per block (a chunk of a list)

// the query lives in LDS when its padded copy takes at most this many bytes, beyond that the rows read it through the cache
constexpr uint32_t kCandQueryLdsMax = 40u * 1024u;
inline uint32_t cand_query_bytes(uint8_t dtype, int G, uint32_t J) { return (uint32_t)G * J * (dtype == 1 ? 32u : 16u); }

// Grid (chunks of kGatherChunk list positions, groups of qg queries).  The G-lane group of K1's one-query shape loads a
// row's 16-byte vectors once and scores it against every query of the block's group with K1's arithmetic (k1_rowscore.h);
// composites (key << 32 | local row).  Query q scores the rows list[q * list_stride ..]: the first counts[q] of m positions,
// or all m where counts is NULL.  lists != NULL: per query, the chunk's best min(kcap, rows) composites, sorted, ~0-padded,
// to lists[q][chunk][kcap] (the input of K3, select_final_kernel).  dump != NULL: the rank entry of every list position
// i < m goes to dump[q][i] (positions past the count dead), for the whole-list sort of k > MVFGPU_K_PER_PASS.
struct GatherScoreParams {
    const unsigned char* rows;
    const void* queries;     // device [nq][dim]: f32, or the space's int type
    const uint32_t* list;    // local rows, ascending
    uint32_t list_stride;    // 0: one list for all queries
    const uint32_t* counts;  // [nq], or NULL; needs qg == 1
    uint32_t m, nq, dim, pitch, V, J;
    uint64_t* lists;
    uint32_t kcap;
    uint64_t* dump;
};
// qg: queries per block, 1 or 4 (lists that differ per query: 1)
hipError_t gather_score_launch(uint8_t dtype, int metric, int G, uint32_t qg, const GatherScoreParams& p, hipStream_t s);

// The sort buffers of a window (sort_composites: [W][m] entries each), which a GatherSource's prep may use before the scores do.
struct GatherScratch {
    uint64_t *a, *b;
    void* tmp;
    size_t tmp_bytes;
    uint32_t* rows;    // [W][m], per-query lists only
    uint32_t* counts;  // [W]
};
// The lists a call scores: one list of m rows for every query (qg queries per block), or -- list == NULL -- per-query lists
// of m positions that prep(w0, wn, scratch) lays down for the window's queries [w0, w0 + wn) as scratch.rows / scratch.counts.
struct GatherSource {
    uint32_t m = 0, qg = 1;
    const uint32_t* list = nullptr;
    bool prep_sorts = false;  // prep needs scratch.a / b / tmp
    std::function<int(uint32_t, uint32_t, const GatherScratch&)> prep;
};
// K1's one-query lane group of a handle's rows -- the gathered-row kernel scores with its bits -- with the bytes of a padded
// query and the queries per block (GatherSource::qg) of a search that scores one list for all queries
struct OneQueryGroup {
    int G = 64;
    uint32_t J = 1, qbytes = 0, qg = 1;
};
inline OneQueryGroup one_query_group(const CorpusView& v) {
    OneQueryGroup g;
    k1_group(v.V, 1, v.k1_g, &g.G, &g.J);
    g.qbytes = cand_query_bytes(v.dtype, g.G, g.J);
    g.qg = filter_group_queries(g.qbytes);
    return g;
}
// The exact top-k of every query over its listed rows (m > 0), formatted as a search's results; in windows of queries so that
// the scratch stays bounded, everything on `s`, no host wait.  k <= MVFGPU_K_PER_PASS and at most kSelectMaxLists chunks: each
// chunk's sorted best k are merged and formatted by K3 (select_final_kernel); beyond, every position's rank entry is ranked by
// sort_composites and the first k formatted by write_sorted_kernel.
int gather_topk(const CorpusView& v, uint8_t metric, const void* d_queries, uint32_t nq, const GatherSource& src, uint32_t k,
                float* d_scores, uint64_t* d_indices, int32_t* d_raw, hipStream_t s);
// nothing listed: every entry of nq result rows padding
int fill_padding(uint8_t metric, uint32_t nq, uint32_t k, float* d_scores, uint64_t* d_indices, int32_t* d_raw, hipStream_t s);

}  // namespace mvf
