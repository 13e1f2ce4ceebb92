// candidates.hip — mvfgpu_search_candidates / mvfgpu_search_candidates_device: the exact top-k over given lists of rows
// (include/mvf_gpu.h; DESIGN.md §3 "Candidate search", §5 "C0 / C1 — candidate search").
//
// Per window of queries (the scratch stays bounded whatever nq and m are), on one stream, gather_topk (scan_gather.hip) runs
//   1. C0 (scan_candidates.hip; handed to it as the lists' preparation) that turns each query's list into its distinct live
//      local rows, ascending, and their count;
//   2. C1, the gathered-row kernel on those rows with K1's one-query arithmetic, chunk by chunk;
//   3. k <= MVFGPU_K_PER_PASS: each chunk's sorted best k are merged and formatted by K3 (select_final_kernel);
//      larger k (or more chunks than K3 merges): every row's rank entry is ranked by sort_composites and the first k
//      formatted by write_sorted_kernel.
// The host call runs the same device work per host window (host_staging.h) and maps each window's vector ids back to
// positions on the host first (corpus_ids_to_positions); both calls keep mvfgpu_search_device's stream discipline
// (corpus_device_call).

#include "../../include/mvf_gpu.h"

#include "aux_kernels.h"
#include "host_staging.h"
#include "internal.h"
#include "mvf_common.h"
#include "scan_candidates.h"

#include <string>
#include <vector>

using namespace mvf;

namespace {

int check_candidate_args(const mvfgpu_corpus* c, uint8_t metric, const void* queries, uint8_t query_dtype, uint32_t query_dim,
                         uint32_t nq, const uint64_t* candidates, uint32_t m, uint32_t k, const void* out_scores,
                         const void* out_indices) {
    // what needs no handle first (mvfgpu_search's codes and messages), then mvfgpu_search's own checks: nothing below
    // touches the device on a refusal
    if (const int rc = check_search_scalars(metric, nq, k, queries, out_scores, out_indices)) return rc;
    if (!candidates && m > 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer (candidates)");
    return check_search_args(c, metric, queries, query_dtype, query_dim, nq, k, out_scores, out_indices);
}

// The device work of both calls: queries, lists and results in device memory, everything on `s`, no host wait.
int candidates_core(const CorpusView& v, uint8_t metric, const void* d_queries, uint32_t nq, const uint64_t* d_cand, uint32_t m,
                    uint32_t k, float* d_scores, uint64_t* d_indices, int32_t* d_raw, uint64_t* d_counts, hipStream_t s) {
    if (m == 0) {  // nothing listed: counts 0, every entry padding
        if (const int rc = fill_padding(metric, nq, k, d_scores, d_indices, d_raw, s)) return rc;
        if (d_counts) MVF_HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)nq * 8, s));
        return MVF_OK;
    }
    const bool long_lists = m > kCandLdsSort;  // C0 ranks them through the window's sort buffers
    GatherSource src;
    src.m = m;
    src.prep_sorts = long_lists;
    src.prep = [&, long_lists](uint32_t w0, uint32_t wn, const GatherScratch& sc) -> int {  // C0
        CandPrepParams pp{};
        pp.cand = d_cand + (size_t)w0 * m;
        pp.m = m;
        pp.index_base = v.index_base;
        pp.n = v.n;
        pp.tomb = v.tomb;
        pp.ent = sc.a;
        pp.rows = sc.rows;
        pp.counts = sc.counts;
        pp.out_counts = d_counts ? d_counts + w0 : nullptr;
        if (!long_lists) {
            MVF_HIP_TRY(cand_prep_launch(pp, wn, s));
        } else {
            MVF_HIP_TRY(cand_map_launch(pp, wn, s));
            size_t tb = sc.tmp_bytes;
            uint64_t* sorted = nullptr;
            MVF_HIP_TRY(sort_composites(sc.tmp, &tb, sc.a, sc.b, m, m, &sorted, s, wn, m));
            MVF_HIP_TRY(cand_compact_launch(pp, sorted, wn, s));
        }
        return MVF_OK;
    };
    return gather_topk(v, metric, d_queries, nq, src, k, d_scores, d_indices, d_raw, s);  // C1 and the selection
}

}  // namespace

extern "C" {

int mvfgpu_search_candidates_device(const mvfgpu_corpus* c, uint8_t metric, const void* d_queries, uint8_t query_dtype,
                                    uint32_t query_dim, uint32_t nq, const uint64_t* d_candidates, uint32_t m, uint32_t k,
                                    float* d_scores, uint64_t* d_indices, int32_t* d_raw, uint64_t* d_counts, void* hip_stream) {
    const int rc = check_candidate_args(c, metric, d_queries, query_dtype, query_dim, nq, d_candidates, m, k, d_scores, d_indices);
    if (rc != MVF_OK) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return corpus_device_call(c, s, [&]() {
        return candidates_core(corpus_view(c), metric, d_queries, nq, d_candidates, m, k, d_scores, d_indices, d_raw, d_counts, s);
    });
}

int mvfgpu_search_candidates(const mvfgpu_corpus* c, uint8_t metric, const void* queries, uint8_t query_dtype, uint32_t query_dim,
                             uint32_t nq, const uint64_t* candidates, uint32_t m, uint32_t k, float* out_scores,
                             uint64_t* out_indices, int32_t* out_raw, uint64_t* out_counts) {
    const int rc0 = check_candidate_args(c, metric, queries, query_dtype, query_dim, nq, candidates, m, k, out_scores, out_indices);
    if (rc0 != MVF_OK) return rc0;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));
    const CorpusView v = corpus_view(c);
    hipStream_t s = static_cast<hipStream_t>(v.stream);
    const HostIn in[] = {{queries, query_row_bytes(v)}, {candidates, (size_t)m * 8}};
    const HostOut out[] = {{out_indices, (size_t)k * 8}, {out_scores, (size_t)k * 4}, {out_raw, (size_t)k * 4}, {out_counts, 8, true}};
    std::vector<uint64_t> mapped;
    auto map_ids = [&](uint32_t, uint32_t wn, const void** src) {  // ids attached: a window's entries are ids
        const size_t nl = (size_t)wn * m;
        if (!nl || !v.ids) return;
        mapped.resize(nl);
        if (corpus_ids_to_positions(c, static_cast<const uint64_t*>(src[1]), nl, mapped.data())) src[1] = mapped.data();
    };
    return stage_host_windows(c, s, nq, in, out, map_ids, [&](uint32_t, uint32_t wn, void* const* d_in, void* const* d_out) {
        return candidates_core(v, metric, d_in[0], wn, static_cast<const uint64_t*>(d_in[1]), m, k, static_cast<float*>(d_out[1]),
                               static_cast<uint64_t*>(d_out[0]), static_cast<int32_t*>(d_out[2]), static_cast<uint64_t*>(d_out[3]), s);
    });
}

}  // extern "C"
