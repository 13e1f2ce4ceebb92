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
// The host call maps vector ids back to positions on the host (corpus_ids_to_positions), stages small windows through the
// handle's pinned mirrors and runs the same device work on the handle's stream; both calls keep mvfgpu_search_device's
// stream discipline (corpus_device_call).

#include "../../include/mvf_gpu.h"

#include "aux_kernels.h"
#include "internal.h"
#include "mvf_common.h"
#include "scan_candidates.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace mvf;

namespace {

constexpr size_t kHostWindowBytes = 256ull << 20;   // the host call's device copies of queries, lists and results per window
constexpr size_t kPinnedBytes = 1ull << 20;         // host windows up to this size travel through the handle's pinned mirrors

int check_candidate_args(const mvfgpu_corpus* c, uint8_t metric, const void* queries, uint8_t query_dtype, uint32_t query_dim,
                         uint32_t nq, const uint64_t* candidates, uint32_t m, uint32_t k, const void* out_scores,
                         const void* out_indices) {
    // what needs no handle first (mvfgpu_search's codes and messages), then mvfgpu_search's own checks: nothing below
    // touches the device on a refusal
    if (const int mrc = check_metric(metric)) return mrc;
    if (nq == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "nq must be > 0");
    if (k == 0 || k > MVFGPU_MAX_K) return set_fail(MVF_ERR_INVALID_ARGUMENT, "k must be in 1..2^31");
    if (!queries || !out_scores || !out_indices) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
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
    const size_t qrow = (size_t)v.dim * (is_int_dtype(v.dtype) ? 1 : 4);
    const size_t in_q = qrow + (size_t)m * 8, out_q = (size_t)k * 16 + 8;  // bytes per query in / out
    const uint32_t W = (uint32_t)std::max<size_t>(1, std::min<size_t>(nq, kHostWindowBytes / (in_q + out_q)));
    AsyncBuf dq, dcand, dsc, didx, draw, dcnt;
    MVF_HIP_TRY(dq.alloc((size_t)W * qrow, s));
    MVF_HIP_TRY(dcand.alloc((size_t)W * m * 8, s));
    MVF_HIP_TRY(dsc.alloc((size_t)W * k * 4, s));
    MVF_HIP_TRY(didx.alloc((size_t)W * k * 8, s));
    if (out_raw) MVF_HIP_TRY(draw.alloc((size_t)W * k * 4, s));
    MVF_HIP_TRY(dcnt.alloc((size_t)W * 8, s));
    std::vector<uint64_t> mapped;
    for (uint32_t w0 = 0; w0 < nq; w0 += W) {
        const uint32_t wn = std::min(W, nq - w0);
        const size_t nl = (size_t)wn * m, nr = (size_t)wn * k;
        const unsigned char* hq = static_cast<const unsigned char*>(queries) + (size_t)w0 * qrow;
        const uint64_t* hc = candidates ? candidates + (size_t)w0 * m : nullptr;
        if (nl && v.ids) {
            mapped.resize(nl);
            if (corpus_ids_to_positions(c, hc, nl, mapped.data())) hc = mapped.data();  // ids attached: entries are ids
        }
        // small windows through the pinned mirrors: in = queries | lists, out = indices | scores | raw | counts
        const size_t in_bytes = (size_t)wn * qrow + nl * 8, out_bytes = nr * 16 + (size_t)wn * 8;
        const bool pinned = in_bytes + out_bytes <= kPinnedBytes;
        unsigned char *pin_in = nullptr, *pin_out = nullptr;
        if (pinned) {
            void *pi = nullptr, *po = nullptr;
            const int rc = corpus_pinned_mirrors(c, in_bytes, out_bytes, &pi, &po);
            if (rc != MVF_OK) return rc;
            pin_in = static_cast<unsigned char*>(pi);
            pin_out = static_cast<unsigned char*>(po);
            std::memcpy(pin_in, hq, (size_t)wn * qrow);
            if (nl) std::memcpy(pin_in + (size_t)wn * qrow, hc, nl * 8);
        }
        const size_t o_sc = nr * 8, o_raw = nr * 12, o_cnt = nr * 16;
        const int rc = corpus_device_call(c, s, [&]() -> int {
            MVF_HIP_TRY(hipMemcpyAsync(dq.p, pinned ? pin_in : hq, (size_t)wn * qrow, hipMemcpyHostToDevice, s));
            if (nl) MVF_HIP_TRY(hipMemcpyAsync(dcand.p, pinned ? pin_in + (size_t)wn * qrow : reinterpret_cast<const unsigned char*>(hc), nl * 8,
                                            hipMemcpyHostToDevice, s));
            const int rc1 = candidates_core(v, metric, dq.p, wn, static_cast<const uint64_t*>(dcand.p), m, k, static_cast<float*>(dsc.p),
                                            static_cast<uint64_t*>(didx.p), static_cast<int32_t*>(draw.p), static_cast<uint64_t*>(dcnt.p), s);
            if (rc1 != MVF_OK) return rc1;
            if (pinned) {
                MVF_HIP_TRY(hipMemcpyAsync(pin_out, didx.p, nr * 8, hipMemcpyDeviceToHost, s));
                MVF_HIP_TRY(hipMemcpyAsync(pin_out + o_sc, dsc.p, nr * 4, hipMemcpyDeviceToHost, s));
                if (out_raw) MVF_HIP_TRY(hipMemcpyAsync(pin_out + o_raw, draw.p, nr * 4, hipMemcpyDeviceToHost, s));
                MVF_HIP_TRY(hipMemcpyAsync(pin_out + o_cnt, dcnt.p, (size_t)wn * 8, hipMemcpyDeviceToHost, s));
            } else {
                MVF_HIP_TRY(hipMemcpyAsync(out_indices + (size_t)w0 * k, didx.p, nr * 8, hipMemcpyDeviceToHost, s));
                MVF_HIP_TRY(hipMemcpyAsync(out_scores + (size_t)w0 * k, dsc.p, nr * 4, hipMemcpyDeviceToHost, s));
                if (out_raw) MVF_HIP_TRY(hipMemcpyAsync(out_raw + (size_t)w0 * k, draw.p, nr * 4, hipMemcpyDeviceToHost, s));
                if (out_counts) MVF_HIP_TRY(hipMemcpyAsync(out_counts + w0, dcnt.p, (size_t)wn * 8, hipMemcpyDeviceToHost, s));
            }
            return MVF_OK;
        });
        if (rc != MVF_OK) return rc;
        MVF_HIP_TRY(hipStreamSynchronize(s));
        if (pinned) {
            std::memcpy(out_indices + (size_t)w0 * k, pin_out, nr * 8);
            std::memcpy(out_scores + (size_t)w0 * k, pin_out + o_sc, nr * 4);
            if (out_raw) std::memcpy(out_raw + (size_t)w0 * k, pin_out + o_raw, nr * 4);
            if (out_counts) std::memcpy(out_counts + w0, pin_out + o_cnt, (size_t)wn * 8);
        }
    }
    return MVF_OK;
}

}  // extern "C"
