// mmr.hip — mvfgpu_search_mmr / mvfgpu_search_mmr_device: diversified re-ranking over given lists of rows
// (include/mvf_gpu_mmr.h; DESIGN.md §3 "Diversified re-ranking", §5 "D0 — diversified re-ranking").
//
// The whole output is filled with padding first (fill_padding).  Then, per window of queries (the scratch stays bounded
// whatever nq is), on one stream:
//   1. C0 (scan_candidates.hip, its LDS form: m <= 1024) turns each query's list into its distinct live local rows,
//      ascending, and their count;
//   2. the gathered-row kernel (scan_gather.hip) scores those rows with K1's one-query arithmetic and dumps one rank entry
//      per list position: the relevance;
//   3. D0 (scan_mmr.hip) walks each query's entries in one block and writes its picks.
// Scratch per query of a window: the dump (8 m bytes), C0's list and count (4 m + 4) and, where the padded query exceeds the
// gathered-row kernel's LDS limit, one f32 row.  The host call runs the same device work per host window (host_staging.h) and
// maps each window's vector ids to positions first; both calls keep mvfgpu_search_device's stream discipline
// (corpus_device_call).  mvfgpu_selftest_mmr_walk is the walk on the host with D0's arithmetic (mmr_walk.h).

#include "../../include/mvf_gpu_mmr.h"

#include "host_staging.h"
#include "internal.h"
#include "mmr_walk.h"
#include "mvf_common.h"
#include "scan_candidates.h"
#include "scan_mmr.h"

#include <algorithm>
#include <string>
#include <vector>

using namespace mvf;

static_assert(MVFGPU_MMR_MAX_CANDIDATES == kMmrMaxCandidates, "the header's limit is D0's");
static_assert(kMmrMaxCandidates <= kCandLdsSort, "C0 takes every list in its LDS form");

namespace {

constexpr uint32_t kWindow = 1024;              // queries per window at most
constexpr size_t kScratchBytes = 512ull << 20;  // device scratch of a window

int check_lambda(float lambda) {
    if (!(lambda >= 0.0f && lambda <= 1.0f))
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "lambda must be in [0, 1], got " + std::to_string(lambda));
    return MVF_OK;
}

int check_mmr_args(const mvfgpu_corpus* c, uint8_t metric, const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                   const uint64_t* candidates, uint32_t m, uint32_t k, float lambda, const void* out_scores, const void* out_indices) {
    // the candidate search's checks in its order (nothing below touches the device on a refusal), then this call's own
    if (const int rc = check_search_scalars(metric, nq, k, queries, out_scores, out_indices)) return rc;
    if (!candidates && m > 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer (candidates)");
    if (const int rc = check_search_args(c, metric, queries, query_dtype, query_dim, nq, k, out_scores, out_indices)) return rc;
    if (const int rc = check_lambda(lambda)) return rc;
    if (m > MVFGPU_MMR_MAX_CANDIDATES)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "at most " + std::to_string(MVFGPU_MMR_MAX_CANDIDATES) +
                                                      " candidates per query (MVFGPU_MMR_MAX_CANDIDATES), got " + std::to_string(m));
    return MVF_OK;
}

// The device work of both calls: queries, lists and results in device memory, everything on `s`, no host wait.
// marks (the stage timer only): per window three events, recorded at its start, behind the relevance and behind D0.
int mmr_core(const CorpusView& v, uint8_t metric, const void* d_queries, uint32_t nq, const uint64_t* d_cand, uint32_t m, uint32_t k,
             float lambda, float* d_scores, uint64_t* d_indices, int32_t* d_raw, float* d_objective, uint64_t* d_counts, hipStream_t s,
             std::vector<hipEvent_t>* marks = nullptr) {
    if (const int rc = fill_padding(metric, nq, k, d_scores, d_indices, d_raw, s)) return rc;
    if (d_objective)
        MVF_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_objective), (int)f32_bits(pad_score(metric)), (size_t)nq * k, s));
    if (m == 0) {  // nothing listed: counts 0, every entry padding
        if (d_counts) MVF_HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)nq * 8, s));
        return MVF_OK;
    }
    const OneQueryGroup g1 = one_query_group(v);
    const bool qscratch = !mmr_form(v.dtype, g1.G, g1.J).qlds;
    const size_t qrow = query_row_bytes(v);
    const size_t per_q = (size_t)m * 12 + 4 + (qscratch ? (size_t)v.dim * 4 : 0);
    const uint32_t W = (uint32_t)std::max<size_t>(1, std::min<size_t>({(size_t)nq, (size_t)kWindow, kScratchBytes / per_q}));
    AsyncBuf ddump, drows, dcnt, dq;
    MVF_HIP_TRY(ddump.alloc((size_t)W * m * 8, s));
    MVF_HIP_TRY(drows.alloc((size_t)W * m * 4, s));
    MVF_HIP_TRY(dcnt.alloc((size_t)W * 4, s));
    if (qscratch) MVF_HIP_TRY(dq.alloc((size_t)W * v.dim * 4, s));

    for (uint32_t w0 = 0; w0 < nq; w0 += W) {
        const uint32_t wn = std::min(W, nq - w0);
        auto mark = [&]() -> hipError_t {
            if (!marks) return hipSuccess;
            hipEvent_t e = nullptr;
            hipError_t rc = hipEventCreate(&e);
            if (rc != hipSuccess) return rc;
            marks->push_back(e);
            return hipEventRecord(e, s);
        };
        MVF_HIP_TRY(mark());
        CandPrepParams pp{};  // C0
        pp.cand = d_cand + (size_t)w0 * m;
        pp.m = m;
        pp.index_base = v.index_base;
        pp.n = v.n;
        pp.tomb = v.tomb;
        pp.rows = static_cast<uint32_t*>(drows.p);
        pp.counts = static_cast<uint32_t*>(dcnt.p);
        pp.out_counts = d_counts ? d_counts + w0 : nullptr;
        MVF_HIP_TRY(cand_prep_launch(pp, wn, s));
        GatherScoreParams sp{};  // the relevance: one rank entry per list position
        sp.rows = v.rows;
        sp.queries = static_cast<const unsigned char*>(d_queries) + (size_t)w0 * qrow;
        sp.list = pp.rows;
        sp.list_stride = m;
        sp.counts = pp.counts;
        sp.m = m;
        sp.nq = wn;
        sp.dim = v.dim;
        sp.pitch = v.pitch;
        sp.V = v.V;
        sp.J = g1.J;
        sp.dump = static_cast<uint64_t*>(ddump.p);
        MVF_HIP_TRY(gather_score_launch(v.dtype, metric, g1.G, 1, sp, s));
        MVF_HIP_TRY(mark());
        MmrWalkParams wp{};  // D0
        wp.rows = v.rows;
        wp.dump = sp.dump;
        wp.counts = pp.counts;
        wp.qscratch = static_cast<float*>(dq.p);
        wp.m = m;
        wp.nq = wn;
        wp.dim = v.dim;
        wp.pitch = v.pitch;
        wp.V = v.V;
        wp.J = g1.J;
        wp.k = k;
        wp.a = lambda;
        wp.b = 1.0f - lambda;
        wp.index_base = v.index_base;
        wp.ids = v.ids;
        wp.out_scores = d_scores + (size_t)w0 * k;
        wp.out_indices = d_indices + (size_t)w0 * k;
        wp.out_raw = d_raw ? d_raw + (size_t)w0 * k : nullptr;
        wp.out_objective = d_objective ? d_objective + (size_t)w0 * k : nullptr;
        MVF_HIP_TRY(mmr_walk_launch(v.dtype, metric, g1.G, wp, s));
        MVF_HIP_TRY(mark());
    }
    return MVF_OK;
}

}  // namespace

extern "C" {

int mvfgpu_search_mmr_device(const mvfgpu_corpus* c, uint8_t metric, const void* d_queries, uint8_t query_dtype, uint32_t query_dim,
                             uint32_t nq, const uint64_t* d_candidates, uint32_t m, uint32_t k, float lambda, float* d_scores,
                             uint64_t* d_indices, int32_t* d_raw, float* d_objective, uint64_t* d_counts, void* hip_stream) {
    const int rc = check_mmr_args(c, metric, d_queries, query_dtype, query_dim, nq, d_candidates, m, k, lambda, d_scores, d_indices);
    if (rc != MVF_OK) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return corpus_device_call(c, s, [&]() {
        return mmr_core(corpus_view(c), metric, d_queries, nq, d_candidates, m, k, lambda, d_scores, d_indices, d_raw, d_objective,
                        d_counts, s);
    });
}

int mvfgpu_search_mmr(const mvfgpu_corpus* c, uint8_t metric, const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                      const uint64_t* candidates, uint32_t m, uint32_t k, float lambda, float* out_scores, uint64_t* out_indices,
                      int32_t* out_raw, float* out_objective, uint64_t* out_counts) {
    const int rc0 = check_mmr_args(c, metric, queries, query_dtype, query_dim, nq, candidates, m, k, lambda, out_scores, out_indices);
    if (rc0 != MVF_OK) return rc0;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));
    const CorpusView v = corpus_view(c);
    hipStream_t s = static_cast<hipStream_t>(v.stream);
    const HostIn in[] = {{queries, query_row_bytes(v)}, {candidates, (size_t)m * 8}};
    const HostOut out[] = {{out_indices, (size_t)k * 8}, {out_scores, (size_t)k * 4}, {out_raw, (size_t)k * 4},
                           {out_objective, (size_t)k * 4}, {out_counts, 8}};
    std::vector<uint64_t> mapped;
    auto map_ids = [&](uint32_t, uint32_t wn, const void** src) {  // ids attached: a window's entries are ids
        const size_t nl = (size_t)wn * m;
        if (!nl || !v.ids) return;
        mapped.resize(nl);
        if (corpus_ids_to_positions(c, static_cast<const uint64_t*>(src[1]), nl, mapped.data())) src[1] = mapped.data();
    };
    return stage_host_windows(c, s, nq, in, out, map_ids, [&](uint32_t, uint32_t wn, void* const* d_in, void* const* d_out) {
        return mmr_core(v, metric, d_in[0], wn, static_cast<const uint64_t*>(d_in[1]), m, k, lambda, static_cast<float*>(d_out[1]),
                        static_cast<uint64_t*>(d_out[0]), static_cast<int32_t*>(d_out[2]), static_cast<float*>(d_out[3]),
                        static_cast<uint64_t*>(d_out[4]), s);
    });
}

int mvfgpu_selftest_mmr_walk(const float* rel_scores, const float* sim_scores, uint32_t m, uint8_t metric, float lambda, uint32_t k,
                             uint32_t* out_order, float* out_objective) {
    if (check_metric(metric) != MVF_OK) return -MVF_ERR_INVALID_ARGUMENT;
    if (k == 0 || k > MVFGPU_MAX_K) return -set_fail(MVF_ERR_INVALID_ARGUMENT, "k must be in 1..2^31");
    if (!out_order || (!rel_scores && m > 0) || (!sim_scores && m > 1 && k > 1)) return -set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (check_lambda(lambda) != MVF_OK) return -MVF_ERR_INVALID_ARGUMENT;
    if (m > MVFGPU_MMR_MAX_CANDIDATES)
        return -set_fail(MVF_ERR_INVALID_ARGUMENT, "at most " + std::to_string(MVFGPU_MMR_MAX_CANDIDATES) +
                                                       " candidates per query (MVFGPU_MMR_MAX_CANDIDATES), got " + std::to_string(m));
    const float a = lambda, b = 1.0f - lambda;
    const uint32_t npick = std::min(k, m);
    std::vector<float> rel(m), red(m, -INFINITY);
    std::vector<uint8_t> taken(m, 0);
    for (uint32_t i = 0; i < m; i++) rel[i] = mmr::value(rel_scores[i], metric);
    for (uint32_t j = 0; j < npick; j++) {
        uint64_t best = kPadComposite;
        for (uint32_t i = 0; i < m; i++) {
            if (taken[i]) continue;
            const uint32_t key = j == 0 ? key_from_score(rel_scores[i], metric) : mmr::order_key(mmr::objective(a, rel[i], b, red[i]));
            best = std::min(best, ((uint64_t)key << 32) | i);
        }
        const uint32_t s = (uint32_t)best;
        out_order[j] = s;
        if (out_objective) out_objective[j] = mmr::reported(j == 0 ? mmr::relevance_term(a, rel[s]) : mmr::objective(a, rel[s], b, red[s]));
        taken[s] = 1;
        if (j + 1 == npick) break;
        for (uint32_t i = 0; i < m; i++)
            if (!taken[i]) red[i] = mmr::max_ignoring_nan(red[i], mmr::value(sim_scores[(size_t)s * m + i], metric));
    }
    for (uint32_t j = npick; j < k; j++) {
        out_order[j] = 0xFFFFFFFFu;
        if (out_objective) out_objective[j] = pad_score(metric);
    }
    return (int)npick;
}

int mvfgpu_selftest_mmr_form(uint8_t data_type, uint32_t dimension, uint32_t forced_g, uint32_t* out_g, uint32_t* out_j,
                             uint32_t* out_qlds) {
    if (!out_g || !out_j || !out_qlds) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (elem_size(data_type) == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "unsupported vector data type code " + std::to_string(data_type));
    if (dimension == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "dimension must be > 0");
    if (is_int_dtype(data_type) && dimension > MVFGPU_MAX_INT_DIM)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "Int8/UInt8 dimension exceeds the exact-i32 bound (33025)");
    if ((uint64_t)dimension * elem_size(data_type) > (1ull << 30)) return set_fail(MVF_ERR_INVALID_ARGUMENT, "a row holds at most 1 GiB");
    if (forced_g != 0 && forced_g != 1 && forced_g != 4 && forced_g != 8 && forced_g != 16 && forced_g != 32 && forced_g != 64)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "forced_g must be 0, 1, 4, 8, 16, 32 or 64, got " + std::to_string(forced_g));
    const uint32_t V = (uint32_t)(((uint64_t)dimension * elem_size(data_type) + 15u) / 16u);  // alloc_rows' pitch / 16
    int G = 0;
    uint32_t J = 0;
    k1_group(V, 1, (int)forced_g, &G, &J);  // one_query_group's
    *out_g = (uint32_t)G;
    *out_j = J;
    *out_qlds = mmr_form(data_type, G, J).qlds ? 1u : 0u;
    return MVF_OK;
}

int mvfgpu_selftest_mmr_stage_ms(const mvfgpu_corpus* c, uint8_t metric, const void* d_queries, uint8_t query_dtype, uint32_t query_dim,
                                 uint32_t nq, const uint64_t* d_candidates, uint32_t m, uint32_t k, float lambda, float* d_scores,
                                 uint64_t* d_indices, int32_t* d_raw, float* d_objective, uint64_t* d_counts, void* hip_stream,
                                 float* out_ms) {
    if (!out_ms) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    int rc = check_mmr_args(c, metric, d_queries, query_dtype, query_dim, nq, d_candidates, m, k, lambda, d_scores, d_indices);
    if (rc != MVF_OK) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    std::vector<hipEvent_t> ev;
    rc = corpus_device_call(c, s, [&]() {
        return mmr_core(corpus_view(c), metric, d_queries, nq, d_candidates, m, k, lambda, d_scores, d_indices, d_raw, d_objective,
                        d_counts, s, &ev);
    });
    if (rc == MVF_OK && hipStreamSynchronize(s) != hipSuccess) rc = set_fail(MVF_ERR_DEVICE, "hipStreamSynchronize failed");
    out_ms[0] = out_ms[1] = 0.0f;
    for (size_t i = 0; i + 2 < ev.size() && rc == MVF_OK; i += 3)
        for (int st = 0; st < 2 && rc == MVF_OK; st++) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, ev[i + st], ev[i + st + 1]) != hipSuccess) rc = set_fail(MVF_ERR_DEVICE, "hipEventElapsedTime failed");
            out_ms[st] += ms;
        }
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    return rc;
}

}  // extern "C"
