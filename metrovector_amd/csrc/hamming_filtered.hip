// hamming_filtered.hip — mvfgpu_search_hamming_filtered / mvfgpu_search_hamming_filtered_device: the exact Hamming top-k among
// the bit-packed rows a filter admits (include/mvf_gpu_hamming_filtered.h; DESIGN.md §3 "Filtered Hamming search", §5 "HG").
//
// Per window of up to 1024 queries, on one stream, one of two routes (hamming_filter_route, scan_hamming_gather.h):
//   mask: hamming_core (hamming.hip) with the filter's deny mask in the tombstones' place -- the Hamming search's own kernels;
//   list: HQ prepares the queries, HG (scan_hamming_gather.hip) scans the rows the filter's list names, H1 merges.
// The scratch -- lists, prepared queries, candidate buffers -- is stream-ordered and per call.  The host call runs the same
// device work per host window (host_staging.h); both calls keep mvfgpu_search_device's stream discipline (corpus_device_call).
// Nothing here reads norms, shadows or the repair feedback, and nothing is kept in the handle or the filter.

#include "../../include/mvf_gpu_hamming_filtered.h"

#include "host_staging.h"
#include "internal.h"
#include "mvf_common.h"
#include "scan_hamming_gather.h"

#include <algorithm>
#include <string>

using namespace mvf;

namespace {

constexpr uint32_t kWindow = 1024;  // queries per window at most: hamming_gather_form's nq

int check_hamming_filtered_args(const mvfgpu_corpus* c, const mvfgpu_filter* f, const void* queries, uint8_t query_dtype,
                                uint32_t query_dim, uint32_t nq, uint32_t k, const void* out_scores, const void* out_indices,
                                FilterUse* use) {
    // the Hamming search's order with the filter's checks around the handle's: nothing below touches the device on a refusal
    if (const int rc = check_search_scalars(MVF_METRIC_L2, nq, k, queries, out_scores, out_indices)) return rc;
    if (k > MVFGPU_K_PER_PASS)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "k above 1024 is not built for filtered Hamming search, got " + std::to_string(k));
    if (!f) return set_fail(MVF_ERR_INVALID_ARGUMENT, "filter is NULL");
    if (!c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    if (corpus_view(c).dtype != MVF_DTYPE_UINT8)
        return set_fail(MVF_ERR_BUILD, "filtered Hamming search takes a UInt8 corpus of bit-packed rows");
    if (const int rc = check_search_args(c, MVF_METRIC_L2, queries, query_dtype, query_dim, nq, k, out_scores, out_indices)) return rc;
    return filter_check_use(c, f, use);
}

// One window on the list route: HQ, HG, H1 on `s`.  marks: the stage timer's four events, or NULL.
int gather_window(const CorpusView& v, const FilterUse& flt, const void* d_queries, uint32_t wn, uint32_t k, float* d_scores,
                  uint64_t* d_indices, int32_t* d_raw, hipStream_t s, hipEvent_t* marks) {
    const HammingGatherForm f = hamming_gather_form(v.dim, wn, k, flt.admitted, (uint32_t)v.num_cus);
    AsyncBuf dlists, dprepared, dcand;
    hipError_t ea = dlists.alloc((size_t)wn * f.list_slices * f.kcap * 8, s);
    if (ea == hipSuccess) ea = dprepared.alloc((size_t)f.prepared_bytes, s);
    if (ea == hipSuccess) ea = dcand.alloc((size_t)f.scratch_bytes, s);
    if (ea != hipSuccess) return set_fail(MVF_ERR_DEVICE, std::string("the list slices' lists: ") + hipGetErrorString(ea));
    HammingGatherParams g{};
    HammingParams& p = g.a.p;
    p.rows = v.rows;
    p.queries = static_cast<const unsigned char*>(d_queries);
    p.tomb = nullptr;  // the list holds admitted live rows only
    p.n = v.n;
    p.dim = v.dim;
    p.pitch = v.pitch;
    p.V = v.V;
    p.nq = wn;
    p.k = k;
    p.kcap = f.kcap;
    p.buf = f.buf;
    p.query_tile = f.query_tile;
    p.row_slices = f.list_slices;
    p.lists = static_cast<uint64_t*>(dlists.p);
    p.index_base = v.index_base;
    p.ids = v.ids;
    p.out_scores = d_scores;
    p.out_indices = d_indices;
    p.out_raw = d_raw;
    g.a.chunks = f.chunks;
    g.a.tiles = f.tiles;
    g.a.prepared = static_cast<unsigned char*>(dprepared.p);
    g.a.starts = reinterpret_cast<float*>(g.a.prepared + (size_t)f.tiles * f.query_tile * ham_mfma_query_bytes(f.chunks));
    g.a.cand = static_cast<uint64_t*>(dcand.p);
    g.list = flt.list;
    g.m = (uint32_t)flt.admitted;  // a shard holds fewer than 2^32 rows
    g.slice_entries = (uint32_t)f.slice_entries;
    const hipError_t e = hamming_gather_launch(f, g, s, marks);
    if (e != hipSuccess) return set_fail(MVF_ERR_DEVICE, std::string("hamming_gather_launch: ") + hipGetErrorString(e));
    return MVF_OK;
}

// The device work of both calls: queries and results in device memory, everything on `s`, no host wait.
// ms (the stage timer only): the windows' times of prepare, scan and merge are added to ms[0..2]; waits for each window.
int hamming_filtered_core(const CorpusView& v, const FilterUse& flt, const void* d_queries, uint32_t nq, uint32_t k, float* d_scores,
                          uint64_t* d_indices, int32_t* d_raw, hipStream_t s, float* ms = nullptr) {
    hipEvent_t marks[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = MVF_OK;
    if (ms)
        for (hipEvent_t& e : marks)
            if (rc == MVF_OK && hipEventCreate(&e) != hipSuccess) rc = set_fail(MVF_ERR_DEVICE, "hipEventCreate failed");
    for (uint32_t w0 = 0; w0 < nq && rc == MVF_OK; w0 += kWindow) {
        const uint32_t wn = std::min(kWindow, nq - w0);
        const void* wq = static_cast<const unsigned char*>(d_queries) + (size_t)w0 * v.dim;
        float* wsc = d_scores + (size_t)w0 * k;
        uint64_t* widx = d_indices + (size_t)w0 * k;
        int32_t* wraw = d_raw ? d_raw + (size_t)w0 * k : nullptr;
        if (hamming_filter_route(v.dim, wn, k, v.n, flt.admitted, flt.list != nullptr, flt.forced_route) != 2u) {
            rc = hamming_core(v, flt.deny, wq, wn, k, wsc, widx, wraw, s, ms ? ms + 1 : nullptr);  // (its two stages: scan, merge)
            continue;
        }
        rc = gather_window(v, flt, wq, wn, k, wsc, widx, wraw, s, ms ? marks : nullptr);
        if (ms && rc == MVF_OK) {
            if (hipStreamSynchronize(s) != hipSuccess) rc = set_fail(MVF_ERR_DEVICE, "hipStreamSynchronize failed");
            for (int st = 0; st < 3 && rc == MVF_OK; st++) {
                float t = 0.0f;
                if (hipEventElapsedTime(&t, marks[st], marks[st + 1]) != hipSuccess) rc = set_fail(MVF_ERR_DEVICE, "hipEventElapsedTime failed");
                ms[st] += t;
            }
        }
    }
    for (hipEvent_t e : marks)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

}  // namespace

extern "C" {

int mvfgpu_search_hamming_filtered_device(const mvfgpu_corpus* c, const mvfgpu_filter* f, const void* d_queries, uint8_t query_dtype,
                                          uint32_t query_dim, uint32_t nq, uint32_t k, float* d_scores, uint64_t* d_indices,
                                          int32_t* d_raw, void* hip_stream) {
    FilterUse use;
    const int rc = check_hamming_filtered_args(c, f, d_queries, query_dtype, query_dim, nq, k, d_scores, d_indices, &use);
    if (rc != MVF_OK) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return corpus_device_call(c, s, [&]() { return hamming_filtered_core(corpus_view(c), use, d_queries, nq, k, d_scores, d_indices, d_raw, s); });
}

int mvfgpu_search_hamming_filtered(const mvfgpu_corpus* c, const mvfgpu_filter* f, const void* queries, uint8_t query_dtype,
                                   uint32_t query_dim, uint32_t nq, uint32_t k, float* out_scores, uint64_t* out_indices,
                                   int32_t* out_raw) {
    FilterUse use;
    const int rc0 = check_hamming_filtered_args(c, f, queries, query_dtype, query_dim, nq, k, out_scores, out_indices, &use);
    if (rc0 != MVF_OK) return rc0;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));
    const CorpusView v = corpus_view(c);
    hipStream_t s = static_cast<hipStream_t>(v.stream);
    const HostIn in[] = {{queries, (size_t)v.dim}};
    const HostOut out[] = {{out_indices, (size_t)k * 8}, {out_scores, (size_t)k * 4}, {out_raw, (size_t)k * 4}};
    return stage_host_windows(c, s, nq, in, out, stage_as_given, [&](uint32_t, uint32_t wn, void* const* d_in, void* const* d_out) {
        return hamming_filtered_core(v, use, d_in[0], wn, k, static_cast<float*>(d_out[1]), static_cast<uint64_t*>(d_out[0]),
                                     static_cast<int32_t*>(d_out[2]), s);
    });
}

int mvfgpu_selftest_hamming_filtered_form(uint32_t dimension, uint32_t nq, uint32_t k, uint64_t rows, uint64_t admitted,
                                          uint32_t has_row_list, int forced_route, uint32_t num_cus, uint32_t* out_route,
                                          uint32_t* out_query_tile, uint32_t* out_chunks, uint32_t* out_list_slices,
                                          uint64_t* out_slice_entries, uint32_t* out_lds_bytes, uint64_t* out_scratch_bytes) {
    if (dimension == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "dimension must be > 0");
    if (dimension > MVFGPU_MAX_INT_DIM) return set_fail(MVF_ERR_INVALID_ARGUMENT, "Int8/UInt8 dimension exceeds the exact-i32 bound (33025)");
    if (nq == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "nq must be > 0");
    if (k == 0 || k > MVFGPU_K_PER_PASS)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "k above 1024 is not built for filtered Hamming search, got " + std::to_string(k));
    if (rows > 0xFFFF0000ull) return set_fail(MVF_ERR_INVALID_ARGUMENT, "a shard holds at most 2^32-65536 rows");
    if (admitted > rows) return set_fail(MVF_ERR_INVALID_ARGUMENT, "a filter admits at most the shard's rows");
    if (has_row_list > 1u) return set_fail(MVF_ERR_INVALID_ARGUMENT, "has_row_list must be 0 or 1");
    if (forced_route < 0 || forced_route > 2) return set_fail(MVF_ERR_INVALID_ARGUMENT, "route must be 0, 1 or 2");
    const uint32_t wn = std::min(nq, kWindow);
    const uint32_t route = hamming_filter_route(dimension, wn, k, rows, admitted, has_row_list != 0u, forced_route);
    const HammingGatherForm f = route == 2u ? hamming_gather_form(dimension, wn, k, admitted, num_cus) : HammingGatherForm{};
    if (out_route) *out_route = route;
    if (out_query_tile) *out_query_tile = f.query_tile;
    if (out_chunks) *out_chunks = f.chunks;
    if (out_list_slices) *out_list_slices = f.list_slices;
    if (out_slice_entries) *out_slice_entries = f.slice_entries;
    if (out_lds_bytes) *out_lds_bytes = f.lds_bytes;
    if (out_scratch_bytes) *out_scratch_bytes = f.scratch_bytes;
    return MVF_OK;
}

int mvfgpu_selftest_hamming_filtered_stage_ms(const mvfgpu_corpus* c, const mvfgpu_filter* f, const void* d_queries, uint8_t query_dtype,
                                              uint32_t query_dim, uint32_t nq, uint32_t k, float* d_scores, uint64_t* d_indices,
                                              int32_t* d_raw, void* hip_stream, float* out_ms) {
    if (!out_ms) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    FilterUse use;
    const int rc = check_hamming_filtered_args(c, f, d_queries, query_dtype, query_dim, nq, k, d_scores, d_indices, &use);
    if (rc != MVF_OK) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    out_ms[0] = out_ms[1] = out_ms[2] = 0.0f;
    return corpus_device_call(c, s, [&]() {
        return hamming_filtered_core(corpus_view(c), use, d_queries, nq, k, d_scores, d_indices, d_raw, s, out_ms);
    });
}

}  // extern "C"
