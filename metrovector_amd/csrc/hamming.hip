// hamming.hip — mvfgpu_search_hamming / mvfgpu_search_hamming_device: the exact top-k by Hamming distance over the bit-packed
// rows of a UInt8 corpus (include/mvf_gpu_hamming.h; DESIGN.md §3 "Hamming search", §5 "H0 / H1 — Hamming search").
//
// Per window of up to 1024 queries, on one stream: H0 scans the rows once per query tile and leaves each row slice's sorted
// best k per query, H1 merges a query's lists and writes its results (scan_hamming.hip).  The scratch is the lists alone.
// Where hamming_route says so (include/mvf_gpu_hamming_route.h), HQ and H2 stand in H0's place: the same lists from the matrix
// unit, with the prepared queries and the candidate buffers as further scratch (scan_hamming_mfma.hip; §5 "HQ / H2").
// The host call runs the same device work per host window (host_staging.h); both calls keep mvfgpu_search_device's stream
// discipline (corpus_device_call).  Nothing here reads norms, shadows or the repair feedback.

#include "../../include/mvf_gpu_hamming.h"
#include "../../include/mvf_gpu_hamming_route.h"

#include "host_staging.h"
#include "internal.h"
#include "mvf_common.h"
#include "scan_hamming.h"
#include "scan_hamming_mfma.h"

#include <algorithm>
#include <string>

using namespace mvf;

namespace {

constexpr uint32_t kWindow = 1024;  // queries per window at most: hamming_form's nq

int check_hamming_args(const mvfgpu_corpus* c, const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t k,
                       const void* out_scores, const void* out_indices) {
    // what needs no handle first (mvfgpu_search's codes and messages), then this call's own limit, then the handle and
    // mvfgpu_search's checks of the query: nothing below touches the device on a refusal
    if (const int rc = check_search_scalars(MVF_METRIC_L2, nq, k, queries, out_scores, out_indices)) return rc;
    if (k > MVFGPU_K_PER_PASS)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "k above 1024 is not built for Hamming search, got " + std::to_string(k));
    if (!c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    if (corpus_view(c).dtype != MVF_DTYPE_UINT8) return set_fail(MVF_ERR_BUILD, "Hamming search takes a UInt8 corpus of bit-packed rows");
    return check_search_args(c, MVF_METRIC_L2, queries, query_dtype, query_dim, nq, k, out_scores, out_indices);
}

}  // namespace

namespace mvf {

// The device work of both calls (internal.h): queries and results in device memory, everything on `s`, no host wait.  tomb: the
// mask of the rows that are never returned -- the handle's tombstones, or a filter's deny mask (hamming_filtered.hip).
// ms (the stage timer only): the windows' times before H1 (H0, or HQ + H2) and of H1 are added to ms[0..1]; waits for each window.
int hamming_core(const CorpusView& v, const uint32_t* tomb, const void* d_queries, uint32_t nq, uint32_t k, float* d_scores,
                 uint64_t* d_indices, int32_t* d_raw, hipStream_t s, float* ms) {
    hipEvent_t marks[3] = {nullptr, nullptr, nullptr};
    int rc = MVF_OK;
    if (ms)
        for (hipEvent_t& e : marks)
            if (rc == MVF_OK && hipEventCreate(&e) != hipSuccess) rc = set_fail(MVF_ERR_DEVICE, "hipEventCreate failed");
    for (uint32_t w0 = 0; w0 < nq && rc == MVF_OK; w0 += kWindow) {
        const uint32_t wn = std::min(kWindow, nq - w0);
        const bool mfma = hamming_route(v.dim, wn, k, v.n, v.hamming_route) == 2u;
        const HammingForm f = hamming_form(v.dim, wn, k, v.n, (uint32_t)v.num_cus);
        const HammingMfmaForm mf = mfma ? hamming_mfma_form(v.dim, wn, k, v.n, (uint32_t)v.num_cus) : HammingMfmaForm{};
        const uint32_t row_slices = mfma ? mf.row_slices : f.row_slices, kcap = f.kcap;
        AsyncBuf dlists, dprepared, dcand;
        hipError_t ea = dlists.alloc((size_t)wn * row_slices * kcap * 8, s);
        if (ea == hipSuccess && mfma) ea = dprepared.alloc((size_t)mf.prepared_bytes, s);
        if (ea == hipSuccess && mfma) ea = dcand.alloc((size_t)mf.scratch_bytes, s);
        if (ea != hipSuccess) {  // (the timer's events are destroyed below)
            rc = set_fail(MVF_ERR_DEVICE, std::string("the slices' lists: ") + hipGetErrorString(ea));
            break;
        }
        HammingParams p{};
        p.rows = v.rows;
        p.queries = static_cast<const unsigned char*>(d_queries) + (size_t)w0 * v.dim;
        p.tomb = tomb;
        p.n = v.n;
        p.slice_rows = mfma ? mf.slice_rows : f.slice_rows;
        p.dim = v.dim;
        p.pitch = v.pitch;
        p.V = v.V;
        p.nq = wn;
        p.k = k;
        p.kcap = f.kcap;
        p.buf = f.buf;
        p.query_tile = mfma ? mf.query_tile : f.query_tile;
        p.row_slices = row_slices;
        p.lists = static_cast<uint64_t*>(dlists.p);
        p.index_base = v.index_base;
        p.ids = v.ids;
        p.out_scores = d_scores + (size_t)w0 * k;
        p.out_indices = d_indices + (size_t)w0 * k;
        p.out_raw = d_raw ? d_raw + (size_t)w0 * k : nullptr;
        hipError_t e;
        if (mfma) {
            HammingMfmaParams a{};
            a.p = p;
            a.chunks = mf.chunks;
            a.tiles = mf.tiles;
            a.prepared = static_cast<unsigned char*>(dprepared.p);
            a.starts = reinterpret_cast<float*>(a.prepared + (size_t)mf.tiles * mf.query_tile * ham_mfma_query_bytes(mf.chunks));
            a.cand = static_cast<uint64_t*>(dcand.p);
            e = hamming_mfma_launch(mf, a, s, ms ? marks : nullptr);
        } else {
            e = hamming_launch(f, p, s, ms ? marks : nullptr);
        }
        if (e != hipSuccess) {
            rc = set_fail(MVF_ERR_DEVICE, std::string("hamming_launch: ") + hipGetErrorString(e));
            break;
        }
        if (ms) {
            if (hipStreamSynchronize(s) != hipSuccess) rc = set_fail(MVF_ERR_DEVICE, "hipStreamSynchronize failed");
            for (int st = 0; st < 2 && rc == MVF_OK; st++) {
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

}  // namespace mvf

extern "C" {

int mvfgpu_search_hamming_device(const mvfgpu_corpus* c, const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                                 uint32_t k, float* d_scores, uint64_t* d_indices, int32_t* d_raw, void* hip_stream) {
    const int rc = check_hamming_args(c, d_queries, query_dtype, query_dim, nq, k, d_scores, d_indices);
    if (rc != MVF_OK) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return corpus_device_call(c, s, [&]() {
        const CorpusView v = corpus_view(c);
        return hamming_core(v, v.tomb, d_queries, nq, k, d_scores, d_indices, d_raw, s);
    });
}

int mvfgpu_search_hamming(const mvfgpu_corpus* c, const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t k,
                          float* out_scores, uint64_t* out_indices, int32_t* out_raw) {
    const int rc0 = check_hamming_args(c, queries, query_dtype, query_dim, nq, k, out_scores, out_indices);
    if (rc0 != MVF_OK) return rc0;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));
    const CorpusView v = corpus_view(c);
    hipStream_t s = static_cast<hipStream_t>(v.stream);
    const HostIn in[] = {{queries, (size_t)v.dim}};
    const HostOut out[] = {{out_indices, (size_t)k * 8}, {out_scores, (size_t)k * 4}, {out_raw, (size_t)k * 4}};
    return stage_host_windows(c, s, nq, in, out, stage_as_given, [&](uint32_t, uint32_t wn, void* const* d_in, void* const* d_out) {
        return hamming_core(v, v.tomb, d_in[0], wn, k, static_cast<float*>(d_out[1]), static_cast<uint64_t*>(d_out[0]),
                            static_cast<int32_t*>(d_out[2]), s);
    });
}

int mvfgpu_selftest_hamming_form(uint32_t dimension, uint32_t nq, uint32_t k, uint64_t rows, uint32_t num_cus, uint32_t* out_form,
                                 uint32_t* out_lanes_per_row, uint32_t* out_query_tile, uint32_t* out_row_slices,
                                 uint32_t* out_lds_bytes, uint32_t* out_merge_entries) {
    if (dimension == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "dimension must be > 0");
    if (dimension > MVFGPU_MAX_INT_DIM) return set_fail(MVF_ERR_INVALID_ARGUMENT, "Int8/UInt8 dimension exceeds the exact-i32 bound (33025)");
    if (nq == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "nq must be > 0");
    if (k == 0 || k > MVFGPU_K_PER_PASS)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "k above 1024 is not built for Hamming search, got " + std::to_string(k));
    if (rows > 0xFFFF0000ull) return set_fail(MVF_ERR_INVALID_ARGUMENT, "a shard holds at most 2^32-65536 rows");
    const HammingForm f = hamming_form(dimension, std::min(nq, kWindow), k, rows, num_cus);
    if (out_form) *out_form = f.form;
    if (out_lanes_per_row) *out_lanes_per_row = f.lanes;
    if (out_query_tile) *out_query_tile = f.query_tile;
    if (out_row_slices) *out_row_slices = f.row_slices;
    if (out_lds_bytes) *out_lds_bytes = f.lds_bytes;
    if (out_merge_entries) *out_merge_entries = kHamMergeMax;
    return MVF_OK;
}

int mvfgpu_selftest_hamming_stage_ms(const mvfgpu_corpus* c, const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                                     uint32_t k, float* d_scores, uint64_t* d_indices, int32_t* d_raw, void* hip_stream, float* out_ms) {
    if (!out_ms) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    const int rc = check_hamming_args(c, d_queries, query_dtype, query_dim, nq, k, d_scores, d_indices);
    if (rc != MVF_OK) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    out_ms[0] = out_ms[1] = 0.0f;
    return corpus_device_call(c, s, [&]() {
        const CorpusView v = corpus_view(c);
        return hamming_core(v, v.tomb, d_queries, nq, k, d_scores, d_indices, d_raw, s, out_ms);
    });
}

int mvfgpu_selftest_hamming_route(uint32_t dimension, uint32_t nq_in_window, uint32_t k, uint64_t rows, int forced, uint32_t* out_route) {
    if (!out_route) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (forced < 0 || forced > 2) return set_fail(MVF_ERR_INVALID_ARGUMENT, "route must be 0, 1 or 2");
    if (const int rc = mvfgpu_selftest_hamming_form(dimension, nq_in_window, k, rows, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) return rc;
    *out_route = hamming_route(dimension, std::min(nq_in_window, kWindow), k, rows, forced);
    return MVF_OK;
}

int mvfgpu_selftest_hamming_mfma_form(uint32_t dimension, uint32_t nq, uint32_t k, uint64_t rows, uint32_t num_cus, uint32_t* out_query_tile,
                                      uint32_t* out_rows_per_wave, uint32_t* out_threads, uint32_t* out_row_slices, uint64_t* out_slice_rows,
                                      uint32_t* out_lds_bytes, uint64_t* out_prepared_bytes, uint64_t* out_scratch_bytes) {
    if (const int rc = mvfgpu_selftest_hamming_form(dimension, nq, k, rows, num_cus, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) return rc;
    if (hamming_route(dimension, 1, k, rows, 2) != 2u)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "rows of more than 512 packed bytes are not eligible for the MFMA route, got " + std::to_string(dimension));
    const HammingMfmaForm f = hamming_mfma_form(dimension, std::min(nq, kWindow), k, rows, num_cus);
    if (out_query_tile) *out_query_tile = f.query_tile;
    if (out_rows_per_wave) *out_rows_per_wave = f.wave_rows;
    if (out_threads) *out_threads = f.threads;
    if (out_row_slices) *out_row_slices = f.row_slices;
    if (out_slice_rows) *out_slice_rows = f.slice_rows;
    if (out_lds_bytes) *out_lds_bytes = f.lds_bytes;
    if (out_prepared_bytes) *out_prepared_bytes = f.prepared_bytes;
    if (out_scratch_bytes) *out_scratch_bytes = f.scratch_bytes;
    return MVF_OK;
}

}  // extern "C"
