// tanimoto.hip — mvfgpu_search_tanimoto / mvfgpu_search_tanimoto_device: the exact top-k by Jaccard / Tanimoto similarity of
// UInt8 queries against the bit-packed rows of a UInt8 corpus, T(q, x) = popcount(q & x) / popcount(q | x)
// (include/mvf_gpu_tanimoto.h; DESIGN.md §3 "Tanimoto search", §5 "TQ / T2").
//
// Per window of up to 1024 queries, on one stream: TQ prepares the queries in the matrix unit's order, T2 scans the rows once per
// query tile and leaves each row slice's sorted best k per query, H1 (the Hamming search's merge) writes the results
// (scan_tanimoto.hip).  The scratch -- prepared queries, candidate buffers, lists -- is stream-ordered and per call, as
// hamming.hip's.  The host call runs the same device work per host window (host_staging.h); both calls keep
// mvfgpu_search_device's stream discipline (corpus_device_call).  Nothing here reads norms, shadows or the repair feedback, and
// nothing is kept in the handle: the rows' popcounts come out of the scan itself.

#include "../../include/mvf_gpu_tanimoto.h"

#include "host_staging.h"
#include "internal.h"
#include "mvf_common.h"
#include "scan_tanimoto.h"

#include <algorithm>
#include <string>

using namespace mvf;

namespace {

constexpr uint32_t kWindow = 1024;  // queries per window at most: tanimoto_form's nq

int check_tanimoto_args(const mvfgpu_corpus* c, const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t k,
                        const void* out_scores, const void* out_indices) {
    // the sign-bit search's order: what needs no handle first (mvfgpu_search's codes and messages), then this call's own limit,
    // then the handle and the query: nothing below touches the device on a refusal
    if (const int rc = check_search_scalars(MVF_METRIC_INNER_PRODUCT, nq, k, queries, out_scores, out_indices)) return rc;
    if (k > MVFGPU_K_PER_PASS)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "k above 1024 is not built for Tanimoto search, got " + std::to_string(k));
    if (!c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    const CorpusView v = corpus_view(c);
    if (v.dtype != MVF_DTYPE_UINT8) return set_fail(MVF_ERR_BUILD, "Tanimoto search takes a UInt8 corpus of bit-packed rows");
    if (v.dim > kTaniMaxDim)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "rows above 512 packed bytes are not built for Tanimoto search, got " + std::to_string(v.dim));
    if (query_dtype != MVF_DTYPE_UINT8) return set_fail(MVF_ERR_BUILD, "Tanimoto search takes UInt8 queries");
    if (query_dim != v.dim)
        return set_fail(MVF_ERR_DIMENSION_MISMATCH, "Dimension mismatch: expected " + std::to_string(v.dim) + ", got " + std::to_string(query_dim));
    return MVF_OK;
}

// The device work of both calls: queries and results in device memory, everything on `s`, no host wait.
// ms (the stage timer only): the windows' times of TQ, T2 and H1 are added to ms[0..2]; waits for each window.
int tanimoto_core(const CorpusView& v, const void* d_queries, uint32_t nq, uint32_t k, float* d_scores, uint64_t* d_indices, hipStream_t s,
                  float* ms = nullptr) {
    hipEvent_t marks[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = MVF_OK;
    if (ms)
        for (hipEvent_t& e : marks)
            if (rc == MVF_OK && hipEventCreate(&e) != hipSuccess) rc = set_fail(MVF_ERR_DEVICE, "hipEventCreate failed");
    for (uint32_t w0 = 0; w0 < nq && rc == MVF_OK; w0 += kWindow) {
        const uint32_t wn = std::min(kWindow, nq - w0);
        const TanimotoForm f = tanimoto_form(v.dim, wn, k, v.n, (uint32_t)v.num_cus);
        AsyncBuf dlists, dprepared, dcand;
        hipError_t ea = dlists.alloc((size_t)wn * f.row_slices * f.kcap * 8, s);
        if (ea == hipSuccess) ea = dprepared.alloc((size_t)f.prepared_bytes, s);
        if (ea == hipSuccess) ea = dcand.alloc((size_t)f.scratch_bytes, s);
        if (ea != hipSuccess) {  // (the timer's events are destroyed below)
            rc = set_fail(MVF_ERR_DEVICE, std::string("the Tanimoto search's scratch: ") + hipGetErrorString(ea));
            break;
        }
        TanimotoParams a{};
        HammingParams& p = a.p;
        p.rows = v.rows;
        p.queries = static_cast<const unsigned char*>(d_queries) + (size_t)w0 * v.dim;
        p.tomb = v.tomb;
        p.n = v.n;
        p.slice_rows = f.slice_rows;
        p.dim = v.dim;
        p.pitch = v.pitch;
        p.V = v.V;
        p.nq = wn;
        p.k = k;
        p.kcap = f.kcap;
        p.buf = f.buf;
        p.query_tile = f.query_tile;
        p.row_slices = f.row_slices;
        p.lists = static_cast<uint64_t*>(dlists.p);
        p.index_base = v.index_base;
        p.ids = v.ids;
        p.out_scores = d_scores + (size_t)w0 * k;
        p.out_indices = d_indices + (size_t)w0 * k;
        p.out_raw = nullptr;
        p.score_bias = kTaniBias;
        p.float_key = 1u;
        a.chunks = f.chunks;
        a.tiles = f.tiles;
        a.prepared = static_cast<unsigned char*>(dprepared.p);
        a.pops = reinterpret_cast<float*>(a.prepared + (size_t)f.tiles * f.query_tile * tani_query_bytes(f.chunks));
        a.cand = static_cast<uint64_t*>(dcand.p);
        const hipError_t e = tanimoto_launch(f, a, s, ms ? marks : nullptr);
        if (e != hipSuccess) {
            rc = set_fail(MVF_ERR_DEVICE, std::string("tanimoto_launch: ") + hipGetErrorString(e));
            break;
        }
        if (ms) {
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

int mvfgpu_search_tanimoto_device(const mvfgpu_corpus* c, const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                                  uint32_t k, float* d_scores, uint64_t* d_indices, void* hip_stream) {
    const int rc = check_tanimoto_args(c, d_queries, query_dtype, query_dim, nq, k, d_scores, d_indices);
    if (rc != MVF_OK) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return corpus_device_call(c, s, [&]() { return tanimoto_core(corpus_view(c), d_queries, nq, k, d_scores, d_indices, s); });
}

int mvfgpu_search_tanimoto(const mvfgpu_corpus* c, const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t k,
                           float* out_scores, uint64_t* out_indices) {
    const int rc0 = check_tanimoto_args(c, queries, query_dtype, query_dim, nq, k, out_scores, out_indices);
    if (rc0 != MVF_OK) return rc0;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));
    const CorpusView v = corpus_view(c);
    hipStream_t s = static_cast<hipStream_t>(v.stream);
    const HostIn in[] = {{queries, (size_t)v.dim}};
    const HostOut out[] = {{out_indices, (size_t)k * 8}, {out_scores, (size_t)k * 4}};
    return stage_host_windows(c, s, nq, in, out, stage_as_given, [&](uint32_t, uint32_t wn, void* const* d_in, void* const* d_out) {
        return tanimoto_core(v, d_in[0], wn, k, static_cast<float*>(d_out[1]), static_cast<uint64_t*>(d_out[0]), s);
    });
}

int mvfgpu_selftest_tanimoto_form(uint32_t dimension, uint32_t nq, uint32_t k, uint64_t rows, uint32_t num_cus, uint32_t* out_query_tile,
                                  uint32_t* out_chunks, uint32_t* out_row_slices, uint64_t* out_slice_rows, uint32_t* out_lds_bytes,
                                  uint64_t* out_scratch_bytes) {
    if (dimension == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "dimension must be > 0");
    if (dimension > kTaniMaxDim)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "rows above 512 packed bytes are not built for Tanimoto search, got " + std::to_string(dimension));
    if (nq == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "nq must be > 0");
    if (k == 0 || k > MVFGPU_K_PER_PASS)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "k above 1024 is not built for Tanimoto search, got " + std::to_string(k));
    if (rows > 0xFFFF0000ull) return set_fail(MVF_ERR_INVALID_ARGUMENT, "a shard holds at most 2^32-65536 rows");
    const TanimotoForm f = tanimoto_form(dimension, std::min(nq, kWindow), k, rows, num_cus);
    if (out_query_tile) *out_query_tile = f.query_tile;
    if (out_chunks) *out_chunks = f.chunks;
    if (out_row_slices) *out_row_slices = f.row_slices;
    if (out_slice_rows) *out_slice_rows = f.slice_rows;
    if (out_lds_bytes) *out_lds_bytes = f.lds_bytes;
    if (out_scratch_bytes) *out_scratch_bytes = f.scratch_bytes;
    return MVF_OK;
}

int mvfgpu_selftest_tanimoto_stage_ms(const mvfgpu_corpus* c, const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                                      uint32_t k, float* d_scores, uint64_t* d_indices, void* hip_stream, float* out_ms) {
    if (!out_ms) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    const int rc = check_tanimoto_args(c, d_queries, query_dtype, query_dim, nq, k, d_scores, d_indices);
    if (rc != MVF_OK) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    out_ms[0] = out_ms[1] = out_ms[2] = 0.0f;
    return corpus_device_call(c, s, [&]() { return tanimoto_core(corpus_view(c), d_queries, nq, k, d_scores, d_indices, s, out_ms); });
}

}  // extern "C"
