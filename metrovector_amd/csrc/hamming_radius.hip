// hamming_radius.hip — mvfgpu_search_hamming_radius: every row within r bits of each query over the bit-packed rows of a UInt8
// corpus, counted exactly and listed best first (include/mvf_gpu_hamming_radius.h; DESIGN.md §3 "Hamming radius search", §5
// "HR2 / HRP").
//
// Per window of up to 1024 queries, on the handle's host-call stream: HQ prepares the queries for the matrix unit, HR2 scans
// the rows once per query tile, counts every match and appends the first MVFGPU_RADIUS_LIST_CAP of each query to its list, HRP
// sorts the lists that hold all of their query's matches and writes counts and entries (scan_hamming_radius.hip).  The scratch
// -- prepared queries, counters, lists -- is stream-ordered and per call.  Queries, radii and results travel in host windows
// (host_staging.h) under corpus_device_call.  A query with more matches than its list holds (and max_per_query > 0) has more
// than max_per_query of them, so its entries ARE its Hamming top-max_per_query: one mvfgpu_search_hamming over just those
// queries completes them, as mvfgpu_search_radius completes its overflowed queries with mvfgpu_search.  Nothing here reads
// norms, shadows or the repair feedback, and nothing is kept in the handle.

#include "../../include/mvf_gpu_hamming_radius.h"
#include "../../include/mvf_gpu_hamming.h"

#include "host_staging.h"
#include "internal.h"
#include "mvf_common.h"
#include "scan_hamming_radius.h"

#include <algorithm>
#include <string>
#include <vector>

using namespace mvf;

namespace {

constexpr uint32_t kWindow = 1024;  // queries per window at most: hamming_radius_form's nq

static_assert(kHamRadiusListCap == MVFGPU_RADIUS_LIST_CAP && kHamRadiusMaxOut == MVFGPU_K_PER_PASS, "the header's limits");

int check_hamming_radius_args(const mvfgpu_corpus* c, const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                              const void* radii, uint64_t max_per_query, const void* out_counts, const void* out_scores,
                              const void* out_indices) {
    // what needs no handle first (mvfgpu_search_radius' codes and messages: the required buffers are the queries, the radii and
    // the counts), then this call's own limit, then the handle and the query: nothing below touches the device on a refusal
    if (const int rc = check_search_scalars(MVF_METRIC_L2, nq, 1, queries, radii, out_counts)) return rc;
    if (max_per_query > 0 && (!out_scores || !out_indices))
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer (out_scores / out_indices are required when max_per_query > 0)");
    if (max_per_query > kHamRadiusMaxOut)
        return set_fail(MVF_ERR_INVALID_ARGUMENT,
                        "max_per_query above 1024 is not built for Hamming radius search, got " + std::to_string(max_per_query));
    if (!c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    const CorpusView v = corpus_view(c);
    if (v.dtype != MVF_DTYPE_UINT8) return set_fail(MVF_ERR_BUILD, "Hamming radius search takes a UInt8 corpus of bit-packed rows");
    if (v.dim > kHamRadiusMaxDim)
        return set_fail(MVF_ERR_INVALID_ARGUMENT,
                        "rows above 512 packed bytes are not built for Hamming radius search, got " + std::to_string(v.dim));
    return check_search_args(c, MVF_METRIC_L2, queries, query_dtype, query_dim, nq, 1, radii, out_counts);
}

// The device work: queries, radii and results in device memory, everything on `s`, no host wait.  The entry outputs are
// [nq][maxq] (unused where maxq = 0; d_raw nullable).
// ms (the stage timer only): the windows' times of HQ, HR2 and HRP are added to ms[0..2]; waits for each window.
int hamming_radius_core(const CorpusView& v, const void* d_queries, const uint32_t* d_radii, uint32_t nq, uint32_t maxq, uint64_t* d_counts,
                        float* d_scores, uint64_t* d_indices, int32_t* d_raw, hipStream_t s, float* ms = nullptr) {
    hipEvent_t marks[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = MVF_OK;
    if (ms)
        for (hipEvent_t& e : marks)
            if (rc == MVF_OK && hipEventCreate(&e) != hipSuccess) rc = set_fail(MVF_ERR_DEVICE, "hipEventCreate failed");
    for (uint32_t w0 = 0; w0 < nq && rc == MVF_OK; w0 += kWindow) {
        const uint32_t wn = std::min(kWindow, nq - w0);
        const HammingRadiusForm f = hamming_radius_form(v.dim, wn, v.n, (uint32_t)v.num_cus);
        AsyncBuf dprepared, dctr, dlists;
        hipError_t ea = dprepared.alloc((size_t)f.prepared_bytes, s);
        if (ea == hipSuccess) ea = dctr.alloc((size_t)wn * 8u, s);
        if (ea == hipSuccess && maxq) ea = dlists.alloc((size_t)wn * kHamRadiusListCap * 8u, s);
        if (ea == hipSuccess) ea = hipMemsetAsync(dctr.p, 0, (size_t)wn * 8u, s);
        if (ea != hipSuccess) {  // (the timer's events are destroyed below)
            rc = set_fail(MVF_ERR_DEVICE, std::string("the Hamming radius search's scratch: ") + hipGetErrorString(ea));
            break;
        }
        HammingRadiusParams r{};
        HammingParams& p = r.a.p;
        p.rows = v.rows;
        p.queries = static_cast<const unsigned char*>(d_queries) + (size_t)w0 * v.dim;
        p.tomb = v.tomb;
        p.n = v.n;
        p.slice_rows = f.slice_rows;
        p.dim = v.dim;
        p.pitch = v.pitch;
        p.V = v.V;
        p.nq = wn;
        p.k = maxq;
        p.query_tile = f.query_tile;
        p.row_slices = f.row_slices;
        p.index_base = v.index_base;
        p.ids = v.ids;
        p.out_scores = maxq ? d_scores + (size_t)w0 * maxq : nullptr;
        p.out_indices = maxq ? d_indices + (size_t)w0 * maxq : nullptr;
        p.out_raw = maxq && d_raw ? d_raw + (size_t)w0 * maxq : nullptr;
        r.a.chunks = f.chunks;
        r.a.tiles = f.tiles;
        r.a.prepared = static_cast<unsigned char*>(dprepared.p);
        r.a.starts = reinterpret_cast<float*>(r.a.prepared + (size_t)f.tiles * f.query_tile * ham_mfma_query_bytes(f.chunks));
        r.radii = d_radii + w0;
        r.counts = static_cast<uint32_t*>(dctr.p);
        r.fill = r.counts + wn;
        r.lists = static_cast<uint64_t*>(dlists.p);
        r.cap = kHamRadiusListCap;
        r.kout = maxq;
        r.out_counts = d_counts + w0;
        const hipError_t e = hamming_radius_launch(f, r, s, ms ? marks : nullptr);
        if (e != hipSuccess) {
            rc = set_fail(MVF_ERR_DEVICE, std::string("hamming_radius_launch: ") + hipGetErrorString(e));
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

int mvfgpu_search_hamming_radius(const mvfgpu_corpus* c, const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                                 const uint32_t* radii, uint64_t max_per_query, uint64_t* out_counts, float* out_scores,
                                 uint64_t* out_indices, int32_t* out_raw) {
    const int rc0 = check_hamming_radius_args(c, queries, query_dtype, query_dim, nq, radii, max_per_query, out_counts, out_scores, out_indices);
    if (rc0 != MVF_OK) return rc0;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    const uint32_t maxq = (uint32_t)max_per_query;
    size_t dim = 0;
    {
        std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));
        const CorpusView v = corpus_view(c);
        dim = v.dim;
        hipStream_t s = static_cast<hipStream_t>(v.stream);
        const HostIn in[] = {{queries, (size_t)v.dim}, {radii, 4}};
        const HostOut out[] = {{out_counts, 8, true}, {out_indices, (size_t)maxq * 8}, {out_scores, (size_t)maxq * 4}, {out_raw, (size_t)maxq * 4}};
        const int rc = stage_host_windows(c, s, nq, in, out, stage_as_given, [&](uint32_t, uint32_t wn, void* const* d_in, void* const* d_out) {
            return hamming_radius_core(v, d_in[0], static_cast<const uint32_t*>(d_in[1]), wn, maxq, static_cast<uint64_t*>(d_out[0]),
                                       static_cast<float*>(d_out[2]), static_cast<uint64_t*>(d_out[1]), static_cast<int32_t*>(d_out[3]), s);
        });
        if (rc != MVF_OK) return rc;
    }
    if (maxq == 0) return MVF_OK;
    // the top-k identity: a query whose list ran over has more than cap >= max_per_query matches, so its entries are its Hamming
    // top-max_per_query and every one of them is a match; one search for all such queries (the host knows the counts: the call
    // is blocking)
    std::vector<uint32_t> over;
    for (uint32_t q = 0; q < nq; q++)
        if (out_counts[q] > kHamRadiusListCap) over.push_back(q);
    if (over.empty()) return MVF_OK;
    const uint32_t no = (uint32_t)over.size();
    std::vector<unsigned char> qb((size_t)no * dim);
    for (uint32_t i = 0; i < no; i++)
        std::copy_n(static_cast<const unsigned char*>(queries) + (size_t)over[i] * dim, dim, qb.data() + (size_t)i * dim);
    std::vector<float> sc((size_t)no * maxq);
    std::vector<uint64_t> idx((size_t)no * maxq);
    std::vector<int32_t> raw((size_t)no * maxq);
    const int rc = mvfgpu_search_hamming(c, qb.data(), query_dtype, query_dim, no, maxq, sc.data(), idx.data(), raw.data());
    if (rc != MVF_OK) return rc;
    for (uint32_t i = 0; i < no; i++) {
        const size_t src = (size_t)i * maxq, dst = (size_t)over[i] * maxq;
        std::copy_n(sc.begin() + src, maxq, out_scores + dst);
        std::copy_n(idx.begin() + src, maxq, out_indices + dst);
        if (out_raw) std::copy_n(raw.begin() + src, maxq, out_raw + dst);
    }
    return MVF_OK;
}

int mvfgpu_selftest_hamming_radius_form(uint32_t dimension, uint32_t nq, uint64_t rows, uint32_t num_cus, uint32_t* out_query_tile,
                                        uint32_t* out_row_slices, uint32_t* out_blocks_per_cu, uint32_t* out_chunks,
                                        uint32_t* out_lds_bytes, uint64_t* out_scratch_bytes) {
    if (dimension == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "dimension must be > 0");
    if (dimension > kHamRadiusMaxDim)
        return set_fail(MVF_ERR_INVALID_ARGUMENT,
                        "rows above 512 packed bytes are not built for Hamming radius search, got " + std::to_string(dimension));
    if (nq == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "nq must be > 0");
    if (rows > 0xFFFF0000ull) return set_fail(MVF_ERR_INVALID_ARGUMENT, "a shard holds at most 2^32-65536 rows");
    const HammingRadiusForm f = hamming_radius_form(dimension, std::min(nq, kWindow), rows, num_cus);
    if (out_query_tile) *out_query_tile = f.query_tile;
    if (out_row_slices) *out_row_slices = f.row_slices;
    if (out_blocks_per_cu) *out_blocks_per_cu = f.blocks_per_cu;
    if (out_chunks) *out_chunks = f.chunks;
    if (out_lds_bytes) *out_lds_bytes = f.lds_bytes;
    if (out_scratch_bytes) *out_scratch_bytes = f.scratch_bytes;
    return MVF_OK;
}

int mvfgpu_selftest_hamming_radius_stage_ms(const mvfgpu_corpus* c, const void* d_queries, uint8_t query_dtype, uint32_t query_dim,
                                            uint32_t nq, const uint32_t* d_radii, uint64_t max_per_query, uint64_t* d_counts,
                                            float* d_scores, uint64_t* d_indices, int32_t* d_raw, void* hip_stream, float* out_ms) {
    if (!out_ms) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    const int rc = check_hamming_radius_args(c, d_queries, query_dtype, query_dim, nq, d_radii, max_per_query, d_counts, d_scores, d_indices);
    if (rc != MVF_OK) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    out_ms[0] = out_ms[1] = out_ms[2] = 0.0f;
    return corpus_device_call(c, s, [&]() {
        return hamming_radius_core(corpus_view(c), d_queries, d_radii, nq, (uint32_t)max_per_query, d_counts, d_scores, d_indices, d_raw, s, out_ms);
    });
}

}  // extern "C"
