// grouped.hip — mvfgpu_search_grouped / mvfgpu_search_grouped_device: the exact top-k of every query with at most per_key rows
// of any one key of a partition index, and mvfgpu_column_gather (include/mvf_gpu.h; DESIGN.md §3 "Grouped search", §5 "G0 / G1
// — grouped search").
//
// Per window of queries: G0 scores every row the index holds, in the index's key order, with the gathered-row kernel
// (scan_gather.hip: K1's one-query bits, four queries per read of the rows); G1 (scan_grouped.hip) keeps the per_key best
// entries of every key and writes them to a row-indexed array in which every other row is dead; the whole-list select and
// sort (sort_topk.hip) rank that array and write_sorted formats the first k.  Exact for every distribution of key sizes:
// nothing is over-fetched.  No host wait, no plan: the segments are read from the index's device key table.
// The host call runs the same device work per host window (host_staging.h).

#include "../../include/mvf_gpu.h"

#include "aux_kernels.h"
#include "host_staging.h"
#include "internal.h"
#include "mvf_common.h"
#include "scan_filter.h"
#include "scan_gather.h"
#include "scan_grouped.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace mvf;

namespace {

constexpr uint32_t kWindow = 1024;                 // queries per window at most
constexpr size_t kScratchBytes = 512ull << 20;     // device scratch of a window: scan_gather.hip's budget (one group of queries may exceed it)

// the checks of both searches, none of which touches the device: mvfgpu_search_partitioned's, with per_key in the keys' place
int check_grouped_args(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* queries, uint8_t query_dtype,
                       uint32_t query_dim, uint32_t nq, uint32_t k, uint32_t per_key, const void* out_scores, const void* out_indices) {
    if (const int rc = check_search_scalars(metric, nq, k, queries, out_scores, out_indices)) return rc;
    if (per_key == 0 || per_key > MVFGPU_GROUP_MAX_PER_KEY)
        return set_fail(MVF_ERR_INVALID_ARGUMENT,
                        "per_key must be in 1.." + std::to_string(MVFGPU_GROUP_MAX_PER_KEY) + ", got " + std::to_string(per_key));
    if (!part) return set_fail(MVF_ERR_INVALID_ARGUMENT, "partition is NULL");
    if (const int rc = check_search_args(c, metric, queries, query_dtype, query_dim, nq, k, out_scores, out_indices)) return rc;
    return check_partition_use(c, part);
}

// The device work of both calls: queries and results in device memory; everything on `s`.  Runs under corpus_device_call.
// marks (the stage timer only; one window): events recorded at the start and behind the bounds, G0, G1 and the tail.
int grouped_core(const CorpusView& v, const PartitionView& pv, uint8_t metric, const void* d_queries, uint32_t nq, uint32_t k,
                 uint32_t per_key, float* d_scores, uint64_t* d_indices, int32_t* d_raw, hipStream_t s, hipEvent_t* marks = nullptr) {
    if (v.n == 0 || pv.live == 0 || pv.n_keys == 0) return fill_padding(metric, nq, k, d_scores, d_indices, d_raw, s);
    const OneQueryGroup g1 = one_query_group(v);
    const uint32_t qg = g1.qg;
    const size_t qrow = query_row_bytes(v);
    const uint32_t live = (uint32_t)pv.live, n = (uint32_t)v.n;  // a shard holds fewer than 2^32 rows
    const uint32_t tiles = group_tiles(live);
    // per query: the two sort buffers over all rows (the second one is G0's dump first) and the crossing runs' lists
    const size_t per_q = (size_t)n * 16 + (size_t)tiles * 128 * 8;
    // at least one group of G0's queries -- a window of fewer would read all rows for it again --, then whole groups
    uint32_t W = (uint32_t)std::max<size_t>(std::min(nq, qg), std::min<size_t>({(size_t)nq, (size_t)kWindow, kScratchBytes / per_q}));
    if (W > qg) W -= W % qg;
    if (marks && W < nq) return set_fail(MVF_ERR_INVALID_ARGUMENT, "the stage timer takes one window of queries");
    size_t tmp_bytes = 0;
    MVF_HIP_TRY(sort_composites(nullptr, &tmp_bytes, nullptr, nullptr, n, n, nullptr, s, W, n));

    AsyncBuf da, db, dtmp, dpart, dbounds;
    MVF_HIP_TRY(da.alloc((size_t)W * n * 8, s));
    MVF_HIP_TRY(db.alloc((size_t)W * n * 8, s));
    MVF_HIP_TRY(dtmp.alloc(tmp_bytes, s));
    MVF_HIP_TRY(dpart.alloc((size_t)W * tiles * 128 * 8, s));
    MVF_HIP_TRY(dbounds.alloc((size_t)live * 8, s));
    uint64_t *a = static_cast<uint64_t*>(da.p), *b = static_cast<uint64_t*>(db.p);
    if (marks) MVF_HIP_TRY(hipEventRecord(marks[0], s));
    MVF_HIP_TRY(group_bounds_launch(pv.table + pv.n_keys, pv.n_keys, live, static_cast<uint2*>(dbounds.p), s));

    if (marks) MVF_HIP_TRY(hipEventRecord(marks[1], s));

    SelectParams fp{};
    fp.k = k;
    fp.metric = metric;
    fp.dtype = v.dtype;
    fp.index_base = v.index_base;
    fp.ids = v.ids;
    fp.out_scores = d_scores;
    fp.out_indices = d_indices;
    fp.out_raw = d_raw;
    for (uint32_t w0 = 0; w0 < nq; w0 += W) {
        const uint32_t wn = std::min(W, nq - w0);
        // G0: every held row's rank entry, in key order, to b[q][live]
        GatherScoreParams sp{};
        sp.rows = v.rows;
        sp.queries = static_cast<const unsigned char*>(d_queries) + (size_t)w0 * qrow;
        sp.list = pv.rows_by_key;
        sp.m = live;
        sp.nq = wn;
        sp.dim = v.dim;
        sp.pitch = v.pitch;
        sp.V = v.V;
        sp.J = g1.J;
        sp.dump = b;
        MVF_HIP_TRY(gather_score_launch(v.dtype, metric, g1.G, qg, sp, s));
        if (marks) MVF_HIP_TRY(hipEventRecord(marks[2], s));
        // G1: the per_key best of every key to a[q][n], row-indexed, every other row dead
        MVF_HIP_TRY(group_dead_fill_launch(a, n, wn, s));
        GroupParams gp{};
        gp.scored = b;
        gp.bounds = static_cast<const uint2*>(dbounds.p);
        gp.partial = static_cast<uint64_t*>(dpart.p);
        gp.out = a;
        gp.live = live;
        gp.n = n;
        gp.nq = wn;
        gp.per_key = per_key;
        MVF_HIP_TRY(group_best_launch(gp, s));
        if (marks) MVF_HIP_TRY(hipEventRecord(marks[3], s));
        // the tail: entries in ascending position, as the whole-shard sort takes them
        size_t tb = tmp_bytes;
        uint64_t* sorted = nullptr;
        MVF_HIP_TRY(sort_composites(dtmp.p, &tb, a, b, n, std::min<size_t>(k, n), &sorted, s, wn, n));
        for (uint32_t i = 0; i < wn; i++) MVF_HIP_TRY(launch_write_sorted(fp, sorted + (size_t)i * n, n, (size_t)(w0 + i) * k, s));
        if (marks) MVF_HIP_TRY(hipEventRecord(marks[4], s));
    }
    return MVF_OK;
}

}  // namespace

extern "C" {

int mvfgpu_search_grouped_device(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* d_queries,
                                 uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t k, uint32_t per_key, float* d_scores,
                                 uint64_t* d_indices, int32_t* d_raw, void* hip_stream) {
    const int rc = check_grouped_args(c, part, metric, d_queries, query_dtype, query_dim, nq, k, per_key, d_scores, d_indices);
    if (rc != MVF_OK) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return corpus_device_call(c, s, [&]() {
        return grouped_core(corpus_view(c), partition_view(part), metric, d_queries, nq, k, per_key, d_scores, d_indices, d_raw, s);
    });
}

int mvfgpu_search_grouped(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* queries, uint8_t query_dtype,
                          uint32_t query_dim, uint32_t nq, uint32_t k, uint32_t per_key, float* out_scores, uint64_t* out_indices,
                          int32_t* out_raw) {
    const int rc0 = check_grouped_args(c, part, metric, queries, query_dtype, query_dim, nq, k, per_key, out_scores, out_indices);
    if (rc0 != MVF_OK) return rc0;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));
    const CorpusView v = corpus_view(c);
    const PartitionView pv = partition_view(part);
    hipStream_t s = static_cast<hipStream_t>(v.stream);
    const HostIn in[] = {{queries, query_row_bytes(v)}};
    const HostOut out[] = {{out_indices, (size_t)k * 8}, {out_scores, (size_t)k * 4}, {out_raw, (size_t)k * 4}};
    return stage_host_windows(c, s, nq, in, out, stage_as_given, [&](uint32_t, uint32_t wn, void* const* d_in, void* const* d_out) {
        return grouped_core(v, pv, metric, d_in[0], wn, k, per_key, static_cast<float*>(d_out[1]), static_cast<uint64_t*>(d_out[0]),
                            static_cast<int32_t*>(d_out[2]), s);
    });
}

int mvfgpu_selftest_grouped_stage_ms(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* d_queries,
                                     uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t k, uint32_t per_key, float* d_scores,
                                     uint64_t* d_indices, void* hip_stream, float* out_ms) {
    if (!out_ms) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    const int rc0 = check_grouped_args(c, part, metric, d_queries, query_dtype, query_dim, nq, k, per_key, d_scores, d_indices);
    if (rc0 != MVF_OK) return rc0;
    const PartitionView pv = partition_view(part);
    if (corpus_view(c).n == 0 || pv.live == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "the stage timer needs held rows");
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int rc = MVF_OK;
    for (auto& e : ev)
        if (rc == MVF_OK && hipEventCreate(&e) != hipSuccess) rc = set_fail(MVF_ERR_DEVICE, "hipEventCreate failed");
    if (rc == MVF_OK)
        rc = corpus_device_call(c, s, [&]() { return grouped_core(corpus_view(c), pv, metric, d_queries, nq, k, per_key, d_scores, d_indices, nullptr, s, ev); });
    if (rc == MVF_OK && hipStreamSynchronize(s) != hipSuccess) rc = set_fail(MVF_ERR_DEVICE, "hipStreamSynchronize failed");
    for (int i = 0; i < 4 && rc == MVF_OK; i++)
        if (hipEventElapsedTime(&out_ms[i], ev[i], ev[i + 1]) != hipSuccess) rc = set_fail(MVF_ERR_DEVICE, "hipEventElapsedTime failed");
    for (auto e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

int mvfgpu_selftest_group_plan(const uint64_t* run_lengths, const uint8_t* crossing, uint32_t n, uint32_t per_key, uint32_t* out_tier) {
    if (!run_lengths || !crossing || !out_tier) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (per_key == 0 || per_key > MVFGPU_GROUP_MAX_PER_KEY)
        return set_fail(MVF_ERR_INVALID_ARGUMENT,
                        "per_key must be in 1.." + std::to_string(MVFGPU_GROUP_MAX_PER_KEY) + ", got " + std::to_string(per_key));
    for (uint32_t i = 0; i < n; i++) {
        if (run_lengths[i] == 0 || run_lengths[i] > kGroupTile)
            return set_fail(MVF_ERR_INVALID_ARGUMENT, "a run holds 1.." + std::to_string(kGroupTile) + " entries of one tile");
        out_tier[i] = group_run_tier((uint32_t)run_lengths[i], per_key, crossing[i] != 0);
    }
    return MVF_OK;
}

int mvfgpu_column_gather(const mvfgpu_column* column, const uint64_t* indices, uint64_t count, uint64_t* out_values) {
    if (!column) return set_fail(MVF_ERR_INVALID_ARGUMENT, "column is NULL");
    if (count && (!indices || !out_values)) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (count == 0) return MVF_OK;
    const ColumnOrigin col = column_origin(column);
    const mvfgpu_corpus* c = col.owner;
    const CorpusView v = corpus_view(c);
    // with vector ids a search reports ids: back to positions, then to local rows
    std::vector<uint64_t> rows(count);
    const bool ids = corpus_ids_to_positions(c, indices, count, rows.data());
    for (uint64_t i = 0; i < count; i++) {
        const uint64_t g = ids ? rows[i] : indices[i];
        if (indices[i] == ~0ull) {  // padding of a short result list: 0
            rows[i] = ~0ull;
        } else if (ids && g == ~0ull) {
            return set_fail(MVF_ERR_INDEX_OUT_OF_BOUNDS, "Index out of bounds: vector id " + std::to_string(indices[i]) + " is not in this shard");
        } else if (g < v.index_base || g - v.index_base >= v.n) {
            return set_fail(MVF_ERR_INDEX_OUT_OF_BOUNDS, "Index out of bounds: " + std::to_string(g) + " >= " + std::to_string(v.index_base + v.n));
        } else {
            rows[i] = g - v.index_base;
        }
    }
    DevScope guard(v.device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));  // the handle's own stream belongs to the host-buffer calls
    hipStream_t s = static_cast<hipStream_t>(v.stream);
    AsyncBuf drows, dout;
    MVF_HIP_TRY(drows.alloc((size_t)count * 8, s));
    MVF_HIP_TRY(dout.alloc((size_t)count * 8, s));
    const int rc = corpus_device_call(c, s, [&]() -> int {
        MVF_HIP_TRY(hipMemcpyAsync(drows.p, rows.data(), (size_t)count * 8, hipMemcpyHostToDevice, s));
        MVF_HIP_TRY(column_gather_launch(col.values, col.dtype == MVF_DTYPE_UINT64, static_cast<const uint64_t*>(drows.p), count,
                                         static_cast<uint64_t*>(dout.p), s));
        MVF_HIP_TRY(hipMemcpyAsync(out_values, dout.p, (size_t)count * 8, hipMemcpyDeviceToHost, s));
        return MVF_OK;
    });
    if (rc != MVF_OK) return rc;
    MVF_HIP_TRY(hipStreamSynchronize(s));
    return MVF_OK;
}

}  // extern "C"
