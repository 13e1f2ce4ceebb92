// hamming_maxsim.hip — mvfgpu_search_hamming_maxsim / mvfgpu_search_hamming_maxsim_device: the k keys of a partition index of
// smallest summed per-token best Hamming distance, for every SET of bit-packed query tokens (include/mvf_gpu_hamming_maxsim.h;
// DESIGN.md §3 "Binary MaxSim", §5 "B0").
//
// Per window of query sets: HQ (scan_hamming_mfma.hip, unchanged) prepares the window's (set, token) rows as FP4 operands once;
// per chunk of tokens B0 (scan_hamming_maxsim.hip) scores every row the index holds, in the index's key order, and keeps the
// smallest distance per (token, key), and the integer sums advance every key's S; behind the last chunk the multi-vector
// search's tail -- the sort of the rank entries (sort_topk.hip) and its writer -- gives the result rows.  The arithmetic is
// integer-exact: no bound, no repair path, no second pass.  Nothing is kept in the handle and no repair feedback is read or
// posted.  The host call runs the same device work per host window (host_staging.h).

#include "../../include/mvf_gpu_hamming_maxsim.h"

#include "aux_kernels.h"
#include "host_staging.h"
#include "internal.h"
#include "mvf_common.h"
#include "scan_gather.h"
#include "scan_hamming_maxsim.h"
#include "stage_marks.h"

#include <algorithm>
#include <string>

using namespace mvf;

namespace {

constexpr uint8_t kPadMetric = MVF_METRIC_L2;  // smaller is better: the padding's score is +inf

// none of the checks touches the device; the order is the header's
int check_args(const mvfgpu_corpus* c, const mvfgpu_partition* part, const void* queries, uint8_t query_dtype, uint32_t query_dim,
               uint32_t nq, uint32_t n_tokens, uint32_t k, const void* out_scores, const void* out_keys) {
    if (const int rc = check_search_scalars(kPadMetric, nq, k, queries, out_scores, out_keys)) return rc;
    if (n_tokens == 0 || n_tokens > MVFGPU_MAXSIM_MAX_TOKENS)
        return set_fail(MVF_ERR_INVALID_ARGUMENT,
                        "n_tokens must be in 1.." + std::to_string(MVFGPU_MAXSIM_MAX_TOKENS) + ", got " + std::to_string(n_tokens));
    if (!part) return set_fail(MVF_ERR_INVALID_ARGUMENT, "partition is NULL");
    if (!c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    const CorpusView v = corpus_view(c);
    if (v.dtype != MVF_DTYPE_UINT8) return set_fail(MVF_ERR_BUILD, "binary MaxSim takes a UInt8 corpus of bit-packed rows");
    if (v.dim > kBinMaxsimMaxDim)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "rows above 512 packed bytes are not built for binary MaxSim, got " + std::to_string(v.dim));
    if (query_dtype != MVF_DTYPE_UINT8) return set_fail(MVF_ERR_BUILD, "binary MaxSim takes UInt8 queries");
    if (query_dim != v.dim)
        return set_fail(MVF_ERR_DIMENSION_MISMATCH, "Dimension mismatch: expected " + std::to_string(v.dim) + ", got " + std::to_string(query_dim));
    return check_partition_use(c, part);
}

// The device work of both calls: query sets and results in device memory; everything on `s`, no host wait.  Runs under
// corpus_device_call.  marks (the stage timer only): stage 0 the ordinals, the clear and HQ, 1 B0, 2 the sums, 3 the tail.
int hamming_maxsim_core(const CorpusView& v, const PartitionView& pv, const void* d_queries, uint32_t nq, uint32_t n_tokens, uint32_t k,
                        float* d_scores, uint64_t* d_keys, uint32_t* d_counts, hipStream_t s, StageMarks* marks = nullptr) {
    if (v.n == 0 || pv.live == 0 || pv.n_keys == 0) {
        if (d_counts) MVF_HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)nq * 4, s));
        return fill_padding(kPadMetric, nq, k, d_scores, d_keys, nullptr, s);
    }
    const uint32_t live = (uint32_t)pv.live, nk = (uint32_t)pv.n_keys;  // n_keys <= live rows < 2^32
    const HammingMaxsimForm f = hamming_maxsim_form(v.dim, nq, n_tokens, nk, v.maxsim_scratch);
    const uint32_t W = f.window;
    const size_t set_bytes = (size_t)v.dim * n_tokens, kk = std::min<size_t>(k, nk);
    const uint64_t prep_rows = bin_maxsim_prepared_rows((uint64_t)W * n_tokens);
    size_t tmp_bytes = 0;
    MVF_HIP_TRY(sort_composites(nullptr, &tmp_bytes, nullptr, nullptr, nk, kk, nullptr, s, W, nk));

    AsyncBuf dord, dprep, dbest, dsum, da, db, dtmp;
    MVF_HIP_TRY(dord.alloc((size_t)live * 4, s));
    MVF_HIP_TRY(dprep.alloc((size_t)(prep_rows * f.prepared_row), s));  // the FP4 operands, then the starts
    MVF_HIP_TRY(dbest.alloc((size_t)W * f.chunk * nk * 4, s));
    MVF_HIP_TRY(dsum.alloc((size_t)W * nk * 4, s));
    MVF_HIP_TRY(da.alloc((size_t)W * nk * 8, s));
    MVF_HIP_TRY(db.alloc((size_t)W * nk * 8, s));
    MVF_HIP_TRY(dtmp.alloc(tmp_bytes, s));
    unsigned char* prepared = static_cast<unsigned char*>(dprep.p);
    float* starts = reinterpret_cast<float*>(prepared + (size_t)prep_rows * ham_mfma_query_bytes(f.chunks));
    if (marks) MVF_HIP_TRY(marks->mark(-1, s));
    MVF_HIP_TRY(maxsim_ordinals_launch(pv.table + pv.n_keys, pv.n_keys, live, static_cast<uint32_t*>(dord.p), s));
    MVF_HIP_TRY(hamming_maxsim_clear_launch(static_cast<uint32_t*>(dbest.p), (size_t)W * f.chunk * nk, s));

    for (uint32_t w0 = 0; w0 < nq; w0 += W) {
        const uint32_t wn = std::min(W, nq - w0);
        // HQ: the window's (set, token) rows as queries, in tiles of kBinMaxsimTile
        HammingMfmaParams hq{};
        hq.p.queries = static_cast<const unsigned char*>(d_queries) + (size_t)w0 * set_bytes;
        hq.p.dim = v.dim;
        hq.p.nq = wn * n_tokens;
        hq.p.query_tile = kBinMaxsimTile;
        hq.chunks = f.chunks;
        hq.tiles = (uint32_t)(bin_maxsim_prepared_rows(hq.p.nq) / kBinMaxsimTile);
        hq.prepared = prepared;
        hq.starts = starts;
        MVF_HIP_TRY(hamming_prepare_launch(hq, s));
        if (marks) MVF_HIP_TRY(marks->mark(0, s));
        for (uint32_t t0 = 0; t0 < n_tokens; t0 += f.chunk) {
            const uint32_t tc = std::min(f.chunk, n_tokens - t0);
            HammingMaxsimParams sp{};
            sp.rows = v.rows;
            sp.prepared = prepared;
            sp.starts = starts;
            sp.list = pv.rows_by_key;
            sp.ord = static_cast<const uint32_t*>(dord.p);
            sp.best = static_cast<uint32_t*>(dbest.p);
            sp.m = live;
            sp.n_keys = nk;
            sp.sets = wn;
            sp.n_tokens = n_tokens;
            sp.t0 = t0;
            sp.tc = tc;
            sp.dim = v.dim;
            sp.pitch = v.pitch;
            sp.V = v.V;
            sp.chunks = f.chunks;
            MVF_HIP_TRY(hamming_maxsim_score_launch(sp, s));
            if (marks) MVF_HIP_TRY(marks->mark(1, s));
            HammingMaxsimSumParams mp{};
            mp.best = sp.best;
            mp.sum = static_cast<float*>(dsum.p);
            mp.rank = static_cast<uint64_t*>(da.p);
            mp.n_keys = nk;
            mp.sets = wn;
            mp.tc = tc;
            mp.first = t0 == 0;
            mp.last = t0 + tc == n_tokens;
            MVF_HIP_TRY(hamming_maxsim_sum_launch(mp, s));
            if (marks) MVF_HIP_TRY(marks->mark(2, s));
        }
        // the tail: entries in ascending ordinal -- ascending key value --, as the sort takes them
        size_t tb = tmp_bytes;
        uint64_t* sorted = nullptr;
        MVF_HIP_TRY(sort_composites(dtmp.p, &tb, static_cast<uint64_t*>(da.p), static_cast<uint64_t*>(db.p), nk, kk, &sorted, s, wn, nk));
        MaxsimWriteParams wp{};
        wp.sorted = sorted;
        wp.sum = static_cast<const float*>(dsum.p);
        wp.keys = pv.table;
        wp.out_scores = d_scores + (size_t)w0 * k;
        wp.out_keys = d_keys + (size_t)w0 * k;
        wp.out_counts = d_counts ? d_counts + w0 : nullptr;
        wp.n_keys = nk;
        wp.sets = wn;
        wp.k = k;
        wp.metric = kPadMetric;
        MVF_HIP_TRY(maxsim_write_launch(wp, s));
        if (marks) MVF_HIP_TRY(marks->mark(3, s));
    }
    return MVF_OK;
}

}  // namespace

extern "C" {

int mvfgpu_search_hamming_maxsim_device(const mvfgpu_corpus* c, const mvfgpu_partition* part, const void* d_queries, uint8_t query_dtype,
                                        uint32_t query_dim, uint32_t nq, uint32_t n_tokens, uint32_t k, float* d_scores, uint64_t* d_keys,
                                        uint32_t* d_counts, void* hip_stream) {
    const int rc = check_args(c, part, d_queries, query_dtype, query_dim, nq, n_tokens, k, d_scores, d_keys);
    if (rc != MVF_OK) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return corpus_device_call(c, s, [&]() {
        return hamming_maxsim_core(corpus_view(c), partition_view(part), d_queries, nq, n_tokens, k, d_scores, d_keys, d_counts, s);
    });
}

int mvfgpu_search_hamming_maxsim(const mvfgpu_corpus* c, const mvfgpu_partition* part, const void* queries, uint8_t query_dtype,
                                 uint32_t query_dim, uint32_t nq, uint32_t n_tokens, uint32_t k, float* out_scores, uint64_t* out_keys,
                                 uint32_t* out_counts) {
    const int rc0 = check_args(c, part, queries, query_dtype, query_dim, nq, n_tokens, k, out_scores, out_keys);
    if (rc0 != MVF_OK) return rc0;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));
    const CorpusView v = corpus_view(c);
    const PartitionView pv = partition_view(part);
    hipStream_t s = static_cast<hipStream_t>(v.stream);
    const HostIn in[] = {{queries, (size_t)v.dim * n_tokens}};
    const HostOut out[] = {{out_keys, (size_t)k * 8}, {out_scores, (size_t)k * 4}, {out_counts, 4}};
    return stage_host_windows(c, s, nq, in, out, stage_as_given, [&](uint32_t, uint32_t wn, void* const* d_in, void* const* d_out) {
        return hamming_maxsim_core(v, pv, d_in[0], wn, n_tokens, k, static_cast<float*>(d_out[1]), static_cast<uint64_t*>(d_out[0]),
                                   static_cast<uint32_t*>(d_out[2]), s);
    });
}

int mvfgpu_selftest_hamming_maxsim_form(uint32_t dimension, uint32_t nq, uint32_t n_tokens, uint64_t n_keys, uint64_t held_rows,
                                        uint64_t budget_bytes, uint32_t num_cus, uint32_t* out_query_tile, uint32_t* out_chunks,
                                        uint32_t* out_rows_in_registers, uint32_t* out_chunk_tokens, uint32_t* out_window_sets,
                                        uint32_t* out_lds_bytes, uint64_t* out_scratch_bytes) {
    (void)num_cus;  // B0's grid follows the list, not the part
    if (dimension == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "dimension must be > 0");
    if (dimension > kBinMaxsimMaxDim)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "rows above 512 packed bytes are not built for binary MaxSim, got " + std::to_string(dimension));
    if (nq == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "nq must be > 0");
    if (n_tokens == 0 || n_tokens > MVFGPU_MAXSIM_MAX_TOKENS)
        return set_fail(MVF_ERR_INVALID_ARGUMENT,
                        "n_tokens must be in 1.." + std::to_string(MVFGPU_MAXSIM_MAX_TOKENS) + ", got " + std::to_string(n_tokens));
    if (held_rows > 0xFFFF0000ull) return set_fail(MVF_ERR_INVALID_ARGUMENT, "a shard holds at most 2^32-65536 rows");
    if (n_keys > held_rows) return set_fail(MVF_ERR_INVALID_ARGUMENT, "every key holds a row: n_keys <= held_rows");
    const HammingMaxsimForm f = hamming_maxsim_form(dimension, nq, n_tokens, n_keys, budget_bytes);
    if (out_query_tile) *out_query_tile = f.query_tile;
    if (out_chunks) *out_chunks = f.chunks;
    if (out_rows_in_registers) *out_rows_in_registers = f.reg ? 1u : 0u;
    if (out_chunk_tokens) *out_chunk_tokens = f.chunk;
    if (out_window_sets) *out_window_sets = f.window;
    if (out_lds_bytes) *out_lds_bytes = f.lds_bytes;
    if (out_scratch_bytes) *out_scratch_bytes = f.scratch_bytes;
    return MVF_OK;
}

int mvfgpu_selftest_hamming_maxsim_stage_ms(const mvfgpu_corpus* c, const mvfgpu_partition* part, const void* d_queries, uint8_t query_dtype,
                                            uint32_t query_dim, uint32_t nq, uint32_t n_tokens, uint32_t k, float* d_scores,
                                            uint64_t* d_keys, uint32_t* d_counts, void* hip_stream, float* out_ms) {
    if (!out_ms) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    const int rc0 = check_args(c, part, d_queries, query_dtype, query_dim, nq, n_tokens, k, d_scores, d_keys);
    if (rc0 != MVF_OK) return rc0;
    const PartitionView pv = partition_view(part);
    if (corpus_view(c).n == 0 || pv.live == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "the stage timer needs held rows");
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    StageMarks marks;
    int rc = corpus_device_call(c, s, [&]() { return hamming_maxsim_core(corpus_view(c), pv, d_queries, nq, n_tokens, k, d_scores, d_keys, d_counts, s, &marks); });
    if (rc == MVF_OK && hipStreamSynchronize(s) != hipSuccess) rc = set_fail(MVF_ERR_DEVICE, "hipStreamSynchronize failed");
    for (int i = 0; i < 4; i++) out_ms[i] = 0.0f;
    return rc == MVF_OK ? stage_sums(marks, out_ms) : rc;
}

}  // extern "C"
