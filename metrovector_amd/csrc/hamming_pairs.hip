// hamming_pairs.hip — mvfgpu_hamming_pairs: every two live rows of a UInt8 corpus of bit-packed rows within r bits of each other,
// counted exactly, with each row's degree, and listed in ascending (i, j) order (include/mvf_gpu_hamming_pairs.h; DESIGN.md §3
// "Hamming pair join", §5 "HJ / HJP").
//
// On one stream under corpus_device_call: the counters and the degrees are cleared, HJ scans the upper triangle of the corpus
// against itself, counts every pair and appends the first `cap` of them to the call's list (scan_hamming_pairs.hip); the host
// waits once for the two counters; where the total fits the caller's room HJP sorts the list and writes it.  The scratch --
// counters, degrees, the list and its sort partner, the passes' counts -- is stream-ordered and per call; the sort partner is
// sized by the total, which is known by then.  The blocking call lets HJP's writer convert the list in its own arrays and copies
// them to the caller; the stage timer has it write the caller's device buffers.  Nothing here reads norms, shadows or the repair
// feedback, and nothing is kept in the handle.

#include "../../include/mvf_gpu_hamming_pairs.h"

#include "internal.h"
#include "mvf_common.h"
#include "scan_hamming_pairs.h"

#include <string>

using namespace mvf;

namespace {

static_assert(kHamPairsMaxPairs == MVFGPU_HAMMING_PAIRS_MAX, "the header's limit");

int check_hamming_pairs_args(const mvfgpu_corpus* c, uint64_t max_pairs, const void* out_total, const void* out_first, const void* out_second,
                             const void* out_listed) {
    // what needs no handle first, then the handle: nothing below touches the device on a refusal
    if (!out_total || !out_listed) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (max_pairs > 0 && (!out_first || !out_second))
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer (out_first / out_second are required when max_pairs > 0)");
    if (max_pairs > kHamPairsMaxPairs)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "max_pairs above 2^24 is not built for the Hamming pair join, got " + std::to_string(max_pairs));
    if (!c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    const CorpusView v = corpus_view(c);
    if (v.dtype != MVF_DTYPE_UINT8) return set_fail(MVF_ERR_BUILD, "the Hamming pair join takes a UInt8 corpus of bit-packed rows");
    if (v.dim > kHamPairsMaxDim)
        return set_fail(MVF_ERR_INVALID_ARGUMENT,
                        "rows above 512 packed bytes are not built for the Hamming pair join, got " + std::to_string(v.dim));
    return MVF_OK;
}

// The join on `s`; waits for the stream.  out_total and out_listed are host words.  to_device: out_degrees (nullable), out_first,
// out_second, out_raw (nullable) are device buffers the kernels write; otherwise they are the caller's host buffers.
// ms (the stage timer only): ms[0..1] = scan, order.
int hamming_pairs_core(const CorpusView& v, uint32_t radius, uint64_t max_pairs, bool to_device, uint64_t* out_total, uint32_t* out_degrees,
                       uint64_t* out_first, uint64_t* out_second, int32_t* out_raw, uint64_t* out_listed, hipStream_t s, float* ms = nullptr) {
    const HammingPairsForm f = hamming_pairs_form(v.dim, v.n, (uint32_t)v.num_cus);
    const uint64_t cap = ham_pairs_list_cap(v.n, max_pairs);
    const size_t deg_bytes = (size_t)v.n * 4u;
    AsyncBuf dctr, ddeg, dlist_a, ddist_a, dlist_b, ddist_b, dbh, dtot;
    MVF_HIP_TRY(dctr.alloc(16, s));
    if (out_degrees && !to_device) MVF_HIP_TRY(ddeg.alloc(deg_bytes, s));
    if (cap) {
        MVF_HIP_TRY(dlist_a.alloc((size_t)cap * 8u, s));
        MVF_HIP_TRY(ddist_a.alloc((size_t)cap * 4u, s));
    }
    uint32_t* d_degrees = to_device ? out_degrees : static_cast<uint32_t*>(ddeg.p);

    hipEvent_t marks[3] = {nullptr, nullptr, nullptr};
    struct Events {
        hipEvent_t* e;
        ~Events() {
            for (int i = 0; i < 3; i++)
                if (e[i]) (void)hipEventDestroy(e[i]);
        }
    } events{marks};
    if (ms) {
        ms[0] = ms[1] = 0.0f;
        for (hipEvent_t& e : marks) MVF_HIP_TRY(hipEventCreate(&e));
        MVF_HIP_TRY(hipEventRecord(marks[0], s));
    }

    MVF_HIP_TRY(hipMemsetAsync(dctr.p, 0, 16, s));
    if (d_degrees && deg_bytes) MVF_HIP_TRY(hipMemsetAsync(d_degrees, 0, deg_bytes, s));
    HammingPairsParams r{};
    r.p.rows = v.rows;
    r.p.tomb = v.tomb;
    r.p.n = v.n;
    r.p.dim = v.dim;
    r.p.pitch = v.pitch;
    r.p.V = v.V;
    r.p.index_base = v.index_base;
    r.p.ids = v.ids;
    r.chunks = f.chunks;
    r.span_rows = f.span_rows;
    r.tiles_per_span = f.tiles_per_span;
    r.spans = f.spans;
    r.radius = radius;
    r.counters = static_cast<uint64_t*>(dctr.p);
    r.degrees = d_degrees;
    r.list = static_cast<uint64_t*>(dlist_a.p);
    r.dist = static_cast<uint32_t*>(ddist_a.p);
    r.cap = cap;
    MVF_HIP_TRY(hamming_pairs_scan_launch(f, r, s));  // HJ
    if (ms) MVF_HIP_TRY(hipEventRecord(marks[1], s));

    // the one wait in the middle: the total decides whether there is a list to order, and sizes the passes
    uint64_t counters[2] = {0, 0};
    MVF_HIP_TRY(hipMemcpyAsync(counters, dctr.p, 16, hipMemcpyDeviceToHost, s));
    MVF_HIP_TRY(hipStreamSynchronize(s));
    const uint64_t total = counters[0];
    const bool listed = max_pairs > 0 && total <= max_pairs;  // (then total <= cap: the list lost no arrival)
    *out_total = total;
    *out_listed = listed ? total : 0;
    if (listed && total) {
        MVF_HIP_TRY(dlist_b.alloc((size_t)total * 8u, s));
        MVF_HIP_TRY(ddist_b.alloc((size_t)total * 4u, s));
        MVF_HIP_TRY(dbh.alloc((size_t)256 * ham_pairs_sort_tiles(total) * 4u, s));
        MVF_HIP_TRY(dtot.alloc(256 * 4, s));
        uint64_t *la = static_cast<uint64_t*>(dlist_a.p), *lb = static_cast<uint64_t*>(dlist_b.p);
        uint32_t* da = static_cast<uint32_t*>(ddist_a.p);
        // HJP; the blocking call's writer converts in place: firsts into the partner, seconds and distances over the sorted list
        MVF_HIP_TRY(hamming_pairs_order_launch(r.p, la, da, lb, static_cast<uint32_t*>(ddist_b.p), total, static_cast<uint32_t*>(dbh.p),
                                               static_cast<uint32_t*>(dtot.p), to_device ? out_first : lb, to_device ? out_second : la,
                                               to_device ? out_raw : reinterpret_cast<int32_t*>(da), s));
        if (!to_device) {
            MVF_HIP_TRY(hipMemcpyAsync(out_first, lb, (size_t)total * 8u, hipMemcpyDeviceToHost, s));
            MVF_HIP_TRY(hipMemcpyAsync(out_second, la, (size_t)total * 8u, hipMemcpyDeviceToHost, s));
            if (out_raw) MVF_HIP_TRY(hipMemcpyAsync(out_raw, da, (size_t)total * 4u, hipMemcpyDeviceToHost, s));
        }
    }
    if (ms) MVF_HIP_TRY(hipEventRecord(marks[2], s));
    if (out_degrees && !to_device && deg_bytes) MVF_HIP_TRY(hipMemcpyAsync(out_degrees, d_degrees, deg_bytes, hipMemcpyDeviceToHost, s));
    MVF_HIP_TRY(hipStreamSynchronize(s));
    if (ms) {
        MVF_HIP_TRY(hipEventElapsedTime(&ms[0], marks[0], marks[1]));
        MVF_HIP_TRY(hipEventElapsedTime(&ms[1], marks[1], marks[2]));  // (the counters' read-back and the wait included: the call pays them)
    }
    return MVF_OK;
}

}  // namespace

extern "C" {

int mvfgpu_hamming_pairs(const mvfgpu_corpus* c, uint32_t radius, uint64_t max_pairs, uint64_t* out_total, uint32_t* out_degrees,
                         uint64_t* out_first, uint64_t* out_second, int32_t* out_raw, uint64_t* out_listed) {
    const int rc0 = check_hamming_pairs_args(c, max_pairs, out_total, out_first, out_second, out_listed);
    if (rc0 != MVF_OK) return rc0;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));
    hipStream_t s = static_cast<hipStream_t>(corpus_view(c).stream);
    return corpus_device_call(c, s, [&]() {
        return hamming_pairs_core(corpus_view(c), radius, max_pairs, false, out_total, out_degrees, out_first, out_second, out_raw, out_listed, s);
    });
}

int mvfgpu_selftest_hamming_pairs_form(uint32_t dimension, uint64_t rows, uint32_t num_cus, uint64_t max_pairs, uint64_t block_index,
                                       uint32_t* out_query_tile, uint32_t* out_chunks, uint32_t* out_span_rows, uint64_t* out_tiles,
                                       uint64_t* out_spans, uint64_t* out_blocks, uint32_t* out_lds_bytes, uint64_t* out_scratch_bytes,
                                       uint64_t* out_block_tile, uint64_t* out_block_span) {
    if (dimension == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "dimension must be > 0");
    if (dimension > kHamPairsMaxDim)
        return set_fail(MVF_ERR_INVALID_ARGUMENT,
                        "rows above 512 packed bytes are not built for the Hamming pair join, got " + std::to_string(dimension));
    if (rows > 0xFFFF0000ull) return set_fail(MVF_ERR_INVALID_ARGUMENT, "a shard holds at most 2^32-65536 rows");
    if (max_pairs > kHamPairsMaxPairs)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "max_pairs above 2^24 is not built for the Hamming pair join, got " + std::to_string(max_pairs));
    const HammingPairsForm f = hamming_pairs_form(dimension, rows, num_cus);
    if ((out_block_tile || out_block_span) && block_index >= f.blocks)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "block_index " + std::to_string(block_index) + " is not one of the grid's " + std::to_string(f.blocks) + " blocks");
    if (out_query_tile) *out_query_tile = f.query_tile;
    if (out_chunks) *out_chunks = f.chunks;
    if (out_span_rows) *out_span_rows = f.span_rows;
    if (out_tiles) *out_tiles = f.tiles;
    if (out_spans) *out_spans = f.spans;
    if (out_blocks) *out_blocks = f.blocks;
    if (out_lds_bytes) *out_lds_bytes = f.lds_bytes;
    if (out_scratch_bytes) *out_scratch_bytes = ham_pairs_scratch_bytes(rows, max_pairs);
    if (out_block_tile || out_block_span) {
        uint64_t tile = 0, span = 0;
        ham_pairs_decode(block_index, f.spans, f.tiles_per_span, &tile, &span);
        if (out_block_tile) *out_block_tile = tile;
        if (out_block_span) *out_block_span = span;
    }
    return MVF_OK;
}

int mvfgpu_selftest_hamming_pairs_stage_ms(const mvfgpu_corpus* c, uint32_t radius, uint64_t max_pairs, uint64_t* out_total, uint32_t* d_degrees,
                                           uint64_t* d_first, uint64_t* d_second, int32_t* d_raw, uint64_t* out_listed, void* hip_stream,
                                           float* out_ms) {
    if (!out_ms) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    const int rc = check_hamming_pairs_args(c, max_pairs, out_total, d_first, d_second, out_listed);
    if (rc != MVF_OK) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return corpus_device_call(c, s, [&]() {
        return hamming_pairs_core(corpus_view(c), radius, max_pairs, true, out_total, d_degrees, d_first, d_second, d_raw, out_listed, s, out_ms);
    });
}

}  // extern "C"
