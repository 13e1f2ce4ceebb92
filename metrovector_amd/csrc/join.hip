// join.hip — mvfgpu_knn_join / mvfgpu_knn_join_device: the exact top-k of queries taken from resident rows
// (include/mvf_gpu.h; DESIGN.md §3 "Join", §5 "J0 / J1 — k-NN join").
//
// Per window of MVFGPU_JOIN_WINDOW query rows, on one stream:
//   1. J0 (scan_join.hip) stages the rows of the query handle as a contiguous block of queries;
//   2. the searched handle's own search for that batch (search_positions_locked: mvfgpu_search_device's routes, repair
//      feedback and timing, reporting positions) writes k' = k + 1 ordered entries per query into scratch;
//   3. J1 removes the query row's own position (or the last entry), applies the searched handle's ids, pads deleted query rows.
// The device call enqueues every window without a host wait.  The host call lets window w's results leave through pinned
// memory on a copy stream while window w + 1 is searched.  Scratch: one window's queries and k' lists -- at most
// 1024 (4 dim + 16 (k + 1)) bytes -- plus, in the host call, two windows of results (2 x 1024 x 16 k bytes on the device and,
// up to kPinnedWindowBytes each, in pinned host memory); none of it grows with `count`.

#include "../../include/mvf_gpu.h"

#include "internal.h"
#include "mvf_common.h"
#include "scan_join.h"

#include <algorithm>
#include <cstring>
#include <string>

using namespace mvf;

namespace {

constexpr size_t kPinnedWindowBytes = 64ull << 20;  // a window's results up to this size leave through pinned memory

struct PinnedBuf {
    void* p = nullptr;
    hipError_t alloc(size_t bytes) {
        const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e == hipSuccess) poison_fill_host(p, bytes);
        return e;
    }
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
};

// the copy stream of a host call and the events between it and the search stream
struct CopyLane {
    hipStream_t cs = nullptr;
    hipEvent_t finished[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
    hipError_t create() {
        hipError_t e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
        for (int b = 0; b < 2 && e == hipSuccess; b++) {
            e = hipEventCreateWithFlags(&finished[b], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&copied[b], hipEventDisableTiming);
        }
        return e;
    }
    ~CopyLane() {
        if (cs) (void)hipStreamSynchronize(cs);  // nothing of this call may still write the caller's buffers
        for (int b = 0; b < 2; b++) {
            if (finished[b]) (void)hipEventDestroy(finished[b]);
            if (copied[b]) (void)hipEventDestroy(copied[b]);
        }
        if (cs) (void)hipStreamDestroy(cs);
    }
};

struct JoinPlan {
    const mvfgpu_corpus* C = nullptr;
    const mvfgpu_corpus* Q = nullptr;
    CorpusView vc, vq;
    uint32_t k = 0, kin = 0;  // kin = k': what the search is asked for
    bool exclude = false;
    size_t qrow = 0;          // bytes of one staged query
};

// Every argument check of both calls; nothing here touches the device.
int plan_join(const mvfgpu_corpus* c, const mvfgpu_corpus* qc, uint8_t metric, uint64_t first, uint64_t count, uint32_t k, uint32_t flags,
              const void* out_scores, const void* out_indices, JoinPlan* plan) {
    // what needs no handle first, as in the other searches
    if (flags & ~(uint32_t)MVFGPU_JOIN_EXCLUDE_SELF) return set_fail(MVF_ERR_INVALID_ARGUMENT, "unknown join flag bits " + std::to_string(flags));
    if (const int mrc = check_metric(metric)) return mrc;
    const bool exclude = (flags & MVFGPU_JOIN_EXCLUDE_SELF) != 0;
    if (k == 0 || k > MVFGPU_MAX_K - (exclude ? 1u : 0u))
        return set_fail(MVF_ERR_INVALID_ARGUMENT, exclude ? "k must be in 1..2^31 - 1 with MVFGPU_JOIN_EXCLUDE_SELF" : "k must be in 1..2^31");
    if (!c) return set_fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    plan->C = c;
    plan->Q = qc ? qc : c;
    plan->vc = corpus_view(plan->C);
    plan->vq = corpus_view(plan->Q);
    const CorpusView &vc = plan->vc, &vq = plan->vq;
    if (vq.dim != vc.dim) {
        set_fail(MVF_ERR_DIMENSION_MISMATCH, "Dimension mismatch: expected " + std::to_string(vc.dim) + ", got " + std::to_string(vq.dim));
        return MVF_ERR_DIMENSION_MISMATCH;
    }
    if (vq.dtype != vc.dtype) return set_fail(MVF_ERR_BUILD, "the query corpus and the searched corpus must hold the same data type");
    if (vq.device != vc.device) return set_fail(MVF_ERR_INVALID_ARGUMENT, "the query corpus and the searched corpus must live on the same device");
    if (first > vq.n || count > vq.n - first) return set_fail(MVF_ERR_INVALID_ARGUMENT, "row range outside the query corpus");
    if (count > 0 && (!out_scores || !out_indices)) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    // the two row ranges meet: only then can a query row be among its own results
    const bool meet = vq.index_base < vc.index_base + vc.n && vc.index_base < vq.index_base + vq.n;
    plan->k = k;
    plan->exclude = exclude && meet;
    plan->kin = plan->exclude ? k + 1 : k;
    plan->qrow = query_row_bytes(vc);
    return MVF_OK;
}

// corpus_device_call on the searched handle and, where it is another one, on the query handle as well: both locks in a
// fixed order (by address), `s` behind the newest work of both, ev_done of both recorded on every way out.
int both_device_call(const JoinPlan& p, hipStream_t s, const std::function<int()>& body) {
    if (p.Q == p.C) return corpus_device_call(p.C, s, body);
    const mvfgpu_corpus* a = std::less<const mvfgpu_corpus*>()(p.C, p.Q) ? p.C : p.Q;
    const mvfgpu_corpus* b = a == p.C ? p.Q : p.C;
    return corpus_device_call(a, s, [&]() { return corpus_device_call(b, s, body); });
}

struct WindowScratch {
    AsyncBuf dq, ds, di, dr;
    int alloc(const JoinPlan& p, uint32_t W, bool raw, hipStream_t s) {
        MVF_HIP_TRY(dq.alloc((size_t)W * p.qrow, s));
        MVF_HIP_TRY(ds.alloc((size_t)W * p.kin * 4, s));
        MVF_HIP_TRY(di.alloc((size_t)W * p.kin * 8, s));
        if (raw) MVF_HIP_TRY(dr.alloc((size_t)W * p.kin * 4, s));
        return MVF_OK;
    }
};

// One window on `s`: J0, the search, J1 into out_* (device memory, the window's first entry).  The caller holds the locks.
int join_window(const JoinPlan& p, uint8_t metric, uint64_t row0, uint32_t wn, const WindowScratch& w, float* out_scores,
                uint64_t* out_indices, int32_t* out_raw, hipStream_t s) {
    JoinStageParams sp{};
    sp.rows = p.vq.rows;
    sp.pitch = p.vq.pitch;
    sp.V = p.vq.V;
    sp.dim = p.vq.dim;
    sp.dtype = p.vq.dtype;
    sp.first = row0;
    sp.queries = w.dq.p;
    MVF_HIP_TRY(join_stage_launch(sp, wn, s));
    const int rc = search_positions_locked(p.C, metric, w.dq.p, wn, p.kin, static_cast<float*>(w.ds.p), static_cast<uint64_t*>(w.di.p),
                                           out_raw ? static_cast<int32_t*>(w.dr.p) : nullptr, s);
    if (rc != MVF_OK) return rc;
    JoinFinishParams fp{};
    fp.in_scores = static_cast<const float*>(w.ds.p);
    fp.in_indices = static_cast<const uint64_t*>(w.di.p);
    fp.in_raw = static_cast<const int32_t*>(w.dr.p);
    fp.kin = p.kin;
    fp.k = p.k;
    fp.exclude = p.exclude ? 1u : 0u;
    fp.metric = metric;
    fp.q_pos0 = p.vq.index_base + row0;
    fp.q_row0 = row0;
    fp.q_tomb = p.vq.tomb;
    fp.c_index_base = p.vc.index_base;
    fp.c_ids = p.vc.ids;
    fp.out_scores = out_scores;
    fp.out_indices = out_indices;
    fp.out_raw = out_raw;
    MVF_HIP_TRY(join_finish_launch(fp, wn, s));
    return MVF_OK;
}

}  // namespace

extern "C" {

int mvfgpu_knn_join_device(const mvfgpu_corpus* corpus, const mvfgpu_corpus* query_corpus, uint8_t metric, uint64_t first, uint64_t count,
                           uint32_t k, uint32_t flags, float* d_scores, uint64_t* d_indices, int32_t* d_raw, void* hip_stream) {
    JoinPlan p;
    const int rc0 = plan_join(corpus, query_corpus, metric, first, count, k, flags, d_scores, d_indices, &p);
    if (rc0 != MVF_OK) return rc0;
    if (count == 0) return MVF_OK;
    DevScope guard(p.vc.device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return both_device_call(p, s, [&]() -> int {
        const uint32_t W = (uint32_t)std::min<uint64_t>(count, MVFGPU_JOIN_WINDOW);
        WindowScratch w;  // one window's, reused in stream order
        int rc = w.alloc(p, W, d_raw != nullptr, s);
        for (uint64_t off = 0; rc == MVF_OK && off < count; off += W) {
            const uint32_t wn = (uint32_t)std::min<uint64_t>(W, count - off);
            rc = join_window(p, metric, first + off, wn, w, d_scores + off * k, d_indices + off * k, d_raw ? d_raw + off * k : nullptr, s);
        }
        return rc;
    });
}

int mvfgpu_knn_join(const mvfgpu_corpus* corpus, const mvfgpu_corpus* query_corpus, uint8_t metric, uint64_t first, uint64_t count,
                    uint32_t k, uint32_t flags, float* out_scores, uint64_t* out_indices, int32_t* out_raw) {
    JoinPlan p;
    const int rc0 = plan_join(corpus, query_corpus, metric, first, count, k, flags, out_scores, out_indices, &p);
    if (rc0 != MVF_OK) return rc0;
    if (count == 0) return MVF_OK;
    DevScope guard(p.vc.device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(p.C));
    hipStream_t s = static_cast<hipStream_t>(p.vc.stream);
    const uint32_t W = (uint32_t)std::min<uint64_t>(count, MVFGPU_JOIN_WINDOW);
    const size_t wres = (size_t)W * k;          // entries of a full window
    const size_t o_sc = wres * 8, o_raw = wres * 12, wbytes = wres * 16;  // a result buffer: indices | scores | raw
    const bool pinned = wbytes <= kPinnedWindowBytes;
    // (the copy lane is declared last: it is drained before any buffer its copies touch is released)
    PinnedBuf pin[2];
    AsyncBuf res[2];  // two windows of results: one is copied out while the other is written
    WindowScratch w;
    CopyLane lane;
    MVF_HIP_TRY(lane.create());
    if (pinned)
        for (auto& b : pin) MVF_HIP_TRY(b.alloc(wbytes));
    {
        const int rc = w.alloc(p, W, out_raw != nullptr, s);
        if (rc != MVF_OK) return rc;
        for (auto& r : res) MVF_HIP_TRY(r.alloc(wbytes, s));
    }
    // window w's results are the caller's once its copy has finished: a wait on the COPY stream's event, never on the search stream
    auto drain = [&](uint64_t off, int b) -> int {
        MVF_HIP_TRY(hipEventSynchronize(lane.copied[b]));
        if (pinned) {
            const size_t nr = (size_t)std::min<uint64_t>(W, count - off) * k;
            const unsigned char* src = static_cast<const unsigned char*>(pin[b].p);
            std::memcpy(out_indices + off * k, src, nr * 8);
            std::memcpy(out_scores + off * k, src + o_sc, nr * 4);
            if (out_raw) std::memcpy(out_raw + off * k, src + o_raw, nr * 4);
        }
        return MVF_OK;
    };
    int b = 0;
    for (uint64_t off = 0; off < count; off += W, b ^= 1) {
        const uint32_t wn = (uint32_t)std::min<uint64_t>(W, count - off);
        const size_t nr = (size_t)wn * k;
        unsigned char* r = static_cast<unsigned char*>(res[b].p);
        int rc = both_device_call(p, s, [&]() -> int {
            if (off >= 2ull * W) MVF_HIP_TRY(hipStreamWaitEvent(s, lane.copied[b], 0));  // the copy of two windows ago read this buffer
            const int rc1 = join_window(p, metric, first + off, wn, w, reinterpret_cast<float*>(r + o_sc), reinterpret_cast<uint64_t*>(r),
                                        out_raw ? reinterpret_cast<int32_t*>(r + o_raw) : nullptr, s);
            if (rc1 != MVF_OK) return rc1;
            MVF_HIP_TRY(hipEventRecord(lane.finished[b], s));
            return MVF_OK;
        });
        if (rc != MVF_OK) return rc;
        MVF_HIP_TRY(hipStreamWaitEvent(lane.cs, lane.finished[b], 0));
        if (pinned) {
            MVF_HIP_TRY(hipMemcpyAsync(pin[b].p, r, out_raw ? o_raw + nr * 4 : o_sc + nr * 4, hipMemcpyDeviceToHost, lane.cs));
        } else {
            MVF_HIP_TRY(hipMemcpyAsync(out_indices + off * k, r, nr * 8, hipMemcpyDeviceToHost, lane.cs));
            MVF_HIP_TRY(hipMemcpyAsync(out_scores + off * k, r + o_sc, nr * 4, hipMemcpyDeviceToHost, lane.cs));
            if (out_raw) MVF_HIP_TRY(hipMemcpyAsync(out_raw + off * k, r + o_raw, nr * 4, hipMemcpyDeviceToHost, lane.cs));
        }
        MVF_HIP_TRY(hipEventRecord(lane.copied[b], lane.cs));
        if (off > 0) {  // the window before this one, while this one is searched
            rc = drain(off - W, b ^ 1);
            if (rc != MVF_OK) return rc;
        }
    }
    const uint64_t last = (count - 1) / W * W;
    return drain(last, b ^ 1);
}

}  // extern "C"
