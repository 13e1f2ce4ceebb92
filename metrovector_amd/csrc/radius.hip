// radius.hip — mvfgpu_search_radius: every row within a score threshold of each query (include/mvf_gpu.h).
//
// Host orchestration of the radius search.  Per window of up to kWindow queries on the handle's host-call stream:
//   1. R1 (scan_radius.hip) streams the rows once per 1 or 4 queries, counts every match exactly and appends the first
//      MVFGPU_RADIUS_LIST_CAP of each query to its device list (not at all when only counts are asked for);
//   2. R2 orders every list that holds all of its query's matches best first and writes the first max_per_query;
//   3. counts and entries come back in one wait.
// A query with more matches than its list holds (and max_per_query > 0) is completed through the identity of DESIGN.md §3:
// its best max_per_query matches ARE its top-max_per_query result, so one mvfgpu_search over just those queries, cut at
// the count, finishes them.  The host knows the counts at that point (the call is blocking), so the decision is a host one.

#include "../../include/mvf_gpu.h"

#include "internal.h"
#include "mvf_common.h"
#include "scan_mfma.h"
#include "scan_radius.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace mvf;

namespace {

constexpr uint32_t kWindow = 1024;  // queries per window: lists 64 MiB, entries up to 128 MiB of device memory

// The largest R >= 0 with sqrtf((float)R) <= radius (L2 on the exact sum of squared differences); -1 when there is none.
int32_t l2_raw_bound(float radius) {
    if (!(0.0f <= radius)) return -1;
    auto ok = [&](int64_t R) { return sqrtf((float)R) <= radius; };
    int64_t lo = 0, hi = INT32_MAX;
    if (ok(hi)) return INT32_MAX;
    while (hi - lo > 1) {  // ok(lo), !ok(hi)
        const int64_t mid = lo + (hi - lo) / 2;
        (ok(mid) ? lo : hi) = mid;
    }
    return (int32_t)lo;
}

// The smallest R with (float)R >= radius (InnerProduct on the exact dot product); INT32_MAX -- a value no dot product of
// MVFGPU_MAX_INT_DIM elements reaches -- when there is none.
int32_t ip_raw_bound(float radius) {
    auto ok = [&](int64_t R) { return (float)R >= radius; };
    int64_t lo = INT32_MIN, hi = INT32_MAX;
    if (ok(lo)) return INT32_MIN;
    if (!ok(hi)) return INT32_MAX;
    while (hi - lo > 1) {  // !ok(lo), ok(hi)
        const int64_t mid = lo + (hi - lo) / 2;
        (ok(mid) ? hi : lo) = mid;
    }
    return (int32_t)hi;
}

// The radius as the largest matching order key (mvf_common.h): exact integers compare their i32, everything else the
// key of the float score.
uint32_t radius_bound_key(uint8_t dtype, uint8_t metric, float radius, int32_t* raw_out) {
    int32_t R = 0;
    uint32_t key;
    if (key_is_raw(dtype, metric)) {
        R = metric == MVF_METRIC_L2 ? l2_raw_bound(radius) : ip_raw_bound(radius);
        key = key_from_raw(R, metric);
    } else {
        key = key_from_score(radius, metric);
    }
    if (raw_out) *raw_out = R;
    return key;
}

// The route of a radius search: 0 = R1 streams the rows once per 1 or 4 queries, 1 = one thresholded pass of the batched
// f32 MFMA kernel + R3's exact re-scoring (Float32 rows).  A pass of R1 reads the rows once for four queries, the MFMA
// kernel serves 128 queries per tile at its compute rate: on 1M x 768 f32 a pass of R1 is 0.47 ms and the batched pass
// about 1.5 ms for up to 128 queries (profiles/r06_radius.txt), so from 16 queries on the batched route is the cheaper one.
// mvfgpu_set_scan_path 1 forces the streaming route, 2 / 3 / 5 the batched one (Float32 rows).
constexpr uint32_t kRadiusBatchMin = 16;
uint32_t radius_route(uint8_t dtype, uint32_t nq, int scan_path) {
    if (dtype != MVF_DTYPE_FLOAT32 || scan_path == 1) return 0;
    if (scan_path == 2 || scan_path == 3 || scan_path == 5) return 1;
    return nq >= kRadiusBatchMin ? 1u : 0u;
}

// tau of the batched pass: the radius loosened by the f32 kernel's proven bound (the eps formulas of CompactParams), so no
// row inside the radius is left out; the kernel's keys are the GEMM-form squared distance (L2) / the score (IP, cosine).
uint32_t batched_tau(uint8_t metric, float radius, double qq, float xxmax, double eps) {
    const double r = radius, slack = 1e-6;
    double thr;
    if (metric == MVF_METRIC_L2) {
        if (std::isinf(radius)) return key_from_score(radius, metric);
        thr = r < 0 ? -1.0 : r * r * (1.0 + slack) + 2.0 * eps * (qq + (double)xxmax) + 1e-30;
    } else if (metric == MVF_METRIC_INNER_PRODUCT) {
        if (std::isinf(radius)) return key_from_score(radius, metric);
        thr = r - std::fabs(r) * slack - 2.0 * eps * std::sqrt(qq) * std::sqrt((double)xxmax) - 1e-30;
    } else {
        if (std::isinf(radius)) return key_from_score(radius, metric);
        thr = r - std::fabs(r) * slack - 2.0 * eps;
    }
    return key_from_score((float)thr, metric);
}

void pad_entries(uint64_t from, uint64_t to, uint8_t metric, float* sc, uint64_t* idx, int32_t* raw) {
    const float ps = pad_score(metric);
    for (uint64_t i = from; i < to; i++) {
        sc[i] = ps;
        idx[i] = ~0ull;
        if (raw) raw[i] = 0;
    }
}

}  // namespace

extern "C" {

int mvfgpu_selftest_radius_bound(uint8_t data_type, uint8_t metric, float radius, uint32_t* out_key, int32_t* out_raw) {
    if (!out_key) return set_fail(MVF_ERR_INVALID_ARGUMENT, "out_key is NULL");
    if (elem_size(data_type) == 0) return set_fail(MVF_ERR_BUILD, "Unsupported vector data type");
    if (const int mrc = check_metric(metric)) return mrc;
    if (std::isnan(radius)) return set_fail(MVF_ERR_INVALID_ARGUMENT, "radius is NaN");
    *out_key = radius_bound_key(data_type, metric, radius, out_raw);
    return MVF_OK;
}

int mvfgpu_selftest_radius_route(uint8_t data_type, uint32_t nq, int scan_path, uint32_t* out_route) {
    if (!out_route) return set_fail(MVF_ERR_INVALID_ARGUMENT, "out_route is NULL");
    if (elem_size(data_type) == 0) return set_fail(MVF_ERR_BUILD, "Unsupported vector data type");
    if (nq == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "nq must be > 0");
    *out_route = radius_route(data_type, nq, scan_path);
    return MVF_OK;
}

int mvfgpu_search_radius(const mvfgpu_corpus* c, uint8_t metric, const void* queries, uint8_t query_dtype, uint32_t query_dim,
                         uint32_t nq, const float* radii, uint64_t max_per_query, uint64_t* out_counts, float* out_scores,
                         uint64_t* out_indices, int32_t* out_raw) {
    // everything that needs no handle first, then mvfgpu_search's own checks: nothing below touches the device on a refusal
    // (its required buffers are the queries, the radii and the counts; it has no k)
    if (const int rc = check_search_scalars(metric, nq, 1, queries, radii, out_counts)) return rc;
    if (max_per_query > MVFGPU_MAX_K) return set_fail(MVF_ERR_INVALID_ARGUMENT, "max_per_query must be in 0..2^31");
    if (max_per_query > 0 && (!out_scores || !out_indices))
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer (out_scores / out_indices are required when max_per_query > 0)");
    for (uint32_t q = 0; q < nq; q++)
        if (std::isnan(radii[q])) return set_fail(MVF_ERR_INVALID_ARGUMENT, "radius of query " + std::to_string(q) + " is NaN");
    const int rc0 = check_search_args(c, metric, queries, query_dtype, query_dim, nq, 1, radii, out_counts);
    if (rc0 != MVF_OK) return rc0;

    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    const uint64_t maxq = max_per_query;
    const uint32_t cap = MVFGPU_RADIUS_LIST_CAP;
    const uint32_t kk = (uint32_t)std::min<uint64_t>(maxq, cap);  // entries R2 writes per query
    std::vector<uint32_t> over;  // queries whose list lost arrivals and that want entries
    size_t qbytes = 0;  // of one query

    {
        std::lock_guard<std::mutex> lk(corpus_host_mutex(c));
        const hipStream_t s = static_cast<hipStream_t>(corpus_view(c).stream);
        // the handle's own stream, with mvfgpu_search_device's discipline: behind the handle's newest work on another stream (a
        // lazy build enqueued there: the norms below), ev_done recorded on every way out
        const int rc_call = corpus_device_call(c, s, [&]() -> int {
            const CorpusView v = corpus_view(c);  // under the lock: mvfgpu_corpus_reload_tuning changes the tuning under it too
            qbytes = query_row_bytes(v);
            std::vector<uint32_t> bound(nq);
            for (uint32_t q = 0; q < nq; q++) bound[q] = radius_bound_key(v.dtype, metric, radii[q], nullptr);
            // R1's shape for this batch: K1's rule with R1's LDS formula (it keeps no lists in LDS: k and pmax do not matter)
            const K1Shape sh = k1_pass_shape(v.V, nq, 0, v.k1_g,
                                             [&](int G, uint32_t J, int nqv, uint32_t) { return radius_scan_lds_bytes(v.dtype, G, J, nqv); });
            const int nqv = sh.nqv, G = sh.G;
            const uint32_t J = sh.J;
            const size_t lds = sh.lds;
            if (lds > 160 * 1024) return set_fail(MVF_ERR_BUILD, "dimension too large for the radius kernel's LDS query tile");
            const void* fn = radius_scan_kernel_ptr(v.dtype, metric, G, nqv);
            if (!fn) return set_fail(MVF_ERR_BUILD, "no radius kernel for this shape");
            int occ = 1;
            MVF_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 256, lds));
            occ = std::max(occ, 1);
            const uint64_t rows_per_block_step = 16ull * 64u / (uint32_t)G;  // 4 waves x U = 4 groups x 64/G rows
            const uint32_t nblk = (uint32_t)std::max<uint64_t>(
                1, std::min<uint64_t>((v.n + rows_per_block_step - 1) / rows_per_block_step, (uint64_t)occ * v.num_cus));

            const uint32_t W = std::min(nq, kWindow);
            AsyncBuf dq, dbound, dcnt, dlist, dsc, didx, draw;
            MVF_HIP_TRY(dq.alloc((size_t)W * qbytes, s));
            MVF_HIP_TRY(dbound.alloc((size_t)W * 4, s));
            MVF_HIP_TRY(dcnt.alloc((size_t)W * 4, s));
            if (maxq > 0) {
                MVF_HIP_TRY(dlist.alloc((size_t)W * cap * 8, s));
                MVF_HIP_TRY(dsc.alloc((size_t)W * kk * 4, s));
                MVF_HIP_TRY(didx.alloc((size_t)W * kk * 8, s));
                MVF_HIP_TRY(draw.alloc((size_t)W * kk * 4, s));
            }
            std::vector<uint32_t> hcnt(W), hccnt(W);
            std::vector<float> hsc(maxq > 0 ? (size_t)W * kk : 0);
            std::vector<uint64_t> hidx(hsc.size());
            std::vector<int32_t> hraw(hsc.size());
            std::vector<unsigned char> hq((size_t)W * qbytes);
            std::vector<uint32_t> hb(W);

            // a window of the queries `sel[w0 .. w0 + wn)`: queries and bounds to the device, packed contiguously
            auto upload = [&](const std::vector<uint32_t>& sel, uint32_t w0, uint32_t wn) -> int {
                for (uint32_t i = 0; i < wn; i++) {
                    std::memcpy(hq.data() + (size_t)i * qbytes, static_cast<const unsigned char*>(queries) + (size_t)sel[w0 + i] * qbytes, qbytes);
                    hb[i] = bound[sel[w0 + i]];
                }
                MVF_HIP_TRY(hipMemcpyAsync(dq.p, hq.data(), (size_t)wn * qbytes, hipMemcpyHostToDevice, s));
                MVF_HIP_TRY(hipMemcpyAsync(dbound.p, hb.data(), (size_t)wn * 4, hipMemcpyHostToDevice, s));
                MVF_HIP_TRY(hipMemsetAsync(dcnt.p, 0, (size_t)wn * 4, s));
                return MVF_OK;
            };
            // R2 over the window's lists, results back, one wait; `repair` (nullable): the window's candidate counts, a query
            // with more candidates than its list held is collected in *redo instead
            auto finish = [&](const std::vector<uint32_t>& sel, uint32_t w0, uint32_t wn, const uint32_t* dccnt,
                              std::vector<uint32_t>* redo) -> int {
                if (maxq > 0) {
                    RadiusPackParams pp{};
                    pp.lists = static_cast<const uint64_t*>(dlist.p);
                    pp.counts = static_cast<const uint32_t*>(dcnt.p);
                    pp.cap = cap;
                    pp.kout = kk;
                    pp.metric = metric;
                    pp.dtype = v.dtype;
                    pp.index_base = v.index_base;
                    pp.ids = v.ids;
                    pp.out_scores = static_cast<float*>(dsc.p);
                    pp.out_indices = static_cast<uint64_t*>(didx.p);
                    pp.out_raw = static_cast<int32_t*>(draw.p);
                    MVF_HIP_TRY(radius_pack_launch(pp, wn, s));
                    MVF_HIP_TRY(hipMemcpyAsync(hsc.data(), dsc.p, (size_t)wn * kk * 4, hipMemcpyDeviceToHost, s));
                    MVF_HIP_TRY(hipMemcpyAsync(hidx.data(), didx.p, (size_t)wn * kk * 8, hipMemcpyDeviceToHost, s));
                    MVF_HIP_TRY(hipMemcpyAsync(hraw.data(), draw.p, (size_t)wn * kk * 4, hipMemcpyDeviceToHost, s));
                }
                MVF_HIP_TRY(hipMemcpyAsync(hcnt.data(), dcnt.p, (size_t)wn * 4, hipMemcpyDeviceToHost, s));
                if (dccnt) MVF_HIP_TRY(hipMemcpyAsync(hccnt.data(), dccnt, (size_t)wn * 4, hipMemcpyDeviceToHost, s));
                MVF_HIP_TRY(hipStreamSynchronize(s));
                for (uint32_t i = 0; i < wn; i++) {
                    const uint32_t q = sel[w0 + i];
                    if (dccnt && hccnt[i] > kBatchCap) {
                        redo->push_back(q);
                        continue;
                    }
                    out_counts[q] = hcnt[i];
                    if (maxq == 0) continue;
                    if (hcnt[i] > cap) {
                        over.push_back(q);
                        continue;
                    }
                    const uint64_t m = std::min<uint64_t>(hcnt[i], maxq);  // <= kk
                    const size_t src = (size_t)i * kk, dst = (size_t)q * maxq;
                    std::copy(hsc.begin() + src, hsc.begin() + src + m, out_scores + dst);
                    std::copy(hidx.begin() + src, hidx.begin() + src + m, out_indices + dst);
                    if (out_raw) std::copy(hraw.begin() + src, hraw.begin() + src + m, out_raw + dst);
                    pad_entries(dst + m, dst + maxq, metric, out_scores, out_indices, out_raw);
                }
                return MVF_OK;
            };
            // R1 over the rows for the queries `sel`, in windows
            auto stream = [&](const std::vector<uint32_t>& sel) -> int {
                for (uint32_t w0 = 0; w0 < (uint32_t)sel.size(); w0 += W) {
                    const uint32_t wn = std::min<uint32_t>(W, (uint32_t)sel.size() - w0);
                    int rc = upload(sel, w0, wn);
                    if (rc != MVF_OK) return rc;
                    if (v.n > 0) {
                        RadiusParams rp{};
                        rp.rows = v.rows;
                        rp.queries = dq.p;
                        rp.tomb = v.tomb;
                        rp.bound = static_cast<const uint32_t*>(dbound.p);
                        rp.counts = static_cast<uint32_t*>(dcnt.p);
                        rp.lists = maxq > 0 ? static_cast<uint64_t*>(dlist.p) : nullptr;
                        rp.cap = cap;
                        rp.n = (uint32_t)v.n;
                        rp.pitch = v.pitch;
                        rp.dim = v.dim;
                        rp.V = v.V;
                        rp.J = J;
                        rp.q0 = 0;
                        rp.nq_total = wn;
                        MVF_HIP_TRY(radius_scan_launch(v.dtype, metric, G, nqv, rp, dim3(nblk, (wn + nqv - 1) / nqv), lds, s));
                    }
                    rc = finish(sel, w0, wn, nullptr, nullptr);
                    if (rc != MVF_OK) return rc;
                }
                return MVF_OK;
            };

            std::vector<uint32_t> all(nq);
            for (uint32_t q = 0; q < nq; q++) all[q] = q;
            int rc = MVF_OK;
            if (radius_route(v.dtype, nq, v.scan_path) == 0 || v.n == 0) {
                rc = stream(all);
            } else {
                // ---- the batched route (Float32 rows): ONE pass of the f32 MFMA selection kernel over all rows with tau[q] = the
                // radius loosened by the kernel's proven error bound, R3 re-scores the candidates exactly, R2 packs; a query whose
                // candidates overflowed the kernel's list is redone by R1 (the repair)
                const float *xnorm = nullptr, *xx2 = nullptr, *xxmax = nullptr;
                rc = corpus_row_norms(c, s, &xnorm, &xx2, &xxmax);
                if (rc != MVF_OK) return rc;
                float hxxmax = 0.0f;
                MVF_HIP_TRY(hipMemcpyAsync(&hxxmax, xxmax, 4, hipMemcpyDeviceToHost, s));
                MVF_HIP_TRY(hipStreamSynchronize(s));
                const uint32_t nq_pad = (W + 127u) & ~127u, KT = (v.dim + 31u) / 32u, KP = KT * 32u;
                AsyncBuf dqmat, dqn, dtau, dccnt, dcand;
                MVF_HIP_TRY(dqmat.alloc((size_t)nq_pad * KP * 4, s));
                MVF_HIP_TRY(dqn.alloc((size_t)nq_pad * 4, s));
                MVF_HIP_TRY(dtau.alloc((size_t)nq_pad * 4, s));
                MVF_HIP_TRY(dccnt.alloc((size_t)nq_pad * 4, s));
                MVF_HIP_TRY(dcand.alloc((size_t)nq_pad * kBatchCap * 8, s));
                std::vector<uint32_t> htau(nq_pad), redo;
                const double eps = (double)(std::max<uint32_t>(v.dim, 64) + 16) * 1.1920929e-7;  // the f32 kernel's bound (api.hip)
                for (uint32_t w0 = 0; w0 < nq && rc == MVF_OK; w0 += W) {
                    const uint32_t wn = std::min(W, nq - w0), wpad = (wn + 127u) & ~127u;
                    rc = upload(all, w0, wn);
                    if (rc != MVF_OK) break;
                    std::fill(htau.begin(), htau.end(), 0u);
                    for (uint32_t i = 0; i < wn; i++) {
                        const float* qv = reinterpret_cast<const float*>(hq.data() + (size_t)i * qbytes);
                        double qq = 0.0;
                        for (uint32_t e = 0; e < v.dim; e++) qq += (double)qv[e] * qv[e];
                        htau[i] = batched_tau(metric, radii[w0 + i], qq, hxxmax, eps);
                    }
                    MVF_HIP_TRY(hipMemcpyAsync(dtau.p, htau.data(), (size_t)wpad * 4, hipMemcpyHostToDevice, s));
                    MVF_HIP_TRY(hipMemsetAsync(dccnt.p, 0, (size_t)wpad * 4, s));
                    MVF_HIP_TRY(launch_prep_queries(static_cast<const float*>(dq.p), wn, wpad, v.dim, KP, static_cast<float*>(dqmat.p),
                                                static_cast<float*>(dqn.p), s));
                    BatchParams bp{};
                    bp.qmat = static_cast<const float*>(dqmat.p);
                    bp.qnorm = static_cast<const float*>(dqn.p);
                    bp.rows = v.rows;
                    bp.xnorm = xnorm;
                    bp.xx2 = xx2;
                    bp.xxmax = xxmax;
                    bp.tomb = v.tomb;
                    bp.tau = static_cast<const uint32_t*>(dtau.p);
                    bp.cand = static_cast<uint64_t*>(dcand.p);
                    bp.cnt = static_cast<uint32_t*>(dccnt.p);
                    bp.pitch = v.pitch;
                    bp.V = v.V;
                    bp.KP = KP;
                    bp.KT = KT;
                    bp.nq = wn;
                    bp.row_begin = 0;
                    bp.row_end = (uint32_t)v.n;
                    bp.ntiles = (uint32_t)((v.n + 127u) / 128u);
                    bp.mtiles = wpad / 128u;
                    bp.cap = kBatchCap;
                    bp.direct = 0;  // every candidate passes the threshold test
                    MVF_HIP_TRY(launch_scan_mfma_f32(bp, metric, s));
                    RadiusRescoreParams rr{};
                    rr.cand = static_cast<const uint64_t*>(dcand.p);
                    rr.ccnt = static_cast<const uint32_t*>(dccnt.p);
                    rr.ccap = kBatchCap;
                    rr.rows = v.rows;
                    rr.queries = static_cast<const float*>(dq.p);
                    rr.dim = v.dim;
                    rr.pitch = v.pitch;
                    rr.V = v.V;
                    rr.J = J;
                    rr.bound = static_cast<const uint32_t*>(dbound.p);
                    rr.counts = static_cast<uint32_t*>(dcnt.p);
                    rr.lists = maxq > 0 ? static_cast<uint64_t*>(dlist.p) : nullptr;
                    rr.cap = cap;
                    MVF_HIP_TRY(radius_rescore_launch(metric, G, rr, wn, radius_scan_lds_bytes(MVF_DTYPE_FLOAT32, G, J, 1), s));
                    rc = finish(all, w0, wn, static_cast<const uint32_t*>(dccnt.p), &redo);
                }
                if (rc == MVF_OK && !redo.empty()) rc = stream(redo);
            }
            return rc;
        });
        if (rc_call != MVF_OK) return rc_call;
    }

    if (!over.empty()) {
        // the top-k identity: the best min(count, max_per_query) matches of such a query are its top-k result for
        // k = max_per_query, and every row of that result up to the count is a match; one search for all of them
        uint64_t kmax = 0;
        for (uint32_t q : over) kmax = std::max<uint64_t>(kmax, std::min<uint64_t>(out_counts[q], maxq));
        const uint32_t no = (uint32_t)over.size(), k = (uint32_t)kmax;
        std::vector<unsigned char> qb((size_t)no * qbytes);
        for (uint32_t i = 0; i < no; i++)
            std::memcpy(qb.data() + (size_t)i * qbytes, static_cast<const unsigned char*>(queries) + (size_t)over[i] * qbytes, qbytes);
        std::vector<float> sc((size_t)no * k);
        std::vector<uint64_t> idx((size_t)no * k);
        std::vector<int32_t> raw((size_t)no * k);
        const int rc = mvfgpu_search(c, metric, qb.data(), query_dtype, query_dim, no, k, sc.data(), idx.data(), raw.data());
        if (rc != MVF_OK) return rc;
        for (uint32_t i = 0; i < no; i++) {
            const uint32_t q = over[i];
            const uint64_t m = std::min<uint64_t>(out_counts[q], maxq);  // <= k
            const size_t src = (size_t)i * k, dst = (size_t)q * maxq;
            std::copy(sc.begin() + src, sc.begin() + src + m, out_scores + dst);
            std::copy(idx.begin() + src, idx.begin() + src + m, out_indices + dst);
            if (out_raw) std::copy(raw.begin() + src, raw.begin() + src + m, out_raw + dst);
            pad_entries(dst + m, dst + maxq, metric, out_scores, out_indices, out_raw);
        }
    }
    return MVF_OK;
}

}  // extern "C"
