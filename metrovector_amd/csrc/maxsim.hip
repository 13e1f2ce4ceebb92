// maxsim.hip — mvfgpu_search_maxsim / mvfgpu_search_maxsim_device: the k best keys of a partition index for every SET of query
// vectors, a key's score being the sum over the set's vectors of that vector's best score among the key's rows (late
// interaction; include/mvf_gpu.h; DESIGN.md §3 "Multi-vector search", §5 "M0 / M1 — multi-vector search").
//
// Per window of query sets and chunk of tokens: M0 (scan_maxsim.hip) scores every row the index holds, in the index's key
// order, against the chunk's tokens with K1's one-query bits and keeps the smallest order key per (token, key); M1 adds the
// chunk's scores to every key's running sum in token order.  Behind the last chunk the keys' rank entries are ranked by the
// whole-list select and sort (sort_topk.hip) and a writer maps ordinals to key values.  No host wait, no plan on the host but
// the chunk and window sizes (maxsim_plan).  The host call runs the same device work per host window (host_staging.h).
//
// mvfgpu_search_maxsim_candidates / _device restrict every query set to its own list of keys.  The host plans from the index's
// mirror -- per set the distinct held candidates in ascending key value, their segments of rows_by_key and the windows --, the
// plan travels through the index's pinned buffer (partition_upload), E0 expands it into the list M0's candidate form scores,
// and M1, the sort and the writer run per set over its candidates: the cost follows the candidates' rows.

#include "../../include/mvf_gpu.h"
#include "../../include/mvf_gpu_maxsim_align.h"
#include "../../include/mvf_gpu_maxsim_route.h"

#include "aux_kernels.h"
#include "host_staging.h"
#include "internal.h"
#include "mvf_common.h"
#include "scan_gather.h"
#include "scan_maxsim.h"
#include "scan_mfma.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace mvf;

namespace {

// the checks of both searches, none of which touches the device: the grouped search's, with n_tokens in per_key's place
int check_maxsim_args(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* queries, uint8_t query_dtype,
                      uint32_t query_dim, uint32_t nq, uint32_t n_tokens, uint32_t k, const void* out_scores, const void* out_keys) {
    if (const int rc = check_search_scalars(metric, nq, k, queries, out_scores, out_keys)) return rc;
    if (n_tokens == 0 || n_tokens > MVFGPU_MAXSIM_MAX_TOKENS)
        return set_fail(MVF_ERR_INVALID_ARGUMENT,
                        "n_tokens must be in 1.." + std::to_string(MVFGPU_MAXSIM_MAX_TOKENS) + ", got " + std::to_string(n_tokens));
    if (!part) return set_fail(MVF_ERR_INVALID_ARGUMENT, "partition is NULL");
    if (const int rc = check_search_args(c, metric, queries, query_dtype, query_dim, nq, k, out_scores, out_keys)) return rc;
    return check_partition_use(c, part);
}

// the stage timer's events: one behind every stage of every chunk and window, with the stage it closes
struct StageMarks {
    std::vector<std::pair<int, hipEvent_t>> ev;
    hipError_t mark(int stage, hipStream_t s) {
        hipEvent_t e = nullptr;
        hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
        ev.emplace_back(stage, e);
        return hipEventRecord(e, s);
    }
    ~StageMarks() {
        for (auto& m : ev) (void)hipEventDestroy(m.second);
    }
};

// what the stage timer of route 2 asks for beside the marks: per set of the CALL the candidate keys and the blocks re-scored
struct MfmaStats {
    uint32_t* d_stats;  // device [2][nq], zero on entry
    uint32_t nq;
    // the selection's read-out (mvfgpu_selftest_maxsim_mfma_selection), all device memory; d_sums is the switch: where it is set
    // the other five are set too.  What the selection holds around P0, filed under the call's sets while it is valid -- M0 / M1
    // reuse the sums behind P0
    float* d_sums = nullptr;            // [nq][n_keys] the approximate sums P0 reads
    unsigned char* d_forced = nullptr;  // [nq][n_keys] A0's force, in front of P0
    unsigned char* d_cands = nullptr;   // [nq][n_keys] the candidates, behind P0
    double* d_delta = nullptr;          // [nq]
    uint64_t* d_kth = nullptr;          // [nq] the sorted entry P0 takes theta from
    float* d_xxmax = nullptr;           // [1]
};

// The device work of both calls: query sets and results in device memory; everything on `s`.  Runs under corpus_device_call.
// Route 1 (maxsim_route): M0 over every held row.  Route 2: per window A0's approximate scores go through M1 and the sort to the
// kth best approximate sum, P0 makes the candidates' block table, and M0's candidate form, M1, the sort and the writer give the
// answer -- route 1's, byte for byte.
// marks (the stage timers only): route 1: stage 0 the ordinals, 1 M0, 2 M1, 3 the tail; route 2: 0 the preparation, 1 A0, 2 the
// approximate sums, their kth best and P0, 3 M0 over the candidates' blocks, 4 M1 and the mask, 5 the tail.
int maxsim_core(const mvfgpu_corpus* c, const CorpusView& v, const PartitionView& pv, uint8_t metric, const void* d_queries, uint32_t nq,
                uint32_t n_tokens, uint32_t k, float* d_scores, uint64_t* d_keys, uint32_t* d_counts, hipStream_t s,
                StageMarks* marks = nullptr, const MfmaStats* stats = nullptr) {
    if (v.n == 0 || pv.live == 0 || pv.n_keys == 0) {
        if (d_counts) MVF_HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)nq * 4, s));
        return fill_padding(metric, nq, k, d_scores, d_keys, nullptr, s);
    }
    const OneQueryGroup g1 = one_query_group(v);
    const size_t set_bytes = query_row_bytes(v) * n_tokens;
    const uint32_t live = (uint32_t)pv.live, nk = (uint32_t)pv.n_keys;  // n_keys <= live rows < 2^32
    // the timers time one route each: route 1's (marks alone) and route 2's (with stats) whatever the handle would take
    const int forced = stats ? 2 : marks ? 1 : v.maxsim_route;
    const bool mfma = maxsim_route(pv.live, pv.n_keys, v.dim, v.dtype, metric, nq, n_tokens, k, forced) == 2;
    const bool f16 = v.dtype == MVF_DTYPE_FLOAT16;
    const uint32_t kp_bytes = (v.V + 1u) / 2u * 32u;  // a prepared token of route 2: whole 32-byte steps of A0
    MaxsimPlan pl = maxsim_plan(nk, n_tokens, nq, g1.qbytes, v.maxsim_scratch);
    uint32_t achunk = 0;  // route 2: A0's own tokens per chunk
    if (mfma) {
        const MaxsimMfmaPlan mp = maxsim_mfma_plan(nk, live, n_tokens, nq, g1.qbytes, kp_bytes, v.maxsim_scratch);
        pl.chunk = mp.chunk, pl.window = mp.window, achunk = mp.achunk;
    }
    const uint32_t W = pl.window, n_blocks = (live + kMaxsimRows - 1) / kMaxsimRows;
    const size_t kk = std::min<size_t>(k, nk);
    size_t tmp_bytes = 0;
    MVF_HIP_TRY(sort_composites(nullptr, &tmp_bytes, nullptr, nullptr, nk, kk, nullptr, s, W, nk));

    AsyncBuf dord, dbest, dsum, da, db, dtmp;
    MVF_HIP_TRY(dord.alloc((size_t)live * 4, s));
    MVF_HIP_TRY(dbest.alloc((size_t)W * std::max(pl.chunk, achunk) * nk * 4, s));
    MVF_HIP_TRY(dsum.alloc((size_t)W * nk * 4, s));
    MVF_HIP_TRY(da.alloc((size_t)W * nk * 8, s));
    MVF_HIP_TRY(db.alloc((size_t)W * nk * 8, s));
    MVF_HIP_TRY(dtmp.alloc(tmp_bytes, s));
    AsyncBuf dprep, daux, dflag, dblocks, ddelta;  // route 2
    const float *xnorm = nullptr, *xx2 = nullptr, *xxmax = nullptr;
    if (mfma) {
        MVF_HIP_TRY(dprep.alloc((size_t)W * n_tokens * kp_bytes, s));
        MVF_HIP_TRY(daux.alloc((size_t)W * n_tokens * 8, s));  // the undo scales [W * n_tokens], then |q|
        MVF_HIP_TRY(dflag.alloc((size_t)W * nk, s));
        MVF_HIP_TRY(dblocks.alloc((size_t)W * n_blocks * sizeof(MaxsimCandBlock), s));
        MVF_HIP_TRY(ddelta.alloc((size_t)W * 8, s));
    }
    if (marks) MVF_HIP_TRY(marks->mark(-1, s));
    if (mfma)
        if (const int rc = corpus_row_norms(c, s, &xnorm, &xx2, &xxmax)) return rc;
    MVF_HIP_TRY(maxsim_ordinals_launch(pv.table + pv.n_keys, pv.n_keys, live, static_cast<uint32_t*>(dord.p), s));
    if (marks) MVF_HIP_TRY(marks->mark(0, s));

    for (uint32_t w0 = 0; w0 < nq; w0 += W) {
        const uint32_t wn = std::min(W, nq - w0);
        const unsigned char* w_queries = static_cast<const unsigned char*>(d_queries) + (size_t)w0 * set_bytes;
        // M1: S[set][key] advances by the chunk's scores in token order; behind the last chunk the rank entries
        auto sums = [&](uint32_t t0, uint32_t tc) -> int {
            MaxsimSumParams mp{};
            mp.best = static_cast<const uint32_t*>(dbest.p);
            mp.sum = static_cast<float*>(dsum.p);
            mp.rank = static_cast<uint64_t*>(da.p);
            mp.n_keys = nk;
            mp.sets = wn;
            mp.tc = tc;
            mp.metric = metric;
            mp.dtype = v.dtype;
            mp.first = t0 == 0;
            mp.last = t0 + tc == n_tokens;
            MVF_HIP_TRY(maxsim_sum_launch(mp, s));
            return MVF_OK;
        };
        // M0's parameters of a chunk: the smallest order key of every (token of the chunk, key) to best[set][t][key], dead on entry
        auto score_params = [&](uint32_t t0, uint32_t tc) {
            MaxsimScoreParams sp{};
            sp.rows = v.rows;
            sp.queries = w_queries;
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
            sp.J = g1.J;
            return sp;
        };
        if (mfma) {
            // the window's tokens as (set, token) query rows; no key is forced yet
            const uint32_t qrows = wn * n_tokens;
            float *undo = static_cast<float*>(daux.p), *qnorm = undo + (size_t)W * n_tokens;
            if (f16)
                MVF_HIP_TRY(launch_prep_queries16(w_queries, MVF_DTYPE_FLOAT16, qrows, qrows, v.dim, kp_bytes, static_cast<unsigned char*>(dprep.p), undo, qnorm, s));
            else
                MVF_HIP_TRY(launch_prep_queries(reinterpret_cast<const float*>(w_queries), qrows, qrows, v.dim, kp_bytes / 4, static_cast<float*>(dprep.p), qnorm, s));
            MVF_HIP_TRY(hipMemsetAsync(dflag.p, 0, (size_t)wn * nk, s));
            if (marks) MVF_HIP_TRY(marks->mark(0, s));
            for (uint32_t t0 = 0; t0 < n_tokens; t0 += achunk) {
                const uint32_t tc = std::min(achunk, n_tokens - t0);
                MVF_HIP_TRY(hipMemsetAsync(dbest.p, 0xFF, (size_t)wn * tc * nk * 4, s));
                MaxsimMfmaParams ap{};
                ap.rows = v.rows;
                ap.qprep = static_cast<const unsigned char*>(dprep.p);
                ap.undo = f16 ? undo : nullptr;
                ap.qnorm = qnorm;
                ap.xnorm = xnorm;
                ap.list = pv.rows_by_key;
                ap.ord = static_cast<const uint32_t*>(dord.p);
                ap.best = static_cast<uint32_t*>(dbest.p);
                ap.force = static_cast<unsigned char*>(dflag.p);
                ap.m = live;
                ap.n_keys = nk;
                ap.sets = wn;
                ap.n_tokens = n_tokens;
                ap.t0 = t0;
                ap.tc = tc;
                ap.pitch = v.pitch;
                ap.V = v.V;
                ap.kp_bytes = kp_bytes;
                MVF_HIP_TRY(maxsim_mfma_score_launch(v.dtype, metric, ap, s));
                if (marks) MVF_HIP_TRY(marks->mark(1, s));
                if (const int rc = sums(t0, tc)) return rc;
                if (marks) MVF_HIP_TRY(marks->mark(2, s));
            }
            // theta: the kth best approximate sum among the keys whose sum the bound covers; the others rank behind them
            MaxsimMaskParams kp{};
            kp.rank = static_cast<uint64_t*>(da.p);
            kp.sum = static_cast<const float*>(dsum.p);
            kp.flag = static_cast<const unsigned char*>(dflag.p);
            kp.n_keys = nk;
            kp.sets = wn;
            kp.dead = false;
            MVF_HIP_TRY(maxsim_mask_launch(kp, s));
            size_t tb = tmp_bytes;
            uint64_t* approx = nullptr;
            MVF_HIP_TRY(sort_composites(dtmp.p, &tb, static_cast<uint64_t*>(da.p), static_cast<uint64_t*>(db.p), nk, kk, &approx, s, wn, nk));
            MaxsimPickParams pp{};
            pp.sorted = approx;
            pp.sum = static_cast<const float*>(dsum.p);
            pp.qnorm = qnorm;
            pp.xxmax = xxmax;
            pp.ord = static_cast<const uint32_t*>(dord.p);
            pp.flag = static_cast<unsigned char*>(dflag.p);
            pp.blocks = static_cast<MaxsimCandBlock*>(dblocks.p);
            pp.stats = nullptr;
            pp.delta = static_cast<double*>(ddelta.p);
            pp.m = live;
            pp.n_keys = nk;
            pp.sets = wn;
            pp.n_tokens = n_tokens;
            pp.kth = (uint32_t)kk - 1u;
            pp.dim = v.dim;
            pp.metric = metric;
            pp.dtype = v.dtype;
            AsyncBuf dwstats;  // the window's counts [2][wn], filed under the call's sets behind P0
            if (stats) {
                MVF_HIP_TRY(dwstats.alloc((size_t)wn * 8, s));
                MVF_HIP_TRY(hipMemsetAsync(dwstats.p, 0, (size_t)wn * 8, s));
                pp.stats = static_cast<uint32_t*>(dwstats.p);
            }
            const bool readout = stats && stats->d_sums;
            if (readout) MVF_HIP_TRY(hipMemcpyAsync(stats->d_forced + (size_t)w0 * nk, dflag.p, (size_t)wn * nk, hipMemcpyDeviceToDevice, s));
            MVF_HIP_TRY(maxsim_pick_launch(pp, s));
            if (readout) {
                MVF_HIP_TRY(hipMemcpyAsync(stats->d_sums + (size_t)w0 * nk, dsum.p, (size_t)wn * nk * 4, hipMemcpyDeviceToDevice, s));
                MVF_HIP_TRY(hipMemcpyAsync(stats->d_cands + (size_t)w0 * nk, dflag.p, (size_t)wn * nk, hipMemcpyDeviceToDevice, s));
                MVF_HIP_TRY(hipMemcpyAsync(stats->d_delta + w0, ddelta.p, (size_t)wn * 8, hipMemcpyDeviceToDevice, s));
                for (uint32_t q = 0; q < wn; q++)
                    MVF_HIP_TRY(hipMemcpyAsync(stats->d_kth + w0 + q, approx + (size_t)q * nk + pp.kth, 8, hipMemcpyDeviceToDevice, s));
                MVF_HIP_TRY(hipMemcpyAsync(stats->d_xxmax, xxmax, 4, hipMemcpyDeviceToDevice, s));
            }
            if (stats) {
                MVF_HIP_TRY(hipMemcpyAsync(stats->d_stats + w0, pp.stats, (size_t)wn * 4, hipMemcpyDeviceToDevice, s));
                MVF_HIP_TRY(hipMemcpyAsync(stats->d_stats + stats->nq + w0, pp.stats + wn, (size_t)wn * 4, hipMemcpyDeviceToDevice, s));
            }
            if (marks) MVF_HIP_TRY(marks->mark(2, s));
        }
        for (uint32_t t0 = 0; t0 < n_tokens; t0 += pl.chunk) {
            const uint32_t tc = std::min(pl.chunk, n_tokens - t0);
            MVF_HIP_TRY(hipMemsetAsync(dbest.p, 0xFF, (size_t)wn * tc * nk * 4, s));
            MaxsimScoreParams sp = score_params(t0, tc);
            if (mfma) {  // M0's candidate form over the full list, set after set with the set's slice of P0's table
                sp.m = n_blocks * kMaxsimRows;
                for (uint32_t q = 0; q < wn; q++) {
                    sp.blocks = static_cast<const MaxsimCandBlock*>(dblocks.p) + (size_t)q * n_blocks;
                    MVF_HIP_TRY(maxsim_score_candidates_launch(v.dtype, metric, g1.G, sp, s));
                }
            } else {
                MVF_HIP_TRY(maxsim_score_launch(v.dtype, metric, g1.G, sp, s));
            }
            if (marks) MVF_HIP_TRY(marks->mark(mfma ? 3 : 1, s));
            if (const int rc = sums(t0, tc)) return rc;
            if (marks && !mfma) MVF_HIP_TRY(marks->mark(2, s));
        }
        if (mfma) {  // a key that is no candidate may be scored in part: behind every candidate
            MaxsimMaskParams kp{};
            kp.rank = static_cast<uint64_t*>(da.p);
            kp.sum = static_cast<const float*>(dsum.p);
            kp.flag = static_cast<const unsigned char*>(dflag.p);
            kp.n_keys = nk;
            kp.sets = wn;
            kp.dead = true;
            MVF_HIP_TRY(maxsim_mask_launch(kp, s));
            if (marks) MVF_HIP_TRY(marks->mark(4, s));
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
        wp.metric = metric;
        MVF_HIP_TRY(maxsim_write_launch(wp, s));
        if (marks) MVF_HIP_TRY(marks->mark(mfma ? 5 : 3, s));
    }
    return MVF_OK;
}

// ---- the candidate form: mvfgpu_search_maxsim_candidates (DESIGN.md §3 "Candidate keys", §5 "E0")

int check_candidates_args(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* queries, uint8_t query_dtype,
                          uint32_t query_dim, uint32_t nq, uint32_t n_tokens, const uint64_t* candidate_keys, uint32_t m, uint32_t k,
                          const void* out_scores, const void* out_keys, const char* list_name = "candidate_keys") {
    if (const int rc = check_search_scalars(metric, nq, k, queries, out_scores, out_keys)) return rc;
    if (n_tokens == 0 || n_tokens > MVFGPU_MAXSIM_MAX_TOKENS)
        return set_fail(MVF_ERR_INVALID_ARGUMENT,
                        "n_tokens must be in 1.." + std::to_string(MVFGPU_MAXSIM_MAX_TOKENS) + ", got " + std::to_string(n_tokens));
    if (!candidate_keys && (uint64_t)nq * m > 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, std::string("NULL buffer (") + list_name + ")");
    if (!part) return set_fail(MVF_ERR_INVALID_ARGUMENT, "partition is NULL");
    if (const int rc = check_search_args(c, metric, queries, query_dtype, query_dim, nq, k, out_scores, out_keys)) return rc;
    return check_partition_use(c, part);
}

// One set's list, a pure function: of the entries `take` admits the first occurrence of every key as (key, entry), in ascending
// key value.  With take = "the key is held" a pair's place is the candidate's slot ordinal.
template <class Take>
void distinct_entries(const uint64_t* keys, uint32_t m, Take take, std::vector<std::pair<uint64_t, uint32_t>>* out) {
    out->clear();
    for (uint32_t i = 0; i < m; i++)
        if (take(i)) out->emplace_back(keys[i], i);
    std::sort(out->begin(), out->end());  // equal keys in ascending entry: the first occurrence leads
    out->erase(std::unique(out->begin(), out->end(), [](const auto& a, const auto& b) { return a.first == b.first; }), out->end());
}

// the plan of a call: what the device reads, in the order of its upload, and the windows
struct CandWindow {
    uint32_t w0, wn, chunk, n_keys, blk0, n_blocks;
};
struct CandPlan {
    std::vector<uint64_t> keys;           // [segments] the candidates' key values, set after set
    std::vector<MaxsimCandSeg> segs;      // [segments]
    std::vector<MaxsimCandSet> sets;      // [nq]
    std::vector<MaxsimCandBlock> blocks;  // window after window
    std::vector<CandWindow> windows;
};

// Windows: as many sets as maxsim_plan allows for the window's largest candidate count inside what the budget leaves beside the
// window's concatenated list (8 bytes per position), the list itself inside the budget and below 2^32 positions; one set whatever
// the budget.  plan_of and set_bytes (the alignments): the plan function in maxsim_plan's place, and bytes that every set of a
// window takes off the budget beside the list.
using PlanFn = MaxsimPlan (*)(uint64_t, uint32_t, uint32_t, uint64_t, uint64_t);
int plan_candidates(const mvfgpu_partition* part, const uint64_t* cand, uint32_t nq, uint32_t m, uint32_t n_tokens, uint64_t token_bytes,
                    uint64_t budget, CandPlan* plan, PlanFn plan_of = maxsim_plan, uint64_t set_bytes = 0) {
    std::vector<std::pair<uint64_t, uint32_t>> distinct;
    plan->sets.resize(nq);
    for (uint32_t q = 0; q < nq; q++) {
        // the distinct entries first, then one lookup each, in ascending key: held is a function of the key, so dropping the
        // entries that are not held afterwards leaves what take = "held" gives
        distinct_entries(cand + (size_t)q * m, m, [](uint32_t) { return true; }, &distinct);
        if (plan->segs.size() + distinct.size() > 0xFFFFFFFFull)
            return set_fail(MVF_ERR_INVALID_ARGUMENT, "the candidate lists hold more than 2^32 - 1 candidates in all");
        MaxsimCandSet& st = plan->sets[q];
        st.seg0 = (uint32_t)plan->segs.size();
        uint64_t rows = 0, from = 0;  // distinct keys of one index: at most its live rows, < 2^32
        for (const auto& e : distinct) {
            uint64_t off = 0, cnt = 0;
            partition_find(part, e.first, &off, &cnt, &from);
            if (!cnt) continue;
            plan->keys.push_back(e.first);
            plan->segs.push_back(MaxsimCandSeg{(uint32_t)off, (uint32_t)rows});
            rows += cnt;
        }
        st.count = (uint32_t)(plan->segs.size() - st.seg0);
        st.rows = (uint32_t)rows;
        st.list0 = 0;
    }
    for (uint32_t w0 = 0; w0 < nq;) {
        uint32_t wn = std::min(kMaxsimWindow, nq - w0);
        CandWindow w{};
        for (;;) {
            uint64_t pos = 0;
            uint32_t nk = 0;
            for (uint32_t q = w0; q < w0 + wn; q++) {
                pos += maxsim_cand_positions(plan->sets[q].rows);
                nk = std::max(nk, plan->sets[q].count);
            }
            const uint64_t used = pos * 8 + wn * set_bytes;
            const bool list_ok = pos <= 0xFFFFFFFFull && used <= budget;
            const MaxsimPlan pl = plan_of(nk, n_tokens, wn, token_bytes, budget > used ? budget - used : 0);
            if (wn == 1 || (list_ok && pl.window >= wn)) {
                if (pos > 0xFFFFFFFFull) return set_fail(MVF_ERR_INVALID_ARGUMENT, "a candidate list's rows take 2^32 list positions or more");
                w = CandWindow{w0, wn, pl.chunk, nk, (uint32_t)plan->blocks.size(), (uint32_t)(pos / kMaxsimRows)};
                break;
            }
            wn = std::max(1u, std::min(wn - 1, list_ok ? pl.window : wn / 2));
        }
        uint32_t list0 = 0;
        for (uint32_t q = w0; q < w0 + wn; q++) {
            MaxsimCandSet& st = plan->sets[q];
            st.list0 = list0;
            for (uint32_t r = 0; r < st.rows; r += kMaxsimRows) plan->blocks.push_back(MaxsimCandBlock{q - w0, std::min(kMaxsimRows, st.rows - r)});
            list0 += (uint32_t)maxsim_cand_positions(st.rows);
        }
        plan->windows.push_back(w);
        w0 += wn;
    }
    return MVF_OK;
}

int pad_sets(uint8_t metric, uint32_t nq, uint32_t k, float* d_scores, uint64_t* d_keys, uint32_t* d_counts, hipStream_t s) {
    if (d_counts) MVF_HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)nq * 4, s));
    return fill_padding(metric, nq, k, d_scores, d_keys, nullptr, s);
}

// The device work of both candidate calls: query sets and results in device memory, the lists on the host; everything on `s`.
// Runs under corpus_device_call.  marks (the stage timer only): stage 0 the plan's upload and E0, 1 M0, 2 M1, 3 the tail.
int maxsim_candidates_core(const CorpusView& v, const mvfgpu_partition* part, uint8_t metric, const void* d_queries, uint32_t nq,
                           uint32_t n_tokens, const uint64_t* cand, uint32_t m, uint32_t k, float* d_scores, uint64_t* d_keys,
                           uint32_t* d_counts, hipStream_t s, StageMarks* marks = nullptr) {
    const PartitionView pv = partition_view(part);
    if (marks) MVF_HIP_TRY(marks->mark(-1, s));
    if (v.n == 0 || pv.live == 0 || pv.n_keys == 0 || m == 0) return pad_sets(metric, nq, k, d_scores, d_keys, d_counts, s);
    const OneQueryGroup g1 = one_query_group(v);
    const size_t set_bytes = query_row_bytes(v) * n_tokens;
    CandPlan plan;
    if (const int rc = plan_candidates(part, cand, nq, m, n_tokens, g1.qbytes, v.maxsim_scratch, &plan)) return rc;
    if (plan.segs.empty()) return pad_sets(metric, nq, k, d_scores, d_keys, d_counts, s);

    // the plan, one upload: keys | segments | sets | blocks, 8-byte entries throughout
    const size_t nseg = plan.segs.size(), keys_b = nseg * 8, segs_b = nseg * sizeof(MaxsimCandSeg), sets_b = (size_t)nq * sizeof(MaxsimCandSet),
                 blocks_b = plan.blocks.size() * sizeof(MaxsimCandBlock);
    std::vector<unsigned char> blob(keys_b + segs_b + sets_b + blocks_b);
    std::memcpy(blob.data(), plan.keys.data(), keys_b);
    std::memcpy(blob.data() + keys_b, plan.segs.data(), segs_b);
    std::memcpy(blob.data() + keys_b + segs_b, plan.sets.data(), sets_b);
    if (blocks_b) std::memcpy(blob.data() + keys_b + segs_b + sets_b, plan.blocks.data(), blocks_b);
    AsyncBuf dplan;
    MVF_HIP_TRY(dplan.alloc(blob.size(), s));
    if (const int rc = partition_upload(part, blob.data(), blob.size(), dplan.p, s)) return rc;
    const unsigned char* dp = static_cast<const unsigned char*>(dplan.p);
    const uint64_t* p_keys = reinterpret_cast<const uint64_t*>(dp);
    const MaxsimCandSeg* p_segs = reinterpret_cast<const MaxsimCandSeg*>(dp + keys_b);
    const MaxsimCandSet* p_sets = reinterpret_cast<const MaxsimCandSet*>(dp + keys_b + segs_b);
    const MaxsimCandBlock* p_blocks = reinterpret_cast<const MaxsimCandBlock*>(dp + keys_b + segs_b + sets_b);

    for (const CandWindow& w : plan.windows) {
        float* w_scores = d_scores + (size_t)w.w0 * k;
        uint64_t* w_keys = d_keys + (size_t)w.w0 * k;
        uint32_t* w_counts = d_counts ? d_counts + w.w0 : nullptr;
        if (w.n_keys == 0) {  // no set of the window holds a candidate
            if (const int rc = pad_sets(metric, w.wn, k, w_scores, w_keys, w_counts, s)) return rc;
            continue;
        }
        const uint32_t nk = w.n_keys, wn = w.wn;
        const size_t npos = (size_t)w.n_blocks * kMaxsimRows, kk = std::min<size_t>(k, nk);
        size_t tmp_bytes = 0;
        MVF_HIP_TRY(sort_composites(nullptr, &tmp_bytes, nullptr, nullptr, nk, kk, nullptr, s, wn, nk));
        AsyncBuf dlist, dbest, dsum, da, db, dtmp;
        MVF_HIP_TRY(dlist.alloc(npos * 8, s));  // rows [npos], then slot ordinals [npos]
        MVF_HIP_TRY(dbest.alloc((size_t)wn * w.chunk * nk * 4, s));
        MVF_HIP_TRY(dsum.alloc((size_t)wn * nk * 4, s));
        MVF_HIP_TRY(da.alloc((size_t)wn * nk * 8, s));
        MVF_HIP_TRY(db.alloc((size_t)wn * nk * 8, s));
        MVF_HIP_TRY(dtmp.alloc(tmp_bytes, s));
        // E0: the window's concatenated list
        MaxsimExpandParams ep{};
        ep.rows_by_key = pv.rows_by_key;
        ep.sets = p_sets + w.w0;
        ep.segs = p_segs;
        ep.blocks = p_blocks + w.blk0;
        ep.n_blocks = w.n_blocks;
        ep.list = static_cast<uint32_t*>(dlist.p);
        ep.ord = ep.list + npos;
        MVF_HIP_TRY(maxsim_expand_launch(ep, s));
        if (marks) MVF_HIP_TRY(marks->mark(0, s));
        for (uint32_t t0 = 0; t0 < n_tokens; t0 += w.chunk) {
            const uint32_t tc = std::min(w.chunk, n_tokens - t0);
            MVF_HIP_TRY(hipMemsetAsync(dbest.p, 0xFF, (size_t)wn * tc * nk * 4, s));
            MaxsimScoreParams sp{};
            sp.rows = v.rows;
            sp.queries = static_cast<const unsigned char*>(d_queries) + (size_t)w.w0 * set_bytes;
            sp.list = ep.list;
            sp.ord = ep.ord;
            sp.best = static_cast<uint32_t*>(dbest.p);
            sp.m = (uint32_t)npos;
            sp.n_keys = nk;
            sp.sets = wn;
            sp.n_tokens = n_tokens;
            sp.t0 = t0;
            sp.tc = tc;
            sp.dim = v.dim;
            sp.pitch = v.pitch;
            sp.V = v.V;
            sp.J = g1.J;
            sp.blocks = ep.blocks;
            MVF_HIP_TRY(maxsim_score_candidates_launch(v.dtype, metric, g1.G, sp, s));
            if (marks) MVF_HIP_TRY(marks->mark(1, s));
            MaxsimSumParams mp{};
            mp.best = sp.best;
            mp.sum = static_cast<float*>(dsum.p);
            mp.rank = static_cast<uint64_t*>(da.p);
            mp.n_keys = nk;
            mp.sets = wn;
            mp.tc = tc;
            mp.metric = metric;
            mp.dtype = v.dtype;
            mp.first = t0 == 0;
            mp.last = t0 + tc == n_tokens;
            mp.cand = ep.sets;
            MVF_HIP_TRY(maxsim_sum_launch(mp, s));
            if (marks) MVF_HIP_TRY(marks->mark(2, s));
        }
        // the tail: entries in ascending slot ordinal -- ascending key value --, the sets' fillers behind them
        size_t tb = tmp_bytes;
        uint64_t* sorted = nullptr;
        MVF_HIP_TRY(sort_composites(dtmp.p, &tb, static_cast<uint64_t*>(da.p), static_cast<uint64_t*>(db.p), nk, kk, &sorted, s, wn, nk));
        MaxsimWriteParams wp{};
        wp.sorted = sorted;
        wp.sum = static_cast<const float*>(dsum.p);
        wp.keys = p_keys;
        wp.out_scores = w_scores;
        wp.out_keys = w_keys;
        wp.out_counts = w_counts;
        wp.n_keys = nk;
        wp.sets = wn;
        wp.k = k;
        wp.metric = metric;
        wp.cand = ep.sets;
        MVF_HIP_TRY(maxsim_write_launch(wp, s));
        if (marks) MVF_HIP_TRY(marks->mark(3, s));
    }
    return MVF_OK;
}

// the stage timer's sums: every stage's time from the event in front of it
int stage_sums(const StageMarks& marks, float* out_ms, int stages = 4) {
    for (int i = 0; i < stages; i++) out_ms[i] = 0.0f;
    for (size_t i = 1; i < marks.ev.size(); i++) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, marks.ev[i - 1].second, marks.ev[i].second) != hipSuccess) return set_fail(MVF_ERR_DEVICE, "hipEventElapsedTime failed");
        if (marks.ev[i].first >= 0 && marks.ev[i].first < stages) out_ms[marks.ev[i].first] += ms;
    }
    return MVF_OK;
}

// ---- alignments: mvfgpu_maxsim_align (include/mvf_gpu_maxsim_align.h; DESIGN.md §3 "Alignments", §5 "M0-arg and the alignment
// writer")

// check_candidates_args as with k = 1, the list named `keys`; out_raw is nullable
int check_align_args(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* queries, uint8_t query_dtype,
                     uint32_t query_dim, uint32_t nq, uint32_t n_tokens, const uint64_t* keys, uint32_t m, const void* out_scores,
                     const void* out_rows) {
    return check_candidates_args(c, part, metric, queries, query_dtype, query_dim, nq, n_tokens, keys, m, 1, out_scores, out_rows, "keys");
}

// The device work of both alignment calls: query sets and the three outputs [nq][m][n_tokens] in device memory, the lists on the
// host; everything on `s`.  Runs under corpus_device_call.  Per window: E0, then per chunk of tokens M0-arg and the writer;
// every element is written by the writer, the padding of skipped entries and of windows without a candidate included.
// marks (the stage timer only): stage 0 the plan's upload and E0, 1 M0-arg, 2 the writer.
int maxsim_align_core(const CorpusView& v, const mvfgpu_partition* part, uint8_t metric, const void* d_queries, uint32_t nq,
                      uint32_t n_tokens, const uint64_t* keys, uint32_t m, float* d_scores, uint64_t* d_rows, int32_t* d_raw, hipStream_t s,
                      StageMarks* marks = nullptr) {
    const PartitionView pv = partition_view(part);
    if (marks) MVF_HIP_TRY(marks->mark(-1, s));
    if (m == 0) return MVF_OK;
    const size_t per_set = (size_t)m * n_tokens;  // elements of a set in every output
    MaxsimAlignWriteParams wp{};
    wp.ids = v.ids;
    wp.index_base = v.index_base;
    wp.m = m;
    wp.n_tokens = n_tokens;
    wp.metric = metric;
    wp.dtype = v.dtype;
    // the writer over sets [w0, w0 + wn): tokens [t0, t0 + tc) from best64 / slots, or padding throughout where best64 is NULL
    auto write = [&](uint32_t w0, uint32_t wn, uint32_t t0, uint32_t tc, const uint64_t* best64, const uint32_t* slots, uint32_t nk) -> int {
        MaxsimAlignWriteParams p = wp;
        p.best64 = best64;
        p.slots = slots;
        p.out_scores = d_scores + (size_t)w0 * per_set;
        p.out_rows = d_rows + (size_t)w0 * per_set;
        p.out_raw = d_raw ? d_raw + (size_t)w0 * per_set : nullptr;
        p.sets = wn;
        p.n_keys = nk;
        p.t0 = t0;
        p.tc = tc;
        MVF_HIP_TRY(maxsim_align_write_launch(p, s));
        return MVF_OK;
    };
    auto pad = [&](uint32_t w0, uint32_t wn) { return write(w0, wn, 0, n_tokens, nullptr, nullptr, 0); };
    if (v.n == 0 || pv.live == 0 || pv.n_keys == 0) return pad(0, nq);
    const OneQueryGroup g1 = one_query_group(v);
    const size_t set_bytes = query_row_bytes(v) * n_tokens;
    CandPlan plan;
    if (const int rc = plan_candidates(part, keys, nq, m, n_tokens, g1.qbytes, v.maxsim_scratch, &plan, maxsim_align_plan, (uint64_t)m * 4))
        return rc;
    if (plan.segs.empty()) return pad(0, nq);

    // the slot map: an entry's key among its set's candidates (ascending key values) -- a repeat finds its first occurrence's slot
    std::vector<uint32_t> slots((size_t)nq * m);
    for (uint32_t q = 0; q < nq; q++) {
        const uint64_t* held = plan.keys.data() + plan.sets[q].seg0;
        const uint64_t* end = held + plan.sets[q].count;
        for (uint32_t i = 0; i < m; i++) {
            const uint64_t key = keys[(size_t)q * m + i];
            const uint64_t* at = std::lower_bound(held, end, key);
            slots[(size_t)q * m + i] = at != end && *at == key ? (uint32_t)(at - held) : UINT32_MAX;
        }
    }
    // the plan, one upload: segments | sets | blocks (8-byte entries) | slot map
    const size_t segs_b = plan.segs.size() * sizeof(MaxsimCandSeg), sets_b = (size_t)nq * sizeof(MaxsimCandSet),
                 blocks_b = plan.blocks.size() * sizeof(MaxsimCandBlock), slots_b = slots.size() * 4;
    std::vector<unsigned char> blob(segs_b + sets_b + blocks_b + slots_b);
    std::memcpy(blob.data(), plan.segs.data(), segs_b);
    std::memcpy(blob.data() + segs_b, plan.sets.data(), sets_b);
    if (blocks_b) std::memcpy(blob.data() + segs_b + sets_b, plan.blocks.data(), blocks_b);
    std::memcpy(blob.data() + segs_b + sets_b + blocks_b, slots.data(), slots_b);
    AsyncBuf dplan;
    MVF_HIP_TRY(dplan.alloc(blob.size(), s));
    if (const int rc = partition_upload(part, blob.data(), blob.size(), dplan.p, s)) return rc;
    const unsigned char* dp = static_cast<const unsigned char*>(dplan.p);
    const MaxsimCandSeg* p_segs = reinterpret_cast<const MaxsimCandSeg*>(dp);
    const MaxsimCandSet* p_sets = reinterpret_cast<const MaxsimCandSet*>(dp + segs_b);
    const MaxsimCandBlock* p_blocks = reinterpret_cast<const MaxsimCandBlock*>(dp + segs_b + sets_b);
    const uint32_t* p_slots = reinterpret_cast<const uint32_t*>(dp + segs_b + sets_b + blocks_b);

    for (const CandWindow& w : plan.windows) {
        if (w.n_keys == 0) {  // no set of the window holds a candidate
            if (const int rc = pad(w.w0, w.wn)) return rc;
            continue;
        }
        const uint32_t nk = w.n_keys, wn = w.wn;
        const size_t npos = (size_t)w.n_blocks * kMaxsimRows;
        AsyncBuf dlist, dbest;
        MVF_HIP_TRY(dlist.alloc(npos * 8, s));  // rows [npos], then slot ordinals [npos]
        MVF_HIP_TRY(dbest.alloc((size_t)wn * w.chunk * nk * 8, s));
        // E0: the window's concatenated list
        MaxsimExpandParams ep{};
        ep.rows_by_key = pv.rows_by_key;
        ep.sets = p_sets + w.w0;
        ep.segs = p_segs;
        ep.blocks = p_blocks + w.blk0;
        ep.n_blocks = w.n_blocks;
        ep.list = static_cast<uint32_t*>(dlist.p);
        ep.ord = ep.list + npos;
        MVF_HIP_TRY(maxsim_expand_launch(ep, s));
        if (marks) MVF_HIP_TRY(marks->mark(0, s));
        for (uint32_t t0 = 0; t0 < n_tokens; t0 += w.chunk) {
            const uint32_t tc = std::min(w.chunk, n_tokens - t0);
            MVF_HIP_TRY(hipMemsetAsync(dbest.p, 0xFF, (size_t)wn * tc * nk * 8, s));
            MaxsimScoreParams sp{};
            sp.rows = v.rows;
            sp.queries = static_cast<const unsigned char*>(d_queries) + (size_t)w.w0 * set_bytes;
            sp.list = ep.list;
            sp.ord = ep.ord;
            sp.best64 = static_cast<uint64_t*>(dbest.p);
            sp.m = (uint32_t)npos;
            sp.n_keys = nk;
            sp.sets = wn;
            sp.n_tokens = n_tokens;
            sp.t0 = t0;
            sp.tc = tc;
            sp.dim = v.dim;
            sp.pitch = v.pitch;
            sp.V = v.V;
            sp.J = g1.J;
            sp.blocks = ep.blocks;
            MVF_HIP_TRY(maxsim_score_arg_launch(v.dtype, metric, g1.G, sp, s));
            if (marks) MVF_HIP_TRY(marks->mark(1, s));
            if (const int rc = write(w.w0, wn, t0, tc, sp.best64, p_slots + (size_t)w.w0 * m, nk)) return rc;
            if (marks) MVF_HIP_TRY(marks->mark(2, s));
        }
    }
    return MVF_OK;
}

}  // namespace

extern "C" {

int mvfgpu_search_maxsim_device(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* d_queries,
                                uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t n_tokens, uint32_t k, float* d_scores,
                                uint64_t* d_keys, uint32_t* d_counts, void* hip_stream) {
    const int rc = check_maxsim_args(c, part, metric, d_queries, query_dtype, query_dim, nq, n_tokens, k, d_scores, d_keys);
    if (rc != MVF_OK) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return corpus_device_call(c, s, [&]() {
        return maxsim_core(c, corpus_view(c), partition_view(part), metric, d_queries, nq, n_tokens, k, d_scores, d_keys, d_counts, s);
    });
}

int mvfgpu_search_maxsim(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* queries, uint8_t query_dtype,
                         uint32_t query_dim, uint32_t nq, uint32_t n_tokens, uint32_t k, float* out_scores, uint64_t* out_keys,
                         uint32_t* out_counts) {
    const int rc0 = check_maxsim_args(c, part, metric, queries, query_dtype, query_dim, nq, n_tokens, k, out_scores, out_keys);
    if (rc0 != MVF_OK) return rc0;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));
    const CorpusView v = corpus_view(c);
    const PartitionView pv = partition_view(part);
    hipStream_t s = static_cast<hipStream_t>(v.stream);
    const HostIn in[] = {{queries, query_row_bytes(v) * n_tokens}};
    const HostOut out[] = {{out_keys, (size_t)k * 8}, {out_scores, (size_t)k * 4}, {out_counts, 4}};
    return stage_host_windows(c, s, nq, in, out, stage_as_given, [&](uint32_t, uint32_t wn, void* const* d_in, void* const* d_out) {
        return maxsim_core(c, v, pv, metric, d_in[0], wn, n_tokens, k, static_cast<float*>(d_out[1]), static_cast<uint64_t*>(d_out[0]),
                           static_cast<uint32_t*>(d_out[2]), s);
    });
}

int mvfgpu_selftest_maxsim_stage_ms(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* d_queries,
                                    uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t n_tokens, uint32_t k, float* d_scores,
                                    uint64_t* d_keys, void* hip_stream, float* out_ms) {
    if (!out_ms) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    const int rc0 = check_maxsim_args(c, part, metric, d_queries, query_dtype, query_dim, nq, n_tokens, k, d_scores, d_keys);
    if (rc0 != MVF_OK) return rc0;
    const PartitionView pv = partition_view(part);
    if (corpus_view(c).n == 0 || pv.live == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "the stage timer needs held rows");
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    StageMarks marks;
    int rc = corpus_device_call(c, s, [&]() { return maxsim_core(c, corpus_view(c), pv, metric, d_queries, nq, n_tokens, k, d_scores, d_keys, nullptr, s, &marks); });
    if (rc == MVF_OK && hipStreamSynchronize(s) != hipSuccess) rc = set_fail(MVF_ERR_DEVICE, "hipStreamSynchronize failed");
    for (int i = 0; i < 4; i++) out_ms[i] = 0.0f;
    return rc == MVF_OK ? stage_sums(marks, out_ms) : rc;
}

int mvfgpu_selftest_maxsim_mfma_stage_ms(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* d_queries,
                                         uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t n_tokens, uint32_t k,
                                         float* d_scores, uint64_t* d_keys, void* hip_stream, float* out_ms, uint32_t* out_candidates,
                                         uint32_t* out_blocks) {
    if (!out_ms || !out_candidates || !out_blocks) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    const int rc0 = check_maxsim_args(c, part, metric, d_queries, query_dtype, query_dim, nq, n_tokens, k, d_scores, d_keys);
    if (rc0 != MVF_OK) return rc0;
    const PartitionView pv = partition_view(part);
    if (corpus_view(c).n == 0 || pv.live == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "the stage timer needs held rows");
    if (!maxsim_mfma_eligible(corpus_view(c).dtype, metric))
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "the MFMA route takes Float32 / Float16 rows under InnerProduct / Cosine");
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    StageMarks marks;
    std::vector<uint32_t> host((size_t)nq * 2, 0u);
    int rc;
    {
        AsyncBuf dstats;
        rc = corpus_device_call(c, s, [&]() -> int {
            MVF_HIP_TRY(dstats.alloc((size_t)nq * 8, s));
            MVF_HIP_TRY(hipMemsetAsync(dstats.p, 0, (size_t)nq * 8, s));
            const MfmaStats st{static_cast<uint32_t*>(dstats.p), nq};
            const int rc1 = maxsim_core(c, corpus_view(c), pv, metric, d_queries, nq, n_tokens, k, d_scores, d_keys, nullptr, s, &marks, &st);
            if (rc1 != MVF_OK) return rc1;
            MVF_HIP_TRY(hipMemcpyAsync(host.data(), dstats.p, (size_t)nq * 8, hipMemcpyDeviceToHost, s));
            return MVF_OK;
        });
        if (hipStreamSynchronize(s) != hipSuccess && rc == MVF_OK) rc = set_fail(MVF_ERR_DEVICE, "hipStreamSynchronize failed");
    }
    for (int i = 0; i < 6; i++) out_ms[i] = 0.0f;
    if (rc != MVF_OK) return rc;
    std::memcpy(out_candidates, host.data(), (size_t)nq * 4);
    std::memcpy(out_blocks, host.data() + nq, (size_t)nq * 4);
    return stage_sums(marks, out_ms, 6);
}

int mvfgpu_selftest_maxsim_mfma_selection(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* d_queries,
                                          uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t n_tokens, uint32_t k,
                                          float* d_scores, uint64_t* d_keys, void* hip_stream, float* out_sums, uint8_t* out_forced,
                                          uint8_t* out_candidates, double* out_delta, float* out_theta, uint8_t* out_theta_nan,
                                          float* out_xxmax) {
    if (!out_sums || !out_forced || !out_candidates || !out_delta || !out_theta || !out_theta_nan || !out_xxmax)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    const int rc0 = check_maxsim_args(c, part, metric, d_queries, query_dtype, query_dim, nq, n_tokens, k, d_scores, d_keys);
    if (rc0 != MVF_OK) return rc0;
    const PartitionView pv = partition_view(part);
    if (corpus_view(c).n == 0 || pv.live == 0 || pv.n_keys == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "the read-out needs held rows");
    if (!maxsim_mfma_eligible(corpus_view(c).dtype, metric))
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "the MFMA route takes Float32 / Float16 rows under InnerProduct / Cosine");
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const size_t cells = (size_t)nq * pv.n_keys;
    std::vector<float> sums(cells);
    std::vector<unsigned char> forced(cells), cands(cells);
    std::vector<double> delta(nq);
    std::vector<uint64_t> kth(nq);
    float xxmax = 0.0f;
    int rc;
    {
        AsyncBuf dstats, dsums, dforced, dcands, ddelta, dkth, dxxmax;
        rc = corpus_device_call(c, s, [&]() -> int {
            MVF_HIP_TRY(dstats.alloc((size_t)nq * 8, s));
            MVF_HIP_TRY(hipMemsetAsync(dstats.p, 0, (size_t)nq * 8, s));
            MVF_HIP_TRY(dsums.alloc(cells * 4, s));
            MVF_HIP_TRY(dforced.alloc(cells, s));
            MVF_HIP_TRY(dcands.alloc(cells, s));
            MVF_HIP_TRY(ddelta.alloc((size_t)nq * 8, s));
            MVF_HIP_TRY(dkth.alloc((size_t)nq * 8, s));
            MVF_HIP_TRY(dxxmax.alloc(4, s));
            MfmaStats st{static_cast<uint32_t*>(dstats.p), nq};
            st.d_sums = static_cast<float*>(dsums.p);
            st.d_forced = static_cast<unsigned char*>(dforced.p);
            st.d_cands = static_cast<unsigned char*>(dcands.p);
            st.d_delta = static_cast<double*>(ddelta.p);
            st.d_kth = static_cast<uint64_t*>(dkth.p);
            st.d_xxmax = static_cast<float*>(dxxmax.p);
            const int rc1 = maxsim_core(c, corpus_view(c), pv, metric, d_queries, nq, n_tokens, k, d_scores, d_keys, nullptr, s, nullptr, &st);
            if (rc1 != MVF_OK) return rc1;
            MVF_HIP_TRY(hipMemcpyAsync(sums.data(), dsums.p, cells * 4, hipMemcpyDeviceToHost, s));
            MVF_HIP_TRY(hipMemcpyAsync(forced.data(), dforced.p, cells, hipMemcpyDeviceToHost, s));
            MVF_HIP_TRY(hipMemcpyAsync(cands.data(), dcands.p, cells, hipMemcpyDeviceToHost, s));
            MVF_HIP_TRY(hipMemcpyAsync(delta.data(), ddelta.p, (size_t)nq * 8, hipMemcpyDeviceToHost, s));
            MVF_HIP_TRY(hipMemcpyAsync(kth.data(), dkth.p, (size_t)nq * 8, hipMemcpyDeviceToHost, s));
            MVF_HIP_TRY(hipMemcpyAsync(&xxmax, dxxmax.p, 4, hipMemcpyDeviceToHost, s));
            return MVF_OK;
        });
        if (hipStreamSynchronize(s) != hipSuccess && rc == MVF_OK) rc = set_fail(MVF_ERR_DEVICE, "hipStreamSynchronize failed");
    }
    if (rc != MVF_OK) return rc;
    std::memcpy(out_sums, sums.data(), cells * 4);
    std::memcpy(out_forced, forced.data(), cells);
    std::memcpy(out_candidates, cands.data(), cells);
    std::memcpy(out_delta, delta.data(), (size_t)nq * 8);
    for (uint32_t q = 0; q < nq; q++) {  // as P0 reads the entry: the key half, 0xFFFFFFFE a live NaN entry
        const uint32_t te = (uint32_t)kth[q];
        out_theta[q] = score_from_key(te, metric);
        out_theta_nan[q] = te >= 0xFFFFFFFEu ? 1 : 0;
    }
    *out_xxmax = xxmax;
    return MVF_OK;
}

int mvfgpu_selftest_maxsim_route(uint64_t held_rows, uint64_t n_keys, uint32_t dimension, uint8_t data_type, uint8_t metric, uint32_t nq,
                                 uint32_t n_tokens, uint32_t k, int forced, uint32_t* out_route) {
    if (!out_route) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (elem_size(data_type) == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "unsupported vector data type code " + std::to_string(data_type));
    if (const int rc = check_metric(metric)) return rc;
    if (dimension == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "dimension must be > 0");
    if (n_tokens == 0 || n_tokens > MVFGPU_MAXSIM_MAX_TOKENS)
        return set_fail(MVF_ERR_INVALID_ARGUMENT,
                        "n_tokens must be in 1.." + std::to_string(MVFGPU_MAXSIM_MAX_TOKENS) + ", got " + std::to_string(n_tokens));
    if (forced < 0 || forced > 2) return set_fail(MVF_ERR_INVALID_ARGUMENT, "route must be 0, 1 or 2, got " + std::to_string(forced));
    *out_route = maxsim_route(held_rows, n_keys, dimension, data_type, metric, nq, n_tokens, k, forced);
    return MVF_OK;
}

int mvfgpu_selftest_maxsim_margin(uint8_t data_type, uint8_t metric, uint32_t dimension, const float* token_norms, uint32_t n_tokens,
                                  float xxmax, double* out_delta) {
    if (!token_norms || !out_delta) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (!maxsim_mfma_eligible(data_type, metric))
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "the MFMA route takes Float32 / Float16 rows under InnerProduct / Cosine");
    if (dimension == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "dimension must be > 0");
    if (n_tokens == 0 || n_tokens > MVFGPU_MAXSIM_MAX_TOKENS)
        return set_fail(MVF_ERR_INVALID_ARGUMENT,
                        "n_tokens must be in 1.." + std::to_string(MVFGPU_MAXSIM_MAX_TOKENS) + ", got " + std::to_string(n_tokens));
    *out_delta = maxsim_margin(data_type, metric, dimension, token_norms, n_tokens, xxmax);
    return MVF_OK;
}

int mvfgpu_search_maxsim_candidates_device(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* d_queries,
                                           uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t n_tokens,
                                           const uint64_t* candidate_keys, uint32_t m, uint32_t k, float* d_scores, uint64_t* d_keys,
                                           uint32_t* d_counts, void* hip_stream) {
    const int rc = check_candidates_args(c, part, metric, d_queries, query_dtype, query_dim, nq, n_tokens, candidate_keys, m, k, d_scores, d_keys);
    if (rc != MVF_OK) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return corpus_device_call(c, s, [&]() {
        return maxsim_candidates_core(corpus_view(c), part, metric, d_queries, nq, n_tokens, candidate_keys, m, k, d_scores, d_keys, d_counts, s);
    });
}

int mvfgpu_search_maxsim_candidates(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* queries,
                                    uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t n_tokens, const uint64_t* candidate_keys,
                                    uint32_t m, uint32_t k, float* out_scores, uint64_t* out_keys, uint32_t* out_counts) {
    const int rc0 = check_candidates_args(c, part, metric, queries, query_dtype, query_dim, nq, n_tokens, candidate_keys, m, k, out_scores, out_keys);
    if (rc0 != MVF_OK) return rc0;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));
    const CorpusView v = corpus_view(c);
    hipStream_t s = static_cast<hipStream_t>(v.stream);
    const HostIn in[] = {{queries, query_row_bytes(v) * n_tokens}};
    const HostOut out[] = {{out_keys, (size_t)k * 8}, {out_scores, (size_t)k * 4}, {out_counts, 4}};
    return stage_host_windows(c, s, nq, in, out, stage_as_given, [&](uint32_t w0, uint32_t wn, void* const* d_in, void* const* d_out) {
        return maxsim_candidates_core(v, part, metric, d_in[0], wn, n_tokens, candidate_keys ? candidate_keys + (size_t)w0 * m : nullptr, m, k,
                                      static_cast<float*>(d_out[1]), static_cast<uint64_t*>(d_out[0]), static_cast<uint32_t*>(d_out[2]), s);
    });
}

int mvfgpu_selftest_maxsim_candidates_stage_ms(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* d_queries,
                                               uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t n_tokens,
                                               const uint64_t* candidate_keys, uint32_t m, uint32_t k, float* d_scores, uint64_t* d_keys,
                                               void* hip_stream, float* out_ms) {
    if (!out_ms) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    const int rc0 = check_candidates_args(c, part, metric, d_queries, query_dtype, query_dim, nq, n_tokens, candidate_keys, m, k, d_scores, d_keys);
    if (rc0 != MVF_OK) return rc0;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    StageMarks marks;
    int rc = corpus_device_call(c, s, [&]() {
        return maxsim_candidates_core(corpus_view(c), part, metric, d_queries, nq, n_tokens, candidate_keys, m, k, d_scores, d_keys, nullptr, s, &marks);
    });
    if (rc == MVF_OK && hipStreamSynchronize(s) != hipSuccess) rc = set_fail(MVF_ERR_DEVICE, "hipStreamSynchronize failed");
    for (int i = 0; i < 4; i++) out_ms[i] = 0.0f;
    return rc == MVF_OK ? stage_sums(marks, out_ms) : rc;
}

int mvfgpu_selftest_maxsim_candidates_plan(const uint64_t* candidate_keys, const uint64_t* held_counts, uint32_t m, uint32_t* out_slot,
                                           uint32_t* out_distinct, uint64_t* out_rows) {
    if (!out_distinct || !out_rows || (m && (!candidate_keys || !held_counts || !out_slot))) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    std::vector<std::pair<uint64_t, uint32_t>> distinct;
    distinct_entries(candidate_keys, m, [&](uint32_t i) { return held_counts[i] != 0; }, &distinct);
    for (uint32_t i = 0; i < m; i++) out_slot[i] = UINT32_MAX;
    *out_distinct = (uint32_t)distinct.size();
    *out_rows = 0;
    for (size_t j = 0; j < distinct.size(); j++) {
        out_slot[distinct[j].second] = (uint32_t)j;
        *out_rows += held_counts[distinct[j].second];
    }
    return MVF_OK;
}

int mvfgpu_selftest_maxsim_plan(uint64_t n_keys, uint32_t n_tokens, uint32_t nq, uint64_t token_bytes, uint64_t budget_bytes,
                                uint32_t* tokens_per_chunk, uint32_t* sets_per_window) {
    if (!tokens_per_chunk || !sets_per_window) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (n_tokens == 0 || n_tokens > MVFGPU_MAXSIM_MAX_TOKENS)
        return set_fail(MVF_ERR_INVALID_ARGUMENT,
                        "n_tokens must be in 1.." + std::to_string(MVFGPU_MAXSIM_MAX_TOKENS) + ", got " + std::to_string(n_tokens));
    if (nq == 0 || budget_bytes == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "empty batch or budget");
    const MaxsimPlan pl = maxsim_plan(n_keys, n_tokens, nq, token_bytes, budget_bytes);
    *tokens_per_chunk = pl.chunk;
    *sets_per_window = pl.window;
    return MVF_OK;
}

int mvfgpu_selftest_maxsim_form(uint8_t data_type, uint32_t dimension, uint32_t forced_g, uint32_t* out_g, uint32_t* out_j,
                                uint32_t* out_token_bytes, uint32_t* out_form, uint32_t* out_lds_chunk_cap) {
    if (!out_g || !out_j || !out_token_bytes || !out_form || !out_lds_chunk_cap) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
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
    const MaxsimForm f = maxsim_form(data_type, G, J);
    *out_g = (uint32_t)G;
    *out_j = J;
    *out_token_bytes = f.token_bytes;
    *out_form = f.reg ? 0u : f.qlds ? 1u : 2u;
    *out_lds_chunk_cap = maxsim_plan(1, MVFGPU_MAXSIM_MAX_TOKENS, 1, f.token_bytes, ~0ull).chunk;
    return MVF_OK;
}

int mvfgpu_maxsim_align_device(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* d_queries,
                               uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t n_tokens, const uint64_t* keys, uint32_t m,
                               float* d_scores, uint64_t* d_rows, int32_t* d_raw, void* hip_stream) {
    const int rc = check_align_args(c, part, metric, d_queries, query_dtype, query_dim, nq, n_tokens, keys, m, d_scores, d_rows);
    if (rc != MVF_OK) return rc;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return corpus_device_call(c, s, [&]() {
        return maxsim_align_core(corpus_view(c), part, metric, d_queries, nq, n_tokens, keys, m, d_scores, d_rows, d_raw, s);
    });
}

int mvfgpu_maxsim_align(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* queries, uint8_t query_dtype,
                        uint32_t query_dim, uint32_t nq, uint32_t n_tokens, const uint64_t* keys, uint32_t m, float* out_scores,
                        uint64_t* out_rows, int32_t* out_raw) {
    const int rc0 = check_align_args(c, part, metric, queries, query_dtype, query_dim, nq, n_tokens, keys, m, out_scores, out_rows);
    if (rc0 != MVF_OK) return rc0;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    if (m == 0) return MVF_OK;  // nothing to write
    std::lock_guard<std::mutex> host_lk(corpus_host_mutex(c));
    const CorpusView v = corpus_view(c);
    hipStream_t s = static_cast<hipStream_t>(v.stream);
    const size_t per_set = (size_t)m * n_tokens;
    const HostIn in[] = {{queries, query_row_bytes(v) * n_tokens}};
    const HostOut out[] = {{out_rows, per_set * 8}, {out_scores, per_set * 4}, {out_raw, per_set * 4}};
    return stage_host_windows(c, s, nq, in, out, stage_as_given, [&](uint32_t w0, uint32_t wn, void* const* d_in, void* const* d_out) {
        return maxsim_align_core(v, part, metric, d_in[0], wn, n_tokens, keys + (size_t)w0 * m, m, static_cast<float*>(d_out[1]),
                                 static_cast<uint64_t*>(d_out[0]), static_cast<int32_t*>(d_out[2]), s);
    });
}

int mvfgpu_selftest_maxsim_align_stage_ms(const mvfgpu_corpus* c, const mvfgpu_partition* part, uint8_t metric, const void* d_queries,
                                          uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t n_tokens, const uint64_t* keys,
                                          uint32_t m, float* d_scores, uint64_t* d_rows, int32_t* d_raw, void* hip_stream, float* out_ms) {
    if (!out_ms) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    const int rc0 = check_align_args(c, part, metric, d_queries, query_dtype, query_dim, nq, n_tokens, keys, m, d_scores, d_rows);
    if (rc0 != MVF_OK) return rc0;
    DevScope guard(corpus_view(c).device);
    if (!guard.ok) return set_fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    StageMarks marks;
    int rc = corpus_device_call(c, s, [&]() {
        return maxsim_align_core(corpus_view(c), part, metric, d_queries, nq, n_tokens, keys, m, d_scores, d_rows, d_raw, s, &marks);
    });
    if (rc == MVF_OK && hipStreamSynchronize(s) != hipSuccess) rc = set_fail(MVF_ERR_DEVICE, "hipStreamSynchronize failed");
    for (int i = 0; i < 3; i++) out_ms[i] = 0.0f;
    return rc == MVF_OK ? stage_sums(marks, out_ms, 3) : rc;
}

int mvfgpu_selftest_maxsim_align_plan(uint64_t n_keys, uint32_t n_tokens, uint32_t nq, uint64_t token_bytes, uint64_t budget_bytes,
                                      uint32_t* tokens_per_chunk, uint32_t* sets_per_window) {
    if (!tokens_per_chunk || !sets_per_window) return set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (n_tokens == 0 || n_tokens > MVFGPU_MAXSIM_MAX_TOKENS)
        return set_fail(MVF_ERR_INVALID_ARGUMENT,
                        "n_tokens must be in 1.." + std::to_string(MVFGPU_MAXSIM_MAX_TOKENS) + ", got " + std::to_string(n_tokens));
    if (nq == 0 || budget_bytes == 0) return set_fail(MVF_ERR_INVALID_ARGUMENT, "empty batch or budget");
    const MaxsimPlan pl = maxsim_align_plan(n_keys, n_tokens, nq, token_bytes, budget_bytes);
    *tokens_per_chunk = pl.chunk;
    *sets_per_window = pl.window;
    return MVF_OK;
}

}  // extern "C"
