// scan_mmr.hip — D0, the greedy walk of the diversified re-ranking (mmr.hip; DESIGN.md §3 "Diversified re-ranking", §5 "D0").
//
// One block of 256 threads per query, one launch for a window of queries.  The block reads the query's relevance entries
// (the gathered-row kernel's dump over C0's rows: ascending row = ascending list position) into LDS -- row, order key,
// rel = value(score), red = -inf, taken = 0 per position -- and makes min(k, count) picks.  Per pick:
//   1. thread t folds the positions t, t + 256, .. that are not taken into the smallest (order key << 32 | position) -- the
//      search's key for pick 0, the key of the objective (mmr_walk.h) from then on --, the waves reduce by shuffles, the four
//      wave results meet in LDS;
//   2. thread 0 formats the pick (score, position or id, raw, objective) and marks it taken;
//   3. unless it was the last pick: the picked row is staged as a query as K1 stages one (zero padded to J G vectors, Float16
//      widened first, the sum of squares in K1's staging order) -- to LDS, or where the padded query exceeds kCandQueryLdsMax
//      to the query's f32 scratch row, read back through the cache --, and every position that is not taken is scored against
//      it with K1's per-row arithmetic (k1_rowscore.h: accumulate, group_sum, make_key) in the lane group of K1's one-query
//      shape: the gathered-row kernel's inner loop for one query; red = max(red, value(score)), NaN ignored.
// Position i is always scored by the same lane group and folded by the same thread.  The pick count is block-uniform and every
// barrier is reached by all threads; no block waits for another.
//
// Algorithmic bytes per query: (min(k, count) - 1) count pitch, re-read from the cache (+ 8 bytes per position once).

#include "scan_mmr.h"
#include "k1_rowscore.h"
#include "mmr_walk.h"
#include "mvf_common.h"

namespace mvf {
namespace {

template <int DT>
__device__ __forceinline__ typename k1::Traits<DT>::Q row_element(const unsigned char* rp, uint32_t e) {
    if constexpr (DT == MVF_DTYPE_FLOAT32) return reinterpret_cast<const float*>(rp)[e];
    else if constexpr (DT == MVF_DTYPE_FLOAT16) return __half2float(reinterpret_cast<const __half*>(rp)[e]);  // exact
    else return reinterpret_cast<const typename k1::Traits<DT>::Q*>(rp)[e];
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

// grid (nq), block 256; dynamic LDS: the padded query (QLDS), else none
template <int DT, int METRIC, int G, bool QLDS>
__global__ void __launch_bounds__(256) mmr_walk_kernel(MmrWalkParams p) {
    using Tr = k1::Traits<DT>;
    using Acc = typename Tr::Acc;
    using QT = typename Tr::Q;
    constexpr int EPV = 16 / Tr::ES;
    constexpr int RPG = 64 / G;
    constexpr int U = 4;
    constexpr bool NEED_XX = k1::kNeedXX<DT, METRIC>;
    static_assert(QLDS || !Tr::INT, "only a float query is ever read through the cache");

    extern __shared__ __attribute__((aligned(16))) unsigned char qs[];  // [J G vectors] the picked row as a query (QLDS)
    __shared__ uint32_t rowbuf[kMmrMaxCandidates], keybuf[kMmrMaxCandidates];
    __shared__ float rel[kMmrMaxCandidates], red[kMmrMaxCandidates];
    __shared__ uint8_t taken[kMmrMaxCandidates];
    __shared__ Acc qqpart[4];
    __shared__ uint64_t wbest[4];

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t sub = lane % G, rsel = lane / G;
    const uint32_t q = blockIdx.x;
    const uint32_t cnt = min(p.counts[q], p.m);  // block-uniform
    if (cnt == 0) return;
    const uint32_t npick = min(p.k, cnt);

    for (uint32_t i = tid; i < cnt; i += 256) {
        const uint64_t comp = composite_of_rank_entry(p.dump[(size_t)q * p.m + i]);
        const uint32_t key = (uint32_t)(comp >> 32);
        int32_t raw;
        rowbuf[i] = (uint32_t)comp;
        keybuf[i] = key;
        rel[i] = mmr::value(mmr::score_of_key(key, DT, METRIC, &raw), METRIC);
        red[i] = -INFINITY;
        taken[i] = 0;
    }
    __syncthreads();

    const uint32_t VP = p.J * G;
    float* qglobal = QLDS ? nullptr : p.qscratch + (size_t)q * p.dim;
    const uint32_t ngroups = (cnt + RPG - 1) / RPG;
    const size_t ob = (size_t)q * p.k;

    for (uint32_t j = 0; j < npick; j++) {  // block-uniform
        // ---- 1. the best position that is not taken
        uint64_t best = kPadComposite;
        for (uint32_t i = tid; i < cnt; i += 256) {
            if (taken[i]) continue;
            const uint32_t key = j == 0 ? keybuf[i] : mmr::order_key(mmr::objective(p.a, rel[i], p.b, red[i]));
            const uint64_t c = ((uint64_t)key << 32) | i;
            best = c < best ? c : best;
        }
        best = wave_min_u64(best);
        if (lane == 0) wbest[wave] = best;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 4; w++) best = wbest[w] < best ? wbest[w] : best;
        if (best == kPadComposite) break;   // block-uniform; never: j < cnt, some position was left
        const uint32_t s = (uint32_t)best;
        // ---- 2. the pick
        if (tid == 0) {
            int32_t raw;
            p.out_scores[ob + j] = mmr::score_of_key(keybuf[s], DT, METRIC, &raw);
            p.out_indices[ob + j] = p.ids ? p.ids[rowbuf[s]] : p.index_base + rowbuf[s];
            if (p.out_raw) p.out_raw[ob + j] = raw;
            if (p.out_objective) p.out_objective[ob + j] = mmr::reported(j == 0 ? mmr::relevance_term(p.a, rel[s]) : mmr::objective(p.a, rel[s], p.b, red[s]));
            taken[s] = 1;
        }
        if (j + 1 == npick) break;
        // ---- 3. the picked row as a query: K1's staging loop and sum of squares (k1::stage_queries' lines)
        const unsigned char* srow = p.rows + (size_t)rowbuf[s] * p.pitch;
        Acc qq_part = 0;
        for (uint32_t e = tid; e < VP * EPV; e += 256) {
            const QT v = e < p.dim ? row_element<DT>(srow, e) : (QT)0;
            if constexpr (QLDS) reinterpret_cast<QT*>(qs)[e] = v;
            else if (e < p.dim) qglobal[e] = v;
            if constexpr (Tr::INT) qq_part += (int32_t)v * (int32_t)v;
            else qq_part = fmaf(v, v, qq_part);
        }
        {
            const Acc t = k1::group_sum<64>(qq_part);
            if (lane == 0) qqpart[wave] = t;
        }
        __syncthreads();  // the query, its partial sums and taken[s] are visible
        const Acc qq = qqpart[0] + qqpart[1] + qqpart[2] + qqpart[3];

        for (uint32_t g0 = wave * U; g0 < ngroups; g0 += 4 * U) {  // wave-uniform: every lane reaches the shuffles
            uint32_t idx[U];
            bool rv[U];
            const unsigned char* rp[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                idx[u] = (g0 + u) * RPG + rsel;
                rv[u] = idx[u] < cnt && !taken[idx[u]];
                rp[u] = p.rows + (size_t)(rv[u] ? rowbuf[idx[u]] : 0u) * p.pitch;
            }
            Acc acc[1][U], xx[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                xx[u] = 0;
                acc[0][u] = 0;
            }
            for (uint32_t jj = 0; jj < p.J; jj++) {
                const uint32_t v = jj * G + sub;
                const bool vv = v < p.V;
                k1::u32x4 x[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    x[u] = k1::u32x4{0, 0, 0, 0};
                    if (vv && rv[u]) x[u] = *reinterpret_cast<const k1::u32x4*>(rp[u] + (size_t)v * 16);
                }
                if constexpr (!QLDS) {
                    k1::accumulate<DT, METRIC, U, 1>(acc, xx, x, [&](int, int half) __attribute__((always_inline)) {
                        return k1::query_global4(qglobal, p.dim, v * EPV + half * 4);
                    });
                } else if constexpr (Tr::INT) {
                    k1::accumulate<DT, METRIC, U, 1>(acc, xx, x, [&](int, int) __attribute__((always_inline)) {
                        return *reinterpret_cast<const uint4*>(qs + (size_t)v * 16);
                    });
                } else {
                    k1::accumulate<DT, METRIC, U, 1>(acc, xx, x, [&](int, int half) __attribute__((always_inline)) {
                        return *reinterpret_cast<const float4*>(qs + (size_t)v * (EPV * 4) + half * 16);
                    });
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                Acc xxs = 0;
                if constexpr (NEED_XX) xxs = k1::group_sum<G>(xx[u]);
                const uint32_t key = k1::make_key<DT, METRIC>(k1::group_sum<G>(acc[0][u]), xxs, qq);
                if (sub == 0 && rv[u]) {
                    int32_t raw;
                    const float sim = mmr::value(mmr::score_of_key(key, DT, METRIC, &raw), METRIC);
                    red[idx[u]] = mmr::max_ignoring_nan(red[idx[u]], sim);
                }
            }
        }
        __syncthreads();  // red is whole; qs, qqpart and wbest are free again
    }
}

template <int DT>
const void* pick_kernel(int metric, int G, bool qlds) {
    return k1::for_metric(metric, [&](auto m) {
        return k1::for_group(G, [&](auto g) -> const void* {
            constexpr int M = decltype(m)::value, GG = decltype(g)::value;
            if constexpr (!k1::Traits<DT>::INT) {
                if (!qlds) return reinterpret_cast<const void*>(&mmr_walk_kernel<DT, M, GG, false>);
            }
            return reinterpret_cast<const void*>(&mmr_walk_kernel<DT, M, GG, true>);
        });
    });
}

}  // namespace

hipError_t mmr_walk_launch(uint8_t dtype, int metric, int G, const MmrWalkParams& p, hipStream_t s) {
    if (p.nq == 0 || p.m == 0) return hipSuccess;
    if (p.m > kMmrMaxCandidates) return hipErrorInvalidValue;
    const MmrForm form = mmr_form(dtype, G, p.J);
    const uint32_t qbytes = form.qbytes;
    const bool qlds = form.qlds;
    if (!qlds && !p.qscratch) return hipErrorInvalidValue;
    const void* fn = nullptr;
    switch (dtype) {
        case MVF_DTYPE_FLOAT32: fn = pick_kernel<MVF_DTYPE_FLOAT32>(metric, G, qlds); break;
        case MVF_DTYPE_FLOAT16: fn = pick_kernel<MVF_DTYPE_FLOAT16>(metric, G, qlds); break;
        case MVF_DTYPE_INT8: fn = pick_kernel<MVF_DTYPE_INT8>(metric, G, qlds); break;
        case MVF_DTYPE_UINT8: fn = pick_kernel<MVF_DTYPE_UINT8>(metric, G, qlds); break;
        default: break;
    }
    if (!fn) return hipErrorInvalidValue;
    MmrWalkParams arg = p;
    void* args[] = {&arg};
    return hipLaunchKernel(fn, dim3(p.nq), dim3(256), args, qlds ? (size_t)qbytes : 0, s);
}

}  // namespace mvf
