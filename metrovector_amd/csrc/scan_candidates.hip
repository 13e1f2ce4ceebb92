// scan_candidates.hip — C0 (a query's candidate list -> its distinct live local rows, ascending) and C1 (K1's scores of those
// rows, chunk by chunk) of the candidate search (candidates.hip, DESIGN.md §5 "C0 / C1 — candidate search").
//
// C0 maps every entry to a local row (UINT64_MAX, positions outside the shard and deleted rows become dead), sorts the list
// and keeps the first of every run of equal rows: exact counts, distinct rows for the selection, and the gathers of C1 in
// ascending row order.  Lists of up to kCandLdsSort entries are sorted in one block's LDS, longer ones by sort_composites.
// C1 gives each chunk of kCandChunk rows one block: the query is staged as K1 stages it (zero padded to J G vectors; its sum
// of squares in K1's order), each G-lane group of K1's one-query shape scores one row with K1's per-row arithmetic
// (k1_rowscore.h), U = 4 rows in flight per wave.  The keys are K1's bits; ties and NaN follow from the composites.
//
// Algorithmic HBM bytes: the distinct rows' pitch each (+ 12 bytes per list entry).

#include "scan_candidates.h"
#include "aux_kernels.h"
#include "bitonic.h"
#include "k1_rowscore.h"
#include "mvf_common.h"

#include <algorithm>
#include <type_traits>

namespace mvf {
namespace {

constexpr uint32_t kDeadRow = 0xFFFFFFFFu;  // no local row is this large (a shard holds at most 2^32 - 65536 rows)

__device__ __forceinline__ uint32_t local_row(uint64_t g, const CandPrepParams& p) {
    if (g == ~0ull || g < p.index_base || g - p.index_base >= p.n) return kDeadRow;
    const uint32_t r = (uint32_t)(g - p.index_base);
    if (p.tomb && ((p.tomb[r >> 5] >> (r & 31)) & 1u)) return kDeadRow;
    return r;
}

// The first of every run of equal rows of an ascending list (dead entries last) -> out, in order; block of 1024 threads.
// get(i): the list's row i.  wsum: 16 words of LDS.
template <class Get>
__device__ __forceinline__ void compact_rows(Get get, uint32_t m, uint32_t* out, uint32_t* cnt, uint64_t* cnt64, uint32_t* wsum) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t base = 0;
    for (uint32_t t0 = 0; t0 < m; t0 += 1024) {
        const uint32_t i = t0 + tid;
        const uint32_t r = i < m ? get(i) : kDeadRow;
        const bool keep = r != kDeadRow && (i == 0 || get(i - 1) != r);
        const unsigned long long bm = __builtin_amdgcn_ballot_w64(keep);
        if (lane == 0) wsum[wave] = (uint32_t)__builtin_popcountll(bm);
        __syncthreads();
        uint32_t off = base, tot = 0;
#pragma unroll
        for (uint32_t w = 0; w < 16; w++) {
            const uint32_t c = wsum[w];
            off += w < wave ? c : 0u;
            tot += c;
        }
        if (keep) out[off + __builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u))] = r;
        base += tot;
        __syncthreads();
    }
    if (tid == 0) {
        *cnt = base;
        if (cnt64) *cnt64 = base;
    }
}

// C0, lists of up to kCandLdsSort entries: grid (nq), block 1024, dynamic LDS next_pow2(m) * 8
__global__ void __launch_bounds__(1024) cand_prep_kernel(CandPrepParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* buf = reinterpret_cast<uint64_t*>(smem);
    __shared__ uint32_t wsum[16];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t P = next_pow2(p.m < 2 ? 2u : p.m);
    const uint64_t* c = p.cand + (size_t)q * p.m;
    for (uint32_t i = tid; i < P; i += 1024) buf[i] = i < p.m ? (uint64_t)local_row(c[i], p) : (uint64_t)kDeadRow;
    __syncthreads();
    if (P <= 1024) bitonic_sort_u64_reg<1024, 1>(buf, P, (int)tid);
    else if (P <= 2048) bitonic_sort_u64_reg<1024, 2>(buf, P, (int)tid);
    else if (P <= 4096) bitonic_sort_u64_reg<1024, 4>(buf, P, (int)tid);
    else bitonic_sort_u64<1024>(buf, P, (int)tid);
    compact_rows([&](uint32_t i) { return (uint32_t)buf[i]; }, p.m, p.rows + (size_t)q * p.m, p.counts + q,
                 p.out_counts ? p.out_counts + q : nullptr, wsum);
}

// C0, longer lists, step 1: rank entries (list position << 32 | local row) for sort_composites, which orders them by row
__global__ void __launch_bounds__(256) cand_map_kernel(CandPrepParams p) {
    const uint32_t q = blockIdx.y;
    const uint64_t* c = p.cand + (size_t)q * p.m;
    uint64_t* e = p.ent + (size_t)q * p.m;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < p.m; i += gridDim.x * 256) e[i] = ((uint64_t)i << 32) | local_row(c[i], p);
}

// C0, longer lists, step 2: the sorted entries -> distinct rows; grid (nq), block 1024
__global__ void __launch_bounds__(1024) cand_compact_kernel(CandPrepParams p, const uint64_t* sorted) {
    __shared__ uint32_t wsum[16];
    const uint32_t q = blockIdx.x;
    const uint64_t* e = sorted + (size_t)q * p.m;
    compact_rows([&](uint32_t i) { return (uint32_t)e[i]; }, p.m, p.rows + (size_t)q * p.m, p.counts + q,
                 p.out_counts ? p.out_counts + q : nullptr, wsum);
}

template <int DT> struct CTraits;
template <> struct CTraits<MVF_DTYPE_FLOAT32> { static constexpr int ES = 4; static constexpr bool INT = false; using Q = float; using Acc = float; };
template <> struct CTraits<MVF_DTYPE_FLOAT16> { static constexpr int ES = 2; static constexpr bool INT = false; using Q = float; using Acc = float; };
template <> struct CTraits<MVF_DTYPE_INT8> { static constexpr int ES = 1; static constexpr bool INT = true; using Q = int8_t; using Acc = int32_t; };
template <> struct CTraits<MVF_DTYPE_UINT8> { static constexpr int ES = 1; static constexpr bool INT = true; using Q = uint8_t; using Acc = int32_t; };

template <int G, typename T>
__device__ __forceinline__ T gsum(T v) {
    if constexpr (std::is_integral<T>::value) return k1::group_sum_i32<G>(v);
    else return k1::group_sum<G>(v);
}

// C1: grid (ceil(m / kCandChunk), nq), block 256; dynamic LDS kCandChunk * 12 + 16 (+ the padded query when QLDS)
template <int DT, int METRIC, int G, bool QLDS>
__global__ void __launch_bounds__(256) cand_score_kernel(CandScoreParams p) {
    using Tr = CTraits<DT>;
    using Acc = typename Tr::Acc;
    using QT = typename Tr::Q;
    constexpr int EPV = 16 / Tr::ES;
    constexpr int RPG = 64 / G;
    constexpr int U = 4;
    constexpr bool NEED_XX = (METRIC == MVF_METRIC_COSINE) || (Tr::INT && METRIC == MVF_METRIC_L2);
    static_assert(QLDS || !Tr::INT, "integer queries always fit LDS");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* buf = reinterpret_cast<uint64_t*>(smem);                            // [kCandChunk] composites
    uint32_t* rowbuf = reinterpret_cast<uint32_t*>(smem + kCandChunk * 8);        // [kCandChunk] the chunk's rows
    Acc* red = reinterpret_cast<Acc*>(smem + kCandChunk * 12);                    // [4] qq partials
    unsigned char* qs = smem + kCandChunk * 12 + 16;                              // [J G vectors] the query (QLDS)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane % G, rsel = lane / G;
    const uint32_t q = blockIdx.y, c0 = blockIdx.x * kCandChunk;
    const uint32_t cnt = p.counts[q];
    const uint32_t nr = cnt > c0 ? min(kCandChunk, cnt - c0) : 0u;
    const uint32_t span = min(kCandChunk, p.m - c0);  // list positions of this chunk
    uint64_t* lout = p.lists ? p.lists + ((size_t)q * gridDim.x + blockIdx.x) * p.kcap : nullptr;
    uint64_t* dout = p.dump ? p.dump + (size_t)q * p.m + c0 : nullptr;
    if (dout)
        for (uint32_t i = nr + tid; i < span; i += 256) dout[i] = rank_entry(0u, c0 + i, true);
    if (nr == 0) {  // block-uniform
        if (lout)
            for (uint32_t i = tid; i < p.kcap; i += 256) lout[i] = kPadComposite;
        return;
    }

    // ---- the query: K1's staging loop (zero padded to J G vectors) and sum of squares
    const uint32_t VP = p.J * G;
    const QT* src = reinterpret_cast<const QT*>(p.queries) + (size_t)q * p.dim;
    Acc qq_part = 0;
    for (uint32_t e = tid; e < VP * EPV; e += 256) {
        const QT v = e < p.dim ? src[e] : (QT)0;
        if constexpr (QLDS) reinterpret_cast<QT*>(qs)[e] = v;
        if constexpr (Tr::INT) qq_part += (int32_t)v * (int32_t)v;
        else qq_part = fmaf(v, v, qq_part);
    }
    {
        const Acc s = gsum<64>(qq_part);
        if (lane == 0) red[wave] = s;
    }
    for (uint32_t i = tid; i < nr; i += 256) rowbuf[i] = p.cand_rows[(size_t)q * p.m + c0 + i];
    __syncthreads();
    const Acc qq = red[0] + red[1] + red[2] + red[3];

    auto qload = [&](uint32_t v, int half) __attribute__((always_inline)) -> float4 {  // float types: 4 query elements
        if constexpr (QLDS) {
            return *reinterpret_cast<const float4*>(qs + (size_t)v * (EPV * 4) + half * 16);
        } else {
            const uint32_t e = v * EPV + half * 4;
            const float* f = reinterpret_cast<const float*>(src);
            return float4{e < p.dim ? f[e] : 0.0f, e + 1 < p.dim ? f[e + 1] : 0.0f, e + 2 < p.dim ? f[e + 2] : 0.0f,
                          e + 3 < p.dim ? f[e + 3] : 0.0f};
        }
    };

    const uint32_t ngroups = (nr + RPG - 1) / RPG;
    for (uint32_t g0 = (uint32_t)wave * U; g0 < ngroups; g0 += 4 * U) {  // wave-uniform: every lane reaches the shuffles
        uint32_t idx[U];
        bool rv[U];
        const unsigned char* rp[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            idx[u] = (g0 + u) * RPG + rsel;
            rv[u] = idx[u] < nr;
            rp[u] = p.rows + (size_t)(rv[u] ? rowbuf[idx[u]] : 0u) * p.pitch;
        }
        Acc acc[U], xx[U];
#pragma unroll
        for (int u = 0; u < U; u++) acc[u] = 0, xx[u] = 0;
        for (uint32_t j = 0; j < p.J; j++) {
            const uint32_t v = j * G + sub;
            const bool vv = v < p.V;
            k1::u32x4 x[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                x[u] = k1::u32x4{0, 0, 0, 0};
                if (vv && rv[u]) x[u] = __builtin_nontemporal_load(reinterpret_cast<const k1::u32x4*>(rp[u] + (size_t)v * 16));
            }
            if constexpr (DT == MVF_DTYPE_FLOAT32) {
                const float4 qv = qload(v, 0);
#pragma unroll
                for (int u = 0; u < U; u++) {
                    acc[u] = k1::acc4<METRIC>(acc[u], qv, x[u]);
                    if constexpr (NEED_XX) xx[u] = k1::xx4(xx[u], x[u]);
                }
            } else if constexpr (DT == MVF_DTYPE_FLOAT16) {
                const float4 qa = qload(v, 0), qb = qload(v, 1);
#pragma unroll
                for (int u = 0; u < U; u++) {
                    float xf[8];
                    k1::widen_f16(x[u], xf);
                    acc[u] = k1::acc8_f16<METRIC>(acc[u], qa, qb, xf);
                    if constexpr (NEED_XX) xx[u] = k1::xx8_f16(xx[u], xf);
                }
            } else {
                const uint4 qv = *reinterpret_cast<const uint4*>(qs + (size_t)v * 16);
#pragma unroll
                for (int u = 0; u < U; u++) {
                    acc[u] = k1::dot16_int<DT == MVF_DTYPE_INT8>(acc[u], qv, x[u]);
                    if constexpr (NEED_XX) xx[u] = k1::dot16_int<DT == MVF_DTYPE_INT8>(xx[u], uint4{x[u].x, x[u].y, x[u].z, x[u].w}, x[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const Acc s = gsum<G>(acc[u]);
            Acc xxs = 0;
            if constexpr (NEED_XX) xxs = gsum<G>(xx[u]);
            uint32_t key;
            if constexpr (Tr::INT) key = k1::key_int<METRIC>(s, xxs, qq);
            else key = k1::key<METRIC>(s, xxs, qq);
            if (sub == 0 && rv[u]) {
                const uint32_t row = rowbuf[idx[u]];
                if (dout) dout[idx[u]] = rank_entry(key, row, false);
                else buf[idx[u]] = ((uint64_t)key << 32) | row;
            }
        }
    }
    if (!lout) return;
    // ---- the chunk's best min(kcap, nr), sorted
    __syncthreads();
    const uint32_t P = next_pow2(nr < 2 ? 2u : nr);
    for (uint32_t i = nr + tid; i < P; i += 256) buf[i] = kPadComposite;
    __syncthreads();
    bitonic_sort_u64_reg<256, kCandChunk / 256>(buf, P, tid);
    for (uint32_t i = tid; i < p.kcap; i += 256) lout[i] = i < nr ? buf[i] : kPadComposite;
}

template <int DT, int METRIC, bool QLDS>
const void* pick_g(int G) {
    switch (G) {
        case 1: return reinterpret_cast<const void*>(&cand_score_kernel<DT, METRIC, 1, QLDS>);
        case 4: return reinterpret_cast<const void*>(&cand_score_kernel<DT, METRIC, 4, QLDS>);
        case 8: return reinterpret_cast<const void*>(&cand_score_kernel<DT, METRIC, 8, QLDS>);
        case 16: return reinterpret_cast<const void*>(&cand_score_kernel<DT, METRIC, 16, QLDS>);
        case 32: return reinterpret_cast<const void*>(&cand_score_kernel<DT, METRIC, 32, QLDS>);
        case 64: return reinterpret_cast<const void*>(&cand_score_kernel<DT, METRIC, 64, QLDS>);
        default: return nullptr;
    }
}

template <int DT, bool QLDS>
const void* pick_metric(int metric, int G) {
    switch (metric) {
        case MVF_METRIC_L2: return pick_g<DT, MVF_METRIC_L2, QLDS>(G);
        case MVF_METRIC_INNER_PRODUCT: return pick_g<DT, MVF_METRIC_INNER_PRODUCT, QLDS>(G);
        case MVF_METRIC_COSINE: return pick_g<DT, MVF_METRIC_COSINE, QLDS>(G);
        default: return nullptr;
    }
}

}  // namespace

hipError_t cand_prep_launch(const CandPrepParams& p, uint32_t nq, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    if (p.m > kCandLdsSort) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cand_prep_kernel, dim3(nq), dim3(1024), (size_t)next_pow2(p.m < 2 ? 2u : p.m) * 8u, s, p);
    return hipGetLastError();
}

hipError_t cand_map_launch(const CandPrepParams& p, uint32_t nq, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    const uint32_t bx = std::min<uint32_t>((p.m + 255u) / 256u, 1024u);
    hipLaunchKernelGGL(cand_map_kernel, dim3(bx, nq), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t cand_compact_launch(const CandPrepParams& p, const uint64_t* sorted, uint32_t nq, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(cand_compact_kernel, dim3(nq), dim3(1024), 0, s, p, sorted);
    return hipGetLastError();
}

hipError_t cand_score_launch(uint8_t dtype, int metric, int G, const CandScoreParams& p, uint32_t nq, hipStream_t s) {
    if (nq == 0 || p.m == 0) return hipSuccess;
    const uint32_t qbytes = cand_query_bytes(dtype, G, p.J);
    const bool qlds = is_int_dtype(dtype) || qbytes <= kCandQueryLdsMax;
    const void* fn = nullptr;
    switch (dtype) {
        case MVF_DTYPE_FLOAT32: fn = qlds ? pick_metric<MVF_DTYPE_FLOAT32, true>(metric, G) : pick_metric<MVF_DTYPE_FLOAT32, false>(metric, G); break;
        case MVF_DTYPE_FLOAT16: fn = qlds ? pick_metric<MVF_DTYPE_FLOAT16, true>(metric, G) : pick_metric<MVF_DTYPE_FLOAT16, false>(metric, G); break;
        case MVF_DTYPE_INT8: fn = pick_metric<MVF_DTYPE_INT8, true>(metric, G); break;
        case MVF_DTYPE_UINT8: fn = pick_metric<MVF_DTYPE_UINT8, true>(metric, G); break;
        default: break;
    }
    if (!fn) return hipErrorInvalidValue;
    const size_t lds = (size_t)kCandChunk * 12u + 16u + (qlds ? qbytes : 0u);
    const dim3 grid((p.m + kCandChunk - 1) / kCandChunk, nq);
    CandScoreParams arg = p;
    void* args[] = {&arg};
    return hipLaunchKernel(fn, grid, dim3(256), args, lds, s);
}

}  // namespace mvf
