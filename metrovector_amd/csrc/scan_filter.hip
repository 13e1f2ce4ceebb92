// scan_filter.hip — F0 (allow bits -> deny mask + block counts), F1 (the ascending list of admitted rows) and F2 (K1's scores of
// the listed rows for groups of queries) of the filtered search (filter.hip, DESIGN.md §5 "F0 / F1 / F2 — filtered search").
//
// F0 re-bases the caller's bits to local rows -- a word of the mask is a funnel of two adjacent words of the upload, shifted by
// 0 .. 31 -- and combines them with the handle's tombstones: deny = ~allow | tomb, zero at and beyond the last row, which is
// the layout every scan kernel already takes as its deletion bitmap.  A block covers kFilterBlockRows rows and leaves their
// admitted count.  F1 scans those counts and scatters every block's admitted rows in ascending order: a ballot per wave, the
// waves' counts through LDS -- no sort.  F2 gives each chunk of kFilterChunk listed rows and each group of up to kFilterGroup
// queries one block: the queries are staged as K1 stages one (zero padded to J G vectors; sums of squares in K1's order), each
// G-lane group of K1's one-query shape loads a row once (non-temporal 16-byte loads, U = 4 rows in flight per wave) and
// accumulates it against every query of the group with K1's per-row arithmetic (k1_rowscore.h): K1's one-query bits for any
// number of queries.
//
// Algorithmic HBM bytes of F2: the listed rows' pitch once per group of queries (+ 4 bytes per listed row and block).

#include "scan_filter.h"
#include "aux_kernels.h"
#include "bitonic.h"
#include "k1_rowscore.h"
#include "mvf_common.h"
#include "scan_candidates.h"

#include <algorithm>
#include <type_traits>

namespace mvf {
namespace {

// the sum of `v` over the 1024 threads of a block, returned to every thread; wsum: 16 words of LDS
__device__ __forceinline__ uint32_t block_sum_1024(uint32_t v, uint32_t* wsum) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) wsum[wave] = v;
    __syncthreads();
    uint32_t tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < 16; w++) tot += wsum[w];
    return tot;
}

// F0: grid (filter_blocks(n)), block 1024; thread t of block b owns word b * 1024 + t of the mask
__global__ void __launch_bounds__(1024) filter_mask_kernel(FilterMaskParams p) {
    __shared__ uint32_t wsum[16];
    const uint64_t nw = (p.n + 31) / 32;
    const uint64_t w = (uint64_t)blockIdx.x * 1024u + threadIdx.x;
    uint32_t admitted = 0;
    if (w < nw) {
        const uint32_t lo = p.allow[w];
        // (a shift of 0 takes the word as it lies: `hi << 32` is undefined, and the device form's last word has no neighbour)
        const uint32_t allow = p.shift ? (lo >> p.shift) | (p.allow[w + 1] << (32u - p.shift)) : lo;
        const uint64_t left = p.n - w * 32u;
        const uint32_t valid = left >= 32u ? 0xFFFFFFFFu : (1u << (uint32_t)left) - 1u;
        const uint32_t deny = (~allow | (p.tomb ? p.tomb[w] : 0u)) & valid;
        p.deny[w] = deny;
        admitted = (uint32_t)__builtin_popcount(~deny & valid);
    } else if (w == nw) {
        p.deny[w] = 0u;
    }
    const uint32_t tot = block_sum_1024(admitted, wsum);
    if (threadIdx.x == 0) p.block_cnt[blockIdx.x] = tot;
}

// F1, step 1: one block of 1024 threads; block_off[b] = the counts in front of block b, *total = all of them
__global__ void __launch_bounds__(1024) filter_scan_kernel(const uint32_t* block_cnt, uint32_t nb, uint64_t* block_off, uint64_t* total) {
    __shared__ uint64_t wtot[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t per = (nb + 1023u) / 1024u;
    const uint32_t b0 = tid * per, b1 = min(nb, b0 + per);
    uint64_t mine = 0;
    for (uint32_t b = b0; b < b1; b++) mine += block_cnt[b];
    uint64_t incl = mine;  // inclusive scan inside the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t o = __shfl_up(incl, off, 64);
        if ((int)lane >= off) incl += o;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint64_t base = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < 16; w++) {
        base += w < wave ? wtot[w] : 0ull;
        all += wtot[w];
    }
    uint64_t run = base + incl - mine;
    for (uint32_t b = b0; b < b1; b++) {
        block_off[b] = run;
        run += block_cnt[b];
    }
    if (tid == 0) *total = all;
}

// F1, step 2: grid (filter_blocks(n)), block 1024; block b scatters the admitted rows of [b, b + 1) * kFilterBlockRows
__global__ void __launch_bounds__(1024) filter_compact_kernel(const uint32_t* deny, uint64_t n, const uint64_t* block_off, uint32_t* list) {
    __shared__ uint32_t wsum[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint64_t base = block_off[blockIdx.x];
    const uint64_t r0 = (uint64_t)blockIdx.x * kFilterBlockRows;
    for (uint32_t t0 = 0; t0 < kFilterBlockRows; t0 += 1024u) {
        if (r0 + t0 >= n) break;  // block-uniform
        const uint64_t r = r0 + t0 + tid;
        const bool keep = r < n && !((deny[r >> 5] >> (r & 31u)) & 1u);
        const unsigned long long bm = __builtin_amdgcn_ballot_w64(keep);
        if (lane == 0) wsum[wave] = (uint32_t)__builtin_popcountll(bm);
        __syncthreads();
        uint32_t off = 0, tot = 0;
#pragma unroll
        for (uint32_t w = 0; w < 16; w++) {
            const uint32_t c = wsum[w];
            off += w < wave ? c : 0u;
            tot += c;
        }
        if (keep) list[base + off + __builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0u))] = (uint32_t)r;
        base += tot;
        __syncthreads();
    }
}

template <int DT> struct FTraits;
template <> struct FTraits<MVF_DTYPE_FLOAT32> { static constexpr int ES = 4; static constexpr bool INT = false; using Q = float; using Acc = float; };
template <> struct FTraits<MVF_DTYPE_FLOAT16> { static constexpr int ES = 2; static constexpr bool INT = false; using Q = float; using Acc = float; };
template <> struct FTraits<MVF_DTYPE_INT8> { static constexpr int ES = 1; static constexpr bool INT = true; using Q = int8_t; using Acc = int32_t; };
template <> struct FTraits<MVF_DTYPE_UINT8> { static constexpr int ES = 1; static constexpr bool INT = true; using Q = uint8_t; using Acc = int32_t; };

template <int G, typename T>
__device__ __forceinline__ T gsum(T v) {
    if constexpr (std::is_integral<T>::value) return k1::group_sum_i32<G>(v);
    else return k1::group_sum<G>(v);
}

// F2: grid (ceil(m / kFilterChunk), ceil(nq / QG)), block 256; dynamic LDS QG * kFilterChunk * 8 (composites) +
// kFilterChunk * 4 (rows) + QG * 16 (qq partials) (+ QG padded queries when QLDS)
template <int DT, int METRIC, int G, int QG, bool QLDS>
__global__ void __launch_bounds__(256) filter_score_kernel(FilterScoreParams p) {
    using Tr = FTraits<DT>;
    using Acc = typename Tr::Acc;
    using QT = typename Tr::Q;
    constexpr int EPV = 16 / Tr::ES;
    constexpr int RPG = 64 / G;
    constexpr int U = 4;
    constexpr bool NEED_XX = (METRIC == MVF_METRIC_COSINE) || (Tr::INT && METRIC == MVF_METRIC_L2);
    static_assert(QLDS || (!Tr::INT && QG == 1), "only one float query is ever read through the cache");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* buf = reinterpret_cast<uint64_t*>(smem);                                       // [QG][kFilterChunk] composites
    uint32_t* rowbuf = reinterpret_cast<uint32_t*>(smem + QG * kFilterChunk * 8);            // [kFilterChunk] the chunk's rows
    Acc* red = reinterpret_cast<Acc*>(smem + QG * kFilterChunk * 8 + kFilterChunk * 4);      // [QG][4] qq partials
    unsigned char* qs = smem + QG * kFilterChunk * 8 + kFilterChunk * 4 + QG * 16;           // [QG][J G vectors] the queries (QLDS)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane % G, rsel = lane / G;
    const uint32_t q0 = blockIdx.y * QG, c0 = blockIdx.x * kFilterChunk;
    const uint32_t nqg = min((uint32_t)QG, p.nq - q0);   // queries of this group that exist
    const uint32_t nr = min(kFilterChunk, p.m - c0);     // >= 1: the grid covers m

    // ---- the queries: K1's staging loop (zero padded to J G vectors) and sums of squares, one query after the other
    const uint32_t VP = p.J * G;
    const size_t qstride = (size_t)VP * (EPV * sizeof(QT));  // bytes of a padded query in LDS
    const QT* src0 = reinterpret_cast<const QT*>(p.queries) + (size_t)q0 * p.dim;
#pragma unroll
    for (int qi = 0; qi < QG; qi++) {
        const QT* src = src0 + (size_t)qi * p.dim;
        const bool have = (uint32_t)qi < nqg;
        Acc qq_part = 0;
        for (uint32_t e = tid; e < VP * EPV; e += 256) {
            const QT v = (have && e < p.dim) ? src[e] : (QT)0;
            if constexpr (QLDS) reinterpret_cast<QT*>(qs + qi * qstride)[e] = v;
            if constexpr (Tr::INT) qq_part += (int32_t)v * (int32_t)v;
            else qq_part = fmaf(v, v, qq_part);
        }
        const Acc s = gsum<64>(qq_part);
        if (lane == 0) red[qi * 4 + wave] = s;
    }
    for (uint32_t i = tid; i < nr; i += 256) rowbuf[i] = p.list[c0 + i];
    __syncthreads();
    Acc qq[QG];
#pragma unroll
    for (int qi = 0; qi < QG; qi++) qq[qi] = red[qi * 4] + red[qi * 4 + 1] + red[qi * 4 + 2] + red[qi * 4 + 3];

    auto qload = [&](int qi, uint32_t v, int half) __attribute__((always_inline)) -> float4 {  // float types: 4 query elements
        if constexpr (QLDS) {
            return *reinterpret_cast<const float4*>(qs + qi * qstride + (size_t)v * (EPV * 4) + half * 16);
        } else {
            const uint32_t e = v * EPV + half * 4;
            const float* f = reinterpret_cast<const float*>(src0);
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
        Acc acc[QG][U], xx[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            xx[u] = 0;
#pragma unroll
            for (int qi = 0; qi < QG; qi++) acc[qi][u] = 0;
        }
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
#pragma unroll
                for (int u = 0; u < U; u++)
                    if constexpr (NEED_XX) xx[u] = k1::xx4(xx[u], x[u]);
#pragma unroll
                for (int qi = 0; qi < QG; qi++) {
                    const float4 qv = qload(qi, v, 0);
#pragma unroll
                    for (int u = 0; u < U; u++) acc[qi][u] = k1::acc4<METRIC>(acc[qi][u], qv, x[u]);
                }
            } else if constexpr (DT == MVF_DTYPE_FLOAT16) {
#pragma unroll
                for (int u = 0; u < U; u++) {
                    float xf[8];
                    k1::widen_f16(x[u], xf);
                    if constexpr (NEED_XX) xx[u] = k1::xx8_f16(xx[u], xf);
#pragma unroll
                    for (int qi = 0; qi < QG; qi++) {
                        const float4 qa = qload(qi, v, 0), qb = qload(qi, v, 1);
                        acc[qi][u] = k1::acc8_f16<METRIC>(acc[qi][u], qa, qb, xf);
                    }
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; u++)
                    if constexpr (NEED_XX) xx[u] = k1::dot16_int<DT == MVF_DTYPE_INT8>(xx[u], uint4{x[u].x, x[u].y, x[u].z, x[u].w}, x[u]);
#pragma unroll
                for (int qi = 0; qi < QG; qi++) {
                    const uint4 qv = *reinterpret_cast<const uint4*>(qs + qi * qstride + (size_t)v * 16);
#pragma unroll
                    for (int u = 0; u < U; u++) acc[qi][u] = k1::dot16_int<DT == MVF_DTYPE_INT8>(acc[qi][u], qv, x[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            Acc xxs = 0;
            if constexpr (NEED_XX) xxs = gsum<G>(xx[u]);
#pragma unroll
            for (int qi = 0; qi < QG; qi++) {
                const Acc s = gsum<G>(acc[qi][u]);
                uint32_t key;
                if constexpr (Tr::INT) key = k1::key_int<METRIC>(s, xxs, qq[qi]);
                else key = k1::key<METRIC>(s, xxs, qq[qi]);
                if (sub == 0 && rv[u] && (uint32_t)qi < nqg) {
                    const uint32_t row = rowbuf[idx[u]];
                    if (p.dump) p.dump[(size_t)(q0 + qi) * p.m + c0 + idx[u]] = rank_entry(key, row, false);
                    else buf[qi * kFilterChunk + idx[u]] = ((uint64_t)key << 32) | row;
                }
            }
        }
    }
    if (!p.lists) return;
    // ---- per query, the chunk's best min(kcap, nr), sorted
    __syncthreads();
    const uint32_t P = next_pow2(nr < 2 ? 2u : nr);
    for (uint32_t qi = 0; qi < nqg; qi++) {  // block-uniform
        uint64_t* b = buf + qi * kFilterChunk;
        for (uint32_t i = nr + tid; i < P; i += 256) b[i] = kPadComposite;
        __syncthreads();
        bitonic_sort_u64_reg<256, kFilterChunk / 256>(b, P, tid);
        uint64_t* lout = p.lists + ((size_t)(q0 + qi) * gridDim.x + blockIdx.x) * p.kcap;
        for (uint32_t i = tid; i < p.kcap; i += 256) lout[i] = i < nr ? b[i] : kPadComposite;
    }
}

template <int DT, int METRIC, int QG, bool QLDS>
const void* pick_g(int G) {
    switch (G) {
        case 1: return reinterpret_cast<const void*>(&filter_score_kernel<DT, METRIC, 1, QG, QLDS>);
        case 4: return reinterpret_cast<const void*>(&filter_score_kernel<DT, METRIC, 4, QG, QLDS>);
        case 8: return reinterpret_cast<const void*>(&filter_score_kernel<DT, METRIC, 8, QG, QLDS>);
        case 16: return reinterpret_cast<const void*>(&filter_score_kernel<DT, METRIC, 16, QG, QLDS>);
        case 32: return reinterpret_cast<const void*>(&filter_score_kernel<DT, METRIC, 32, QG, QLDS>);
        case 64: return reinterpret_cast<const void*>(&filter_score_kernel<DT, METRIC, 64, QG, QLDS>);
        default: return nullptr;
    }
}

template <int DT, int QG, bool QLDS>
const void* pick_metric(int metric, int G) {
    switch (metric) {
        case MVF_METRIC_L2: return pick_g<DT, MVF_METRIC_L2, QG, QLDS>(G);
        case MVF_METRIC_INNER_PRODUCT: return pick_g<DT, MVF_METRIC_INNER_PRODUCT, QG, QLDS>(G);
        case MVF_METRIC_COSINE: return pick_g<DT, MVF_METRIC_COSINE, QG, QLDS>(G);
        default: return nullptr;
    }
}

template <int DT>
const void* pick_group(int metric, int G, uint32_t qg, bool qlds) {
    if (qg == kFilterGroup) return pick_metric<DT, (int)kFilterGroup, true>(metric, G);
    if constexpr (DT == MVF_DTYPE_FLOAT32 || DT == MVF_DTYPE_FLOAT16) {
        if (!qlds) return pick_metric<DT, 1, false>(metric, G);
    }
    return pick_metric<DT, 1, true>(metric, G);
}

}  // namespace

hipError_t filter_mask_launch(const FilterMaskParams& p, hipStream_t s) {
    hipLaunchKernelGGL(filter_mask_kernel, dim3(filter_blocks(p.n)), dim3(1024), 0, s, p);
    return hipGetLastError();
}

hipError_t filter_scan_launch(const uint32_t* block_cnt, uint32_t nb, uint64_t* block_off, uint64_t* total, hipStream_t s) {
    hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(1024), 0, s, block_cnt, nb, block_off, total);
    return hipGetLastError();
}

hipError_t filter_compact_launch(const uint32_t* deny, uint64_t n, const uint64_t* block_off, uint32_t* list, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(filter_compact_kernel, dim3((uint32_t)((n + kFilterBlockRows - 1) / kFilterBlockRows)), dim3(1024), 0, s, deny, n,
                       block_off, list);
    return hipGetLastError();
}

uint32_t filter_group_queries(uint32_t qbytes) { return (size_t)qbytes * kFilterGroup <= kCandQueryLdsMax ? kFilterGroup : 1u; }

hipError_t filter_score_launch(uint8_t dtype, int metric, int G, const FilterScoreParams& p, hipStream_t s) {
    if (p.nq == 0 || p.m == 0) return hipSuccess;
    const uint32_t qbytes = cand_query_bytes(dtype, G, p.J);
    const uint32_t qg = filter_group_queries(qbytes);
    const bool qlds = qg > 1 || is_int_dtype(dtype) || qbytes <= kCandQueryLdsMax;
    const void* fn = nullptr;
    switch (dtype) {
        case MVF_DTYPE_FLOAT32: fn = pick_group<MVF_DTYPE_FLOAT32>(metric, G, qg, qlds); break;
        case MVF_DTYPE_FLOAT16: fn = pick_group<MVF_DTYPE_FLOAT16>(metric, G, qg, qlds); break;
        case MVF_DTYPE_INT8: fn = pick_group<MVF_DTYPE_INT8>(metric, G, qg, qlds); break;
        case MVF_DTYPE_UINT8: fn = pick_group<MVF_DTYPE_UINT8>(metric, G, qg, qlds); break;
        default: break;
    }
    if (!fn) return hipErrorInvalidValue;
    const size_t lds = (size_t)qg * kFilterChunk * 8u + kFilterChunk * 4u + qg * 16u + (qlds ? (size_t)qg * qbytes : 0u);
    const dim3 grid((p.m + kFilterChunk - 1) / kFilterChunk, (p.nq + qg - 1) / qg);
    FilterScoreParams arg = p;
    void* args[] = {&arg};
    return hipLaunchKernel(fn, grid, dim3(256), args, lds, s);
}

}  // namespace mvf
