// k1_rowscore.h — K1's per-row arithmetic (scan_stream.inc), stated once for every kernel outside K1 that must return K1's
// bits: R1 and R3 of the radius search (scan_radius.hip), the gathered-row kernel of the candidate and filtered searches
// (scan_gather.hip) and the one-query re-scoring of the int8-shadow stream (scan_mfma.hip: rescore_k1_kernel).  Every
// piece is the order of operations K1 uses on one query:
//   * lane `sub` of a G-lane group owns the 16-B vectors v = j G + sub, j = 0 .. J-1 (J G >= V: the steps past the row's
//     last vector read zeros from the row and the zero-padded query, as K1's do), and accumulates one fmaf per element
//     in element order (L2: the squared difference; IP / Cosine: the product; Cosine also the row's sum of squares).
//     Float16 rows are widened exactly and meet 8 f32 query elements per vector (32 bytes of LDS); Int8 / UInt8 rows go
//     through sdot4 / udot4 -- exact i32, so any order gives the same sums (accumulate);
//   * the G partial sums are combined by the xor butterfly G/2, G/4, .., 1 (K1's reduce-scatter for G >= 4 pairs the
//     partial sums the same way: identical totals) (group_sum);
//   * the query's sum of squares in K1's staging order: thread t of the 256-thread block sums elements t, t + 256, ..
//     by fmaf, each wave's 64 partials meet in the butterfly, the four wave sums are added as ((w0 + w1) + w2) + w3
//     (stage_queries; query_qq_wave for a kernel whose waves work alone; R1 and the gathered-row kernel keep the loop
//     written out: the shared form costs some of their instantiations a wave per SIMD);
//   * the key: L2 sqrt(s), IP s, Cosine s / (sqrt(qq) sqrt(xx)) (0 when the denominator is 0), then key_from_score;
//     exact integer sums rank on the i32 itself for L2 and InnerProduct (make_key).
// K1 itself keeps its own copy of these lines (it is the yardstick); tests/test_gpu_stream_i8_default.py,
// tests/test_gpu_radius.py, tests/test_gpu_candidates.py and tests/test_gpu_filtered.py hold the kernels that include this
// header to K1's bits.
#pragma once

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "mvf_common.h"

namespace mvf {
namespace k1 {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// element size of the rows, whether the sums are exact integers, the query's element type and the accumulator
template <int DT> struct Traits;
template <> struct Traits<MVF_DTYPE_FLOAT32> { static constexpr int ES = 4; static constexpr bool INT = false; using Q = float; using Acc = float; };
template <> struct Traits<MVF_DTYPE_FLOAT16> { static constexpr int ES = 2; static constexpr bool INT = false; using Q = float; using Acc = float; };
template <> struct Traits<MVF_DTYPE_INT8> { static constexpr int ES = 1; static constexpr bool INT = true; using Q = int8_t; using Acc = int32_t; };
template <> struct Traits<MVF_DTYPE_UINT8> { static constexpr int ES = 1; static constexpr bool INT = true; using Q = uint8_t; using Acc = int32_t; };

// does the key need the row's sum of squares?
template <int DT, int METRIC>
constexpr bool kNeedXX = METRIC == MVF_METRIC_COSINE || (Traits<DT>::INT && METRIC == MVF_METRIC_L2);

template <int METRIC>
__device__ __forceinline__ float acc4(float acc, float4 qv, u32x4 x) {
    const float x0 = __uint_as_float(x.x), x1 = __uint_as_float(x.y), x2 = __uint_as_float(x.z), x3 = __uint_as_float(x.w);
    if constexpr (METRIC == MVF_METRIC_L2) {
        float t0 = qv.x - x0, t1 = qv.y - x1, t2 = qv.z - x2, t3 = qv.w - x3;
        acc = fmaf(t0, t0, acc);
        acc = fmaf(t1, t1, acc);
        acc = fmaf(t2, t2, acc);
        acc = fmaf(t3, t3, acc);
    } else {
        acc = fmaf(qv.x, x0, acc);
        acc = fmaf(qv.y, x1, acc);
        acc = fmaf(qv.z, x2, acc);
        acc = fmaf(qv.w, x3, acc);
    }
    return acc;
}

__device__ __forceinline__ float xx4(float xx, u32x4 x) {
    const float x0 = __uint_as_float(x.x), x1 = __uint_as_float(x.y), x2 = __uint_as_float(x.z), x3 = __uint_as_float(x.w);
    xx = fmaf(x0, x0, xx);
    xx = fmaf(x1, x1, xx);
    xx = fmaf(x2, x2, xx);
    xx = fmaf(x3, x3, xx);
    return xx;
}

template <int G, typename T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int METRIC>
__device__ __forceinline__ uint32_t key(float s, float xxs, float qq) {
    float sc;
    if constexpr (METRIC == MVF_METRIC_L2) sc = sqrtf(s);
    else if constexpr (METRIC == MVF_METRIC_INNER_PRODUCT) sc = s;
    else {
        const float den = sqrtf(qq) * sqrtf(xxs);
        sc = den > 0.0f ? s / den : 0.0f;
    }
    return key_from_score(sc, METRIC);
}

// The four wave sums of the query's sum of squares (K1's staging order), computed by ONE wave: lane l stands in for
// thread w 64 + l of each of the four waves.  Every lane returns ((w0 + w1) + w2) + w3.
__device__ __forceinline__ float query_qq_wave(const float* q, uint32_t dim, int lane) {
    float part[4];
#pragma unroll
    for (int w = 0; w < 4; w++) {
        part[w] = 0.0f;
        for (uint32_t e = (uint32_t)(w * 64 + lane); e < dim; e += 256) part[w] = fmaf(q[e], q[e], part[w]);
        part[w] = group_sum<64>(part[w]);
    }
    return part[0] + part[1] + part[2] + part[3];
}

__device__ __forceinline__ void widen_f16(u32x4 x, float xf[8]) {
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        xf[2 * i] = __half2float(__ushort_as_half((unsigned short)(w[i] & 0xFFFFu)));
        xf[2 * i + 1] = __half2float(__ushort_as_half((unsigned short)(w[i] >> 16)));
    }
}

template <int METRIC>
__device__ __forceinline__ float acc8_f16(float acc, float4 qa, float4 qb, const float xf[8]) {
    const float qf[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if constexpr (METRIC == MVF_METRIC_L2) {
            float t = qf[i] - xf[i];
            acc = fmaf(t, t, acc);
        } else {
            acc = fmaf(qf[i], xf[i], acc);
        }
    }
    return acc;
}

__device__ __forceinline__ float xx8_f16(float xx, const float xf[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) xx = fmaf(xf[i], xf[i], xx);
    return xx;
}

template <bool SIGNED>
__device__ __forceinline__ int32_t dot16_int(int32_t acc, uint4 a, u32x4 b) {
    if constexpr (SIGNED) {
        acc = __builtin_amdgcn_sdot4((int)a.x, (int)b.x, acc, false);
        acc = __builtin_amdgcn_sdot4((int)a.y, (int)b.y, acc, false);
        acc = __builtin_amdgcn_sdot4((int)a.z, (int)b.z, acc, false);
        acc = __builtin_amdgcn_sdot4((int)a.w, (int)b.w, acc, false);
    } else {
        acc = (int32_t)__builtin_amdgcn_udot4(a.x, b.x, (uint32_t)acc, false);
        acc = (int32_t)__builtin_amdgcn_udot4(a.y, b.y, (uint32_t)acc, false);
        acc = (int32_t)__builtin_amdgcn_udot4(a.z, b.z, (uint32_t)acc, false);
        acc = (int32_t)__builtin_amdgcn_udot4(a.w, b.w, (uint32_t)acc, false);
    }
    return acc;
}

// K1's key of exact integer sums: L2 and InnerProduct on the i32 itself, Cosine on the float score
template <int METRIC>
__device__ __forceinline__ uint32_t key_int(int32_t s, int32_t xxs, int32_t qq) {
    if constexpr (METRIC == MVF_METRIC_L2) return key_from_raw(qq + xxs - 2 * s, METRIC);
    else if constexpr (METRIC == MVF_METRIC_INNER_PRODUCT) return key_from_raw(s, METRIC);
    else {
        const float den = sqrtf((float)qq) * sqrtf((float)xxs);
        return key_from_score(den > 0.0f ? (float)s / den : 0.0f, METRIC);
    }
}

template <int DT, int METRIC>
__device__ __forceinline__ uint32_t make_key(typename Traits<DT>::Acc s, typename Traits<DT>::Acc xxs, typename Traits<DT>::Acc qq) {
    if constexpr (Traits<DT>::INT) return key_int<METRIC>(s, xxs, qq);
    else return key<METRIC>(s, xxs, qq);
}

// Four elements e .. e + 3 of a float query read where it lies (no LDS copy), zero beyond the dimension as the padded copy.
__device__ __forceinline__ float4 query_global4(const float* f, uint32_t dim, uint32_t e) {
    return float4{e < dim ? f[e] : 0.0f, e + 1 < dim ? f[e + 1] : 0.0f, e + 2 < dim ? f[e + 2] : 0.0f, e + 3 < dim ? f[e + 3] : 0.0f};
}

// K1's staging of NQ queries by a block of 256 threads, one query after the other: src[q]'s `dim` elements (NULL: a query
// of zeros), zero padded to `nelem` (J G vectors), go to qs + q qstride when STORE, and qq[q] receives the sum of squares.
// red: NQ x 4 accumulators of LDS.  Holds a __syncthreads(): the copies and whatever the caller wrote to LDS before are
// visible after it.
template <int DT, int NQ, bool STORE>
__device__ __forceinline__ void stage_queries(const typename Traits<DT>::Q* const* src, uint32_t dim, uint32_t nelem, unsigned char* qs,
                                              size_t qstride, typename Traits<DT>::Acc* red, typename Traits<DT>::Acc (&qq)[NQ]) {
    using QT = typename Traits<DT>::Q;
    using Acc = typename Traits<DT>::Acc;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        Acc part = 0;
        for (uint32_t e = tid; e < nelem; e += 256) {
            const QT v = (src[q] && e < dim) ? src[q][e] : (QT)0;
            if constexpr (STORE) reinterpret_cast<QT*>(qs + q * qstride)[e] = v;
            if constexpr (Traits<DT>::INT) part += (int32_t)v * (int32_t)v;
            else part = fmaf(v, v, part);
        }
        const Acc s = group_sum<64>(part);
        if (lane == 0) red[q * 4 + wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; q++) qq[q] = red[q * 4] + red[q * 4 + 1] + red[q * 4 + 2] + red[q * 4 + 3];
}

// One 16-byte step of U rows against NQ queries: x[u] is lane `sub`'s vector of row u (zeros past the row's end or for a
// missing row), qload(q, half) the matching query elements -- a float4 (Float16: half 0 and 1, the vector's 8 elements) or
// the uint4 of 16 packed integers.  acc[q][u] and, where the key needs it, xx[u] advance in K1's order.
template <int DT, int METRIC, int U, int NQ, class QLoad>
__device__ __forceinline__ void accumulate(typename Traits<DT>::Acc (&acc)[NQ][U], typename Traits<DT>::Acc (&xx)[U], const u32x4 (&x)[U],
                                           QLoad qload) {
    constexpr bool NEED_XX = kNeedXX<DT, METRIC>;
    if constexpr (DT == MVF_DTYPE_FLOAT32) {
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const float4 qv = qload(q, 0);
#pragma unroll
            for (int u = 0; u < U; u++) acc[q][u] = acc4<METRIC>(acc[q][u], qv, x[u]);
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            if constexpr (NEED_XX) xx[u] = xx4(xx[u], x[u]);
    } else if constexpr (DT == MVF_DTYPE_FLOAT16) {
        float xf[U][8];
#pragma unroll
        for (int u = 0; u < U; u++) widen_f16(x[u], xf[u]);
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const float4 qa = qload(q, 0), qb = qload(q, 1);
#pragma unroll
            for (int u = 0; u < U; u++) acc[q][u] = acc8_f16<METRIC>(acc[q][u], qa, qb, xf[u]);
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            if constexpr (NEED_XX) xx[u] = xx8_f16(xx[u], xf[u]);
    } else {
        constexpr bool S = DT == MVF_DTYPE_INT8;
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const uint4 qv = qload(q, 0);
#pragma unroll
            for (int u = 0; u < U; u++) acc[q][u] = dot16_int<S>(acc[q][u], qv, x[u]);
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            if constexpr (NEED_XX) xx[u] = dot16_int<S>(xx[u], uint4{x[u].x, x[u].y, x[u].z, x[u].w}, x[u]);
    }
}

// The kernel instantiated for a lane-group width / a metric known at run time: f receives std::integral_constant<int, G>
// (or <int, METRIC>) and returns the kernel's address; NULL for a value that has no kernel.
template <class F>
const void* for_group(int G, F f) {
    switch (G) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 8: return f(std::integral_constant<int, 8>{});
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        default: return nullptr;
    }
}

template <class F>
const void* for_metric(int metric, F f) {
    switch (metric) {
        case MVF_METRIC_L2: return f(std::integral_constant<int, MVF_METRIC_L2>{});
        case MVF_METRIC_INNER_PRODUCT: return f(std::integral_constant<int, MVF_METRIC_INNER_PRODUCT>{});
        case MVF_METRIC_COSINE: return f(std::integral_constant<int, MVF_METRIC_COSINE>{});
        default: return nullptr;
    }
}

}  // namespace k1
}  // namespace mvf
