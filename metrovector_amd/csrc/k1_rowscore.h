// k1_rowscore.h — K1's per-row arithmetic (scan_stream.inc), for the kernels that re-score rows and must return K1's bits:
// R3 (scan_radius.hip: radius_rescore_kernel) and the one-query re-scoring of the int8-shadow stream (scan_mfma.hip:
// rescore_k1_kernel) on Float32 rows, and C1 of the candidate search (scan_candidates.hip) on all four types.  Every
// piece is the order of operations K1 uses on one query:
//   * lane `sub` of a G-lane group owns the 16-B vectors v = j G + sub, j = 0 .. J-1 (J G >= V: the steps past the row's
//     last vector read zeros from the row and the zero-padded query, as K1's do), and accumulates one fmaf per element
//     in x, y, z, w order (L2: the squared difference; IP / Cosine: the product; Cosine also the row's sum of squares);
//   * the G partial sums are combined by the xor butterfly G/2, G/4, .., 1 (K1's reduce-scatter for G >= 4 pairs the
//     partial sums the same way: identical totals);
//   * the query's sum of squares in K1's staging order: thread t of the 256-thread block sums elements t, t + 256, ..
//     by fmaf, each wave's 64 partials meet in the butterfly, the four wave sums are added as ((w0 + w1) + w2) + w3;
//   * the key: L2 sqrt(s), IP s, Cosine s / (sqrt(qq) sqrt(xx)) (0 when the denominator is 0), then key_from_score.
// K1 itself keeps its own copy of these lines (it is the yardstick); tests/test_gpu_stream_i8_default.py,
// tests/test_gpu_radius.py and tests/test_gpu_candidates.py hold the kernels that include this header to K1's bits.
#pragma once

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mvf_common.h"

namespace mvf {
namespace k1 {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

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

template <int G>
__device__ __forceinline__ float group_sum(float v) {
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

// ---- Float16 / Int8 / UInt8 rows (the candidate search C1, scan_candidates.hip): K1's per-row arithmetic of those types, as
// R1 (scan_radius.hip: radius_scan_kernel) restates it.  Float16: every element is widened exactly, the f32 query holds 8
// elements per 16-B vector (32 bytes in LDS) and the fmaf order is element 0 .. 7; the key is key() above.  Int8 / UInt8:
// sdot4 / udot4 in x, y, z, w order -- exact i32, so any order gives the same sums.

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

template <int G>
__device__ __forceinline__ int32_t group_sum_i32(int32_t v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
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

}  // namespace k1
}  // namespace mvf
