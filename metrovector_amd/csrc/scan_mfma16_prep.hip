// scan_mfma16_prep.hip — the inputs of K2 for the narrow types (scan_mfma16_dma.hip, scan_mfma16_pp.hip,
// scan_mfma16_sb.hip): the prepared queries (one f16 plane, int8, or shifted uint8), the row norms of Float16 / Int8 /
// UInt8 rows, and the scaled-f16 shadow of a Float32 corpus.

#include "scan_mfma.h"

#include "mvf_common.h"
#include "row_builders.h"

#include <hip/hip_fp16.h>

#include <cstdlib>

namespace mvf {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---- query preparation ---------------------------------------------------------------
// f16: per query, scale = 2^e with max|q|*2^e in [2^14, 2^15); one plane q~ = f16(q*2^e) (round to nearest).
//      qaux0 = 2^-e, qaux1 = |q| (f32 norm of the ORIGINAL query).
__global__ void prep_queries_f16_kernel(const float* q, uint32_t nq, uint32_t nq_pad, uint32_t dim, uint32_t KPB,
                                        unsigned char* qprep, float* qaux0, float* qaux1) {
    const uint32_t row = blockIdx.x;
    const uint32_t KP = KPB / 2;
    __shared__ float red[8];
    float mx = 0.f, ss = 0.f;
    if (row < nq)
        for (uint32_t c = threadIdx.x; c < dim; c += blockDim.x) {
            const float v = q[(size_t)row * dim + c];
            mx = fmaxf(mx, fabsf(v));
            ss = fmaf(v, v, ss);
        }
    for (int off = 32; off > 0; off >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        ss += __shfl_xor(ss, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = mx;
        red[4 + (threadIdx.x >> 6)] = ss;
    }
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    ss = red[4] + red[5] + red[6] + red[7];
    int e = 0;
    if (mx > 0.f && mx < 3.0e38f) {
        int ex;
        (void)frexpf(mx, &ex);  // mx = m * 2^ex, m in [0.5, 1)
        e = 15 - ex;            // mx * 2^e in [2^14, 2^15)
    }
    const float up = ldexpf(1.0f, e), down = ldexpf(1.0f, -e);
    __half* hi = reinterpret_cast<__half*>(qprep + (size_t)row * KPB);
    for (uint32_t c = threadIdx.x; c < KP; c += blockDim.x) {
        float v = (row < nq && c < dim) ? q[(size_t)row * dim + c] * up : 0.f;
        hi[c] = __float2half_rn(v);
    }
    if (threadIdx.x == 0) {
        qaux0[row] = down;
        qaux1[row] = sqrtf(ss);
    }
}

// i8: zero-padded copy; qaux0 = bit pattern of the i32 sum q^2.
__global__ void prep_queries_i8_kernel(const int8_t* q, uint32_t nq, uint32_t nq_pad, uint32_t dim, uint32_t KPB,
                                       unsigned char* qprep, float* qaux0, float* qaux1) {
    const uint32_t row = blockIdx.x;
    __shared__ int red[4];
    int ss = 0;
    for (uint32_t c = threadIdx.x; c < KPB; c += blockDim.x) {
        const int8_t v = (row < nq && c < dim) ? q[(size_t)row * dim + c] : (int8_t)0;
        reinterpret_cast<int8_t*>(qprep)[(size_t)row * KPB + c] = v;
        ss += (int)v * (int)v;
    }
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    if (threadIdx.x == 0) {
        qaux0[row] = __int_as_float(red[0] + red[1] + red[2] + red[3]);
        qaux1[row] = 0.f;
    }
}

// u8: shifted int8 copy (q ^ 0x80), zero padded in the SIGNED domain; qaux0 = bits of sum q_s^2,
// qaux1 = bits of 128 * sum q_s + 16384 * dim.
__global__ void prep_queries_u8_kernel(const uint8_t* q, uint32_t nq, uint32_t nq_pad, uint32_t dim, uint32_t KPB,
                                       unsigned char* qprep, float* qaux0, float* qaux1) {
    const uint32_t row = blockIdx.x;
    __shared__ int red[8];
    int ss = 0, su = 0;
    for (uint32_t c = threadIdx.x; c < KPB; c += blockDim.x) {
        const int v = (row < nq && c < dim) ? (int)q[(size_t)row * dim + c] - 128 : 0;
        reinterpret_cast<int8_t*>(qprep)[(size_t)row * KPB + c] = (int8_t)v;
        ss += v * v;
        su += v;
    }
    for (int off = 32; off > 0; off >>= 1) {
        ss += __shfl_xor(ss, off, 64);
        su += __shfl_xor(su, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = ss;
        red[4 + (threadIdx.x >> 6)] = su;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        qaux0[row] = __int_as_float(red[0] + red[1] + red[2] + red[3]);
        qaux1[row] = __int_as_float(128 * (red[4] + red[5] + red[6] + red[7]) + 16384 * (int)dim);
    }
}

// ---- K4 for the narrow types: one wave per row (the bodies, and the shadow row's: row_builders.h) ---------------
__global__ void __launch_bounds__(256) row_norms_f16_kernel(const unsigned char* rows, uint32_t n, uint32_t pitch,
                                                             uint32_t V, float* xnorm, float* xx2, float* xxmax) {
    float mx = 0.f;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, nwaves = (gridDim.x * 256u) >> 6;
    for (uint32_t r = wave; r < n; r += nwaves) norms_f16_row(rows, pitch, V, r, lane, xnorm, xx2, mx);
    fold_norm_max(xxmax, lane, mx);
}

// Scaled-f16 SHADOW of a Float32 corpus, used for selection only (api.hip): row r is multiplied by 2^s_r with
// max|x| 2^s_r in [2^14, 2^15) -- nothing overflows f16 and every element keeps 11 significant bits relative to
// itself (elements more than 2^29 below the row's largest fall into the f16 subnormals: absolute error 2^-25, i.e.
// < 2^-39 of the largest) -- and rounded to nearest; xscale[r] = 2^-s_r.  Rows holding Inf keep s_r = 0.
__global__ void __launch_bounds__(256) shadow_f16_kernel(const unsigned char* rows32, uint32_t n, uint32_t pitch32,
                                                          uint32_t dim, unsigned char* rows16, uint32_t pitch16,
                                                          float* xscale) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, nwaves = (gridDim.x * 256u) >> 6;
    for (uint32_t r = wave; r < n; r += nwaves) shadow_f16_row(rows32, pitch32, rows16, pitch16, xscale, r, lane);
}

__global__ void __launch_bounds__(256) row_norms_i8_kernel(const unsigned char* rows, uint32_t n, uint32_t pitch,
                                                            uint32_t V, int32_t* xx) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, nwaves = (gridDim.x * 256u) >> 6;
    for (uint32_t r = wave; r < n; r += nwaves) norms_i8_row(rows, pitch, V, r, lane, xx);
}

// UInt8 rows: xx[r] = sum (x-128)^2, xbias[r] = 128 * sum (x-128), over the row's REAL elements
__global__ void __launch_bounds__(256) row_norms_u8_kernel(const unsigned char* rows, uint32_t n, uint32_t pitch,
                                                            uint32_t V, uint32_t dim, int32_t* xx, int32_t* xbias) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, nwaves = (gridDim.x * 256u) >> 6;
    for (uint32_t r = wave; r < n; r += nwaves) norms_u8_row(rows, pitch, V, dim, r, lane, xx, xbias);
}

}  // namespace

hipError_t launch_prep_queries16(const void* q, int dtype, uint32_t nq, uint32_t nq_pad, uint32_t dim, uint32_t KPB,
                                 unsigned char* qprep, float* qaux0, float* qaux1, hipStream_t s) {
    if (dtype == MVF_DTYPE_FLOAT16)
        hipLaunchKernelGGL(prep_queries_f16_kernel, dim3(nq_pad), dim3(256), 0, s, static_cast<const float*>(q), nq, nq_pad,
                           dim, KPB, qprep, qaux0, qaux1);
    else if (dtype == MVF_DTYPE_UINT8)
        hipLaunchKernelGGL(prep_queries_u8_kernel, dim3(nq_pad), dim3(256), 0, s, static_cast<const uint8_t*>(q), nq, nq_pad,
                           dim, KPB, qprep, qaux0, qaux1);
    else
        hipLaunchKernelGGL(prep_queries_i8_kernel, dim3(nq_pad), dim3(256), 0, s, static_cast<const int8_t*>(q), nq, nq_pad,
                           dim, KPB, qprep, qaux0, qaux1);
    return hipGetLastError();
}

hipError_t launch_shadow_f16(const unsigned char* rows32, uint32_t n, uint32_t pitch32, uint32_t dim, unsigned char* rows16,
                             uint32_t pitch16, float* xscale, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n + 3) / 4, 256u * 16u);
    hipLaunchKernelGGL(shadow_f16_kernel, dim3(blocks), dim3(256), 0, s, rows32, n, pitch32, dim, rows16, pitch16, xscale);
    return hipGetLastError();
}

hipError_t launch_row_norms16(const unsigned char* rows, int dtype, uint32_t n, uint32_t pitch, uint32_t dim, void* out,
                              float* xx2, float* xxmax, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n + 3) / 4, 256u * 8u);
    if (dtype == MVF_DTYPE_FLOAT16)
        hipLaunchKernelGGL(row_norms_f16_kernel, dim3(blocks), dim3(256), 0, s, rows, n, pitch, pitch / 16, static_cast<float*>(out),
                           xx2, xxmax);
    else if (dtype == MVF_DTYPE_UINT8)
        hipLaunchKernelGGL(row_norms_u8_kernel, dim3(blocks), dim3(256), 0, s, rows, n, pitch, pitch / 16, dim,
                           static_cast<int32_t*>(out), reinterpret_cast<int32_t*>(xx2));
    else
        hipLaunchKernelGGL(row_norms_i8_kernel, dim3(blocks), dim3(256), 0, s, rows, n, pitch, pitch / 16, static_cast<int32_t*>(out));
    return hipGetLastError();
}

}  // namespace mvf
