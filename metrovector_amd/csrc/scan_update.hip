// scan_update.hip — the kernels of a row write (update.hip; DESIGN.md §3 "Row writes", §5 "W0 / W1").
//
// W0 scatters the caller's rows into the resident row array; W1 refreshes, for the same rows, each derived array that is
// resident: the norms, the scaled-f16 shadow, the int8 shadow, the 6-bit shadow in either layout.  Every kernel is one wave
// per LISTED row (r = list[i], i = wave, wave + nwaves, ...) where the builders of a whole corpus walk a range; the per-row
// bodies are the builders' own (row_builders.h), so a refreshed row holds what an upload of the changed array would have put
// there, bit for bit.  The list holds distinct rows: no two waves write the same byte, and nothing is read-modify-written --
// in the tiled 6-bit layouts a row owns its 16-byte slots of each plane.
// A write is O(count): 2 x pitch bytes of traffic per row for W0 and, per resident item, one read of the row and one write of
// the item.  The launches of a write are at most five whatever the count.

#include "scan_update.h"

#include "mvf_common.h"
#include "row_builders.h"

#include <algorithm>

namespace mvf {
namespace {

// ---- W0 -------------------------------------------------------------------------------------------------------------
// Lane l of the wave makes the 16-byte vectors l, l + 64, ... of the destination row: a 16-byte load where the source row
// starts on a 16-byte boundary and the vector lies inside the row's bytes, byte loads otherwise (a misaligned source, and the
// row's last, partial vector); bytes at and beyond row_bytes are zero.  Every store is one aligned 16-byte vector.
__global__ void __launch_bounds__(256) write_scatter_kernel(const unsigned char* src, uint64_t stride, uint32_t row_bytes,
                                                             const uint32_t* list, uint32_t count, unsigned char* rows, uint32_t pitch) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, nwaves = (gridDim.x * 256u) >> 6;
    const uint32_t V = pitch / 16;
    for (uint32_t i = wave; i < count; i += nwaves) {
        const unsigned char* sp = src + (size_t)i * stride;
        unsigned char* dp = rows + (size_t)list[i] * pitch;
        const bool aligned = (reinterpret_cast<uintptr_t>(sp) & 15u) == 0;  // wave-uniform
        for (uint32_t v = lane; v < V; v += 64) {
            const uint32_t at = v * 16;
            rb_u32x4 x = rb_u32x4{0, 0, 0, 0};
            if (aligned && at + 16 <= row_bytes) {
                x = *reinterpret_cast<const rb_u32x4*>(sp + at);
            } else {
#pragma unroll
                for (uint32_t b = 0; b < 16; b++)
                    if (at + b < row_bytes) x[b >> 2] |= (uint32_t)sp[at + b] << (8 * (b & 3));
            }
            *reinterpret_cast<rb_u32x4*>(dp + at) = x;
        }
    }
}

// ---- W1: the list drivers ---------------------------------------------------------------------------------------------
#define MVF_LIST_WAVES()                                  \
    const uint32_t lane = threadIdx.x & 63;              \
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, nwaves = (gridDim.x * 256u) >> 6

template <int DT>
__global__ void __launch_bounds__(256) refresh_norms_kernel(const unsigned char* rows, uint32_t pitch, uint32_t V, uint32_t dim,
                                                             const uint32_t* list, uint32_t count, void* out, float* xx2, float* xxmax) {
    MVF_LIST_WAVES();
    float mx = 0.f;
    for (uint32_t i = wave; i < count; i += nwaves) {
        const uint32_t r = list[i];
        if (DT == MVF_DTYPE_FLOAT32) norms_f32_row(rows, pitch, V, r, lane, static_cast<float*>(out), xx2, mx);
        else if (DT == MVF_DTYPE_FLOAT16) norms_f16_row(rows, pitch, V, r, lane, static_cast<float*>(out), xx2, mx);
        else if (DT == MVF_DTYPE_UINT8) norms_u8_row(rows, pitch, V, dim, r, lane, static_cast<int32_t*>(out), reinterpret_cast<int32_t*>(xx2));
        else norms_i8_row(rows, pitch, V, r, lane, static_cast<int32_t*>(out));
    }
    if (DT == MVF_DTYPE_FLOAT32 || DT == MVF_DTYPE_FLOAT16) fold_norm_max(xxmax, lane, mx);
}

__global__ void __launch_bounds__(256) refresh_shadow_f16_kernel(const unsigned char* rows32, uint32_t pitch32, const uint32_t* list,
                                                                  uint32_t count, unsigned char* rows16, uint32_t pitch16, float* xscale) {
    MVF_LIST_WAVES();
    for (uint32_t i = wave; i < count; i += nwaves) shadow_f16_row(rows32, pitch32, rows16, pitch16, xscale, list[i], lane);
}

template <int SRC>
__global__ void __launch_bounds__(256) refresh_shadow_i8_kernel(const unsigned char* rows, uint32_t pitch, uint32_t dim,
                                                                 const uint32_t* list, uint32_t count, uint32_t covered,
                                                                 unsigned char* rows8, uint32_t pitch8, float* xscale8, float* stats) {
    MVF_LIST_WAVES();
    ShadowMaxima m;
    for (uint32_t i = wave; i < count; i += nwaves) {
        const uint32_t r = list[i];
        if (r < covered) shadow_i8_row<SRC>(rows, pitch, dim, rows8, pitch8, xscale8, r, lane, m);  // wave-uniform
    }
    fold_shadow_maxima(stats, lane, m);
}

template <bool P51>
__global__ void __launch_bounds__(256) refresh_shadow_6b_kernel(const unsigned char* rows, uint32_t pitch, uint32_t dim,
                                                                 const uint32_t* list, uint32_t count, unsigned char* rows6,
                                                                 float* xscale6, float* stats) {
    MVF_LIST_WAVES();
    ShadowMaxima m;
    for (uint32_t i = wave; i < count; i += nwaves) shadow_6b_row<P51>(rows, pitch, dim, rows6, xscale6, list[i], lane, m);
    fold_shadow_maxima(stats, lane, m);
}

#undef MVF_LIST_WAVES

// four rows per block, at most eight blocks per CU of the part: the range builders' grid
dim3 list_grid(uint32_t count) { return dim3((uint32_t)std::min<uint64_t>(((uint64_t)count + 3) / 4, 256u * 8u)); }

}  // namespace

hipError_t launch_write_scatter(const unsigned char* src, uint64_t stride, uint32_t row_bytes, const uint32_t* list, uint32_t count,
                                unsigned char* rows, uint32_t pitch, hipStream_t s) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(write_scatter_kernel, list_grid(count), dim3(256), 0, s, src, stride, row_bytes, list, count, rows, pitch);
    return hipGetLastError();
}

hipError_t launch_refresh_norms(const unsigned char* rows, int dtype, uint32_t pitch, uint32_t dim, const uint32_t* list, uint32_t count,
                                void* out, float* xx2, float* xxmax, hipStream_t s) {
    if (count == 0) return hipSuccess;
    const dim3 g = list_grid(count);
    const uint32_t V = pitch / 16;
    if (dtype == MVF_DTYPE_FLOAT32)
        hipLaunchKernelGGL(refresh_norms_kernel<MVF_DTYPE_FLOAT32>, g, dim3(256), 0, s, rows, pitch, V, dim, list, count, out, xx2, xxmax);
    else if (dtype == MVF_DTYPE_FLOAT16)
        hipLaunchKernelGGL(refresh_norms_kernel<MVF_DTYPE_FLOAT16>, g, dim3(256), 0, s, rows, pitch, V, dim, list, count, out, xx2, xxmax);
    else if (dtype == MVF_DTYPE_UINT8)
        hipLaunchKernelGGL(refresh_norms_kernel<MVF_DTYPE_UINT8>, g, dim3(256), 0, s, rows, pitch, V, dim, list, count, out, xx2, xxmax);
    else
        hipLaunchKernelGGL(refresh_norms_kernel<MVF_DTYPE_INT8>, g, dim3(256), 0, s, rows, pitch, V, dim, list, count, out, xx2, xxmax);
    return hipGetLastError();
}

hipError_t launch_refresh_shadow_f16(const unsigned char* rows32, uint32_t pitch32, const uint32_t* list, uint32_t count,
                                     unsigned char* rows16, uint32_t pitch16, float* xscale, hipStream_t s) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(refresh_shadow_f16_kernel, list_grid(count), dim3(256), 0, s, rows32, pitch32, list, count, rows16, pitch16, xscale);
    return hipGetLastError();
}

hipError_t launch_refresh_shadow_i8(const unsigned char* rows, int src_dtype, uint32_t pitch, uint32_t dim, const uint32_t* list,
                                    uint32_t count, uint32_t covered, unsigned char* rows8, uint32_t pitch8, float* xscale8, float* stats,
                                    hipStream_t s) {
    if (count == 0) return hipSuccess;
    const dim3 g = list_grid(count);
    if (src_dtype == MVF_DTYPE_FLOAT32)
        hipLaunchKernelGGL(refresh_shadow_i8_kernel<MVF_DTYPE_FLOAT32>, g, dim3(256), 0, s, rows, pitch, dim, list, count, covered, rows8,
                           pitch8, xscale8, stats);
    else
        hipLaunchKernelGGL(refresh_shadow_i8_kernel<MVF_DTYPE_FLOAT16>, g, dim3(256), 0, s, rows, pitch, dim, list, count, covered, rows8,
                           pitch8, xscale8, stats);
    return hipGetLastError();
}

hipError_t launch_refresh_shadow_6b(const unsigned char* rows, uint32_t pitch, uint32_t dim, const uint32_t* list, uint32_t count,
                                    unsigned char* rows6, float* xscale6, float* stats, bool p51, hipStream_t s) {
    if (count == 0) return hipSuccess;
    const dim3 g = list_grid(count);
    if (p51) hipLaunchKernelGGL(refresh_shadow_6b_kernel<true>, g, dim3(256), 0, s, rows, pitch, dim, list, count, rows6, xscale6, stats);
    else hipLaunchKernelGGL(refresh_shadow_6b_kernel<false>, g, dim3(256), 0, s, rows, pitch, dim, list, count, rows6, xscale6, stats);
    return hipGetLastError();
}

}  // namespace mvf
