// scan_update.h — the kernels of a row write (scan_update.hip; DESIGN.md §5 "W0 / W1"), launched by update.hip.
// `list` holds `count` DISTINCT local rows below the corpus' row count (update.hip refuses anything else before any device
// work); every launch is one wave per listed row, and none writes outside the listed rows' own bytes.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mvf {

// W0: row i of the source (count rows of row_bytes at `stride`, any alignment) into rows + list[i] * pitch, the tail of the
// pitch zero-filled.  The bytes between two source rows are not read.
hipError_t launch_write_scatter(const unsigned char* src, uint64_t stride, uint32_t row_bytes, const uint32_t* list, uint32_t count,
                                unsigned char* rows, uint32_t pitch, hipStream_t s);
// W1: the per-row items of one derived array for the listed rows, by row_builders.h's bodies -- the range builders' own -- and
// the corpus-wide maxima folded with the same atomicMax.
// the norms: `out`, xx2, xxmax as launch_row_norms_f32 / launch_row_norms16 take them
hipError_t launch_refresh_norms(const unsigned char* rows, int dtype, uint32_t pitch, uint32_t dim, const uint32_t* list, uint32_t count,
                                void* out, float* xx2, float* xxmax, hipStream_t s);
hipError_t launch_refresh_shadow_f16(const unsigned char* rows32, uint32_t pitch32, const uint32_t* list, uint32_t count,
                                     unsigned char* rows16, uint32_t pitch16, float* xscale, hipStream_t s);
// rows at or beyond `covered` have no int8 shadow (a partial shadow) and are skipped
hipError_t launch_refresh_shadow_i8(const unsigned char* rows, int src_dtype, uint32_t pitch, uint32_t dim, const uint32_t* list,
                                    uint32_t count, uint32_t covered, unsigned char* rows8, uint32_t pitch8, float* xscale8, float* stats,
                                    hipStream_t s);
hipError_t launch_refresh_shadow_6b(const unsigned char* rows, uint32_t pitch, uint32_t dim, const uint32_t* list, uint32_t count,
                                    unsigned char* rows6, float* xscale6, float* stats, bool p51, hipStream_t s);

}  // namespace mvf
