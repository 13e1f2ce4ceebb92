/*
 * mvf_gpu_stream_5p1.h — C ABI of libmvf_gpu.so, continued: diagnostic entry points of the 5+1 layout of the 6-bit shadow
 * ("5+1"; csrc/shadow_5p1.h).  Additions to ABI version 3, outside the versioned structs.
 */
#ifndef MVF_GPU_STREAM_5P1_H
#define MVF_GPU_STREAM_5P1_H

#include "mvf_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * What the handle's newest one-query search over the 6-bit shadow read of the shadow's LOW-BIT planes, in 128-byte lines (eight
 * rows' 16 bytes of one 128-element unit): *out_fetched lines requested out of *out_total lines of the rows scanned, counted per
 * scan block and added up here.  Both 0 where that search read the 6-bit layout (or none ran yet).  Waits for the handle's
 * newest call; a host-side call under the handle's lock, no device work of its own beyond one small copy.
 */
int mvfgpu_debug_stream_lo_lines(const mvfgpu_corpus* corpus, uint64_t* out_fetched, uint64_t* out_total);

/*
 * The 5+1 layout on the host (no GPU needed; csrc/shadow_5p1.h), as mvfgpu_selftest_shadow6_*: the bytes the shadow of `rows` x
 * `dimension` holds; `codes` (rows x dimension values in [-31, 31]) packed into `out` as the build kernel packs them (the
 * bytes behind the last row zero); and the codes read back out of such a shadow.
 */
uint64_t mvfgpu_selftest_shadow51_bytes(uint64_t rows, uint32_t dimension);
int mvfgpu_selftest_shadow51_pack(const int8_t* codes, uint64_t rows, uint32_t dimension, uint8_t* out, uint64_t out_bytes);
int mvfgpu_selftest_shadow51_unpack(const uint8_t* shadow, uint64_t shadow_bytes, uint64_t rows, uint32_t dimension, int8_t* out_codes);

#ifdef __cplusplus
}
#endif

#endif
