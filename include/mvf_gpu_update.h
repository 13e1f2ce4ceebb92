/*
 * mvf_gpu_update.h — C ABI of libmvf_gpu.so, continued: row writes.  New bytes go into positions of a resident corpus, and
 * everything the handle derived from those rows is refreshed for exactly the rows written.  The functions are additions to
 * ABI version 3.
 */
#ifndef MVF_GPU_UPDATE_H
#define MVF_GPU_UPDATE_H

#include "mvf_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mvfgpu_write_report::refreshed */
#define MVFGPU_WRITE_NORMS 1u      /* the row norms */
#define MVFGPU_WRITE_SHADOW_F16 2u /* the scaled-f16 shadow and its scales */
#define MVFGPU_WRITE_SHADOW_I8 4u  /* the int8 shadow and its scales */
#define MVFGPU_WRITE_SHADOW_6B 8u  /* the 6-bit shadow (either layout) and its scales */

typedef struct mvfgpu_write_report {
    uint32_t struct_size;   /* MVFGPU_INIT convention */
    uint32_t launches;      /* kernel launches the call enqueued: W0 and one per refreshed item, whatever the count */
    uint64_t rows_written;
    /* algorithmic: rows_written x (pitch + every refreshed per-row item).  The items: norms 8 bytes (Int8: 4); f16 shadow
     * round16(2 dim) + 4; int8 shadow round16(dim) + 4 -- for the rows a partial shadow covers only --; 6-bit shadow
     * 48 ceil(dim / 64) + 4 (5+1 layout: 96 ceil(dim / 128) + 4). */
    uint64_t bytes_written;
    uint32_t refreshed;     /* bit 0 norms, bit 1 scaled-f16 shadow, bit 2 int8 shadow, bit 3 6-bit shadow (either layout) */
    uint32_t reserved;
} mvfgpu_write_report;

/*
 * Row writes ("Row writes"; section 5 "W0 / W1").  `rows` holds `count` rows in the space's stored type,
 * stride_bytes apart (stride_bytes >= dimension x element size, any alignment on the host); the bytes between two rows are never
 * read into the handle.  Afterwards the handle answers every entry point as a handle created from the changed row array would,
 * with the same tombstones, ids, scan path, tuning and attached objects: the stored rows (pad bytes up to the 16-byte pitch
 * zero), and the per-row items of all derived state that is RESIDENT at the time of the write -- norms, f16 / int8 / 6-bit codes
 * and their scales -- for exactly the rows written.  State that has not been built yet stays unbuilt and is built from the new
 * bytes when first needed.  The corpus-wide maxima (the norm maximum and the shadows' bound maxima) are raised by the written
 * rows and never lowered: a handle that has held an outlier -- or an Inf / NaN row, which sends the shadow routes back to the
 * stored rows -- keeps the wider margin until it is re-created.  That costs time only: results are those of the exact paths.
 *
 * mvfgpu_corpus_write_rows: `indices` as mvfgpu_corpus_gather_rows takes them -- global positions, or vector ids where ids are
 * attached (the first row holding the id).  Returns when the write is complete.
 * mvfgpu_corpus_write_rows_device: global positions in a HOST array (never ids), rows in device memory; asynchronous on
 * hip_stream, no host wait; `positions` may be reused when the call returns, d_rows when the stream reaches the end of the write.
 *
 * Refused before any device work, the handle untouched, in this order: a NULL corpus; NULL indices / rows with count > 0;
 * stride_bytes below a row's bytes (MVF_ERR_INVALID_ARGUMENT); an index outside [index_base, index_base + rows), UINT64_MAX
 * included, or an unknown id (MVF_ERR_INDEX_OUT_OF_BOUNDS); the same row named twice in one call (MVF_ERR_INVALID_ARGUMENT,
 * naming the first repeated position: a parallel scatter has no "last wins").  count == 0: MVF_OK, nothing done.
 *
 * Ordering: a write is ordered like a search -- behind the handle's newest work, and every later call on the handle, on any
 * stream, behind it.  A search enqueued before the write sees none of it, a call enqueued after it all of it.
 * A deleted row may be written; it stays deleted until mvfgpu_corpus_set_tombstones says otherwise.  A write starts no tombstone
 * generation: filters, columns, partitions and the id table describe positions, not values, and stay valid.
 *
 * Not built: growing a handle beyond its rows (create it with spare, tombstoned rows); writing changed rows back into the .mvf
 * file; lowering the maxima; positions in device memory; a shard-set call (write to the shard's own handle).
 */
int mvfgpu_corpus_write_rows(mvfgpu_corpus* corpus, const uint64_t* indices, uint64_t count, const void* rows, uint64_t stride_bytes,
                             mvfgpu_write_report* out_report /* nullable */);
int mvfgpu_corpus_write_rows_device(mvfgpu_corpus* corpus, const uint64_t* positions /* HOST */, uint64_t count, const void* d_rows,
                                    uint64_t stride_bytes, void* hip_stream, mvfgpu_write_report* out_report /* nullable */);

#ifdef __cplusplus
}
#endif
#endif
