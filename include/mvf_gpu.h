/*
 * mvf_gpu.h — C ABI of libmvf_gpu.so: MI355X (gfx950) brute-force top-k
 * similarity search over one MVF vector space.
 *
 * WHAT IT REPLACES.  The reference has no FFI for this path; the scan is the
 * inline loop `find_top_k_similar` (reference examples/similarity_search.rs:
 * 140-176): per row VectorSpace::get_vector (src/vectors/vector_space.rs:
 * 101-142) -> Vector::as_f32 (src/vectors/vector.rs:71-92) -> scalar distance
 * (similarity_search.rs:152-157) -> BinaryHeap (:159-168) -> sort (:172-173).
 * This library replaces that whole loop.  The hand-off is what
 * VectorSpace::map_vector_range(0, total) (vector_space.rs:155-188) +
 * VectorSlice::as_ptr (src/vectors/mem.rs:75-77) already expose: base
 * pointer, row stride, row count, DataType; plus dimension()/distance_metric().
 * INTEGRATION.md shows the Rust `extern "C"` block a maintainer would add.
 *
 * CONVENTIONS
 *  - every call returns enum mvf_status (mvf_status.h), 0 = OK; a thread-local
 *    detail string is kept for the last failure (mvfgpu_last_error_message).
 *  - dtype / metric arguments use the schema's codes (schema/types.fbs).
 *  - a corpus handle is one ROW-RANGE SHARD resident on ONE GPU; it is
 *    immutable after creation, owned by the library, freed by
 *    mvfgpu_corpus_destroy.  Multi-GPU = one handle per GPU (one process per
 *    GPU under torch.distributed/RCCL, or several handles in one process) and
 *    a merge of the per-shard results (mvfgpu_merge_topk_*).
 *  - searches on one handle may be issued from several threads; they are
 *    serialised on the handle's scratch space internally.
 *  - there is NO CPU fallback: without a gfx950 device every compute entry
 *    point returns MVF_ERR_DEVICE.
 *
 * SEMANTICS (the reference only pins L2 over f32/f16)
 *  - L2: sqrt(sum (q-x)^2), k smallest.  InnerProduct: sum q*x, k largest.
 *    Cosine: dot/(|q||x|), 0 when a norm is 0, k largest.
 *  - Float32/Float16 spaces take f32 queries (f16 widened exactly, as
 *    Vector::as_f32).  Int8/UInt8 spaces take queries of the space's own
 *    dtype; sums are exact i32 (dimension <= 33025), bit-exact vs the CPU.
 *  - results are sorted best-first, ties by ascending row index, NaN last;
 *    when k > rows the tail is padded with index UINT64_MAX and score
 *    +inf (L2) / -inf (InnerProduct, Cosine).
 */
#ifndef MVF_GPU_H
#define MVF_GPU_H

#include <stddef.h>
#include <string.h>
#include <stdint.h>

#include "mvf_status.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mvfgpu_corpus mvfgpu_corpus;

#define MVFGPU_MAX_K 0x80000000u  /* largest k a search accepts (the reference takes any usize, similarity_search.rs:143);
                                     entries beyond the shard's live rows are the padding result */
#define MVFGPU_K_PER_PASS 1024u   /* results one pass over the rows selects.  Beyond it a search either runs ceil(k / 1024)
                                     passes of the streaming kernel per 1..4 queries, each returning the rows ranked strictly
                                     behind the last one of the pass before, or -- when that is cheaper, and always beyond
                                     MVFGPU_K_BY_PASSES -- has the streaming kernel write every row's order key (8 bytes per
                                     row) and ranks the WHOLE shard with a device-wide sort (16 bytes of scratch per row and
                                     query of a pass).  Both exact, whatever the batch size, no host wait */
#define MVFGPU_K_BY_PASSES 16384u /* largest k the pass formulation serves (the fallback when the sort's scratch does not fit) */
#define MVFGPU_MAX_INT_DIM 33025u /* d*255^2 < 2^31 */

/*
 * OUT-STRUCTS GROW.  Every struct a getter fills starts with `struct_size`: the CALLER sets it to sizeof(its struct)
 * before the call, the library writes at most that many bytes (fields a newer library knows and the caller does not are
 * dropped; fields a newer caller knows and an older library does not stay as the caller initialised them) and stores
 * the number of bytes it filled back into struct_size.  struct_size < 8 -> MVF_ERR_INVALID_ARGUMENT ("struct_size not
 * set").  MVFGPU_INIT(s) zeroes a struct and sets the field.
 */
#define MVFGPU_INIT(s) (memset(&(s), 0, sizeof(s)), (s).struct_size = (uint32_t)sizeof(s))

typedef struct mvfgpu_corpus_info {
    uint32_t struct_size; /* in: sizeof(mvfgpu_corpus_info); out: bytes filled */
    int32_t device;
    uint64_t rows;        /* rows in this shard */
    uint64_t index_base;  /* global index of the shard's first row */
    uint32_t dimension;
    uint32_t pitch_bytes; /* device row pitch: dimension*elem_size rounded up to 16 */
    uint8_t data_type;    /* enum mvf_data_type */
    uint8_t has_vector_ids; /* 1 when vector ids are attached (searches then report ids, not positions) */
    uint8_t shadows;      /* bit 0: the int8 selection shadow is resident (all rows), bit 1: the scaled-f16 one, bit 2: an int8
                             shadow of a PREFIX of the rows (all rows did not fit: batched searches run as two row ranges),
                             bit 3: the 6-bit selection shadow of a Float32 corpus is resident (one streamed query) */
    uint8_t selection_state; /* bit 0: the repair feedback has switched the int8-shadow selection off for this corpus,
                                bit 1: it has switched the folded pre-filter of the int8 kernels off,
                                bit 2: it has sent one-query searches from the 6-bit shadow back to the int8 shadow */
    uint32_t reserved2;
    uint64_t device_bytes; /* HBM held by the handle: rows, deletion bitmap, ids, norms, every scratch buffer and the
                              selection shadows (int8: +dimension bytes per row; scaled f16: +2*dimension; 6-bit: +0.75*dimension) with their
                              per-row scales and bound statistics, once built */
    uint64_t deleted_rows; /* rows masked by the tombstone bitmap */
} mvfgpu_corpus_info;

typedef struct mvfgpu_timing {
    uint32_t struct_size; /* in: sizeof(mvfgpu_timing); out: bytes filled */
    uint32_t samples;    /* searches averaged */
    /* Device times of searches on the handle, milliseconds, taken (never waited for) while
     * mvfgpu_set_profiling(corpus, 1) is in effect; mvfgpu_last_timing waits for the newest search and reads them back.
     * The streaming routes (scan_kernel 1, 5, 7) time themselves: block 0 of the scan stores the device's wall clock
     * (hipDeviceAttributeWallClockRate) at its start and every block folds it at its end into a per-handle ring, the select behind it adds its own
     * end, and -- scan_kernel 1 and 7 -- the search's last kernel the end of the search.  scan_ms is then block 0
     * started (the first block dispatched, by the dispatcher's habit, not by guarantee) -> last block finished, without the dispatch latency an event pair around the launch includes, and
     * search_ms starts with the first kernel of the search.  The batched routes (and the whole-search time of
     * scan_kernel 5 and 8) are HIP events recorded on the search's own stream. */
    float scan_ms;     /* newest search: the dominant kernel (streaming or MFMA scan) */
    float select_ms;   /* newest search: candidate select / top-k kernels */
    float total_ms;    /* newest search: scan_ms + select_ms */
    float scan_ms_avg;   /* mean over the (up to 64) newest profiled searches */
    float select_ms_avg;
    uint32_t scan_kernel; /* 1 = streaming (K1) on the stored rows, 5 = K1 on the f16 shadow of a Float32
                             corpus (scan path 4); MFMA batched (K2): 2 = f32 kernel on Float32 rows,
                             3 = f16/int8 kernel on the stored rows, 4 = f16 kernel on the f16 shadow,
                             6 = int8 kernel on the int8 shadow of a Float32 / Float16 corpus (scan path 5);
                             7 = K1 on a selection shadow, int8 or 6-bit (scan paths 6 and 7; one query on path 0 once
                             the shadow exists) -- scan_bytes tells the two apart: rows * dimension on the int8 shadow,
                             ceil(rows / 64) * ceil(dimension / 64) * 3072 on the 6-bit one;
                             8 = K1 writing every row's order key + the whole-shard sort (k > MVFGPU_K_PER_PASS) */
    uint32_t scan_launches; /* scan launches of one search (timing covers the first) */
    uint64_t scan_bytes; /* algorithmic bytes one scan launch reads */
    uint64_t scan_flops; /* algorithmic flops of one scan launch (2*nq*rows*dim) */
    /* the WHOLE search on the device: first to last kernel of the call on its stream (query preparation, every scan
     * phase, compactions, re-scoring, the repair launches) */
    float search_ms;      /* newest search */
    float search_ms_avg;  /* mean over the profiled searches */
    uint64_t search_flops; /* 2 * nq * rows * dim of the whole search */
    uint32_t repaired_queries; /* newest BATCHED search (whether profiled or not): queries whose candidate budget or region
                                  overflowed and that the streaming kernel re-did exactly (0 on sane data; a corpus that
                                  keeps producing them goes back to the slower selection paths by itself) */
    uint32_t search_launches; /* newest search (whether profiled or not): kernel launches it enqueued, counted on the host,
                                 on the routes that count them -- the streaming kernel on the stored rows (2: scan + select)
                                 or on a selection shadow (scan_kernel 7: scan, margin select, re-scoring, final select,
                                 the repair pair); 0 = the route does not count (batched searches, scan path 4,
                                 k > MVFGPU_K_PER_PASS).  (`reserved` until round 7.) */
} mvfgpu_timing;

/* ---- library / device ---------------------------------------------------- */

/* Number of visible GPUs (0 and MVF_OK when there is none). */
int mvfgpu_device_count(int* out_count);
const char* mvfgpu_strerror(int status);
/* Detail of the calling thread's last failure ("" if none). */
const char* mvfgpu_last_error_message(void);

/* ---- corpus -------------------------------------------------------------- */

/*
 * Upload `n` rows to HBM on `device`.
 *   rows         : host pointer, any alignment (an mmap'd MVF block starts at
 *                  file offset 4 — src/builder.rs:421); BORROWED for the call
 *                  only, the mapping may be dropped afterwards.
 *   stride_bytes : bytes between consecutive rows; must be >= dimension *
 *                  elem_size.  The reference always passes dimension*elem_size
 *                  (VectorSlice stride, vector_space.rs:177,187).
 *   index_base   : added to every returned index (global row of rows[0]); 0
 *                  for an unsharded space.
 * Errors: MVF_ERR_BUILD for a data type other than Float32/Float16/Int8/UInt8
 * ("Unsupported vector data type", vector_space.rs:126); MVF_ERR_INVALID_
 * ARGUMENT for dimension 0, NULL rows with n > 0, n > 2^32-65536 rows per shard;
 * MVF_ERR_DEVICE for HIP failures (incl. out of memory).
 */
int mvfgpu_corpus_create(const void* rows, uint64_t n, uint32_t dimension,
                         uint8_t data_type, uint64_t stride_bytes, int device,
                         uint64_t index_base, mvfgpu_corpus** out);

/*
 * The same upload with options (NULL = the defaults of mvfgpu_corpus_create).  The upload is a two-stream pipeline
 * (DESIGN.md §6): chunks of `chunk_mib` MiB (0 = 256) cross PCIe on one stream while the other re-pitches the chunk
 * before (rows whose size is not a multiple of 16 bytes, or that lie further apart than their size) and, on request,
 * computes what the first BATCHED search would otherwise build -- the row norms, and for Float32 / Float16 spaces the
 * int8 shadow used for candidate selection (+25 % / +50 % device memory; skipped silently when that would leave < 2 GiB
 * free).
 * Checksum validation of the block (the reference leaves it `todo!()`, src/reader.rs:220) lives in libmvf_host
 * (mvf_reader_validate_with_checksum): run it on another thread beside this call.
 */
typedef struct mvfgpu_upload_options {
    uint32_t struct_size; /* sizeof(mvfgpu_upload_options): lets the struct grow */
    uint32_t flags;       /* MVFGPU_UPLOAD_* */
    uint32_t chunk_mib;   /* chunk size in MiB, 0 = default (64 with pinned staging, else 256) */
    uint32_t reserved;
} mvfgpu_upload_options;
#define MVFGPU_UPLOAD_EAGER_NORMS 1u    /* row norms (K4) per chunk, beside the copy of the next */
#define MVFGPU_UPLOAD_EAGER_SHADOW 2u   /* Float32 / Float16 spaces: norms + the selection shadow batched searches use, per
                                           chunk: the INT8 shadow (+dimension bytes per row; the default selection), or
                                           the scaled-f16 one of a Float32 space when MVF_I8_SHADOW=0 */
#define MVFGPU_UPLOAD_PINNED_STAGING 4u /* double-buffer through two pinned host chunks filled by memcpy threads: the default
                                           for uploads of >= 256 MiB (50 GB/s measured against 10-21 GB/s for the
                                           pageable source handed to the runtime); this flag forces it for small ones */
#define MVFGPU_UPLOAD_PAGEABLE 8u       /* never stage: hand the (pageable / mmap'd) source to the runtime as it is */
int mvfgpu_corpus_create_ex(const void* rows, uint64_t n, uint32_t dimension,
                            uint8_t data_type, uint64_t stride_bytes, int device,
                            uint64_t index_base, const mvfgpu_upload_options* options,
                            mvfgpu_corpus** out);

/*
 * Generate rows [row0, row0+n) of the synthetic corpus on the device
 * (counter-based: element (r,c) = f(seed, r*dimension + c), DESIGN.md §6 —
 * the CPU oracle regenerates any row).  index_base = row0.
 */
int mvfgpu_corpus_create_synthetic(uint64_t n, uint32_t dimension,
                                   uint8_t data_type, uint64_t seed,
                                   uint64_t row0, int device,
                                   mvfgpu_corpus** out);

void mvfgpu_corpus_destroy(mvfgpu_corpus* corpus);
int mvfgpu_corpus_get_info(const mvfgpu_corpus* corpus, mvfgpu_corpus_info* out);

/* Copy `count` rows starting at local row `first` back to the host, tightly
 * packed (dimension*elem_size per row) — the device-side get_vector
 * (vector_space.rs:101-142); MVF_ERR_INDEX_OUT_OF_BOUNDS past the end. */
int mvfgpu_corpus_read_rows(const mvfgpu_corpus* corpus, uint64_t first,
                            uint64_t count, void* out_rows);

/* Gather arbitrary rows by GLOBAL index (as returned by a search) from HBM, tightly packed, in the order given:
 * the payload of the reference's ScoredVector.vector (examples/similarity_search.rs:18,:159-163) without touching
 * the file again.  Indices of UINT64_MAX (padding of a short result list) give zero rows; any other index outside
 * [index_base, index_base + rows) -> MVF_ERR_INDEX_OUT_OF_BOUNDS. */
int mvfgpu_corpus_gather_rows(const mvfgpu_corpus* corpus, const uint64_t* indices,
                              uint64_t count, void* out_rows);

/*
 * Deletions and vector ids (schema/core.fbs:35-39 TombstoneInfo, :54 vector_ids_block_index, :56 tombstones).  The
 * reference neither writes nor honours them (src/builder.rs:483-485), so the semantics are this library's:
 *   - tombstones: bit (first_bit + r) of `bitmap` (bit b of a byte array = byte b >> 3, bit b & 7) set = the shard's
 *     LOCAL row r is deleted; `nbits` = bits the array holds, >= first_bit + rows.  A deleted row is never returned: the
 *     streaming kernel tests the bit where a row would enter a candidate list, the MFMA kernels where a candidate is
 *     appended.  libmvf_host's mvf_space_tombstone_bitmap produces the bitmap from either on-disk format; pass the
 *     whole space's bitmap with first_bit = the shard's first row.  NULL / 0 removes the mask.
 *   - vector ids: one u64 (little endian, any alignment) per LOCAL row; searches then report ids[row] instead of
 *     index_base + row (ties still break by row position, then -- across shards -- by shard order), and
 *     mvfgpu_corpus_gather_rows accepts the reported ids.  NULL / 0 removes them.
 * Both calls wait for the device to go idle; like create / destroy they must not race with searches on the handle.
 */
int mvfgpu_corpus_set_tombstones(mvfgpu_corpus* corpus, const uint8_t* bitmap,
                                 uint64_t first_bit, uint64_t nbits);
int mvfgpu_corpus_set_vector_ids(mvfgpu_corpus* corpus, const void* ids_le, uint64_t n);

/* ---- search -------------------------------------------------------------- */

/*
 * Replaces find_top_k_similar (similarity_search.rs:140-176) for a batch.
 *   queries    : host, row-major [nq][dimension], contiguous; query_dtype
 *                must be Float32 for Float32/Float16 spaces and the space's
 *                dtype for Int8/UInt8 spaces (else MVF_ERR_BUILD).
 *   query_dim  : length of each query; != corpus dimension ->
 *                MVF_ERR_DIMENSION_MISMATCH (the reference's zip silently
 *                truncates, similarity_search.rs:154; we refuse).
 *   out_scores : host [nq][k] f32, out_indices: host [nq][k] u64 (the
 *                reference's ScoredVector.index is u64, :16), both
 *                caller-owned.  out_raw (nullable): [nq][k] exact i32 of
 *                L2 (sum of squared differences) / InnerProduct for Int8/UInt8
 *                spaces, 0 otherwise.
 * Blocking: returns after the results are on the host.  Small transfers (queries <= 64 KiB, results <= 256 KiB) use no
 * copy engine: the kernels read the query from and write the results into pinned host memory of the handle, the CPU
 * copies to / from the caller's (pageable) buffers -- one query on 10k x 128 f32: 61 -> 33 us per call
 * (profiles/r04_host_api_latency.txt).  MVF_HOST_ZC_QUERY / MVF_HOST_ZC_RESULTS (bytes; 0 = always copy) move the limits.
 * Such a call (results in place, no payload) does not wait on its stream either: the final select stores a sequence number into
 * pinned host memory behind its results and the call spins on that word (up to 300 us, then the stream) -- the host learns of a
 * finished kernel ~5 us sooner that way (profiles/r04_flag_wait.txt; MVF_HOST_FLAG_WAIT=0 waits on the stream).
 */
int mvfgpu_search(const mvfgpu_corpus* corpus, uint8_t metric,
                  const void* queries, uint8_t query_dtype, uint32_t query_dim,
                  uint32_t nq, uint32_t k, float* out_scores,
                  uint64_t* out_indices, int32_t* out_raw);

/*
 * The same search, returning the payload as well: out_vectors = host [nq][k][dimension] in the space's stored type -- what
 * the reference's ScoredVector.vector holds (examples/similarity_search.rs:18, :159-163).  Only the first min(k, rows of the
 * corpus) rows of each query's k are WRITTEN (a padding result among them -- deleted rows -- gives a zero row); the rows behind
 * them, whose results are always padding, are left untouched: k far beyond the corpus (the reference takes any k and returns
 * min(k, n) items) costs min(k, n) rows per query on the device and in the copies, and with nq = 1 a buffer of min(k, rows)
 * rows is enough.  The rows are gathered on the device behind the search, from the result
 * indices where the selection kernel left them: one submission and one wait instead of mvfgpu_search +
 * mvfgpu_corpus_gather_rows.  Small results (rows and results <= 256 KiB, positions not ids) need no gather kernel at all:
 * the final select copies its query's k rows behind the results and the call waits on the flag it stores last (10k x 128 f32,
 * top-10 with vectors: 47.5 us for the two calls, 29.8 for this one).  A corpus that reports vector ids maps them back on the
 * host after the search (the two steps, inside this call).
 */
int mvfgpu_search_fetch(const mvfgpu_corpus* corpus, uint8_t metric,
                        const void* queries, uint8_t query_dtype, uint32_t query_dim,
                        uint32_t nq, uint32_t k, float* out_scores,
                        uint64_t* out_indices, int32_t* out_raw, void* out_vectors);

/*
 * Same search with queries and outputs RESIDENT ON THE CORPUS' DEVICE,
 * asynchronous on `hip_stream` (a hipStream_t; NULL = the default stream).
 * This is the timed region of bench.py and the producer of the per-shard
 * lists that RCCL all-gathers.  d_raw may be NULL.
 * The call does not wait for the device -- with ONE bound: a handle keeps at most TWO int8-selected batched searches
 * in flight.  Such a search posts how many of its queries the repair pass redid (a 4-byte copy behind an event) and the
 * search two calls later consumes that sample before it picks its path, waiting for it if it has not arrived: which path
 * a search takes then depends on the sequence of searches alone, never on how far the host runs ahead.  A caller that
 * pipelines three or more batched searches on one handle has its third enqueue wait for the first search to finish.
 * k > MVFGPU_K_PER_PASS: ceil(k / 1024) passes of the streaming kernel (the floor travels on the device) or one dump pass +
 * a device-wide sort of the shard's order keys, whichever is cheaper (see MVFGPU_K_PER_PASS); no host wait either way.
 * Small batches run the streaming kernel (below 32 queries on corpora under
 * 1 GiB; on larger ones a single query, below 5 for Int8/UInt8 and below 9 for Float32 without the f16 shadow -- the
 * measured crossovers: the streaming kernel takes up to 4 queries per pass over the rows, the MFMA path uses a
 * 64-query tile up to 128 queries).  Larger batches run the MFMA path in phases; an adversarially ordered corpus can
 * overflow a query's candidate buffer there, and such queries are redone exactly by the streaming kernel in REPAIR
 * launches that follow every batched search and decide ON THE DEVICE whether they have anything to do (round 1 read
 * the flags back and synchronised; now e.g. an RCCL all-gather can be queued right behind the search).
 */
int mvfgpu_search_device(const mvfgpu_corpus* corpus, uint8_t metric,
                         const void* d_queries, uint8_t query_dtype,
                         uint32_t query_dim, uint32_t nq, uint32_t k,
                         float* d_scores, uint64_t* d_indices, int32_t* d_raw,
                         void* hip_stream);

/*
 * Merge `nlists` per-shard results, each [nq][k] sorted best-first with
 * UINT64_MAX padding, laid out [nlists][nq][k], into the global [nq][k]
 * ordered by (score order, list order, rank inside the list).  The lists must
 * come in ASCENDING ROW-RANGE ORDER (the rank order of an all-gather): each is
 * sorted by (score order, row position), so ties come out in ascending global
 * row position -- also when the shards report vector ids instead of positions
 * (mvfgpu_corpus_set_vector_ids).  nlists * k < 2^32: up to 8192 entries per query merge in one block's LDS, more by a
 * device-wide sort of the query's entries (the _device forms take their scratch from the stream-ordered allocator:
 * hipMallocAsync / hipFreeAsync on hip_stream).  data_type tells whether `raw`
 * carries the exact integer score (Int8/UInt8 with L2/InnerProduct).
 * _host: plain host buffers, no GPU needed.  _device: device buffers on
 * `device` (e.g. the output of an RCCL all-gather), async on hip_stream.
 */
int mvfgpu_merge_topk_host(const float* scores, const uint64_t* indices,
                           const int32_t* raw, uint32_t nlists, uint32_t nq,
                           uint32_t k, uint8_t metric, uint8_t data_type,
                           float* out_scores, uint64_t* out_indices,
                           int32_t* out_raw);
int mvfgpu_merge_topk_device(const float* d_scores, const uint64_t* d_indices,
                             const int32_t* d_raw, uint32_t nlists, uint32_t nq,
                             uint32_t k, uint8_t metric, uint8_t data_type,
                             float* d_out_scores, uint64_t* d_out_indices,
                             int32_t* d_out_raw, int device, void* hip_stream);

/*
 * The same merge over PACKED lists, the form one all-gather delivers: shard l's
 * list occupies MVFGPU_PACKED_LIST_BYTES(nq, k) bytes at d_packed + l * that,
 * laid out { uint64 indices[nq*k]; float scores[nq*k]; int32 raw[nq*k] }.
 * A rank points mvfgpu_search_device's three outputs into its own list and
 * exchanges it with ONE collective instead of three (the exchange is
 * latency-bound: 16 bytes per result).  d_packed must be 8-byte aligned.
 */
#define MVFGPU_PACKED_LIST_BYTES(nq, k) ((size_t)16 * (size_t)(nq) * (size_t)(k))
int mvfgpu_merge_topk_packed_device(const void* d_packed, uint32_t nlists,
                                    uint32_t nq, uint32_t k, uint8_t metric,
                                    uint8_t data_type, float* d_out_scores,
                                    uint64_t* d_out_indices, int32_t* d_out_raw,
                                    int device, void* hip_stream);

/* ---- radius search ------------------------------------------------------- */

/*
 * Every row within a score threshold of each query ("Radius search").
 *   radii        : host [nq] f32, one bound per query.  Row r matches query q iff r is live (not deleted), its score is not
 *                  NaN and its order key is <= that of radii[q]: L2 distance <= radius, InnerProduct / Cosine score >=
 *                  radius; inclusive.  +inf (L2) / -inf (InnerProduct, Cosine) matches every live non-NaN row.  A NaN
 *                  radius -> MVF_ERR_INVALID_ARGUMENT.  Int8 / UInt8 spaces with L2 / InnerProduct compare the EXACT i32:
 *                  the radius becomes the largest R with sqrtf((float)R) <= radius (L2) / the smallest R with
 *                  (float)R >= radius (InnerProduct), so the matches are bit-exact.
 *   out_counts   : host [nq] u64, the EXACT number of matches of each query, also beyond max_per_query.
 *   out_scores / out_indices / out_raw : host [nq][max_per_query] as mvfgpu_search's (out_raw nullable): the first
 *                  min(count, max_per_query) entries of row q are the query's BEST matches, best first, ties by ascending
 *                  position; the rest is mvfgpu_search's padding (index UINT64_MAX).  Vector ids and index_base as there.
 *   max_per_query: 0 .. MVFGPU_MAX_K; 0 = counts only (the entry buffers may then be NULL).
 * Argument checks and error codes are mvfgpu_search's.  Blocking.  A streaming kernel reads the rows once per 1 or 4
 * queries (batches of 16 and more on Float32 corpora: one pass of the batched f32 MFMA selection kernel with the radius
 * loosened by its proven bound, then exact re-scoring; mvfgpu_selftest_radius_route) and appends matches to device lists
 * of MVFGPU_RADIUS_LIST_CAP entries per query; a query with more matches
 * (and max_per_query > 0) is completed by one mvfgpu_search over such queries with k = max_per_query: when count >
 * max_per_query the entries ARE the top-max_per_query result.
 */
#define MVFGPU_RADIUS_LIST_CAP 8192u
int mvfgpu_search_radius(const mvfgpu_corpus* corpus, uint8_t metric,
                         const void* queries, uint8_t query_dtype, uint32_t query_dim,
                         uint32_t nq, const float* radii, uint64_t max_per_query,
                         uint64_t* out_counts, float* out_scores,
                         uint64_t* out_indices, int32_t* out_raw);

/* ---- candidate search (re-ranking) ---------------------------------------- */

/*
 * The exact top-k over a given list of rows per query ("Candidate search"): the rows an index, a
 * filter or several retrievers proposed, scored exactly and ranked.
 *   candidates   : [nq][m] u64, one list per query (shorter lists padded with UINT64_MAX).  An entry is what a search on
 *                  this handle reports: a global position (index_base + local row), or a vector id when ids are attached
 *                  (mapped back as mvfgpu_corpus_gather_rows maps them; duplicate ids: the first position holding the id).
 *                  The device call always takes positions.  UINT64_MAX, positions outside the shard, ids the shard does not
 *                  hold and deleted rows are skipped, not refused: every row-range shard can take the same global lists,
 *                  and mvfgpu_merge_topk_* of their results is the global answer.  A row listed twice counts once.
 *   out_scores / out_indices / out_raw : [nq][k] as mvfgpu_search's (out_raw nullable): the k best of the query's distinct,
 *                  live, in-shard candidates, best first, ties by ascending position, NaN last, then padding.  Every score
 *                  is the one a one-query mvfgpu_search on the stored rows reports for that (query, row): re-ranking rows a
 *                  search returned reproduces its scores, and a list of every row reproduces the search.
 *   out_counts   : [nq] u64 (nullable): the number of such candidates; the first min(count, k) entries are real.  Across
 *                  row-range shards the counts add up.
 *   k            : 1 .. MVFGPU_MAX_K (k > m pads).  m = 0 is allowed (every result is padding; candidates may be NULL).
 * Argument checks and error codes are mvfgpu_search's; candidates NULL while nq * m > 0 -> MVF_ERR_INVALID_ARGUMENT.
 * mvfgpu_search_candidates is blocking (host buffers); mvfgpu_search_candidates_device takes device buffers and is
 * asynchronous on hip_stream (NULL = the null stream), ordered like mvfgpu_search_device.
 */
int mvfgpu_search_candidates(const mvfgpu_corpus* corpus, uint8_t metric,
                             const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                             const uint64_t* candidates, uint32_t m, uint32_t k,
                             float* out_scores, uint64_t* out_indices, int32_t* out_raw, uint64_t* out_counts);
int mvfgpu_search_candidates_device(const mvfgpu_corpus* corpus, uint8_t metric,
                                    const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                                    const uint64_t* d_candidates, uint32_t m, uint32_t k,
                                    float* d_scores, uint64_t* d_indices, int32_t* d_raw, uint64_t* d_counts,
                                    void* hip_stream);

/* ---- filtered search (top-k among the rows a reusable filter admits) -------- */

/*
 * A filter: an immutable set of admitted rows of ONE corpus handle ("Filtered search").  Created once,
 * used by any number of filtered searches from any thread, destroyed before its corpus.  A filter admits a row iff the row's
 * allow bit is set AND the handle's tombstones do not delete it when the filter is created.
 *   mvfgpu_filter_create        : host bits in the convention of mvfgpu_corpus_set_tombstones with the meaning inverted: bit
 *                                 (first_bit + r) of `allow_bitmap` (byte b >> 3, bit b & 7) set = local row r admitted;
 *                                 nbits >= first_bit + rows; first_bit need not be a multiple of 8 (a row-range shard passes
 *                                 the whole space's bitmap and its first row); bits outside the shard's range are ignored.
 *   mvfgpu_filter_create_device : u32 words over local rows in device memory (bit r & 31 of word r >> 5, ceil(rows / 32)
 *                                 words), read on hip_stream (NULL = the null stream); bits at and beyond `rows` are ignored.
 * Creation computes the exact admitted count on the device and WAITS for it: the one host wait that lets no filtered search
 * wait on the host.  Where some batch size could choose the list route (below) it also builds the ascending list of admitted
 * rows.  device memory: rows / 8 bytes of mask (+ 4 bytes per admitted row with the list): mvfgpu_filter_info::device_bytes.
 * mvfgpu_corpus_set_tombstones starts a new tombstone generation: a filter of an older generation -- or of another handle --
 * is refused by the searches, before any device call, with MVF_ERR_INVALID_ARGUMENT and a message naming the cause; create a
 * new filter.  mvfgpu_filter_destroy (NULL is allowed) waits for the handle's newest work.
 *
 * mvfgpu_search_filtered / mvfgpu_search_filtered_device are mvfgpu_search / mvfgpu_search_device among the admitted rows:
 * arguments, checks, error codes, order (best first, ties by ascending position, NaN last), padding where fewer than k rows
 * are admitted, ids and index_base, out_raw, k up to MVFGPU_MAX_K and the stream discipline are theirs.  The answer is DEFINED
 * as mvfgpu_search on a twin handle whose tombstones are `deleted | ~allow`: Int8 / UInt8 spaces are bit-exact to that twin
 * on every route, float spaces return the same rows up to ties within the project tolerance, and ONE query on a Float32 space
 * has the score bits of scan path 1 on the twin whichever route answers.  Two routes, chosen per call by a pure rule of
 * rows, dimension, data type, nq, k and the admitted count (mvfgpu_selftest_filter_route; MVF_FILTER_ROUTE forces one):
 *   mask : the plain search's routes and kernels with the filter's deny mask in the tombstones' place;
 *   list : only the admitted rows are read, once per group of up to 4 queries, with the streaming kernel's one-query arithmetic.
 * A filtered search leaves the handle's later plain searches as they were: it may build what a plain search builds (norms,
 * shadows), but it neither reads nor feeds the repair feedback (mvfgpu_corpus_info::selection_state stays).
 * Per-query filters are not an API: a filter serves every query of its call -- one call per filter (one KEY per query: the
 * partitioned search below).  Radius, candidate, join
 * and fetch calls take no filter (a candidate list already is one; gather rows afterwards).
 */
typedef struct mvfgpu_filter mvfgpu_filter;

typedef struct mvfgpu_filter_info {
    uint32_t struct_size;  /* in: sizeof(mvfgpu_filter_info); out: bytes filled */
    uint32_t has_row_list; /* 1: the ascending list of admitted rows was built (the list route is available) */
    uint64_t rows;         /* rows of the handle the filter was created for */
    uint64_t admitted;     /* rows the filter admits (allow bit set, not deleted at creation) */
    uint64_t device_bytes; /* device memory the filter holds */
} mvfgpu_filter_info;

int mvfgpu_filter_create(const mvfgpu_corpus* corpus, const uint8_t* allow_bitmap, uint64_t first_bit, uint64_t nbits,
                         mvfgpu_filter** out);
int mvfgpu_filter_create_device(const mvfgpu_corpus* corpus, const uint32_t* d_allow_words, void* hip_stream,
                                mvfgpu_filter** out);
void mvfgpu_filter_destroy(mvfgpu_filter* filter);
int mvfgpu_filter_get_info(const mvfgpu_filter* filter, mvfgpu_filter_info* out);
int mvfgpu_search_filtered(const mvfgpu_corpus* corpus, const mvfgpu_filter* filter, uint8_t metric,
                           const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t k,
                           float* out_scores, uint64_t* out_indices, int32_t* out_raw);
int mvfgpu_search_filtered_device(const mvfgpu_corpus* corpus, const mvfgpu_filter* filter, uint8_t metric,
                                  const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t k,
                                  float* d_scores, uint64_t* d_indices, int32_t* d_raw, void* hip_stream);

/*
 * Self-test of the route a filtered search takes (no GPU needed): *out_route = 1 (mask) or 2 (list) for `nq` queries and `k`
 * results on a corpus of `rows` x `dimension` of `data_type` whose filter admits `admitted` rows, under the default tuning.
 * For fixed other arguments the route is the list at and below some admitted count and the mask above it; admitted = rows is
 * always the mask.
 */
int mvfgpu_selftest_filter_route(uint64_t rows, uint32_t dimension, uint8_t data_type, uint32_t nq, uint32_t k, uint64_t admitted,
                                 uint32_t* out_route);

/* ---- metadata columns and filters from predicates ---------------------------- */

/*
 * A device column: one value per LOCAL row of ONE corpus handle, UInt32 or UInt64 (enum mvf_data_type), copied into device
 * memory of its own next to the rows ("Column filters").  Immutable; used by any number of
 * mvfgpu_filter_create_where calls from any thread; destroyed before its corpus.  The values are what an MVF file keeps in a
 * metadata column (mvf_reader_metadata_column in mvf_file.h: little-endian values, one per row) -- tenant, category, timestamp.
 *   mvfgpu_column_create        : host values; value (first_value + r) belongs to local row r, and first_value + rows <=
 *                                 n_values (a row-range shard passes the whole space's column and its first row, as first_bit
 *                                 does for bitmaps).  `values_le` may have ANY alignment: a file block starts at any byte.
 *                                 The values are copied before the call returns.
 *   mvfgpu_column_create_device : values over local rows in device memory, aligned to their element size, copied device-to-
 *                                 device on hip_stream (NULL = the null stream).
 * Any other data type (StringRef included: the format never defines its bytes) -> MVF_ERR_BUILD "Unsupported metadata column
 * data type".  Columns do not depend on tombstones: mvfgpu_corpus_set_tombstones leaves them valid.  device memory: rows x
 * element size, reported by mvfgpu_column_info::device_bytes and, like a filter's, not counted in mvfgpu_corpus_info.
 * mvfgpu_column_destroy (NULL is allowed) waits for the handle's newest work.
 */
typedef struct mvfgpu_column mvfgpu_column;

typedef struct mvfgpu_column_info {
    uint32_t struct_size;  /* in: sizeof(mvfgpu_column_info); out: bytes filled */
    uint8_t data_type;     /* MVF_DTYPE_UINT32 or MVF_DTYPE_UINT64 */
    uint8_t reserved[3];
    uint64_t rows;         /* rows of the handle the column was created for */
    uint64_t device_bytes; /* device memory the column holds */
} mvfgpu_column_info;

int mvfgpu_column_create(const mvfgpu_corpus* corpus, const void* values_le, uint8_t data_type, uint64_t first_value,
                         uint64_t n_values, mvfgpu_column** out);
int mvfgpu_column_create_device(const mvfgpu_corpus* corpus, const void* d_values, uint8_t data_type, void* hip_stream,
                                mvfgpu_column** out);
void mvfgpu_column_destroy(mvfgpu_column* column);
int mvfgpu_column_get_info(const mvfgpu_column* column, mvfgpu_column_info* out);

/*
 * A filter from predicates over device columns, evaluated on the device: no bitmap is built on the host.
 *
 *   "tenant == 7 AND ts >= T" from a file's columns:
 *       mvf_metadata_column mc;  mvfgpu_column *tenant, *ts;  mvfgpu_filter* f;
 *       mvf_reader_metadata_column(reader, "tenant", &mc);     // UInt32 or UInt64, one value per row of the space
 *       mvfgpu_column_create(corpus, mc.data, mc.data_type, index_base, mc.size / 4, &tenant);   // / 8 for UInt64
 *       mvf_reader_metadata_column(reader, "ts", &mc);
 *       mvfgpu_column_create(corpus, mc.data, mc.data_type, index_base, mc.size / 8, &ts);
 *       mvfgpu_predicate p[2] = {{tenant, MVFGPU_OP_EQ, 0, 7, 0, NULL}, {ts, MVFGPU_OP_GE, 0, T, 0, NULL}};
 *       mvfgpu_filter_create_where(corpus, p, 2, MVFGPU_WHERE_ALL, NULL, &f);                    // once per predicate
 *       mvfgpu_search_filtered(corpus, f, ...);                                                  // any number of searches
 *
 * v is the column's value of local row r, zero-extended to 64 bits; every comparison is unsigned 64-bit, so an operand of
 * 2^32 or more on a UInt32 column is legal and means what the arithmetic says.  BETWEEN is inclusive and a > b admits nothing;
 * IN with no values admits nothing, NOT_IN with no values every row.  Row r is admitted iff the clauses, combined by
 * `combine`, hold AND `base` is NULL or admits r AND the handle's tombstones do not delete r at creation.  The result is an
 * ordinary mvfgpu_filter, indistinguishable from the one mvfgpu_filter_create builds from the bitmap of that predicate: the
 * same mvfgpu_filter_info, staleness rule, routes and search results.  It does not refer to the columns (or to `base`) after
 * creation, which -- like every filter's -- waits for the admitted count.
 * Refused before any device call, with MVF_ERR_INVALID_ARGUMENT and a message naming the cause: NULL arguments; n_clauses
 * outside 1 .. MVFGPU_WHERE_MAX_CLAUSES; an unknown op or combine; more than MVFGPU_WHERE_MAX_SET_VALUES distinct IN / NOT_IN
 * values over the clauses of the call (build the bitmap and call mvfgpu_filter_create for larger sets); a column of another
 * handle; a `base` of another handle or of an older tombstone generation (the searches' own messages).
 */
enum {
    MVFGPU_OP_EQ = 0, MVFGPU_OP_NE = 1, MVFGPU_OP_LT = 2, MVFGPU_OP_LE = 3, MVFGPU_OP_GT = 4, MVFGPU_OP_GE = 5,
    MVFGPU_OP_BETWEEN = 6, MVFGPU_OP_IN = 7, MVFGPU_OP_NOT_IN = 8
};

typedef struct mvfgpu_predicate {
    const mvfgpu_column* column;
    uint32_t op;            /* MVFGPU_OP_* */
    uint32_t n_values;      /* IN / NOT_IN: entries of `values` */
    uint64_t a, b;          /* EQ .. GE: a;  BETWEEN: a <= v <= b */
    const uint64_t* values; /* IN / NOT_IN: host array, any order, repeats allowed; may be NULL when n_values == 0 */
} mvfgpu_predicate;

#define MVFGPU_WHERE_ALL 0u              /* every clause holds */
#define MVFGPU_WHERE_ANY 1u              /* at least one does */
#define MVFGPU_WHERE_MAX_CLAUSES 8u
#define MVFGPU_WHERE_MAX_SET_VALUES 4096u /* over all clauses of one call, each clause's repeats removed */

int mvfgpu_filter_create_where(const mvfgpu_corpus* corpus, const mvfgpu_predicate* clauses, uint32_t n_clauses,
                               uint32_t combine, const mvfgpu_filter* base, mvfgpu_filter** out);

/* ---- partitioned search: one key per query ------------------------------------ */

/*
 * A partition index: the rows of ONE corpus handle that are live when it is created, grouped by the value of ONE device column
 * (UInt32 or UInt64), the rows of a group in ascending position ("Partitioned search").  Built once, on
 * the device; immutable; used by any number of searches from any thread; destroyed before its corpus.  It does not refer to
 * the column after creation, which -- like a filter's -- waits on the host (twice).  Like a filter it is bound to the handle's
 * tombstone generation: a partition of an older generation -- or of another handle -- is refused by the searches, before any
 * device call, with MVF_ERR_INVALID_ARGUMENT and a message naming the cause; create a new one.  A column of another handle is
 * refused at creation like a where-clause's.  device memory: 4 bytes per live row + 16 bytes per distinct key (+ 8); the key
 * table is mirrored on the host (host_bytes), and lookup / keys / the searches' plans read the mirror: no device work.
 * mvfgpu_partition_destroy (NULL is allowed) waits for the handle's newest work.
 *
 * mvfgpu_search_partitioned / mvfgpu_search_partitioned_device are mvfgpu_search / mvfgpu_search_device with one key per query:
 * the result row of query q is the exact top-k among the live rows whose column value, zero-extended to 64 bits, equals keys[q]
 * (unsigned 64-bit comparison: a key of 2^32 or more matches nothing on a UInt32 column, as in mvfgpu_filter_create_where).
 * Arguments, checks, error codes, order (best first, ties by ascending position, NaN last), padding, ids and index_base,
 * out_raw, k up to MVFGPU_MAX_K and the stream discipline are mvfgpu_search's; NULL `keys` is MVF_ERR_INVALID_ARGUMENT.  A key
 * no live row carries gives a row of padding.  `keys` is a HOST array in both calls, read before the call returns.  Every
 * score is the one a one-query mvfgpu_search on the stored rows reports for that (query, row) -- the candidate search's rule --
 * so query q's row equals, byte for byte, the row of mvfgpu_search_candidates for a list of exactly the rows with that key,
 * and what mvfgpu_search_filtered returns for that one query through mvfgpu_filter_create_where(column == keys[q]) of the same
 * tombstone generation.  No search waits on the host (but, where searches pile up, for the previous search's 12-byte-per-query
 * plan to have left the index's pinned buffer).
 * Cost: keys of up to 1024 live rows (and k <= MVFGPU_K_PER_PASS) share a fixed number of launches per 1024 queries whatever
 * the number of keys; every other distinct key of the batch costs what a filtered search by the list route costs.  A key that
 * holds a large share of the rows is served faster by a filter and mvfgpu_search_filtered (`largest` shows such keys).
 * Radius, candidate, join and shard-set calls take no partition; keys in device memory are not an API.
 */
typedef struct mvfgpu_partition mvfgpu_partition;

typedef struct mvfgpu_partition_info {
    uint32_t struct_size;   /* in: sizeof(mvfgpu_partition_info); out: bytes filled */
    uint8_t key_type;       /* MVF_DTYPE_UINT32 or MVF_DTYPE_UINT64 */
    uint8_t reserved[3];
    uint64_t rows;          /* rows of the handle */
    uint64_t live_rows;     /* rows the index holds (not deleted at creation) */
    uint64_t n_keys;        /* distinct values among them */
    uint64_t largest;       /* rows of the largest partition */
    uint64_t device_bytes;  /* 4 B per live row + the key table */
    uint64_t host_bytes;    /* the host mirror of the key table */
} mvfgpu_partition_info;

int mvfgpu_partition_create(const mvfgpu_corpus* corpus, const mvfgpu_column* column, mvfgpu_partition** out);
void mvfgpu_partition_destroy(mvfgpu_partition* partition);
int mvfgpu_partition_get_info(const mvfgpu_partition* partition, mvfgpu_partition_info* out);
/* no device work: out_counts[i] = live rows carrying keys[i] (0 for an unknown key) */
int mvfgpu_partition_lookup(const mvfgpu_partition* partition, const uint64_t* keys, uint64_t n, uint64_t* out_counts);
/* the distinct keys in ascending order with their row counts, [first, first + count) of n_keys: the column's group-by */
int mvfgpu_partition_keys(const mvfgpu_partition* partition, uint64_t first, uint64_t count, uint64_t* out_keys,
                          uint64_t* out_counts);
int mvfgpu_search_partitioned(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, uint8_t metric,
                              const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                              const uint64_t* keys, uint32_t k, float* out_scores, uint64_t* out_indices, int32_t* out_raw);
int mvfgpu_search_partitioned_device(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, uint8_t metric,
                                     const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                                     const uint64_t* keys, uint32_t k, float* d_scores, uint64_t* d_indices, int32_t* d_raw,
                                     void* hip_stream);
/*
 * Self-test of a partitioned search's plan (no GPU needed): for queries whose keys hold counts[q] live rows, out_tier[q] =
 * 0 (padding), 1 (small tier: count <= 1024 and k <= MVFGPU_K_PER_PASS) or 2 (large tier), and *out_groups = the large tier's
 * distinct keys -- the gathered searches the call makes.
 */
int mvfgpu_selftest_partition_plan(const uint64_t* counts, const uint64_t* keys, uint32_t nq, uint32_t k, uint32_t* out_tier,
                                   uint32_t* out_groups);

/* ---- grouped search: at most per_key results per key -------------------------- */

/*
 * mvfgpu_search_grouped / mvfgpu_search_grouped_device are mvfgpu_search / mvfgpu_search_device with a cap per key of a
 * partition index ("Grouped search"): the rows are passages, the column holds the document, and the caller
 * wants the k best passages with at most per_key of any one document (per_key = 1: the k best documents).
 *   Result row of query q: walk the rows the partition holds (the handle's rows that were live at its creation) in
 *   mvfgpu_search's order for q -- best first, ties by ascending position, NaN last, -0.0 == +0.0 --, take a row iff fewer than
 *   per_key rows with the same column value have been taken, stop after k rows, pad as mvfgpu_search pads.  Equivalently: the
 *   top-k of the union over keys of each key's top-per_key.
 * Exact for every distribution of key sizes: every held row is scored, nothing is over-fetched.  Arguments, checks, error
 * codes, ids and index_base, out_raw, k up to MVFGPU_MAX_K and the stream discipline are mvfgpu_search's; generation and
 * ownership are the partitioned search's (a NULL partition, one of another handle or of an older tombstone generation is
 * refused before any device call, with the same messages).  per_key is 1 .. MVFGPU_GROUP_MAX_PER_KEY (one wave's lanes hold a
 * key's running best); 0 or more is MVF_ERR_INVALID_ARGUMENT with a message naming the range.  per_key -> infinity is a plain
 * search.
 * Every score is the one a one-query mvfgpu_search on the stored rows reports for that (query, row) -- the candidate search's
 * rule -- so, byte for byte (indices, score bits, raw), for every data type and batch composition:
 *   1. with C = mvfgpu_search_candidates over the list of ALL rows the partition holds and k = that count, the grouped result
 *      is the walk above applied to C's row;
 *   2. with per_key >= the partition's `largest`, the result is that candidate search cut at k;
 *   3. with k >= per_key x n_keys, the entries carrying key g, in order, are the row of mvfgpu_search_partitioned for key g
 *      with k = per_key, minus its padding.
 * No search waits on the host; the device call is asynchronous on the caller's stream.  The handle's later searches stay as
 * they were: no repair feedback is read or posted (mvfgpu_corpus_info::selection_state stays).
 * Cost: one gathered pass over all held rows per four queries (one per query where four padded queries exceed 40 KiB), 8 bytes
 * per held row and 8 per row of the handle written and read a few times per query beside it.
 * Not built: per_key above 64; a route over the selection shadows or the batched kernels; grouping by a column without a
 * partition index; radius, join and shard-set calls with a cap; keys in device memory.
 *
 * mvfgpu_column_gather: out_values[i] = the column's value, zero-extended to 64 bits, of the row indices[i] names -- what a
 * search on the column's handle reports: global positions, or vector ids where attached (mapped as mvfgpu_corpus_gather_rows
 * maps them).  UINT64_MAX (padding) gives 0 -- tell it from a real 0 by the index; any other index outside the shard is
 * MVF_ERR_INDEX_OUT_OF_BOUNDS.  Blocking; host buffers.
 */
#define MVFGPU_GROUP_MAX_PER_KEY 64u
int mvfgpu_search_grouped(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, uint8_t metric,
                          const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                          uint32_t k, uint32_t per_key, float* out_scores, uint64_t* out_indices, int32_t* out_raw);
int mvfgpu_search_grouped_device(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, uint8_t metric,
                                 const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                                 uint32_t k, uint32_t per_key, float* d_scores, uint64_t* d_indices, int32_t* d_raw,
                                 void* hip_stream);
int mvfgpu_column_gather(const mvfgpu_column* column, const uint64_t* indices, uint64_t count, uint64_t* out_values);
/*
 * Self-test of G1's tier rule (no GPU needed).  G1 cuts the key-ordered list into tiles of 1024 entries; a RUN is what one
 * tile holds of one key's rows.  out_tier[i] for a run of run_lengths[i] entries (1 .. 1024) whose key does (crossing[i] != 0)
 * or does not go on in another tile: 0 (the whole key in the tile, at most per_key rows: all kept), 1 (the whole key in the
 * tile, at most 128 rows: ranked by counting) or 2 (longer, or crossing: one wave keeps the running best 64).
 */
int mvfgpu_selftest_group_plan(const uint64_t* run_lengths, const uint8_t* crossing, uint32_t n, uint32_t per_key,
                               uint32_t* out_tier);
/*
 * Stage timer of a grouped search (scripts/probe_grouped.py): mvfgpu_search_grouped_device without d_raw, for a batch that fits
 * one window of the device work (MVF_ERR_INVALID_ARGUMENT otherwise), with events between its stages; waits for the stream.
 * out_ms[0..3] = the segment bounds (once per call), G0 (scoring), G1 (the per-key best), the tail (select, sort, format).
 */
int mvfgpu_selftest_grouped_stage_ms(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, uint8_t metric,
                                     const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t k,
                                     uint32_t per_key, float* d_scores, uint64_t* d_indices, void* hip_stream, float* out_ms);

/* ---- multi-vector search: top-k keys by summed per-token best (MaxSim) --------- */

/*
 * mvfgpu_search_maxsim / mvfgpu_search_maxsim_device answer SETS of query vectors with KEYS of a partition index (DESIGN.md
 * section 3, "Multi-vector search"): late interaction, as in ColBERT / ColPali-style retrieval.  The rows are the tokens or
 * passages of documents, the column holds the document, a query is a set of T = n_tokens vectors, and a document's score is the
 * sum over the query's vectors of that vector's best score among the document's rows.
 *   queries     : [nq][n_tokens][query_dim], row-major; type and dimension rules are mvfgpu_search's.  n_tokens is
 *                 1 .. MVFGPU_MAXSIM_MAX_TOKENS and the same for every set of a call (ragged sets: one call per length).
 *   per-token best: for token t of set q and key g, b(t, g) is the score of the first row in mvfgpu_search's order for that
 *                 token -- best first, NaN last, -0.0 == +0.0 -- among the rows the partition holds for g; NaN only when every
 *                 row of g scores NaN.  Every row score is the one a one-query mvfgpu_search on the stored rows reports for
 *                 (token, row): the candidate search's rule.  Int8 / UInt8 rows choose the best on the exact i32 order key.  The
 *                 value is the score reconstructed from the order key, as in every result the library writes (+0.0 for +-0.0).
 *   key score   : S(g) = ((b(0,g) + b(1,g)) + ...) + b(T-1,g): plain f32 additions in token order, not fused, not reassociated.
 *                 Under L2 a sum of smallest distances.
 *   result row  : the k best keys by key_from_score(S, metric) -- ascending S under L2, descending otherwise --, ties by ascending
 *                 key value (the order of mvfgpu_partition_keys), NaN last.  out_scores[q][i] = S, out_keys[q][i] = the column
 *                 value zero-extended to 64 bits.  Entries from min(k, n_keys) on are padding: key UINT64_MAX, score +inf (L2) or
 *                 -inf.  out_counts[q] (nullable) = min(k, n_keys): it tells a real key UINT64_MAX from padding.  k is
 *                 1 .. MVFGPU_MAX_K.  There is no out_raw: a sum of i32 scores can leave i32.
 * Refusals, in this order, all before any device call and leaving no device error: mvfgpu_search's metric, nq, k and NULL-buffer
 * checks; n_tokens 0 or above the maximum (MVF_ERR_INVALID_ARGUMENT, "n_tokens must be in 1..1024, got N"); a NULL partition; the
 * handle checks; a partition of another handle or of an older tombstone generation, with the partitioned search's messages.
 * No rows, no held rows or no keys give rows of padding and counts of 0.  The device call makes no host wait and is asynchronous on
 * the caller's stream.  No repair feedback is read or posted (mvfgpu_corpus_info::selection_state stays).
 * So, byte for byte: with R_t = mvfgpu_search_grouped(per_key = 1, k = n_keys) of token t and the hits' keys from
 * mvfgpu_column_gather, summing R_t's scores per key in f32 in token order and ordering by (order key of the sum, key value)
 * gives this call's score bits, keys and counts.
 * Cost (route 1; include/mvf_gpu_maxsim_route.h): the held rows leave HBM once per chunk of up to 32 tokens (fewer where the padded tokens exceed 40 KiB of LDS or the
 * scratch, chunk x n_keys x 4 + n_keys x 20 bytes per query set, would exceed its budget) and query set.
 * Which row was the best for which token: include/mvf_gpu_maxsim_align.h (mvfgpu_maxsim_align on this call's out_keys).
 * Not built: ragged token counts; per-token weights; a route over the selection shadows (the
 * batched MFMA kernels: include/mvf_gpu_maxsim_route.h); shard sets; a filter on top of the partition.
 */
#define MVFGPU_MAXSIM_MAX_TOKENS 1024u
int mvfgpu_search_maxsim(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, uint8_t metric,
                         const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t n_tokens,
                         uint32_t k, float* out_scores, uint64_t* out_keys, uint32_t* out_counts);
int mvfgpu_search_maxsim_device(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, uint8_t metric,
                                const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t n_tokens,
                                uint32_t k, float* d_scores, uint64_t* d_keys, uint32_t* d_counts, void* hip_stream);
/*
 * Self-test of the multi-vector search's scratch plan (no GPU needed): for n_keys keys, n_tokens tokens per set, nq sets, padded
 * tokens of token_bytes in LDS and a scratch budget, the tokens per chunk and the query sets per window.  A chunk holds at most 32
 * tokens, at most what 40 KiB of LDS take (a larger token is read through the cache) and at least one group of four tokens (all
 * where there are fewer); chunk x n_keys x 4 + n_keys x 20 bytes per set of a window stay inside the budget wherever such a
 * one-group chunk does.  The budget of a search is MVF_MAXSIM_SCRATCH_BYTES (default 512 MiB), read when the handle is created.
 */
int mvfgpu_selftest_maxsim_plan(uint64_t n_keys, uint32_t n_tokens, uint32_t nq, uint64_t token_bytes, uint64_t budget_bytes,
                                uint32_t* tokens_per_chunk, uint32_t* sets_per_window);
/*
 * Self-test of the scoring kernel's form (no GPU, no handle): which instantiation of M0 ("M0 / M1") scores
 * rows of `dimension` elements of `data_type` -- the decision the launch itself takes.  forced_g = 0: the library's own lane-group
 * rule; 1, 4, 8, 16, 32 or 64: the width MVF_K1_G forces on a handle.  *out_g = lanes per row, *out_j = 16-byte steps per lane,
 * *out_token_bytes = a padded token (g x j vectors; Float16 rows keep their tokens widened: 32 bytes per vector),
 * *out_form = 0 where the rows stay in registers over a chunk (j <= 4), 1 where they are read again per token group, 2 where in
 * addition the float tokens exceed 40 KiB and are read through the cache; *out_lds_chunk_cap = tokens_per_chunk of
 * mvfgpu_selftest_maxsim_plan for 1024 tokens and an unbounded budget.  Refused with MVF_ERR_INVALID_ARGUMENT: a NULL output, an
 * unknown data type, dimension 0, an Int8 / UInt8 dimension above MVFGPU_MAX_INT_DIM, a row above 1 GiB, any other forced_g.
 */
int mvfgpu_selftest_maxsim_form(uint8_t data_type, uint32_t dimension, uint32_t forced_g, uint32_t* out_g, uint32_t* out_j,
                                uint32_t* out_token_bytes, uint32_t* out_form, uint32_t* out_lds_chunk_cap);
/*
 * Stage timer of a multi-vector search (scripts/probe_maxsim.py): mvfgpu_search_maxsim_device without d_counts, with events between
 * its stages; waits for the stream.  out_ms[0..3] = the key ordinals (once per call), M0 (scoring and per-key best), M1 (the sums),
 * the tail (select, sort, format), each summed over the call's chunks and windows.
 */
int mvfgpu_selftest_maxsim_stage_ms(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, uint8_t metric,
                                    const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t n_tokens,
                                    uint32_t k, float* d_scores, uint64_t* d_keys, void* hip_stream, float* out_ms);

/*
 * The MFMA selection route of the multi-vector search -- mvfgpu_set_maxsim_route, MVF_MAXSIM_ROUTE and the route's self-tests -- is
 * declared in include/mvf_gpu_maxsim_route.h: the same bytes as this call's, from a selection on the matrix unit.
 */

/*
 * Candidate keys ("Candidate keys"): mvfgpu_search_maxsim restricted, per query set, to a list of keys --
 * the re-ranking step of late-interaction retrieval, whose first stage hands every query a few hundred or thousand documents.
 * queries, n_tokens, metric, k and the outputs are mvfgpu_search_maxsim's, with the same types, limits and padding.
 *   candidate_keys : [nq][m] column values, one list per query set; a HOST array in both calls, read before the call returns (as
 *                    mvfgpu_search_partitioned's keys).  An entry is a candidate of its set iff the partition holds the key
 *                    (mvfgpu_partition_lookup gives a count > 0).  Every other entry is skipped, not refused: unknown keys, keys
 *                    whose rows are all deleted, the conventional pad UINT64_MAX where the column does not hold it.  A key listed
 *                    twice counts once.  m = 0 is allowed: every row is padding, counts are 0, candidate_keys may be NULL.
 *   score          : S(g) is mvfgpu_search_maxsim's, bit for bit: the same b(t, g) and the same plain f32 sum in token order.
 *   result row     : the k best of the set's distinct held candidates by (order key of S, ascending key value), NaN last, then
 *                    mvfgpu_search_maxsim's padding.  out_counts[q] (nullable) = min(k, distinct held candidates of q).
 * So, byte for byte (score bits, keys, counts): the result row of set q is the row of mvfgpu_search_maxsim with k = n_keys on the
 * same partition with the entries whose key is no candidate of q removed, cut at k and padded; a list of every key of
 * mvfgpu_partition_keys reproduces mvfgpu_search_maxsim; b(t, g) is the score mvfgpu_search_partitioned reports for (token t,
 * key g, k = 1).
 * Refusals, all before any device call and leaving no device error: mvfgpu_search_maxsim's up to n_tokens, in its order; then a
 * NULL candidate_keys while nq * m > 0 (MVF_ERR_INVALID_ARGUMENT, "NULL buffer (candidate_keys)"); then mvfgpu_search_maxsim's
 * remaining ones in its order and wording.
 * The device call is asynchronous on the caller's stream and waits on the host only for the previous call's plan to have left the
 * index's pinned buffer (the partitioned search's rule).  No repair feedback is read or posted.
 * Cost: the CANDIDATES' rows leave HBM once per chunk of tokens and query set; scratch per window of query sets is
 * mvfgpu_search_maxsim's with the window's largest distinct-candidate count in n_keys' place, plus 8 bytes per candidate row
 * (each set's rows rounded up to a multiple of 128), inside MVF_MAXSIM_SCRATCH_BYTES wherever one set's fits.
 * Which row was the best for which token: include/mvf_gpu_maxsim_align.h (mvfgpu_maxsim_align on the same lists).
 * Not built: shard sets (a document's rows may span shards); candidate keys in device memory; ragged token counts; per-token
 * weights.
 */
int mvfgpu_search_maxsim_candidates(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, uint8_t metric,
                                    const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t n_tokens,
                                    const uint64_t* candidate_keys, uint32_t m, uint32_t k, float* out_scores, uint64_t* out_keys,
                                    uint32_t* out_counts);
int mvfgpu_search_maxsim_candidates_device(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, uint8_t metric,
                                           const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                                           uint32_t n_tokens, const uint64_t* candidate_keys, uint32_t m, uint32_t k, float* d_scores,
                                           uint64_t* d_keys, uint32_t* d_counts, void* hip_stream);
/*
 * Self-test of the candidate plan of ONE query set (no GPU needed): from a list and every entry's held row count
 * (mvfgpu_partition_lookup's), out_slot[i] = the slot ordinal of entry i -- its key's rank among the set's distinct held keys in
 * ascending key value -- or UINT32_MAX where the entry is skipped (held_counts[i] == 0) or repeats an earlier entry;
 * *out_distinct = the distinct held candidates, *out_rows = the rows they hold.
 */
int mvfgpu_selftest_maxsim_candidates_plan(const uint64_t* candidate_keys, const uint64_t* held_counts, uint32_t m,
                                           uint32_t* out_slot, uint32_t* out_distinct, uint64_t* out_rows);
/*
 * Stage timer of a candidate multi-vector search (scripts/probe_maxsim_candidates.py): the device call without d_counts, with
 * events between its stages; waits for the stream.  out_ms[0..3] = the plan's upload and E0 (the expansion), M0, M1, the tail,
 * each summed over the call's chunks and windows.
 */
int mvfgpu_selftest_maxsim_candidates_stage_ms(const mvfgpu_corpus* corpus, const mvfgpu_partition* partition, uint8_t metric,
                                               const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                                               uint32_t n_tokens, const uint64_t* candidate_keys, uint32_t m, uint32_t k,
                                               float* d_scores, uint64_t* d_keys, void* hip_stream, float* out_ms);

/*
 * Self-test of the host-side normalisation (no GPU needed): every operator but IN / NOT_IN (MVF_ERR_INVALID_ARGUMENT) becomes
 * one range test *out_lo <= v <= *out_hi on a column of `data_type`, negated where *out_negate is 1 (NE only).  The range is
 * clamped to the type's values (hi <= 2^32 - 1 on UInt32); an empty range is reported as lo = 1, hi = 0.
 */
int mvfgpu_selftest_predicate_range(uint8_t data_type, uint32_t op, uint64_t a, uint64_t b, uint64_t* out_lo,
                                    uint64_t* out_hi, uint32_t* out_negate);

/*
 * Measurement aid (scripts/probe_column_filters.py): the predicate kernel alone.  Checks and prepares the call as
 * mvfgpu_filter_create_where does, then launches the kernel `repeats` times (1 .. 64) on the handle's stream between device
 * events and reports each launch's milliseconds in out_ms[repeats].  No filter is built.
 */
int mvfgpu_selftest_where_kernel_ms(const mvfgpu_corpus* corpus, const mvfgpu_predicate* clauses, uint32_t n_clauses,
                                    uint32_t combine, const mvfgpu_filter* base, uint32_t repeats, float* out_ms);

/* ---- k-NN join (queries taken from resident rows) -------------------------- */

#define MVFGPU_JOIN_WINDOW 1024u        /* query rows per search of a join, counted from `first` */
#define MVFGPU_JOIN_EXCLUDE_SELF 1u     /* a query row is never among its own results (decided on positions) */

/*
 * The exact top-k of rows [first, first + count) of `query_corpus` (NULL = `corpus`: the self-join, the k-NN graph) among
 * the live rows of `corpus` ("Join").  Nothing leaves the device but the results: the query rows are
 * staged on the device from the stored rows (Float32 as stored, Float16 widened exactly, Int8 / UInt8 as stored), searched
 * with the metric and arithmetic of mvfgpu_search, and reported in its order and padding ([count][k]; out_raw nullable;
 * entries are corpus' index_base + row, or corpus' vector ids where attached).
 *   flags        : MVFGPU_JOIN_EXCLUDE_SELF: the row of `corpus` whose GLOBAL POSITION equals the query row's global position
 *                  (query_corpus' index_base + row) is not reported for that query.  Positions decide, never ids (duplicate
 *                  ids are legal) and never scores (exact duplicates of a row are its neighbours and are reported).  Where
 *                  the two handles' row ranges do not overlap the flag changes nothing.  Unknown bits are refused.
 *   k            : 1 .. MVFGPU_MAX_K, with the flag 1 .. MVFGPU_MAX_K - 1.
 *   first, count : local rows of query_corpus, first + count <= its rows; count = 0 is allowed (nothing is written).
 * A deleted (tombstoned) query row gets a result row of padding; deleted rows of `corpus` are never reported.
 * The range is processed in windows of MVFGPU_JOIN_WINDOW query rows counted from `first` (the last may be short), and the
 * entries of a query row are exactly -- indices, score bits, raw -- what mvfgpu_search_device on `corpus` returns for its
 * window's staged queries with k' = k + 1 (k' = k without the flag or where the row ranges do not overlap), with the query
 * row's own entry removed if it is among the k', else the last entry dropped.  So dimension limits, refusals, scan_path and
 * tuning are those of mvfgpu_search on `corpus` with that batch size and k'; k = MVFGPU_K_PER_PASS with the flag gives
 * k' = 1025 and takes the large-k route.  The searches ARE searches of `corpus`: its repair feedback sees them, and its rule
 * "at most two int8-selected batched searches in flight" paces the join's windows too.
 * The two handles must agree in dimension (MVF_ERR_DIMENSION_MISMATCH) and data type (MVF_ERR_BUILD) and live on one device
 * (MVF_ERR_INVALID_ARGUMENT); unknown flag bits, NULL outputs while count > 0 and a range outside query_corpus are
 * MVF_ERR_INVALID_ARGUMENT; every check comes before the first device call.
 * mvfgpu_knn_join is blocking (host buffers): window w's results leave through pinned memory on a copy stream while window
 * w + 1 is searched.  mvfgpu_knn_join_device takes device buffers and enqueues every window on hip_stream (NULL = the null
 * stream) without a host wait, ordered like mvfgpu_search_device behind both handles' newest work.  Device scratch is one
 * window's queries and lists, 1024 x (4 dimension + 16 k') bytes at most (the host call: + 2 x 1024 x 16 k bytes of
 * results); it does not grow with count.  Row-range shards: join every shard as query_corpus against every shard as
 * corpus with the flag set and merge the lists in ascending row-range order with mvfgpu_merge_topk_*.
 */
int mvfgpu_knn_join(const mvfgpu_corpus* corpus, const mvfgpu_corpus* query_corpus /* NULL = corpus */,
                    uint8_t metric, uint64_t first, uint64_t count, uint32_t k, uint32_t flags,
                    float* out_scores, uint64_t* out_indices, int32_t* out_raw /* nullable */);
int mvfgpu_knn_join_device(const mvfgpu_corpus* corpus, const mvfgpu_corpus* query_corpus /* NULL = corpus */,
                           uint8_t metric, uint64_t first, uint64_t count, uint32_t k, uint32_t flags,
                           float* d_scores, uint64_t* d_indices, int32_t* d_raw /* nullable */, void* hip_stream);

/*
 * Self-test of the radius conversion (no GPU needed): the largest order key (mvf_common.h) a row may have to match
 * `radius` on a space of `data_type` under `metric`, and in *out_raw (nullable) the exact i32 bound R of Int8 / UInt8
 * spaces under L2 / InnerProduct (0 otherwise; L2 -1 = nothing matches, InnerProduct INT32_MAX = nothing can match).
 */
int mvfgpu_selftest_radius_bound(uint8_t data_type, uint8_t metric, float radius, uint32_t* out_key, int32_t* out_raw);

/*
 * Self-test of the route a radius search takes (no GPU needed): *out_route = 0 when the streaming radius kernel serves `nq`
 * queries on a corpus of `data_type` (one read of the rows per 1 or 4 queries), 1 when ONE thresholded pass of the batched
 * f32 MFMA selection kernel (the radius loosened by its proven error bound) + exact re-scoring of its candidates does
 * (Float32 corpora, nq >= 16; queries whose candidates overflow are redone by the streaming kernel).  scan_path as in
 * mvfgpu_set_scan_path: 1 forces the streaming route, 2 / 3 / 5 the batched one on Float32 corpora, anything else is automatic.
 */
int mvfgpu_selftest_radius_route(uint8_t data_type, uint32_t nq, int scan_path, uint32_t* out_route);

/* ---- several GPUs in one process ------------------------------------------ */

/*
 * A shard set = the row-range shards of ONE vector space, one corpus handle per GPU, searched as a whole
 * (SURVEY.md §8e): every shard searches its rows with global indices on its own device and stream, the per-shard
 * top-k lists cross xGMI in ONE packed RCCL all-gather (ncclCommInitAll over the shards' devices; single process, no
 * MPI, no torch), and the (score order, shard order, rank) merge runs on the first shard's device.  This is what a
 * Rust host that owns all GPUs of a node binds; one process per GPU (torch.distributed / RCCL) composes
 * mvfgpu_search_device + an all-gather + mvfgpu_merge_topk_packed_device itself (metrovector_amd/sharded.py).
 *   shards : handles on DISTINCT devices, in ascending row-range order (index_base ascending, ranges disjoint), all of
 *            one dimension and data type; BORROWED -- they must outlive the set and are not destroyed with it.
 *            A single shard is allowed (a 1-rank RCCL communicator: the same exchange code path).  Shards that share
 *            a device (rehearsing the protocol on fewer GPUs than shards; RCCL refuses duplicate devices), or
 *            MVF_SHARDSET_NO_RCCL=1, exchange their lists with device-to-device copies instead.
 * RCCL is loaded lazily (dlopen librccl.so) by the first mvfgpu_shardset_create; MVF_ERR_DEVICE if it is needed and
 * cannot be loaded.  Any k the shards take (n_shards * k < 2^32).  One search at a time per set (calls serialise); results as mvfgpu_search.
 */
typedef struct mvfgpu_shardset mvfgpu_shardset;
typedef struct mvfgpu_shardset_info {
    uint32_t struct_size; /* in: sizeof(mvfgpu_shardset_info); out: bytes filled */
    uint32_t n_shards;
    uint32_t rccl_ranks; /* ranks of the RCCL communicator (= n_shards), 0 when the lists travel by device copies */
    uint32_t dimension;
    uint8_t data_type;
    uint8_t reserved[7];
    uint64_t rows;       /* over all shards */
} mvfgpu_shardset_info;
#define MVFGPU_MAX_SHARDS 64
typedef struct mvfgpu_shardset_timing { /* the newest search, milliseconds */
    uint32_t struct_size;    /* in: sizeof(mvfgpu_shardset_timing); out: bytes filled */
    uint32_t n_shards;
    uint64_t searches;       /* searches the set has served */
    float total_ms;          /* HOST wall clock, call to return: query upload, searches, exchange, merge, results on the host */
    float enqueue_ms;        /* HOST wall clock until every shard's search and the exchange step were enqueued */
    float search_ms;         /* DEVICE (HIP events on the shard's own stream): query upload + local search of the SLOWEST
                                shard; the shards run concurrently */
    float exchange_merge_ms; /* DEVICE, first shard's stream: from the end of ITS local search to the end of the merge =
                                waiting for the slowest shard + the all-gather (RCCL, or device copies) + merge_shards */
    float shard_search_ms[MVFGPU_MAX_SHARDS]; /* DEVICE: query upload + local search per shard (row-range order) */
} mvfgpu_shardset_timing;
int mvfgpu_shardset_create(mvfgpu_corpus* const* shards, int n_shards, mvfgpu_shardset** out);
void mvfgpu_shardset_destroy(mvfgpu_shardset* set);
int mvfgpu_shardset_get_info(const mvfgpu_shardset* set, mvfgpu_shardset_info* out);
int mvfgpu_shardset_search(mvfgpu_shardset* set, uint8_t metric, const void* queries,
                           uint8_t query_dtype, uint32_t query_dim, uint32_t nq, uint32_t k,
                           float* out_scores, uint64_t* out_indices, int32_t* out_raw);
int mvfgpu_shardset_last_timing(const mvfgpu_shardset* set, mvfgpu_shardset_timing* out);

/* ---- utilities ----------------------------------------------------------- */

/* Fill a device buffer [nq][dimension] with synthetic queries (query dtype of
 * `data_type`: f32 for Float32/Float16 spaces, else the int type). */
int mvfgpu_synth_queries_device(void* d_queries, uint32_t nq, uint32_t dimension,
                                uint8_t data_type, uint64_t seed, int device,
                                void* hip_stream);

int mvfgpu_set_profiling(mvfgpu_corpus* corpus, int enabled);
int mvfgpu_last_timing(const mvfgpu_corpus* corpus, mvfgpu_timing* out);

/* Force a scan path for A/B measurements and tests: 0 = automatic,
 * 1 = streaming kernel (K1) for every nq, 2 = MFMA batched kernel (K2) on the
 * stored rows, 3 = K2 with the f16 shadow on Float32 corpora (same as 2 on
 * the other types), 4 = as 0, but one or two queries on a Float32 corpus
 * STREAM THE F16 SHADOW instead of the stored rows (half the bytes, so about
 * half the time; same proven-margin selection and exact re-scoring as the
 * batched path: the same rows as path 1, scores within the 1e-5 tolerance --
 * the re-scoring kernel sums in another order than the streaming kernel).
 * Off by default: the default single-query path reads the stored rows,
 * whatever the handle has served before.
 * 5 = K2 selecting on an INT8 SHADOW of a Float32 / Float16 corpus (per-row
 * scale; built on first use, `dimension` bytes per row; also enabled by
 * MVF_I8_SHADOW=1): the int8 MFMA runs at about twice the f16 kernel's rate
 * under the part's power limit; every row whose approximate score is within a
 * PROVEN bound of the k-th best (5-8 x k rows per query on uniform data; the
 * f16 shadow keeps a handful) is re-scored from the stored rows and the f32
 * query, so the rows are again those of the exact path (up to ties within
 * the tolerance; tests/test_gpu_round3.py compares all 1024 lists of the
 * benchmark batch).  Same as 0 on Int8 /
 * UInt8 corpora, and for k > 409 (path 6's streaming: k > 204): the margin
 * would not fit the candidate budget, such requests take the f16 shadow / the
 * stored rows.
 * 6 = as 5, and ONE TO FOUR queries STREAM THE INT8 SHADOW through K1
 * (`dimension` bytes per row instead of 4x / 2x that; same bound, exact
 * re-scoring: ~1.2 ms for one query instead of 4.5 on 10M x 768 f32).  On
 * Float32 rows the re-scoring uses K1's own arithmetic, so a single query gets
 * the bits of path 1.  Path 0 does the same BY DEFAULT for ONE query on a
 * Float32 corpus of at least 512 MiB of rows (k <= 204), once its whole int8
 * shadow is held or fits beside it (+25 % of the rows' HBM, built by the first
 * such query, ~13 ms on 10M x 768) and its rows are finite; the answer does not
 * depend on the route.  MVF_STREAM_I8=0 keeps path 0 on the stored rows;
 * MVF_STREAM_I8=1 also takes the route below 512 MiB, and on Float16 corpora,
 * once the corpus holds a whole int8 shadow.  Two to four queries are served
 * as fast by the 64-query MFMA tile.
 * From 4 GiB of Float32 rows on, path 0 sends that ONE query over a 6-BIT SHADOW
 * instead (0.75 x the int8 shadow's bytes, tiled for the scan; the query is
 * taken at sixteen bits, the bound is proven as before, the re-scoring is K1's:
 * the same bits once more) -- where the margin of the 6-bit bound is predicted
 * to hold at most 8192 rows (10M x 768 at k = 100: ~5 300; k = 204 there and
 * 10M x 1024 stay on int8).  It is built by the first such query straight from
 * the stored rows (+19 % of the rows' HBM; whole or not at all, the same
 * free-memory rule), needs no int8 shadow and leaves one alone.  MVF_STREAM_6B=0
 * keeps path 0 on the int8 shadow, MVF_STREAM_I8=0 on the stored rows.  A corpus
 * whose queries keep overflowing the 6-bit margin goes back to the int8 route
 * by itself (selection_state bit 2).  Filtered, radius, candidate and join
 * searches and two to four queries stay on the int8 shadow.
 * 7 = as 6, but ONE unfiltered Float32 query streams the 6-bit shadow at any
 * size (tests), until the handle's 6-bit switch goes off.
 *
 * Selection shadows: batched searches on a Float32 / Float16 corpus select
 * candidates on an INT8 copy of the rows (path 5's, the default: built by the
 * first such search or an eager upload; skipped when it would leave < 2 GiB
 * free; MVF_I8_SHADOW=0 opts out) -- or, Float32 corpora on scan path 3 /
 * without the int8 one, on a scaled-f16 copy (+50 %; MVF_F16_SHADOW=0 opts
 * out) -- keep every row whose approximate score is within a proven error bound
 * of the k-th, and re-score the kept rows from the stored rows and the f32
 * query.  Rows and order are those of the exact path; only the selection
 * arithmetic differs.  mvfgpu_corpus_get_info reports which shadows a handle
 * holds (`shadows`) and counts them in `device_bytes`. */
int mvfgpu_set_scan_path(mvfgpu_corpus* corpus, int path);

/*
 * The tuning switches of the environment (MVF_K1_G, MVF_K2_*, MVF_I8_SHADOW, MVF_F16_SHADOW, MVF_QS_REFINE,
 * MVF_STREAM_I8, MVF_STREAM_6B, MVF_REPAIR_WINDOW, MVF_UPLOAD_THREADS, MVF_HOST_ZC_*, MVF_HOST_FLAG_WAIT, MVF_LARGE_K, MVF_FILTER_ROUTE, MVF_MAXSIM_ROUTE, MVF_DEBUG_REPAIR; INTEGRATION.md lists them) are read ONCE per
 * handle, when it is created: a search never calls getenv.  An A/B script that changes the environment of a live handle
 * calls this to have it read again.  A development aid: it waits for the handle's host-buffer searches, but
 * mvfgpu_search_device reads the switches unlocked -- do not call it beside device-pointer searches of the same handle.
 */
int mvfgpu_corpus_reload_tuning(mvfgpu_corpus* corpus);

/*
 * ABI version of the library: bumped whenever a struct layout or a function signature of this header changes in a way
 * an older caller would misread (2: every out-struct starts with struct_size, round 3; 3: corpus_info.selection_state,
 * reload_tuning, k beyond 1024; the later lift of the k <= 16384 limit changed no layout and no signature, nor did the
 * radius search, which only ADDS mvfgpu_search_radius and mvfgpu_selftest_radius_bound, nor did the candidate search, which
 * only adds mvfgpu_search_candidates and mvfgpu_search_candidates_device, nor did the k-NN join, which only adds mvfgpu_knn_join and
 * mvfgpu_knn_join_device, nor did the filtered search, which only adds mvfgpu_filter_*, mvfgpu_search_filtered,
 * mvfgpu_search_filtered_device and mvfgpu_selftest_filter_route, nor did the metadata columns, which only add mvfgpu_column_*,
 * mvfgpu_filter_create_where, mvfgpu_selftest_predicate_range and mvfgpu_selftest_where_kernel_ms, nor did mvfgpu_selftest_poison, nor did the partitioned search, which only
 * adds mvfgpu_partition_*, mvfgpu_search_partitioned, mvfgpu_search_partitioned_device and mvfgpu_selftest_partition_plan, nor did
 * the grouped search, which only adds mvfgpu_search_grouped, mvfgpu_search_grouped_device, mvfgpu_column_gather,
 * mvfgpu_selftest_group_plan and mvfgpu_selftest_grouped_stage_ms, nor did the multi-vector search, which only adds
 * mvfgpu_search_maxsim, mvfgpu_search_maxsim_device, mvfgpu_selftest_maxsim_plan and mvfgpu_selftest_maxsim_stage_ms, nor did
 * its candidate form, which only adds mvfgpu_search_maxsim_candidates, mvfgpu_search_maxsim_candidates_device,
 * mvfgpu_selftest_maxsim_candidates_plan and mvfgpu_selftest_maxsim_candidates_stage_ms, nor did mvfgpu_selftest_maxsim_form, nor did
 * the multi-vector search's MFMA route, whose functions include/mvf_gpu_maxsim_route.h declares).  A binding compares it with the MVFGPU_ABI_VERSION it was built against
 * at load time.
 */
#define MVFGPU_ABI_VERSION 3u
uint32_t mvfgpu_abi_version(void);

/*
 * Self-test of the automatic path choice (no GPU needed).  Batched searches watch how many of their queries the repair
 * pass had to redo and switch a corpus whose data defeats the cheap bounds back to slower selections: first the folded
 * pre-filter of the int8 kernels goes, then the int8-shadow selection.  `samples` holds n_samples records of four u32
 * {queries of the search, queries repaired, ran with the folded pre-filter, selected on the int8 shadow} in the order
 * the searches were consumed; out_state receives {queries counted, repairs counted, pre-filter off, int8 selection off}.
 */
int mvfgpu_selftest_feedback(const uint32_t* samples, uint32_t n_samples, uint32_t* out_state);

/*
 * Self-test of the route a search takes (no GPU needed): which kernels serve `nq` queries for `k` results on a corpus of
 * `rows` x `dimension` of `data_type` under the default tuning, scan path 0 and no history -- a function of these numbers
 * alone (the thresholds come from the measured crossover tables under profiles/).
 * *out_route: 0 = the streaming kernel K1 (one pass per 1..4 queries), 1 = the batched MFMA route; for k >
 * MVFGPU_K_PER_PASS: 2 = passes of K1 behind a floor, 3 = K1 as a dump + the whole-shard sort.
 */
int mvfgpu_selftest_route(uint64_t rows, uint32_t dimension, uint8_t data_type, uint8_t metric, uint32_t nq, uint32_t k,
                          uint32_t* out_route);

/*
 * Self-test of the rows a search on path 0 reads (no GPU needed; same arguments and tuning as mvfgpu_selftest_route, whose
 * answer it refines for route 0): *out_rows = 1 where ONE query streams the int8 shadow of the Float32 rows (K1 over a
 * quarter of the bytes, re-scored with K1's arithmetic: the same bits), 0 where K1 reads the stored rows.  The shape part of
 * the rule only: at run time the shadow must also be whole, fit (or be held) and have finite bound maxima.
 */
int mvfgpu_selftest_stream_rows(uint64_t rows, uint32_t dimension, uint8_t data_type, uint8_t metric, uint32_t nq, uint32_t k,
                                uint32_t* out_rows);

/*
 * ... and WHICH shadow (no GPU needed; the same arguments): *out_bits = 0 where K1 reads the stored rows, 8 where the one
 * query streams the int8 shadow, 6 where it streams the 6-bit shadow -- at least 4 GiB of rows and at most 8192 rows predicted
 * inside the 6-bit bound's margin (a Gaussian-tail model with per-metric constants measured on the oracle's rows: api.hip,
 * stream_6b_shape).  The shape part of the rule only, as above.
 */
int mvfgpu_selftest_stream_bits(uint64_t rows, uint32_t dimension, uint8_t data_type, uint8_t metric, uint32_t nq, uint32_t k,
                                uint32_t* out_bits);

/*
 * The 6-bit shadow's layout on the host (no GPU needed; csrc/shadow_6b.h): the bytes the shadow of `rows` x `dimension`
 * holds; `codes` (rows x dimension values in [-31, 31]) packed into `out` as the build kernel packs them (the bytes
 * behind the last row zero); and the codes read back out of such a shadow.
 */
uint64_t mvfgpu_selftest_shadow6_bytes(uint64_t rows, uint32_t dimension);
int mvfgpu_selftest_shadow6_pack(const int8_t* codes, uint64_t rows, uint32_t dimension, uint8_t* out, uint64_t out_bytes);
int mvfgpu_selftest_shadow6_unpack(const uint8_t* shadow, uint64_t shadow_bytes, uint64_t rows, uint32_t dimension, int8_t* out_codes);

/*
 * Self-test of a batched search's phase schedule (no GPU needed): the row boundaries R_1 .. R_last = rows of the geometric phases a
 * batch of `nq` queries for `k` results runs over `rows` rows under the default tuning (int8_selection != 0: the lists of the
 * int8-shadow selection, 8192 slots per query; 0: 4096), the growth factor between them, and in *out_refined_mask bit i set where the
 * threshold is refined with exact scores BEHIND phase i (in front of phase i + 1).  DESIGN.md section 5; the constants come from
 * the in-process A/B runs of profiles/r05_k2_walk_and_phase_costs.txt.  k <= MVFGPU_K_PER_PASS.
 */
int mvfgpu_selftest_schedule(uint64_t rows, uint32_t nq, uint32_t k, int int8_selection, uint64_t* out_bounds, uint32_t max_bounds,
                             uint32_t* out_n_bounds, uint32_t* out_growth, uint32_t* out_refined_mask);

/*
 * The debug switch MVF_DEBUG_POISON=<0..255> as this process read it (no GPU needed): the byte every allocation of the library
 * is filled with before its first use, or -1 when the variable is unset, not a number or out of range (nothing is filled then).
 * Read once per process, at the first allocation or the first call of this function.  Tests start a child process with the
 * variable set and assert through this that the child really ran poisoned ("Poisoned allocations").
 */
int mvfgpu_selftest_poison(void);

#ifdef __cplusplus
}
#endif
#endif
