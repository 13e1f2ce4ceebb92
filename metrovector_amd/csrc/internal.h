// internal.h — pieces of api.hip the other translation units of libmvf_gpu.so use.
#pragma once

#include "../../include/mvf_status.h"

#include "mvf_common.h"
#include "scan_stream.h"

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>

typedef struct mvfgpu_corpus mvfgpu_corpus;
typedef struct mvfgpu_filter mvfgpu_filter;
typedef struct mvfgpu_column mvfgpu_column;
typedef struct mvfgpu_partition mvfgpu_partition;

namespace mvf {

// records the calling thread's failure detail (mvfgpu_last_error_message) and returns `status`
int set_fail(int status, const std::string& msg);

// a HIP call that fails ends the function with MVF_ERR_DEVICE and the call's text + the runtime's message as the detail
#define MVF_HIP_TRY(expr)                                                                                  \
    do {                                                                                                   \
        hipError_t e__ = (expr);                                                                           \
        if (e__ != hipSuccess)                                                                             \
            return mvf::set_fail(MVF_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e__));      \
    } while (0)

// the metric code of every entry point that takes one
inline int check_metric(uint8_t metric) {
    if (metric != MVF_METRIC_L2 && metric != MVF_METRIC_INNER_PRODUCT && metric != MVF_METRIC_COSINE)
        return set_fail(MVF_ERR_INVALID_ARGUMENT, "unsupported distance metric code " + std::to_string(metric));
    return MVF_OK;
}

// the calling thread's current device set to `dev` for a scope
struct DevScope {
    int prev = -1;
    bool ok = false;
    explicit DevScope(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DevScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// MVF_DEBUG_POISON=<0..255> (debug only; DESIGN.md §2 "Poisoned allocations"): every allocation the library makes is filled
// with that byte before its first use, so that a test can tell whether an answer depends on memory nobody wrote.  Read ONCE
// per process -- not per handle, not through Tuning: AsyncBuf has no handle, and nothing on the per-search path calls getenv.
// -1 = unset (or not a number in 0..255): one predictable branch per allocation.
inline int debug_poison_byte() {
    static const int byte = [] {
        const char* e = getenv("MVF_DEBUG_POISON");
        if (!e || !*e) return -1;
        char* end = nullptr;
        const long v = strtol(e, &end, 0);
        return (*end || v < 0 || v > 255) ? -1 : (int)v;
    }();
    return byte;
}
// The fill itself, directly behind the allocation; explicit initialisations stay where they are and run after it.
// stream-ordered memory: on the allocation's own stream
inline hipError_t poison_fill(void* p, size_t bytes, hipStream_t s) {
    const int b = debug_poison_byte();
    return (b < 0 || !p || !bytes) ? hipSuccess : hipMemsetAsync(p, b, bytes, s);
}
// hipMalloc memory: a synchronous fill and a host wait (a poisoned run tests dependence on CONTENT, not on timing)
inline hipError_t poison_fill(void* p, size_t bytes) {
    const int b = debug_poison_byte();
    if (b < 0 || !p || !bytes) return hipSuccess;
    const hipError_t e = hipMemset(p, b, bytes);
    return e != hipSuccess ? e : hipStreamSynchronize(nullptr);
}
// pinned host memory
inline void poison_fill_host(void* p, size_t bytes) {
    const int b = debug_poison_byte();
    if (b >= 0 && p && bytes) memset(p, b, bytes);
}

// The stream-ordered pool the library's scratch comes from: its own pool on the calling thread's current device, created on
// first use and kept for the life of the process, which never hands memory back to the OS between calls.  The device's DEFAULT
// pool releases everything unused at every synchronisation, so each call's scratch was memory fresh from the OS -- and under
// the platform's HIP runtime a kernel's stores into such memory were intermittently lost to the next kernel on the same
// stream (zeros read back: an all-padding or all-NaN answer from the filter's list route, an admitted count of 0;
// profiles/r13_fresh_process.txt).  A pool that keeps its memory also spares every search the OS allocation.  What it holds
// is bounded by the largest scratch a call takes (the 512-MiB windows of scan_gather.hip, the radius lists).
hipError_t scratch_pool(hipMemPool_t* out);

// stream-ordered scratch, released on every way out
struct AsyncBuf {
    void* p = nullptr;
    hipStream_t s = nullptr;
    hipError_t alloc(size_t bytes, hipStream_t st) {
        s = st;
        if (!bytes) return hipSuccess;
        hipMemPool_t pool = nullptr;
        hipError_t e = scratch_pool(&pool);
        if (e == hipSuccess) e = hipMallocFromPoolAsync(&p, bytes, pool, st);
        return e != hipSuccess ? e : poison_fill(p, bytes, st);
    }
    ~AsyncBuf() {
        if (p) (void)hipFreeAsync(p, s);
    }
};

// Out-structs of the C ABI start with a caller-set `struct_size` (include/mvf_gpu.h "OUT-STRUCTS GROW"): copy at most
// that many bytes of `full` and report how many were filled.
template <class T>
int copy_out_struct(T* out, T full) {
    const uint32_t have = out->struct_size;
    if (have < 8u) return set_fail(MVF_ERR_INVALID_ARGUMENT, "struct_size not set (MVFGPU_INIT the out-struct before the call)");
    const uint32_t n = have < (uint32_t)sizeof(T) ? have : (uint32_t)sizeof(T);
    full.struct_size = n;
    std::memcpy(out, &full, n);
    return 0;
}

// Tuning switches of the environment (INTEGRATION.md lists them).  Read ONCE per handle, when it is created
// (mvfgpu_corpus_reload_tuning re-reads them for A/B scripts): nothing on the per-search path calls getenv.
// -1 / 0 = "not set: the library's own rule".
struct Tuning {
    int k1_g = 0;               // MVF_K1_G: lanes per row of the streaming kernel (sweeps)
    int k2_pp = -1;             // MVF_K2_PP=0|1: force the lockstep / ping-pong schedule on 256-query Float16 tiles
    uint32_t k2_growth = 4;     // MVF_K2_GROWTH: largest phase-to-phase growth of the batched scan
    uint32_t k2_growth_small = 6;  // MVF_K2_GROWTH_SMALL: ... of batches of up to 128 queries (HBM-bound scans: their records cost them little); follows MVF_K2_GROWTH where only that is set
    bool k2_bias = true;        // MVF_K2_BIAS=0: round 2's epilogue instead of the folded pre-filter
    int k2_tile = 0;            // MVF_K2_TILE=64|128|256: force a query-tile shape
    bool f16_shadow = true;     // MVF_F16_SHADOW=0
    bool i8_shadow = true;      // MVF_I8_SHADOW=0
    bool i8_shadow_partial = true;  // MVF_I8_SHADOW_PARTIAL=0: no int8 shadow of a prefix of the rows where all rows do not fit
    uint64_t i8_shadow_rows = 0;    // MVF_I8_SHADOW_ROWS=n (tests): as if only the first n rows' shadow fitted
    bool qs_refine = true;      // MVF_QS_REFINE=0
    uint32_t qs_refine_phases = 2;  // MVF_QS_REFINE_PHASES: the threshold is refined in front of this many of the last phases (round 5: 2; each costs ~70 us for 1024 queries and spares the phase behind it two thirds of its records)
    bool debug_repair = false;  // MVF_DEBUG_REPAIR: report repaired queries on stderr (synchronises inside a search)
    uint32_t repair_window = 0; // MVF_REPAIR_WINDOW: queries per repair launch pair (tests: several windows)
    uint64_t region_records = 0;  // MVF_K2_REGION_RECORDS: size of the candidate regions (tests: force overflows)
    int stream_i8 = -1;         // MVF_STREAM_I8: unset -1 (the automatic rule), 0 off, 1 on (any size once a shadow exists)
    bool stream_6b = true;      // MVF_STREAM_6B=0: ONE Float32 query never streams the 6-bit shadow (it stays on the int8 shadow / the stored rows)
    int stream_5p1 = -1;        // MVF_STREAM_5P1: unset -1 (the 5+1 layout of the 6-bit shadow from kStream51MinBytes of rows on, shadow_5p1.h), 0 never, 1 wherever it is no larger than the 6-bit layout
    unsigned upload_threads = 0;  // MVF_UPLOAD_THREADS
    size_t host_zc_query = 64u << 10;     // MVF_HOST_ZC_QUERY: mvfgpu_search reads queries up to this size in place (pinned host)
    size_t host_zc_results = 256u << 10;  // MVF_HOST_ZC_RESULTS: ... and writes results up to this size in place
    bool host_flag_wait = true; // MVF_HOST_FLAG_WAIT=0: the blocking host call always waits on its stream (not on the flag the final select writes)
    int filter_route = 0;       // MVF_FILTER_ROUTE=1|2: a filtered search always by the mask route (1) / always by the list route (2; the list is then built whatever the count); 0: the rule (filter_route_rule)
    size_t maxsim_scratch = 512ull << 20;  // MVF_MAXSIM_SCRATCH_BYTES: the multi-vector search's scratch per window (tests: several token chunks and windows at a small shape)
    int maxsim_route = 0;       // MVF_MAXSIM_ROUTE=1|2: a multi-vector search always by the one-pass route (1) / by the MFMA selection route where it is eligible (2); 0: the rule (maxsim_route, scan_maxsim.h)
    int large_k = 0;            // MVF_LARGE_K=1|2: k beyond one pass always by passes (1; k <= 16384) / always by the whole-shard sort (2); 0: the cheaper one
};
Tuning read_tuning();

// What the radius and candidate searches (radius.hip, candidates.hip) read of a handle: the resident rows and their masks
// (set_tombstones / set_vector_ids must not race with searches), and the stream of the host-buffer calls.  The row ARRAY and
// its shape are fixed for the handle's life; the rows' bytes change only through a row write (update.hip), which is ordered
// like a search: a call that reads the view under corpus_device_call sees every write enqueued before it and none after it.
struct CorpusView {
    int device = 0, num_cus = 256, k1_g = 0;
    uint64_t n = 0, index_base = 0;
    uint32_t dim = 0, pitch = 0, V = 0;
    uint8_t dtype = 0;
    const unsigned char* rows = nullptr;
    const uint32_t* tomb = nullptr;  // NULL = no deletions
    const uint64_t* ids = nullptr;   // NULL = index_base + row
    void* stream = nullptr;          // hipStream_t of the host-buffer API (used under host_mutex)
    int scan_path = 0;               // mvfgpu_set_scan_path
    uint64_t tomb_gen = 0;           // the generation of `tomb`: every mvfgpu_corpus_set_tombstones starts a new one
    int filter_route = 0;            // Tuning::filter_route
    size_t maxsim_scratch = 0;       // Tuning::maxsim_scratch
    int maxsim_route = 0;            // mvfgpu_set_maxsim_route, else Tuning::maxsim_route
};
CorpusView corpus_view(const mvfgpu_corpus* c);
// bytes of one query of the handle's space: Float32, or the space's own type for Int8 / UInt8
inline size_t query_row_bytes(const CorpusView& v) { return (size_t)v.dim * (is_int_dtype(v.dtype) ? 1 : 4); }
std::mutex& corpus_host_mutex(const mvfgpu_corpus* c);  // serialises the host-buffer calls of a handle
// Float32 / Float16 corpora: the row norms the batched kernels read (built on first use, on `stream`): xnorm[n] = |x|,
// xx2[n] = sum x^2, xxmax[1] = max of xx2.  The caller runs under corpus_device_call(c, stream, ...): the handle's lock is held,
// and `stream` is ordered behind a build that another stream's call enqueued.
int corpus_row_norms(const mvfgpu_corpus* c, void* stream, const float** xnorm, const float** xx2, const float** xxmax);
// K1's lane-group width for rows of V 16-byte vectors and nqv queries per pass (MVF_K1_G forces one: `forced`)
void k1_group(uint32_t V, int nqv, int forced, int* G, uint32_t* J);
// The shape of one pass of K1 -- or of R1, the radius kernel built on it -- over rows of V vectors with `queries` queries
// left to serve at list length k: four queries per pass from two queries on (one read of the rows instead of two to four),
// one per pass where the four-query LDS tile exceeds 150 KiB.  lds_bytes(G, J, nqv, pmax) is the kernel's own LDS formula;
// the caller refuses a shape whose `lds` exceeds the part's 160 KiB with its own message.
struct K1Shape {
    int nqv = 1, G = 64;                       // queries per pass, lanes per row
    uint32_t J = 1, chunk_rows = 0, pmax = 0;  // 16-byte steps per lane and row, rows per chunk, LDS list entries per query
    size_t lds = 0;
};
template <class LdsBytes>
inline K1Shape k1_pass_shape(uint32_t V, uint32_t queries, uint32_t k, int forced, LdsBytes lds_bytes) {
    K1Shape sh;
    for (sh.nqv = queries >= 2 ? 4 : 1;; sh.nqv = 1) {
        k1_group(V, sh.nqv, forced, &sh.G, &sh.J);  // the lane-group width depends on the queries per pass
        sh.chunk_rows = scan_chunk_rows(sh.G, sh.J, sh.nqv);
        sh.pmax = next_pow2(k + scan_chunk_safe(sh.G));
        sh.lds = lds_bytes(sh.G, sh.J, sh.nqv, sh.pmax);
        if (sh.nqv == 1 || sh.lds <= 150 * 1024) return sh;
    }
}
// The part of mvfgpu_search's argument checks that needs no handle, in its order: metric, nq, k = 1 .. MVFGPU_MAX_K, non-NULL
// query and output buffers.  A search with arguments of its own calls it, then checks those, then check_search_args: what
// needs no handle is refused before `corpus is NULL`.
int check_search_scalars(uint8_t metric, uint32_t nq, uint32_t k, const void* queries, const void* out_scores, const void* out_indices);
// mvfgpu_search's argument checks: `corpus is NULL`, check_search_scalars, then the query's type and dimension
int check_search_args(const mvfgpu_corpus* c, uint8_t metric, const void* queries, uint8_t query_dtype, uint32_t query_dim,
                      uint32_t nq, uint32_t k, const void* out_scores, const void* out_indices);
// With vector ids attached (mvfgpu_corpus_set_vector_ids): out[i] = the global position (index_base + row) of the FIRST row
// holding ids[i], through the sorted (id, row) table the first call builds; UINT64_MAX and ids the shard does not hold give
// UINT64_MAX.  Returns false, out untouched, when the handle has no ids (entries are positions then).
bool corpus_ids_to_positions(const mvfgpu_corpus* c, const uint64_t* ids, uint64_t count, uint64_t* out);
// The handle's pinned host mirrors of the host-buffer calls (search_host's), at least in_bytes / out_bytes; the caller holds
// corpus_host_mutex.  Waits for the handle's newest work first: a search may still write the old ones in place.
int corpus_pinned_mirrors(const mvfgpu_corpus* c, size_t in_bytes, size_t out_bytes, void** pin_in, void** pin_out);
// mvfgpu_search_device's stream discipline around `body`, which enqueues work on `stream` -- any number of searches among
// it: under the handle's lock, ordered behind the handle's newest work on another stream (ev_done), and ev_done recorded on
// `stream` on every way out.
int corpus_device_call(const mvfgpu_corpus* c, void* stream, const std::function<int()>& body);
// mvfgpu_search_device's search -- its routes, kernels, repair feedback and timing -- for a caller that already runs under
// corpus_device_call(c, stream, ...): no argument checks, the handle's lock is not taken again, and the id mapping of the final
// kernels is switched off: every entry is a global position (index_base + row) even where vector ids are attached (the join
// excludes by position and maps ids itself).
int search_positions_locked(const mvfgpu_corpus* c, uint8_t metric, const void* d_queries, uint32_t nq, uint32_t k, float* d_scores,
                            uint64_t* d_indices, int32_t* d_raw, void* stream);


// ---- filtered search (filter.hip; DESIGN.md §3 "Filtered search")
// What a search reads of a filter: its deny mask in the tombstone buffer's layout (the handle's tombstones included), the
// ascending list of its admitted rows where it was built, and the route this search takes.
struct FilterUse {
    const uint32_t* deny = nullptr;
    const uint32_t* list = nullptr;
    uint64_t admitted = 0;
    bool by_list = false;
};
// mvfgpu_search / mvfgpu_search_device restricted to the filter's rows (api.hip): the mask route runs the plain search's routes
// and kernels with flt.deny in the tombstones' place; by_list, no admitted row or an empty corpus go to filter_list_search.
// Neither polls nor posts the repair feedback.
int search_filtered_host(const mvfgpu_corpus* c, const FilterUse& flt, uint8_t metric, const void* queries, uint8_t query_dtype,
                         uint32_t query_dim, uint32_t nq, uint32_t k, float* out_scores, uint64_t* out_indices, int32_t* out_raw);
int search_filtered_device(const mvfgpu_corpus* c, const FilterUse& flt, uint8_t metric, const void* d_queries, uint8_t query_dtype,
                           uint32_t query_dim, uint32_t nq, uint32_t k, float* d_scores, uint64_t* d_indices, int32_t* d_raw,
                           void* hip_stream);
// The list route (filter.hip): F2 over flt.list, the results merged and formatted as a search's; everything on `s`, no host
// wait; the caller runs under corpus_device_call.
int filter_list_search(const CorpusView& v, const FilterUse& flt, uint8_t metric, const void* d_queries, uint32_t nq, uint32_t k,
                       float* d_scores, uint64_t* d_indices, int32_t* d_raw, hipStream_t s);
// The route of a filtered search under the default tuning, a pure function (mvfgpu_selftest_filter_route): 1 = mask, 2 = list
uint32_t filter_route_rule(uint64_t rows, uint32_t dim, uint8_t dtype, uint32_t nq, uint32_t k, uint64_t admitted);
// A filter of `c` from ALLOW words over local rows in device memory (mvfgpu_filter_create_device's layout), for a caller that
// already runs under corpus_device_call(c, s, ...) with `v` read there: F0 / F1 on `s` and the one wait for the admitted count.
int filter_from_allow_words(const mvfgpu_corpus* c, const CorpusView& v, const uint32_t* d_allow, hipStream_t s, mvfgpu_filter** out);
// what the column filters (columns.hip) read of a base filter: whose it is, its tombstone generation, its deny mask
struct FilterOrigin {
    const mvfgpu_corpus* owner;
    uint64_t tomb_gen;
    const uint32_t* deny;
};
FilterOrigin filter_origin(const mvfgpu_filter* f);
// what the partition index (partition.hip) reads of a column when it is created: whose it is, its type, its values [rows]
struct ColumnOrigin {
    const mvfgpu_corpus* owner;
    uint8_t dtype;
    const void* values;
};
ColumnOrigin column_origin(const mvfgpu_column* col);
// what the grouped search (grouped.hip) reads of a partition index: whose it is, its tombstone generation, the live rows grouped
// by key (ascending inside a key), the device key table (keys[n_keys] ascending, then offsets[n_keys + 1]) and its counts
struct PartitionView {
    const mvfgpu_corpus* owner;
    uint64_t tomb_gen;
    const uint32_t* rows_by_key;
    const uint64_t* table;
    uint64_t live, n_keys, largest;
};
PartitionView partition_view(const mvfgpu_partition* part);
// a search of `c` may use the index: it was created for this handle and holds the handle's current tombstones
int check_partition_use(const mvfgpu_corpus* c, const mvfgpu_partition* part);
// `bytes` of a host-made plan into the index's pinned buffer and from there to `dst` on `s` (the partitioned search's plan, the
// candidate multi-vector search's).  The caller holds the owner's lock.  Waits only for the previous upload to have left the buffer.
int partition_upload(const mvfgpu_partition* part, const void* src, size_t bytes, void* dst, hipStream_t s);
// mvfgpu_partition_lookup for one key, from the host mirror: (offset, count) of its rows in rows_by_key; count 0 where no live
// row carries it.  from (nullable): a caller that looks keys up in ASCENDING order passes one word, 0 at first, and every search
// covers only the table behind the previous key's place
void partition_find(const mvfgpu_partition* part, uint64_t key, uint64_t* offset, uint64_t* count, uint64_t* from = nullptr);
// waits for the newest work enqueued on the handle
int corpus_wait_newest(const mvfgpu_corpus* c);

// ---- row writes (update.hip; DESIGN.md §3 "Row writes")
// Everything a handle derives from its rows' bytes, as it is RESIDENT now: a NULL array has not been built (or does not exist
// for the space) and stays so.  Read under corpus_device_call.
struct WriteTargets {
    unsigned char* rows = nullptr;
    uint64_t n = 0, index_base = 0;
    uint32_t dim = 0, pitch = 0;
    uint8_t dtype = 0;
    void* norms = nullptr;  // launch_row_norms_f32's / launch_row_norms16's `out`; xx2 and xxmax behind it as they take them
    float *xx2 = nullptr, *xxmax = nullptr;
    unsigned char* shadow16 = nullptr;  // the scaled-f16 shadow, its pitch and scales
    uint32_t pitch16 = 0;
    float* xscale = nullptr;
    unsigned char* shadow8 = nullptr;  // the int8 shadow of the rows [0, shadow8_rows), its pitch, scales and bound maxima
    uint32_t pitch8 = 0;
    uint64_t shadow8_rows = 0;
    float *xscale8 = nullptr, *qs_stats = nullptr;
    unsigned char* shadow6 = nullptr;  // the 6-bit shadow (shadow6_p51: in the 5+1 layout), its scales and bound maxima
    bool shadow6_p51 = false;
    float *xscale6 = nullptr, *qs6_stats = nullptr;
};
WriteTargets corpus_write_targets(const mvfgpu_corpus* c);
// A write refreshed these items (mvfgpu_write_report::refreshed): the cached read-backs of a refreshed shadow's bound maxima go
// back to "not read".  Under corpus_device_call, behind the launches.
void corpus_rows_written(const mvfgpu_corpus* c, uint32_t refreshed);
// the handle's pinned buffer for the positions of a device write (host_staging.h)
struct PinnedUpload;
PinnedUpload& corpus_write_upload(const mvfgpu_corpus* c);

}  // namespace mvf
