// api.hip — the C ABI of libmvf_gpu.so (include/mvf_gpu.h).
//
// Host-side orchestration only: validation in the reference's error
// vocabulary (src/errors.rs:8-40), HBM residency of one row-range shard,
// kernel sequencing on the caller's HIP stream.  No CPU compute path exists
// here: without a device every compute entry point fails with MVF_ERR_DEVICE.

#include "../../include/mvf_gpu.h"
#include "../../include/mvf_gpu_maxsim_route.h"

#include "aux_kernels.h"
#include "host_staging.h"
#include "internal.h"
#include "scan_candidates.h"
#include "scan_filter.h"
#include "mvf_common.h"
#include "scan_mfma.h"
#include "scan_stream.h"
#include "shadow_6b.h"
#include "shadow_5p1.h"
#include "../../include/mvf_gpu_stream_5p1.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace mvf;

namespace {

thread_local std::string g_last_error;

int fail(int status, const std::string& msg) {
    g_last_error = msg;
    return status;
}

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t reserve(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        hipError_t e = hipMalloc(&p, need);
        if (e == hipSuccess) bytes = need, e = poison_fill(p, need);
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// Pinned host memory the device reads and writes in place (hipHostMalloc: mapped, coherent): the host-buffer API's
// mirrors for small queries / results.
struct PinBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t reserve(size_t need) {
        if (need <= bytes) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
        need = (need + 4095) & ~(size_t)4095;
        hipError_t e = hipHostMalloc(&p, need, hipHostMallocDefault);
        if (e == hipSuccess) bytes = need, poison_fill_host(p, need);
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};

}  // namespace

namespace mvf {
int set_fail(int status, const std::string& msg) { return fail(status, msg); }

hipError_t scratch_pool(hipMemPool_t* out) {
    constexpr int kMaxDevices = 64;
    constexpr size_t kScratchAnchorBytes = 4096;
    static std::mutex mu;
    static hipMemPool_t pools[kMaxDevices] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lk(mu);
    if (!pools[dev]) {
        hipMemPoolProps props{};
        props.allocType = hipMemAllocationTypePinned;
        props.handleTypes = hipMemHandleTypeNone;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = dev;
        hipMemPool_t pool = nullptr;
        e = hipMemPoolCreate(&pool, &props);
        if (e != hipSuccess) return e;
        uint64_t keep = ~0ull;  // never trimmed at a synchronisation
        e = hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
        if (e != hipSuccess) {
            (void)hipMemPoolDestroy(pool);
            return e;
        }
        // One block stays in use for the life of the process.  While the pool holds no block in use, a synchronous hipFree
        // elsewhere in the process (a column, a partition index, a filter) leaves the pool's memory zero again, and the zeros
        // land DURING the next call: its first copy or its last store is lost (profiles/r20_fresh_index_routes.txt).
        void* anchor = nullptr;
        e = hipMallocFromPoolAsync(&anchor, kScratchAnchorBytes, pool, nullptr);
        if (e == hipSuccess) e = poison_fill(anchor, kScratchAnchorBytes, nullptr);
        if (e != hipSuccess) {
            if (anchor) (void)hipFreeAsync(anchor, nullptr);
            (void)hipMemPoolDestroy(pool);
            return e;
        }
        pools[dev] = pool;
    }
    *out = pools[dev];
    return hipSuccess;
}

Tuning read_tuning() {
    Tuning t;
    auto num = [](const char* name, long dflt) {
        const char* e = getenv(name);
        return e ? atol(e) : dflt;
    };
    auto flag = [](const char* name, bool dflt) {
        const char* e = getenv(name);
        return e ? atoi(e) != 0 : dflt;
    };
    const long g = num("MVF_K1_G", 0);
    t.k1_g = (g == 64 || g == 32 || g == 16 || g == 8 || g == 4 || g == 1) ? (int)g : 0;
    t.k2_pp = getenv("MVF_K2_PP") ? (int)flag("MVF_K2_PP", false) : -1;
    t.k2_growth = (uint32_t)std::max(2l, num("MVF_K2_GROWTH", 4));
    t.k2_growth_small = (uint32_t)std::max(2l, num("MVF_K2_GROWTH_SMALL", getenv("MVF_K2_GROWTH") ? (long)t.k2_growth : 6));
    t.qs_refine_phases = (uint32_t)std::max(0l, num("MVF_QS_REFINE_PHASES", 2));
    t.k2_bias = flag("MVF_K2_BIAS", true);
    const long tile = num("MVF_K2_TILE", 0);
    t.k2_tile = tile == 0 ? 0 : tile == 64 ? 64 : tile == 128 ? 128 : 256;
    t.f16_shadow = flag("MVF_F16_SHADOW", true);
    t.i8_shadow = flag("MVF_I8_SHADOW", true);
    t.i8_shadow_partial = flag("MVF_I8_SHADOW_PARTIAL", true);
    t.i8_shadow_rows = (uint64_t)std::max(0l, num("MVF_I8_SHADOW_ROWS", 0));
    t.qs_refine = flag("MVF_QS_REFINE", true);
    t.debug_repair = getenv("MVF_DEBUG_REPAIR") != nullptr;
    t.repair_window = (uint32_t)std::max(0l, num("MVF_REPAIR_WINDOW", 0));
    if (const char* e = getenv("MVF_K2_REGION_RECORDS")) t.region_records = strtoull(e, nullptr, 10);
    t.stream_i8 = getenv("MVF_STREAM_I8") ? (flag("MVF_STREAM_I8", false) ? 1 : 0) : -1;
    t.stream_6b = flag("MVF_STREAM_6B", true);
    t.stream_5p1 = getenv("MVF_STREAM_5P1") ? (flag("MVF_STREAM_5P1", false) ? 1 : 0) : -1;
    t.upload_threads = (unsigned)std::max(0l, num("MVF_UPLOAD_THREADS", 0));
    t.host_zc_query = (size_t)std::max(0l, num("MVF_HOST_ZC_QUERY", 64l << 10));
    t.host_zc_results = (size_t)std::max(0l, num("MVF_HOST_ZC_RESULTS", 256l << 10));
    t.large_k = (int)std::min(2l, std::max(0l, num("MVF_LARGE_K", 0)));
    t.host_flag_wait = flag("MVF_HOST_FLAG_WAIT", true);
    t.filter_route = (int)std::min(2l, std::max(0l, num("MVF_FILTER_ROUTE", 0)));
    t.maxsim_scratch = (size_t)std::max(1l, num("MVF_MAXSIM_SCRATCH_BYTES", 512l << 20));
    t.maxsim_route = (int)std::min(2l, std::max(0l, num("MVF_MAXSIM_ROUTE", 0)));
    return t;
}
}  // namespace mvf

// search_host's request to the search it is about to enqueue: "store `seq` to `flag` behind your results if your last kernel
// can" (the streaming path's final select); `armed` comes back true if it will.  Handed to search_device (below) explicitly and
// on to the routes in the search's SearchCall.
struct HostFlagReq {
    uint32_t* flag;
    uint32_t* ticket;
    uint32_t seq;
    bool armed;
    uint64_t gen;  // the handle's work_gen of this search
    unsigned char* gather_out;  // mvfgpu_search_fetch: the final select copies the payload rows here too (pinned host memory); NULL = none
    bool gathered;              // ... and did, for every query
};

struct mvfgpu_corpus {
    int device = 0;
    uint64_t n = 0, index_base = 0;
    uint32_t dim = 0, pitch = 0, V = 0, J = 0;
    int G = 64;
    uint8_t dtype = 0;
    unsigned char* d_rows = nullptr;
    size_t rows_bytes = 0;
    int num_cus = 256;

    mutable std::mutex mu;       // guards the scratch + timing state
    mutable std::mutex host_mu;  // serialises the host-buffer API's device mirrors
    mutable DevBuf cand;                  // scratch: per-block candidate lists (K1)
    mutable DevBuf bq, bstate, bcand, xnorm;  // K2: padded queries + norms; tau/cnt/overflow; candidates; row norms
    mutable DevBuf blk;                   // K2 narrow types: per-block candidate regions + their counts (scan_mfma.h)
    mutable const void* blk_armed_cnt = nullptr;  // the region counters at this address are all zero: the last batched search's scatters left them so
    mutable DevBuf repair;                // K2 overflow repair: gathered queries + their results
    mutable std::vector<std::pair<uint64_t, int>> occ_cache;  // (kernel, dynamic LDS) -> blocks per CU (scan_occupancy)
    mutable const unsigned char* bq_zeros = nullptr;  // where the prepared-query buffer's 64 zero bytes were last set ...
    mutable size_t bq_zero_bytes = 0;                 // ... and the buffer's size then
    mutable DevBuf floor1;                // k > MVFGPU_K_PER_PASS: per query, the last composite the pass before returned, + 1
    mutable DevBuf rank_a, rank_b, rank_tmp;  // k > MVFGPU_K_PER_PASS by the whole-shard sort: the composites of every row (x the queries of a pass), twice, + the sort's scratch
    mutable DevBuf shadow, xscale;        // Float32 corpora: scaled-f16 shadow rows (selection only) + 2^-s_r per row
    DevBuf tomb, ids;                     // deletion bitmap (u32 words over local rows) / vector ids (u64 per local row)
    uint64_t deleted = 0;                 // bits set in the bitmap
    uint64_t tomb_gen = 0;                // bumped by every mvfgpu_corpus_set_tombstones: a filter (filter.hip) holds the bitmap of ONE generation
    std::vector<uint64_t> h_ids;          // host copy of the ids ...
    mutable std::vector<std::pair<uint64_t, uint32_t>> id_index;  // ... and, built by the first gather, (id, row) sorted by id
    mutable int shadow_state = 0;         // 0 not built yet, 1 ready, -1 unavailable (no memory)
    mutable DevBuf shadow8, xscale8, qs_stats;  // Float32 / Float16 corpora: int8 shadow rows, s_r per row, the 4 bound maxima
    mutable int shadow8_state = 0;             // 0 not tried, 1 all rows, 2 a PREFIX of the rows (shadow8_rows; batched path only), -1 no room for all rows, -2 none for a useful prefix either
    mutable uint64_t shadow8_rows = 0;         // rows the int8 shadow covers
    mutable int shadow8_finite = -1;           // the shadow's four bound maxima are finite: -1 not read back yet, 0 no (a row holds Inf / NaN), 1 yes
    mutable DevBuf split_out;                  // partial shadow: the two row ranges' result lists before their merge
    mutable DevBuf shadow6, xscale6, qs6_stats;  // Float32 corpora: the 6-bit shadow in 64-row tiles (shadow_6b.h), s_r per row, its 4 bound maxima
    mutable int shadow6_state = 0;               // 0 not tried, 1 all rows, -1 no room (whole or none: no prefix shadows on this route)
    mutable int shadow6_finite = -1;             // as shadow8_finite
    mutable bool shadow6_p51 = false;            // the shadow is held in the 5+1 layout (shadow_5p1.h; stream_5p1_layout): one of the two formats, whole or none
    // the 5+1 scan's per-block words (ScanParams::pub / lo_stats): kPub51Blocks x 8 bytes of published bests, then kPub51Blocks x
    // 16 bytes of low-plane counters; zeroed once, told apart between searches by pub51_seq
    mutable DevBuf pub51;
    mutable uint32_t pub51_seq = 0, pub51_blocks = 0;  // the newest 5+1 search's sequence number and blocks (0: the newest 6-bit-route search was not one)
    // feedback for the automatic choice: after a search that selected on the int8 shadow the number of queries the
    // repair launches had to redo is copied to pinned host memory (no wait); a later search that finds it large
    // (the data defeats the int8 bound: near-duplicates everywhere, heavy-tailed rows) switches this corpus back to the
    // f16 selection for good
    // Two slots, used alternately: a search first CONSUMES the count the search two before it posted into its slot
    // (waiting for that copy if need be: it is two searches old), then posts its own -- so which path a search takes
    // depends on the sequence of searches alone, never on how fast the host runs ahead of the device.
    // (the count is waited for through the end-of-call event of the search that posted it: ev_done below)
    mutable uint32_t* qs_redo_host = nullptr;  // [2] pinned
    mutable uint32_t qs_redo_done[2] = {0, 0};  // which of the two ev_done covers the slot's count ...
    // ... unless the search that posted it shared its call with others (the windows of a join: corpus_device_call runs them all
    // under ONE end-of-call event, recorded when the last has been enqueued): such a search records an event of its own
    mutable hipEvent_t qs_redo_ev[2] = {nullptr, nullptr};  // created by the first search that needs one
    mutable bool qs_redo_own[2] = {false, false};
    mutable bool qs_redo_pending[2] = {false, false};
    mutable bool qs_disabled = false;
    mutable uint32_t qs_redo_nq[2] = {0, 0};
    mutable uint32_t qs_slot = 0;  // the slot the next post goes to
    mutable uint32_t qs_seen = 0, qs_redone = 0;  // running totals of int8-selected queries / of those the repair pass redid
    // the same feedback guards the folded pre-filter of the i32-accumulator K2 kernels (scan_mfma16_bias.inc): rows whose
    // norms differ wildly inside a lane's four defeat its per-lane bounds, the wave regions overflow and the queries go
    // to the repair pass -- exact, but 50x slower; such a corpus goes back to round 2's epilogue first (fb_bias: the
    // search the pending count belongs to used the folded pre-filter; fb_qs: it selected on the int8 shadow)
    mutable bool bias_disabled = false, fb_bias[2] = {false, false}, fb_qs[2] = {false, false};
    // the 6-bit shadow stream posts into the same two slots (fb_s6) but feeds a switch and totals of its own: a corpus that
    // defeats the 6-bit bound goes back to the int8 route, whose own switch its repairs never touch
    mutable bool s6_disabled = false, fb_s6[2] = {false, false};
    mutable uint32_t s6_seen = 0, s6_redone = 0;
    mutable const uint32_t* last_redo_cnt = nullptr;  // device: the count the newest repair pass produced
    mutable const uint32_t* fb_mirrored = nullptr;    // the pinned slot flag_compact_kernel of the newest repair pass stored that count into itself (no copy then)
    mutable bool xnorm_ready = false;
    mutable uint32_t bstate_slots = 0;    // queries the K2 state arrays are armed for
    mutable DevBuf h_q, h_s, h_i, h_r;    // device mirrors for the host-buffer API
    // Completion of a small blocking search without the stream: the final select stores a sequence number into pinned host
    // memory behind its results and search_host spins on it -- hipStreamSynchronize learns of a finished kernel ~5 us later
    // (end-of-pipe flush, completion signal, wake-up; profiles/r04_flag_wait.txt).
    mutable PinBuf pin_flag;
    mutable DevBuf done_ticket;
    mutable uint32_t flag_seq = 0;
    mutable uint64_t work_gen = 0, confirmed_gen = ~0ull;  // searches enqueued on the handle / the newest one seen complete through the flag
    mutable PinBuf pin_q, pin_out, pin_vec;  // ... and its pinned host mirrors (small queries / results / payload rows: no copy engine at all)
    mutable DevBuf h_v;                   // payload rows of mvfgpu_search_fetch too large for that
    mutable hipStream_t own_stream = nullptr;
    hipStream_t up_stream = nullptr;      // upload pipeline: re-pitch / norms / shadow of chunk i beside the copy of chunk i+1
    // End of the newest call on the handle: ONE event per call, recorded on the call's stream on every way out (record_done).
    // It orders the next call on another stream behind this one, it is what mvfgpu_last_timing and the host-buffer calls wait
    // for, and -- two events used alternately, done_idx the newest -- the repair feedback waits on the same event for the count
    // the search two back posted (until round 7 that search recorded a second event of its own right in front of this one).
    // Where OTHER calls on the handle (a K1 search, a gather) sit between two posting searches, the event a slot remembers has
    // been recorded again by a later call: the poll then waits for that newer call -- the count is still the right one (a later
    // event implies the earlier work), but the host may run one call ahead instead of two searches.
    mutable hipEvent_t ev_done[2] = {nullptr, nullptr};
    mutable uint32_t done_idx = 0;
    mutable hipStream_t last_stream = nullptr;
    mutable bool has_done = false;
    mutable uint32_t search_launches = 0;  // kernel launches of the newest search (mvfgpu_timing::search_launches; SearchCall counts them)
    mutable mvf::PinnedUpload write_up;    // the positions of a device row write on their way to the device (update.hip)

    bool profiling = false;
    int scan_path = 0;
    int maxsim_route = 0;  // mvfgpu_set_maxsim_route; 0: tune.maxsim_route
    mvf::Tuning tune;  // the environment's tuning switches as they were when the handle was created
    struct ProfSlot {
        hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // [0,1] the timed scan launch, [2] end of its select; [3,4] the whole search
        bool scanned = false, whole = false;
        // The K1 routes record no events: five markers in the stream cost a one-query search 18 us (profiles/r07_stream_fixed_cost.txt).
        // Their kernels read the device's wall clock themselves (ScanParams::ts, SelectParams::ts_*) into entry `slot` of prof_ts:
        // [0] first block of the scan to start, [1] last to finish, [2] end of the select behind it, [3] end of the search's last kernel
        bool ts_scan = false, ts_whole = false;
    };
    mutable DevBuf prof_ts;              // [kProfSlots][4] published times, then the pair the scan writes (block 0's start; the maximum of the blocks' ends, 0 when armed)
    double wall_khz = 100000.0;           // ticks of the device's wall clock per millisecond
    static constexpr int kProfSlots = 64;
    mutable ProfSlot prof[kProfSlots];
    mutable uint64_t prof_next = 0;  // searches profiled since profiling was switched on
    mutable mvfgpu_timing timing{};
};

namespace {

// Lanes per row for K1, from the measured sweep of every data type over 64 <= dim <= 2048 at every width the kernel has
// (profiles/r02_k1_shape_sweep.csv, scripts/sweep_k1_shapes.py) and the full-size check of the benchmark shapes
// (profiles/r02_k1_group_full_size.txt).  V = 16-byte vectors per row.
//   V <= 2 (rows <= 32 B): one lane per row; V <= 8 (<= 128 B): 4 lanes; up to 3 KiB rows: 16 lanes -- the widest group
//   is NOT the fastest there (a 2-KiB Float16 row: 6.7 vs 6.3 TB/s; 768-B Int8 rows: 6.6 vs 3.9 TB/s: with 64 lanes on a
//   short row most of the wave idles in the row's last step); 64 lanes from 3 KiB on (10M x 768 f32: 6.9 vs 6.6 TB/s).
//   Four queries per pass (NQ = 4) carry 16 sums per lane group: 16 lanes stay ahead up to 8 KiB rows.
// round 1 picked "the widest group within 80 % of the best lane utilisation": up to 46 % off the best width on the
// shapes it had not been measured on (dim 100 / 200 f32, 512 f16, 384 / 1024 int8).  MVF_K1_G forces a width (sweeps).
void choose_group(uint32_t V, int nqv, int* G_out, uint32_t* J_out, int forced = 0) {
    // round 3: 5..8 vectors (65..128 B) take 8 lanes -- with 4 a row took two steps and every 128-byte line two separate
    // wave-loads.
    int g = V <= 1 ? 1 : V <= 4 ? 4 : V <= 8 ? 8 : (V < 192 || (nqv == 4 && V < 512)) ? 16 : 64;
    // Rows that are not a multiple of 128 B (V % 8 != 0) start in the middle of a cache line: a 16-lane group's load is four
    // separate unaligned spans and the ragged last step idles most lanes (4.0-4.5 TB/s for every such V from 17 up,
    // profiles/r03_k1_vectors_per_row.csv).  The widest group whose ONE load covers whole adjacent rows is better there:
    // 64 lanes from 33 vectors on (800-B rows 4.2 -> 5.1 TB/s, 1600-B 4.8 -> 5.6), 32 lanes for 17..31 (two adjacent rows
    // per wave-load); 32-B rows take 4 lanes, half of them idle, instead of one lane per row (3.4 -> 4.6 TB/s).
    if (nqv == 1 && V % 8 != 0 && V > 16 && V < 192) g = V > 32 ? 64 : 32;
    if (forced) g = forced;  // MVF_K1_G (sweeps)
    *G_out = g;
    *J_out = (V + g - 1) / g;
}

int init_common(mvfgpu_corpus* c) {
    c->tune = mvf::read_tuning();
    hipDeviceProp_t prop;
    MVF_HIP_TRY(hipGetDeviceProperties(&prop, c->device));
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    MVF_HIP_TRY(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    for (auto& e : c->ev_done) MVF_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) == hipSuccess && khz > 0) c->wall_khz = (double)khz;
    else (void)hipGetLastError();
    return MVF_OK;
}

int validate_shape(uint64_t n, uint32_t dim, uint8_t dtype) {
    if (elem_size(dtype) == 0)
        return fail(MVF_ERR_BUILD, "Unsupported vector data type");  // reference src/vectors/vector_space.rs:126
    if (dim == 0) return fail(MVF_ERR_INVALID_ARGUMENT, "dimension must be > 0");
    if (is_int_dtype(dtype) && dim > MVFGPU_MAX_INT_DIM)
        return fail(MVF_ERR_BUILD, "Int8/UInt8 dimension exceeds the exact-i32 bound (33025)");
    if ((uint64_t)dim * elem_size(dtype) > (1ull << 30)) return fail(MVF_ERR_INVALID_ARGUMENT, "a row holds at most 1 GiB");
    // local row numbers are u32, and the streaming kernel rounds the last chunk up (by < 2^16 rows) before it masks
    if (n > 0xFFFF0000ull) return fail(MVF_ERR_INVALID_ARGUMENT, "a shard holds at most 2^32-65536 rows");
    return MVF_OK;
}

int alloc_rows(mvfgpu_corpus* c) {
    c->pitch = (c->dim * elem_size(c->dtype) + 15u) & ~15u;
    c->V = c->pitch / 16;
    choose_group(c->V, 1, &c->G, &c->J, c->tune.k1_g);
    c->rows_bytes = (size_t)c->n * c->pitch;
    if (c->rows_bytes) MVF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->d_rows), c->rows_bytes));
    MVF_HIP_TRY(poison_fill(c->d_rows, c->rows_bytes));  // the upload and repack_rows write every byte, the pitch padding included
    return MVF_OK;
}

// K1: a piece's survivors up to this many join the running list by counting, more go through the sort network (<= 256;
// 128 until the counting loops got eight reads in flight: profiles/r04_k1_merge_ab.txt)
constexpr uint32_t kK1RankMerge = 256;

// One search: what was asked, how, and what it has launched so far.  Lives on the stack of search_device /
// search_positions_locked and travels down the routes by reference; nothing of it outlasts the search.
struct SearchCall {
    // the request
    uint8_t metric;
    const void* d_queries;
    uint32_t nq, k;
    float* d_scores;
    uint64_t* d_indices;
    int32_t* d_raw;
    hipStream_t stream;
    // how
    HostFlagReq* flag_req = nullptr;  // the host-buffer call's request to this search (NULL = none)
    bool positions_only = false;      // report index_base + row even where vector ids are attached (the join's searches)
    bool shared_call = false;         // the enclosing call may hold more searches than this one (the windows of a join)
    bool whole_by_clock = false;      // a profiled search that takes its whole-search time from prof_ts, not from events
    // kernel launches made so far (mvfgpu_timing::search_launches), counted by the routes that know their launches: K1 on the
    // stored rows or a shadow, the margin select, the K1-order re-scoring, the repair
    uint32_t launches = 0;
    bool launches_known = true;
    // the rows the scans skip: the handle's deletion bitmap, or -- a filtered search (filter.hip) -- a filter's deny mask in the
    // same layout (its tombstones included).  Set by new_search_call.
    const uint32_t* deny = nullptr;
};

SearchCall new_search_call(const mvfgpu_corpus* c, uint8_t metric, const void* d_queries, uint32_t nq, uint32_t k, float* d_scores,
                           uint64_t* d_indices, int32_t* d_raw, hipStream_t s, const uint32_t* filter_deny = nullptr) {
    SearchCall sc{metric, d_queries, nq, k, d_scores, d_indices, d_raw, s};
    sc.deny = filter_deny ? filter_deny : static_cast<const uint32_t*>(c->tomb.p);
    return sc;
}

// A filtered search: its repairs describe the filter, not the corpus -- it neither polls nor posts the repair feedback.
bool is_filtered(const mvfgpu_corpus* c, const SearchCall& sc) { return sc.deny != static_cast<const uint32_t*>(c->tomb.p); }

// A search inside `sc` for another k into other buffers (a shadow route's selection, a pass of a large k, one of two row
// ranges): `route` runs on a copy changed so, and what it launches counts for `sc`.
template <class Route>
int inner_search(SearchCall& sc, uint32_t k, float* d_scores, uint64_t* d_indices, int32_t* d_raw, Route route) {
    SearchCall in = sc;
    in.k = k;
    in.d_scores = d_scores;
    in.d_indices = d_indices;
    in.d_raw = d_raw;
    const int rc = route(in);
    sc.launches = in.launches;
    sc.launches_known = in.launches_known;
    return rc;
}

// the id table the final kernels of a search map local rows through (NULL = index_base + row)
const uint64_t* result_ids(const mvfgpu_corpus* c, const SearchCall& sc) {
    return sc.positions_only ? nullptr : static_cast<const uint64_t*>(c->ids.p);
}

// Where a search's results go and in what form: the fields SelectParams, CompactParams and RescoreParams share.
template <class P>
void set_result_format(P& p, const mvfgpu_corpus* c, const SearchCall& sc) {
    p.k = sc.k;
    p.dtype = c->dtype;
    p.index_base = c->index_base;
    p.ids = result_ids(c, sc);
    p.out_scores = sc.d_scores;
    p.out_indices = sc.d_indices;
    p.out_raw = sc.d_raw;
}

hipError_t scan_launch(uint8_t dtype, const ScanParams& p, int metric, int G, int nqv, dim3 grid, size_t lds,
                       hipStream_t s) {
    switch (dtype) {
    case MVF_DTYPE_FLOAT32: return scan_stream_launch_dt0(p, metric, G, nqv, grid, lds, s);
    case MVF_DTYPE_FLOAT16: return scan_stream_launch_dt1(p, metric, G, nqv, grid, lds, s);
    case MVF_DTYPE_INT8: return scan_stream_launch_dt2(p, metric, G, nqv, grid, lds, s);
    default: return scan_stream_launch_dt3(p, metric, G, nqv, grid, lds, s);
    }
}

const void* scan_kernel(uint8_t dtype, int metric, int G, int nqv, bool redo = false, bool floor = false) {
    switch (dtype) {
    case MVF_DTYPE_FLOAT32: return scan_stream_kernel_ptr_dt0(metric, G, nqv, redo, floor);
    case MVF_DTYPE_FLOAT16: return scan_stream_kernel_ptr_dt1(metric, G, nqv, redo, floor);
    case MVF_DTYPE_INT8: return scan_stream_kernel_ptr_dt2(metric, G, nqv, redo, floor);
    default: return scan_stream_kernel_ptr_dt3(metric, G, nqv, redo, floor);
    }
}

// The shape of a pass of K1 (k1_pass_shape, internal.h) with `queries` queries left at list length k over rows of V vectors
// of type `dtype`: the STORED rows unless the caller names a shadow's.
K1Shape k1_shape(const mvfgpu_corpus* c, uint32_t queries, uint32_t k, uint32_t V, uint8_t dtype) {
    return k1_pass_shape(V, queries, k, c->tune.k1_g,
                         [dtype](int G, uint32_t J, int nqv, uint32_t pmax) { return scan_lds_bytes(dtype, G, J, nqv, pmax); });
}
K1Shape k1_shape(const mvfgpu_corpus* c, uint32_t queries, uint32_t k) { return k1_shape(c, queries, k, c->V, c->dtype); }
// ... of the pass over the 6-bit shadow (scan_stream.inc, S6): one query, one lane per row, a step per 64-element unit
// (p51: the 5+1 unit -- `units` of 128 elements; the chunks are those of the 6-bit unit over the same rows)
K1Shape k1_shape_6b(uint32_t units, uint32_t k, bool p51 = false) {
    K1Shape sh;
    sh.nqv = 1;
    sh.G = 1;
    sh.J = units;
    sh.chunk_rows = scan_chunk_rows(1, p51 ? 2u * units : units, 1);
    sh.pmax = next_pow2(k + scan_chunk_safe(1));
    sh.lds = p51 ? scan_lds_bytes_51(units, sh.pmax) : scan_lds_bytes_6b(units, sh.pmax);
    return sh;
}
constexpr uint32_t kPub51Blocks = 4096;  // blocks of a 5+1 scan the handle keeps words for (8 resident blocks on each of 512 CUs)
int k1_shape_fits(const K1Shape& sh) {
    if (sh.lds > 160 * 1024) return fail(MVF_ERR_BUILD, "dimension too large for the streaming kernel's LDS query tile");
    return MVF_OK;
}

// K1's parameters for a pass of shape `sh` over the STORED rows (a shadow route overrides the rows), `nchunks` chunks of
// sh.chunk_rows rows, the blocks' lists going to `cand`.
ScanParams stored_scan_params(const mvfgpu_corpus* c, const SearchCall& sc, const K1Shape& sh, uint32_t nchunks, uint64_t* cand) {
    ScanParams sp{};
    sp.rows = c->d_rows;
    sp.queries = sc.d_queries;
    sp.tomb = sc.deny;
    sp.cand = cand;
    sp.n = (uint32_t)c->n;
    sp.pitch = c->pitch;
    sp.dim = c->dim;
    sp.V = c->V;
    sp.J = sh.J;
    sp.nq_total = sc.nq;
    sp.k = sc.k;
    sp.kcap = next_pow2(sc.k);
    sp.pmax = sh.pmax;
    sp.chunk_rows = sh.chunk_rows;
    sp.chunk_safe = std::min(scan_chunk_safe(sh.G), sh.chunk_rows);
    {
        const uint32_t step = 16u * 64u / (uint32_t)sh.G, want = std::max(sc.k, 64u);
        // (not under the long chunks of short rows: a threshold from 128 rows lets too many of the next 4000 through --
        // 4 GB of <= 128-byte rows at k = 100 lost 5-8 %, profiles/r04_k1_first_piece_ab.txt)
        sp.first_piece = sh.chunk_rows <= scan_chunk_safe(sh.G) ? std::min(sp.chunk_safe, (want + step - 1) / step * step) : sp.chunk_safe;
    }
    sp.nchunks = nchunks;
    sp.rank_merge_max = kK1RankMerge;
    return sp;
}

// select_final's parameters behind such a pass: `nlists` lists per query at `lists`, merged and formatted as the search asks
SelectParams final_select_params(const mvfgpu_corpus* c, const SearchCall& sc, const uint64_t* lists, uint32_t nlists) {
    SelectParams fp{};
    fp.lists = lists;
    fp.nlists = nlists;
    fp.kcap = next_pow2(sc.k);
    fp.heads = nlists ? (sc.k + nlists - 1) / nlists : 1;
    fp.P = 4096;  // 32 KiB of LDS: >= k + kcap (fold path) and >= nlists*heads (nlists <= 2048)
    fp.metric = sc.metric;
    set_result_format(fp, c, sc);
    return fp;
}

// Streaming over the scaled-f16 shadow of a Float32 corpus (scan path 4): K1 reads the shadow rows instead of the stored
// ones and hands the k best COMPOSITES per query to the margin compaction instead of formatting results.
// Buffers of the whole-shard sort (search_sorted_k): a / b hold `nqv` x n composites each, tmp the sort's scratch.
struct RankAll {
    uint64_t *a, *b;
    void* tmp;
    size_t tmp_bytes;
    int nqv;         // queries per dump pass the buffers hold: 4 or 1
    uint32_t k_out;  // the caller's k
};

struct ShadowStream {
    const unsigned char* rows;
    const float* xscale;
    // int8 shadow (dt2x unit) only: K1's prologue quantises the f32 queries itself and leaves their scale / norm / bound in
    // qaux0 / qaux1 / delta (qstats, xxmax: what the bound is made of); xrow: the rows' norm array
    bool i8;
    bool s6;  // ... in 6-bit tiles (dt2y unit: pitch = a tile's bytes, V = the units per row)
    bool p51; // ... held in the 5+1 layout (dt2z unit: 128-element units)
    float *qaux0, *qaux1;
    const float *qstats, *xxmax, *xrow;
    // ... and select_final's margin mode instead of the k best: every row within 2 delta[q] of the rank_k-th best
    float* delta;
    uint32_t *tau, *overflow;
    uint32_t rank_k;
    uint32_t pitch, V, J;
    int G;
    uint64_t* cand;   // [nq][cand_cap]
    uint32_t* cnt;    // [nq]
    uint32_t cand_cap;
};

// Blocks per CU of a streaming-kernel instantiation at a dynamic-LDS size: asked once per (kernel, LDS bytes) and handle -- the
// runtime's answer costs 1-2 us and sits in front of the first launch of every search (a 10k-row search is 25 us in all).
int scan_occupancy(const mvfgpu_corpus* c, const void* kfn, size_t lds, int* occ_out) {
    const uint64_t key = (uint64_t)(reinterpret_cast<uintptr_t>(kfn)) * 0x9E3779B97F4A7C15ull ^ (uint64_t)lds;
    for (const auto& e : c->occ_cache)
        if (e.first == key) {
            *occ_out = e.second;
            return MVF_OK;
        }
    // the attribute is only ever RAISED: to the part's ceiling, once per kernel and handle (set to this miss's size, a later hit at a
    // larger size the cache already knew would launch above it -- a runtime that enforces the attribute would refuse the launch)
    if (lds > 48 * 1024) MVF_HIP_TRY(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    int occ = 0;
    MVF_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kfn, 256, lds));
    if (occ < 1) occ = 1;
    if (c->occ_cache.size() < 64) c->occ_cache.emplace_back(key, occ);
    *occ_out = occ;
    return MVF_OK;
}


// The clock entries of the profiled K1 routes (ProfSlot): allocated and armed by the first profiled search.
int prof_ts_ensure(const mvfgpu_corpus* c, hipStream_t s) {
    if (c->prof_ts.p) return MVF_OK;
    const size_t words = (size_t)mvfgpu_corpus::kProfSlots * 4 + 2;
    MVF_HIP_TRY(c->prof_ts.reserve(words * 8));
    MVF_HIP_TRY(hipMemsetAsync(c->prof_ts.p, 0, words * 8, s));
    MVF_HIP_TRY(hipMemsetAsync(static_cast<uint64_t*>(c->prof_ts.p) + words - 2, 0xFF, 8, s));
    return MVF_OK;
}
uint64_t* prof_ts_entry(const mvfgpu_corpus* c, uint64_t search) {
    return static_cast<uint64_t*>(c->prof_ts.p) + (search % mvfgpu_corpus::kProfSlots) * 4;
}
uint64_t* prof_ts_work(const mvfgpu_corpus* c) { return static_cast<uint64_t*>(c->prof_ts.p) + (size_t)mvfgpu_corpus::kProfSlots * 4; }

int search_stream_path(const mvfgpu_corpus* c, SearchCall& sc, bool profile = true, const ShadowStream* alt = nullptr,
                       const uint64_t* floor1 = nullptr, uint64_t* out_floor1 = nullptr, uint32_t out_stride = 0,
                       uint32_t out_offset = 0, const RankAll* rank = nullptr) {
    // floor1 / out_floor1 / out_stride / out_offset: one pass of a k > MVFGPU_K_PER_PASS search (search_large_k)
    // rank: the whole-shard sort (search_sorted_k) -- the scan DUMPS every row's composite, the selection kernel is replaced
    // by a device-wide sort of each query's n composites + the formatting of its first k_out; `k` is then only the (small)
    // list length the kernel's LDS layout is sized for
    const uint8_t metric = sc.metric;
    const uint32_t nq = sc.nq, k = sc.k;
    hipStream_t s = sc.stream;
    const uint32_t kcap = next_pow2(k);
    const uint32_t ostride = out_stride ? out_stride : k;
    const bool alt8 = alt && alt->i8, alt6 = alt8 && alt->s6, alt51 = alt6 && alt->p51;
    const uint8_t kdtype = alt8 ? (uint8_t)MVF_DTYPE_INT8 : alt ? (uint8_t)MVF_DTYPE_FLOAT16 : c->dtype;
    const uint32_t kV = alt ? alt->V : c->V;

    mvfgpu_timing tm{};
    tm.scan_kernel = alt8 ? 7u : alt ? 5u : 1u;
    bool first = true;
    mvfgpu_corpus::ProfSlot* ps = nullptr;
    uint64_t *ts_work = nullptr, *ts_entry = nullptr;
    if (c->profiling && profile) {
        ps = &c->prof[c->prof_next % mvfgpu_corpus::kProfSlots];
        for (auto& e : ps->e)
            if (!e) MVF_HIP_TRY(hipEventCreate(&e));
        ps->scanned = false;
        ps->ts_scan = false;
        if (!rank) {  // a select_final follows the scan: the pair times itself
            const int trc = prof_ts_ensure(c, s);
            if (trc != MVF_OK) return trc;
            ts_work = prof_ts_work(c);
            ts_entry = prof_ts_entry(c, c->prof_next);
        }
    }

    for (uint32_t q0 = 0; q0 < nq;) {
        // (the f16 shadow's unit and a one-query dump take one query per pass)
        K1Shape sh = alt6 ? k1_shape_6b(kV, k, alt51) : k1_shape(c, (!alt || alt8) && !(rank && rank->nqv == 1) ? nq - q0 : 1u, k, kV, kdtype);
        const int G = sh.G, nqv = sh.nqv;
        const size_t lds = sh.lds;
        uint32_t& chunk_rows = sh.chunk_rows;  // (the small-corpus rule below may shorten it)
        uint32_t nchunks = (uint32_t)((c->n + chunk_rows - 1) / chunk_rows);
        if (const int frc = k1_shape_fits(sh)) return frc;
        uint32_t nq_here = std::min<uint32_t>(nqv, nq - q0);
        uint32_t npass = 1;  // passes of nqv queries in this launch (grid.y)

        uint32_t nblocks = 0;
        if (nchunks > 0) {
            const void* kfn = alt51 ? scan_stream_kernel_ptr_dt2z(metric, G, nqv)
                              : alt6  ? scan_stream_kernel_ptr_dt2y(metric, G, nqv)
                              : alt8  ? scan_stream_kernel_ptr_dt2x(metric, G, nqv)
                              : alt ? scan_stream_kernel_ptr_dt1x(metric, G, nqv)
                                    : scan_kernel(c->dtype, metric, G, nqv, /*redo=*/false, floor1 != nullptr || rank != nullptr);
            int occ = 1;
            {
                const int orc = scan_occupancy(c, kfn, lds, &occ);
                if (orc != MVF_OK) return orc;
            }
            {  // A corpus of fewer 512-row chunks than the GPU holds blocks (n < ~650K rows) would leave most of them idle:
               // smaller chunks, one per resident block -- n / blocks rounded up to the kernel's step (100K x 128 f32: 196
               // blocks -> 782, 52 -> 31 us per search).  Up to four chunks per block the last round is uneven (700K x 256:
               // 1368 chunks on 1280 blocks, i.e. two rounds for 7 % of the blocks): P = ceil(chunks / blocks) rounds of
               // equal, smaller chunks instead (181 -> 144 us; 1M..3M rows: 1-5 %).  Larger corpora keep the 512-row chunks
               // (the headline's 496-row "balanced" chunks measured 1.4 % slower than 512); the long chunks of short rows
               // (scan_chunk_rows) are few per block and stay balanced up to 16 rounds.
                const uint32_t slots = (uint32_t)occ * (uint32_t)c->num_cus, step = 16u * 64u / (uint32_t)G;
                if (nchunks >= slots && nchunks < (chunk_rows > scan_chunk_safe(G) ? 16u : 4u) * slots) {
                    const uint32_t P = (nchunks + slots - 1) / slots;
                    const uint64_t per = (c->n + (uint64_t)P * slots - 1) / ((uint64_t)P * slots);
                    const uint32_t cr = (uint32_t)((per + step - 1) / step * step);
                    if (cr >= step && cr < chunk_rows) {
                        chunk_rows = cr;
                        nchunks = (uint32_t)((c->n + chunk_rows - 1) / chunk_rows);
                    }
                }
                if (nchunks < slots) {
                    const uint64_t per = (c->n + slots - 1) / slots;
                    const uint32_t cr = (uint32_t)((per + step - 1) / step * step);
                    if (cr >= step && cr < chunk_rows) {
                        chunk_rows = cr;
                        nchunks = (uint32_t)((c->n + chunk_rows - 1) / chunk_rows);
                    }
                }
            }
            nblocks = std::min<uint32_t>(nchunks, (uint32_t)occ * (uint32_t)c->num_cus);
            // A corpus that leaves most of the GPU idle (one small chunk per block and blocks to spare) takes ALL its four-query
            // passes in one launch, pass = blockIdx.y: the passes of a small batch were launch pairs in a row, ~40 us each
            // (10k x 128 f32, 16 queries: 165 -> 50 us; profiles/r04_host_api_latency.txt).  Up to 8 passes = every batch the
            // small-corpus rule of use_batched_path leaves to this kernel.
            if (nqv == 4 && !alt && !floor1 && !rank && nblocks == nchunks && 2u * nblocks <= (uint32_t)occ * (uint32_t)c->num_cus) {
                npass = std::min<uint32_t>(8u, (nq - q0 + 3u) / 4u);
                nq_here = std::min<uint32_t>(npass * 4u, nq - q0);
            }
            MVF_HIP_TRY(c->cand.reserve((size_t)npass * nqv * nblocks * kcap * 8));

            ScanParams sp = stored_scan_params(c, sc, sh, nchunks, static_cast<uint64_t*>(c->cand.p));
            if (alt) {  // the shadow's rows instead
                sp.rows = alt->rows;
                sp.xscale = alt->xscale;
                sp.pitch = alt->pitch;
                sp.V = alt->V;
            }
            if (alt8) {
                sp.qaux0 = alt->qaux0;
                sp.qaux1 = alt->qaux1;
                sp.qdelta = alt->delta;
                sp.qstats = alt->qstats;
                sp.xxmax = alt->xxmax;
                sp.xrow = alt->xrow;
            }
            sp.q0 = q0;
            sp.floor1 = floor1;
            sp.dump = rank ? rank->a : nullptr;
            if (ps && first && ts_work) sp.ts = ts_work;
            else if (ps && first) MVF_HIP_TRY(hipEventRecord(ps->e[0], s));
            if (alt6) c->pub51_blocks = 0;
            if (alt51) {  // the blocks' published bests and low-plane counters, under a sequence number of this search's own
                if (nblocks > kPub51Blocks) return fail(MVF_ERR_BUILD, "more scan blocks than the 5+1 stream's per-block words");
                if (!c->pub51.p) {
                    MVF_HIP_TRY(c->pub51.reserve((size_t)kPub51Blocks * 24));
                    MVF_HIP_TRY(hipMemsetAsync(c->pub51.p, 0, (size_t)kPub51Blocks * 24, s));
                    c->pub51_seq = 0;
                }
                if (++c->pub51_seq == 0) c->pub51_seq = 1;  // (0 is what the zeroed words carry)
                sp.pub = static_cast<uint64_t*>(c->pub51.p);
                sp.lo_stats = reinterpret_cast<uint32_t*>(sp.pub + kPub51Blocks);
                sp.pub_seq = c->pub51_seq;
                sp.skip_rank = alt->rank_k;
                // half a safe piece (one iteration of the block's four waves) while a block has neither threshold: its best is
                // published, and the others' are read, 512 rows sooner (>= the longest list of the route, 204 entries)
                sp.first_piece = std::min(sp.first_piece, 512u);
                c->pub51_blocks = nblocks;
                MVF_HIP_TRY(scan_stream_launch_dt2z(sp, metric, G, nqv, dim3(nblocks), lds, s));
            } else if (alt6) MVF_HIP_TRY(scan_stream_launch_dt2y(sp, metric, G, nqv, dim3(nblocks), lds, s));
            else if (alt8) MVF_HIP_TRY(scan_stream_launch_dt2x(sp, metric, G, nqv, dim3(nblocks), lds, s));
            else if (alt) MVF_HIP_TRY(scan_stream_launch_dt1x(sp, metric, G, nqv, dim3(nblocks), lds, s));
            else MVF_HIP_TRY(scan_launch(c->dtype, sp, metric, G, nqv, dim3(nblocks, npass), lds, s));
            if (ps && first) {
                if (!ts_work) MVF_HIP_TRY(hipEventRecord(ps->e[1], s));
                ps->scanned = true;
                ps->ts_scan = ts_work != nullptr;
                // (5+1: the layout's bytes, hi and lo planes -- the 6-bit layout's figure; what the scan fetched of the lo planes:
                // mvfgpu_debug_stream_lo_lines)
                tm.scan_bytes = alt51 ? (uint64_t)s51_bytes(c->n, c->dim) : alt6 ? (uint64_t)s6_bytes(c->n, c->dim) : (uint64_t)c->n * c->dim * elem_size(kdtype);
                tm.scan_flops = 2ull * nq_here * c->n * c->dim;
                if (npass > 1) tm.scan_bytes *= npass;
            }
            tm.scan_launches++;
            sc.launches++;
        }
        if (rank) {  // every row of these queries is ranked: sort each query's n composites, format the first k_out
            SelectParams fp{};
            fp.metric = metric;
            set_result_format(fp, c, sc);
            fp.k = rank->k_out;
            uint64_t* sorted = rank->a;
            if (c->n > 0) {  // the pass's queries in one set of launches
                size_t tb = rank->tmp_bytes;
                MVF_HIP_TRY(sort_composites(rank->tmp, &tb, rank->a, rank->b, (size_t)c->n, (size_t)rank->k_out, &sorted, s, nq_here, (size_t)c->n));
            }
            for (uint32_t q = 0; q < nq_here; q++)
                MVF_HIP_TRY(launch_write_sorted(fp, sorted + (size_t)q * c->n, (uint32_t)c->n, (size_t)(q0 + q) * rank->k_out, s));
            sc.launches_known = false;  // (the device-wide sort's launches are its own business)
        } else {
            SelectParams fp = final_select_params(c, sc, static_cast<const uint64_t*>(c->cand.p), nblocks);
            if (alt) {
                fp.out_cand = alt->cand + (size_t)q0 * alt->cand_cap;
                fp.out_cnt = alt->cnt + q0;
                fp.cand_cap = alt->cand_cap;
                if (alt8) {
                    fp.delta = alt->delta + q0;
                    fp.out_tau = alt->tau + q0;
                    fp.out_overflow = alt->overflow + q0;
                    fp.keep_cap = alt->cand_cap / 2;
                    fp.margin_rank = alt->rank_k;
                }
            } else {
                fp.out_scores = sc.d_scores + (size_t)q0 * ostride;
                fp.out_indices = sc.d_indices + (size_t)q0 * ostride;
                fp.out_raw = sc.d_raw ? sc.d_raw + (size_t)q0 * ostride : nullptr;
                fp.out_stride = out_stride;
                fp.out_offset = out_offset;
                fp.out_floor1 = out_floor1 ? out_floor1 + q0 : nullptr;
                HostFlagReq* req = out_floor1 ? nullptr : sc.flag_req;
                if (req && req->gather_out && !c->ids.p) {  // payload rows behind the results, by the same block
                    fp.gather_rows = c->d_rows;
                    fp.gather_out = req->gather_out + (size_t)q0 * ostride * (c->dim * elem_size(c->dtype));
                    fp.gather_pitch = c->pitch;
                    fp.gather_row_bytes = c->dim * elem_size(c->dtype);
                    if (q0 + nq_here == nq) req->gathered = true;
                }
                if (req && q0 + nq_here == nq) {  // the search's last kernel
                    fp.done_flag = req->flag;
                    fp.done_ticket = req->ticket;
                    fp.done_seq = req->seq;
                    req->armed = true;
                }
            }
            if (ps && first && ps->ts_scan) {
                fp.ts_work = ts_work;
                fp.ts_out = ts_entry;
            }
            if (ps && ts_entry && sc.whole_by_clock && !alt && q0 + nq_here == nq) fp.ts_end = ts_entry + 3;  // the search's last kernel
            MVF_HIP_TRY(launch_select_final(fp, nq_here, s));
            sc.launches++;
        }
        if (ps && first && !ps->ts_scan) MVF_HIP_TRY(hipEventRecord(ps->e[2], s));
        first = false;
        q0 += nq_here;
    }
    if (ps) {
        c->timing = tm;  // event times are read back lazily by mvfgpu_last_timing
        c->prof_next++;
    }
    return MVF_OK;
}


// 256-query tile on Float16 rows / the f16 shadow: the ping-pong schedule (scan_mfma16_pp.hip) or the lockstep LDS-DMA
// kernel.  Measured (MI355X, profiles/r02_k2_ab.txt): 5 % faster on the ping-pong kernel once a block walks several
// tiles (cfg5 last phase 20.7 -> 19.7 ms), short phases a few percent slower (its longer prologue); Int8 rows were slower
// on it as well (cfg4 6.94 vs 7.02 ms) and have no ping-pong kernel.  MVF_K2_PP=0|1 forces one of them on Float16 tiles.
bool k2_pp_wanted(const mvfgpu_corpus* c, uint8_t kdtype, uint32_t ntiles, uint32_t mtiles, int num_cus) {
    if (kdtype != MVF_DTYPE_FLOAT16) return false;
    if (c->tune.k2_pp >= 0) return c->tune.k2_pp != 0;
    return (uint64_t)ntiles * mtiles >= 8ull * (uint64_t)num_cus;
}

// Largest phase-to-phase growth of the K2 scan (MVF_K2_GROWTH overrides, for A/B runs).  A phase lets through
// ~k (g - 1) candidates per query (its threshold is the k-th best of 1/g of the rows it sees); with 1024 queries that is
// several per 256 x 256 tile at g = 8, and every candidate sends its wave through the epilogue's second stage.  g = 4
// costs one or two more (small) launches and measured 2-3 % faster on cfg3 / cfg5 / cfg4 (profiles/r02_k2_ab.txt); g = 16
// and 32 were 4 % slower in round 1.
// Batches of up to 128 queries (round 5, one process, the switch toggled between rounds -- profiles/r05_k2_walk_and_phase_costs.txt 8d): their
// scans are HBM-bound and their small kernels pure latency, so a phase less is worth more than its records cost: g = 6 is 2-4 % faster than
// 4 on 1M-3M rows, 0.6-1.5 % on 10M (g = 8 the same or a little more; 6 keeps a phase's records near half of the list capacity); 128 queries
// -4 % on 3M and 10M rows; 256 queries -2.4 % / -0.9 % / +1.4 % on three shapes, 384 and more: 4 wins.
// Only where a phase's records stay near half of the list capacity: with the int8 selection's margin a phase files about
// 7 k (g - 1) records per query (measured: 1800 at k = 100, g = 4), so g <= 1 + cap / (14 k) -- k <= 117 for g = 6 on 8192 slots.
uint32_t k2_growth_for(const Tuning& t, uint32_t nq, uint32_t k, uint32_t cap) {
    uint32_t g = std::min(t.k2_growth, std::max(2u, cap / (2u * k)));
    if (nq <= 128u) g = std::max(g, std::min(t.k2_growth_small, 1u + cap / (14u * k)));
    return g;
}
uint32_t k2_growth_for(const mvfgpu_corpus* c, uint32_t nq, uint32_t k, uint32_t cap) { return k2_growth_for(c->tune, nq, k, cap); }

// The phase boundaries R_1 .. R_{P+1} = nr of a batched search over nr rows (a pure function: mvfgpu_selftest_schedule pins it
// without a GPU).  Phase 0 passes everything (no threshold yet: R_1 <= cap rows, stored by row offset), later phases grow by g:
// expected survivors per query k (g - 1) + k carried <= cap / 2.  The boundaries are laid out BACKWARDS from the range's end --
// R_j = nr / g^(P - j), P the fewest steps that bring R_1 under cap -- so every phase, the last one included, scans (g - 1)
// times what its threshold has seen, and the last phase is always the largest ((1 - 1/g) of the rows: the launch bench.py times
// and prices).  Round 1 grew forwards from cap rows, which left a small odd phase at the end (and the one before it carrying
// most of the corpus).
std::vector<uint64_t> k2_phase_bounds(uint64_t nr, uint32_t cap, uint32_t g) {
    std::vector<uint64_t> bounds;
    uint32_t P = 0;
    for (uint64_t f = nr; f > cap; f = (f + g - 1) / g) P++;
    for (uint32_t j = 0; j <= P; j++) {
        uint64_t div = 1;
        for (uint32_t i = j; i < P; i++) div *= g;
        uint64_t e = (nr + div - 1) / div;
        e = std::min<uint64_t>(nr, (e + 255) / 256 * 256);
        if (j == 0) e = std::min<uint64_t>(e, cap);  // the direct phase's slots are row offsets
        if (bounds.empty() || e > bounds.back()) bounds.push_back(e);
    }
    if (bounds.empty() || bounds.back() < nr) bounds.push_back(nr);
    return bounds;
}

// The folded pre-filter of the LDS-DMA kernel's i32-accumulator flavours (scan_mfma16_bias.inc); MVF_K2_BIAS=0 keeps
// round 2's epilogue (A/B runs).
bool k2_bias_enabled(const mvfgpu_corpus* c) { return c->tune.k2_bias; }

// ---- scaled-f16 shadow of a Float32 corpus (selection only) -----------------------------------------------------
uint32_t shadow_pitch(uint32_t dim) { return (dim * 2u + 15u) & ~15u; }

bool shadow_enabled(const mvfgpu_corpus* c) {  // MVF_F16_SHADOW=0 keeps Float32 corpora on the exact f32 MFMA kernel (scan path 3 overrides)
    return c->tune.f16_shadow;
}

// Built on the first search that wants it (like the row norms): +50 % of the corpus' HBM.  Unless the caller insists
// (scan paths 3 and 4) it is skipped when that would leave less than 2 GiB free on the device.
hipError_t ensure_shadow(const mvfgpu_corpus* c, hipStream_t s, bool insist) {
    if (c->shadow_state == -1 && insist) c->shadow_state = 0;  // skipped automatically earlier: try now
    if (c->shadow_state != 0) return hipSuccess;
    const size_t need = (size_t)std::max<uint64_t>(c->n, 1) * shadow_pitch(c->dim);
    if (!insist) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < need + ((size_t)2 << 30)) {
            c->shadow_state = -1;
            return hipSuccess;
        }
    }
    if (c->shadow.reserve(need) != hipSuccess || c->xscale.reserve(((size_t)std::max<uint64_t>(c->n, 1) + 256) * 4) != hipSuccess) {
        (void)hipGetLastError();
        c->shadow.release();
        c->xscale.release();
        c->shadow_state = -1;
        return hipSuccess;
    }
    hipError_t e = launch_shadow_f16(c->d_rows, (uint32_t)c->n, c->pitch, c->dim, static_cast<unsigned char*>(c->shadow.p),
                                     shadow_pitch(c->dim), static_cast<float*>(c->xscale.p), s);
    if (e == hipSuccess) c->shadow_state = 1;
    return e;
}

// ---- int8 shadow of a Float32 / Float16 corpus (selection only; shadow_i8.hip) --------------------------------------
uint32_t shadow8_pitch(uint32_t dim) { return (dim + 15u) & ~15u; }
constexpr uint32_t kBatchCapQS = 8192;  // candidate slots per query with int8 selection (5-8 x k rows ride in the margin)

// Batched searches on Float32 / Float16 rows select on the int8 shadow by default (measured on cfg3 / cfg5 and on 2..512
// queries: 1.3-1.6 x the f16 selection at every batch size, profiles/r02_k2_ab.txt, r02_small_batches_*.txt): twice the
// MFMA rate of the f16 kernel under the same power limit, half (a quarter) of the bytes of Float16 (Float32) rows, a 15 x
// wider proven margin.  MVF_I8_SHADOW=0, scan path 3 (f16 selection) and scan path 2 (stored rows) opt out; scan path 5
// insists; a corpus whose data defeats the int8 bound switches itself back (qs_disabled).
// The int8 bound lets ~7-10 x k rows per query through to the re-scoring (0.23 sigma of the score distribution on the
// benchmark's rows), and a query whose margin holds more than half its candidate slots is redone by K1: beyond these k
// the selection is left to the f16 shadow / the stored rows, whose margins hold a handful of rows beyond k (k = 1000 on
// 10M x 768, 16 queries: 42 ms with every query repaired, 3 ms without).
constexpr uint32_t kQsMaxK = kBatchCapQS / 2 / 10;        // batched: 4096 kept candidates per query
constexpr uint32_t kQsStreamMaxK = kBatchCap / 2 / 10;    // streamed (select_final's margin mode): 2048

// Scan paths 6 and 7 both insist on the streamed int8 shadow for one to four queries (7 sends ONE unfiltered Float32 query over
// the 6-bit shadow instead, while the handle's 6-bit switch is on: stream_6b_wanted)
bool path_streams_i8(const mvfgpu_corpus* c) { return c->scan_path == 6 || c->scan_path == 7; }

// everything but the shadow's own state
bool qs_possible(const mvfgpu_corpus* c, uint32_t k) {
    if (is_int_dtype(c->dtype) || c->n == 0) return false;
    if (k > kQsMaxK) return false;
    if ((size_t)((c->dim + 7u) & ~7u) * 4 + kBatchCapQS * 4 > 64 * 1024) return false;  // re-scoring: query + candidates in LDS
    if (c->scan_path == 5 || path_streams_i8(c)) return true;
    if (c->scan_path != 0 && c->scan_path != 4) return false;
    return !c->qs_disabled && c->tune.i8_shadow;
}

bool qs_wanted(const mvfgpu_corpus* c, uint32_t k = 0) {
    if (!qs_possible(c, k)) return false;
    return c->scan_path == 5 || path_streams_i8(c) || c->shadow8_state >= 0;
}

// The batched path alone can live with a shadow of a PREFIX of the rows (search_batched_path): where all rows did not fit
// (state -1) it still asks, once, for what does.
bool qs_wanted_batched(const mvfgpu_corpus* c, uint32_t k) {
    if (!qs_possible(c, k)) return false;
    return c->scan_path == 5 || path_streams_i8(c) || c->shadow8_state >= 0 || (c->shadow8_state == -1 && c->tune.i8_shadow_partial);
}

// The decision itself, a pure function of the sequence of samples (mvfgpu_selftest_feedback runs it without a GPU).
// A sample = (queries of the search, queries its repair pass redid, whether it ran with the folded pre-filter, whether it
// selected on the int8 shadow).  Running totals (a single streamed query says little by itself), halved now and then so
// that old history fades.  Too many repairs blame the folded pre-filter first (its per-lane bounds), the int8 selection
// second.  A sample of a search that still RAN WITH the pre-filter, consumed after the pre-filter has been switched off
// (two searches are in flight), is dropped: its repairs are the suspect's, and counted against the fresh totals they
// would switch the int8 selection off one search later, for good.
void feedback_consume(uint32_t& seen, uint32_t& redone, bool& bias_disabled, bool& qs_disabled, uint32_t nq, uint32_t redo,
                      bool used_bias, bool used_qs) {
    if (used_bias && bias_disabled) return;
    seen += nq;
    redone += std::min(redo, nq);
    if (redone >= 4 && (uint64_t)redone * 8 > seen) {
        if (used_bias && !bias_disabled) {
            bias_disabled = true;
            seen = redone = 0;
        } else if (used_qs) {
            qs_disabled = true;
        }
    } else if (seen >= 8192) {
        seen /= 2;
        redone /= 2;
    }
}

// The end-of-call event (mvfgpu_corpus::ev_done): the older of the two is recorded and becomes the newest.
void record_done(const mvfgpu_corpus* c, hipStream_t s) {
    const uint32_t i = c->done_idx ^ 1u;
    if (hipEventRecord(c->ev_done[i], s) == hipSuccess) {
        c->done_idx = i;
        c->has_done = true;
        c->last_stream = s;
    } else {
        (void)hipGetLastError();
    }
}

// The discipline of every call that enqueues work of a handle on a caller's stream: under the handle's lock, `s` ordered
// behind the handle's newest work on another stream (the scratch buffers are stream-ordered), and -- whatever `body` returns,
// work may already sit on the stream (norms, a shadow build, scratch) -- ev_done recorded on `s` on every way out, for the
// next call on ANOTHER stream to order itself behind.
template <class Body>
int device_call(const mvfgpu_corpus* c, hipStream_t s, Body&& body) {
    std::lock_guard<std::mutex> lk(c->mu);
    c->work_gen++;
    if (c->has_done && c->last_stream != s) MVF_HIP_TRY(hipStreamWaitEvent(s, c->ev_done[c->done_idx], 0));
    struct DoneGuard {
        const mvfgpu_corpus* c;
        hipStream_t s;
        ~DoneGuard() { record_done(c, s); }
    } done_guard{c, s};
    return body();
}

// What the search before the previous one had to repair (its count was copied to pinned memory behind it; waited for
// here -- by now it is two searches old -- so the decision does not depend on timing).
void qs_feedback_poll(const mvfgpu_corpus* c) {
    const uint32_t sl = c->qs_slot;
    if (!c->qs_redo_pending[sl]) return;
    if (hipEventSynchronize(c->qs_redo_own[sl] ? c->qs_redo_ev[sl] : c->ev_done[c->qs_redo_done[sl]]) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    c->qs_redo_pending[sl] = false;
    if (c->fb_s6[sl]) {  // a 6-bit stream's sample: its own totals, its own switch
        bool no_bias = false;
        const bool was = c->s6_disabled;
        feedback_consume(c->s6_seen, c->s6_redone, no_bias, c->s6_disabled, c->qs_redo_nq[sl], c->qs_redo_host[sl], false, true);
        if (c->tune.debug_repair && was != c->s6_disabled)
            fprintf(stderr, "[mvfgpu] 6-bit shadow stream switched off for this corpus: too many queries needed the repair path\n");
        return;
    }
    const bool bias_was = c->bias_disabled, qs_was = c->qs_disabled;
    feedback_consume(c->qs_seen, c->qs_redone, c->bias_disabled, c->qs_disabled, c->qs_redo_nq[sl], c->qs_redo_host[sl],
                     c->fb_bias[sl], c->fb_qs[sl]);
    if (c->tune.debug_repair && (bias_was != c->bias_disabled || qs_was != c->qs_disabled))
        fprintf(stderr, "[mvfgpu] %s switched off for this corpus: too many queries needed the repair path\n",
                bias_was != c->bias_disabled ? "folded pre-filter" : "int8-shadow selection");
}

int feedback_slots(const mvfgpu_corpus* c) {
    if (c->qs_redo_host) return MVF_OK;
    MVF_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->qs_redo_host), 64, hipHostMallocDefault));
    poison_fill_host(c->qs_redo_host, 64);
    return MVF_OK;
}

// The pinned slot the next post will use, for the repair pass's flag_compact_kernel to store its count into directly (round 5:
// the 4-byte copy behind every batched search was a launch of its own, 4.1 us) -- NULL while that slot still holds a sample
// nobody has consumed (the post will skip it too).
uint32_t* feedback_mirror(const mvfgpu_corpus* c, const SearchCall& sc) {
    c->fb_mirrored = nullptr;
    if (is_filtered(c, sc)) return nullptr;
    if (feedback_slots(c) != MVF_OK || c->qs_redo_pending[c->qs_slot]) return nullptr;
    c->fb_mirrored = c->qs_redo_host + c->qs_slot;
    return c->qs_redo_host + c->qs_slot;
}

// ... and the request for it: the repair count of the search just enqueued, in pinned memory behind the event its call
// records on the way out (record_done) where the call holds this search alone (search_device), behind an event of the
// search's own otherwise (the windows of a join).
int qs_feedback_post(const mvfgpu_corpus* c, const SearchCall& sc, bool used_bias = false, bool used_qs = true, bool used_s6 = false) {
    hipStream_t s = sc.stream;
    const uint32_t sl = c->qs_slot;
    if (is_filtered(c, sc)) return MVF_OK;
    if (c->qs_redo_pending[sl] || !c->repair.p) return MVF_OK;  // (pending: this search did not poll -- it took another path first)
    {
        int rc = feedback_slots(c);
        if (rc != MVF_OK) return rc;
    }
    c->fb_bias[sl] = used_bias;
    c->fb_qs[sl] = used_qs;
    c->fb_s6[sl] = used_s6;
    if (c->fb_mirrored != c->qs_redo_host + sl)  // (the repair pass could not store it there itself)
        MVF_HIP_TRY(hipMemcpyAsync(c->qs_redo_host + sl, c->last_redo_cnt, 4, hipMemcpyDeviceToHost, s));
    c->fb_mirrored = nullptr;
    c->qs_redo_own[sl] = sc.shared_call;
    if (c->qs_redo_own[sl]) {  // more searches follow in this call: the end-of-call event comes too late for their polls
        if (!c->qs_redo_ev[sl]) MVF_HIP_TRY(hipEventCreateWithFlags(&c->qs_redo_ev[sl], hipEventDisableTiming));
        MVF_HIP_TRY(hipEventRecord(c->qs_redo_ev[sl], s));
    } else {
        c->qs_redo_done[sl] = c->done_idx ^ 1u;
    }
    c->qs_redo_pending[sl] = true;
    c->qs_redo_nq[sl] = sc.nq;
    c->qs_slot = sl ^ 1u;
    return MVF_OK;
}

// allow_partial (the batched path): where all rows do not fit beside the corpus, shadow the longest PREFIX of rows that does
// (a 204.8-GB Float16 corpus has no room for its 102.4-GB shadow, but for 90+ % of it on this part): the search then runs
// as two row ranges -- int8 selection over the prefix, the f16 kernels over the rest -- whose lists are merged like two
// shards' (search_batched_path).  At least a quarter of the rows and a million, 4 GiB left free for the scratch buffers.
hipError_t ensure_shadow8(const mvfgpu_corpus* c, hipStream_t s, bool insist, bool allow_partial = false) {
    if (c->shadow8_state == -1 && insist) c->shadow8_state = 0;
    if (c->shadow8_state > 0 || c->shadow8_state == -2 || (c->shadow8_state == -1 && !allow_partial)) return hipSuccess;
    const size_t pitch8 = shadow8_pitch(c->dim);
    uint64_t rows = std::max<uint64_t>(c->n, 1);
    const uint64_t forced = c->tune.i8_shadow_rows && c->tune.i8_shadow_rows < c->n ? c->tune.i8_shadow_rows : 0;  // tests
    if (c->shadow8_state == 0 && !insist) {
        size_t free_b = 0, total_b = 0;
        if (forced || hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < rows * pitch8 + ((size_t)2 << 30)) c->shadow8_state = -1;
    }
    if (c->shadow8_state == -1) {
        if (!allow_partial || !c->tune.i8_shadow_partial) return hipSuccess;
        size_t free_b = 0, total_b = 0;
        uint64_t fit = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > ((size_t)4 << 30)) fit = ((free_b - ((size_t)4 << 30)) / (pitch8 + 4)) & ~(uint64_t)65535;
        if (fit >= c->n) fit = c->n;  // (memory was freed meanwhile)
        if (forced) fit = std::min(fit, forced);
        else if (fit < c->n / 4 || fit < (1u << 20)) fit = 0;
        if (fit == 0) {
            c->shadow8_state = -2;
            return hipSuccess;
        }
        rows = fit;
    }
    if (c->shadow8.reserve(rows * pitch8) != hipSuccess || c->xscale8.reserve(((size_t)rows + 256) * 4) != hipSuccess ||
        c->qs_stats.reserve(16) != hipSuccess) {
        (void)hipGetLastError();
        c->shadow8.release();
        c->xscale8.release();
        c->shadow8_state = c->shadow8_state == -1 ? -2 : -1;
        return hipSuccess;
    }
    hipError_t e = hipMemsetAsync(c->qs_stats.p, 0, 16, s);
    if (e == hipSuccess)
        e = launch_shadow_i8(c->d_rows, c->dtype, (uint32_t)rows, c->pitch, c->dim, static_cast<unsigned char*>(c->shadow8.p),
                             (uint32_t)pitch8, static_cast<float*>(c->xscale8.p), static_cast<float*>(c->qs_stats.p), s);
    if (e == hipSuccess) {
        c->shadow8_rows = rows;
        c->shadow8_state = rows == std::max<uint64_t>(c->n, 1) ? 1 : 2;
        c->shadow8_finite = -1;
    }
    return e;
}

// The layout the 6-bit shadow of a handle is held in: 5+1 (shadow_5p1.h) where that is no larger than the 6-bit layout -- the
// dimension modulo 128 is 0 or above 64 -- and the corpus is large enough for the skipped low bits to outweigh what the scan
// pays for them (two tiles in flight instead of four, a short first piece, a second round trip per tile that holds a needing
// row, the skip key's refresh per chunk, and ~0.9M low-plane lines read before the published bests are good -- whatever the size).
// Measured, 768-dim cosine, top-100, device ms per search, 6-bit layout | 5+1 (profiles/r21_stream_5p1.txt): 4 GiB 0.187 |
// 0.210; 8 GiB 0.327 | 0.338; 12 GiB 0.419 | 0.423; 16 GiB 0.554 | 0.519; 20 GiB 0.682 | 0.622; 28.6 GiB 0.944 | 0.845.
// MVF_STREAM_5P1=0 never, =1 wherever it is no larger; a handle on scan path 7 (tests) takes it at any size too.
constexpr uint64_t kStream51MinBytes = 16ull << 30;
bool stream_5p1_layout(const Tuning& t, uint64_t rows, uint32_t dim, bool forced) {
    if (t.stream_5p1 == 0 || !s51_eligible(dim)) return false;
    return t.stream_5p1 == 1 || forced || rows * (uint64_t)dim * 4u >= kStream51MinBytes;
}

// The 6-bit shadow (shadow_6b.hip), built straight from the stored rows beside whatever int8 shadow exists: ensure_shadow8's
// free-memory rule (its bytes + 2 GiB must be free unless the caller insists), all rows or none.
hipError_t ensure_shadow6(const mvfgpu_corpus* c, hipStream_t s, bool insist) {
    if (c->shadow6_state == -1 && insist) c->shadow6_state = 0;
    if (c->shadow6_state != 0) return hipSuccess;
    const uint64_t rows = std::max<uint64_t>(c->n, 1);
    const bool p51 = stream_5p1_layout(c->tune, c->n, c->dim, c->scan_path == 7);
    const size_t need = p51 ? s51_bytes(rows, c->dim) : s6_bytes(rows, c->dim);
    if (!insist) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < need + ((size_t)2 << 30)) {
            (void)hipGetLastError();
            c->shadow6_state = -1;
            return hipSuccess;
        }
    }
    if (c->shadow6.reserve(need) != hipSuccess || c->xscale6.reserve(((size_t)rows + 256) * 4) != hipSuccess ||
        c->qs6_stats.reserve(16) != hipSuccess) {
        (void)hipGetLastError();
        c->shadow6.release();
        c->xscale6.release();
        c->shadow6_state = -1;
        return hipSuccess;
    }
    hipError_t e = hipMemsetAsync(c->qs6_stats.p, 0, 16, s);
    if (e == hipSuccess)
        e = launch_shadow_6b(c->d_rows, (uint32_t)c->n, c->pitch, c->dim, static_cast<unsigned char*>(c->shadow6.p),
                             static_cast<float*>(c->xscale6.p), static_cast<float*>(c->qs6_stats.p), s, p51);
    if (e == hipSuccess) {
        c->shadow6_p51 = p51;
        c->shadow6_state = 1;
        c->shadow6_finite = -1;
    }
    return e;
}

// Threshold refinement of the int8 selection (scan_mfma.h: launch_refine_tau) in front of the LAST phase -- (g - 1) / g of
// the corpus -- when that is at least this many rows (in front of the second largest phase too it cost what it saved);
// MVF_QS_REFINE=0 switches it off (A/B runs).
constexpr uint64_t kRefineMinRows = 200000;
// ... and in front of a phase only where the phase is worth it: a refinement is ~12-16 us of latency whatever the batch, what it
// spares the phase behind it grows with queries x rows.  One process, the switch toggled between rounds (scripts/probe_tune_ab.py,
// profiles/r05_k2_walk_and_phase_costs.txt 8c): 16 / 64 queries on 1M x 768 -4 % without, 32 on 3M -1.3 %, 16 on 10M -1 %;
// 64 on 10M +1 % without, 128 and more: with.
constexpr uint64_t kRefineMinPairs = 256ull << 20;
// is the threshold refined behind phase bi (rows [.., bounds[bi])), in front of the phase [bounds[bi], bounds[bi + 1])?
bool k2_refine_before(const Tuning& t, const std::vector<uint64_t>& bounds, size_t bi, uint32_t nq) {
    if (!t.qs_refine_phases || bi + 1 >= bounds.size()) return false;
    const uint64_t next_rows = bounds[bi + 1] - bounds[bi];
    return bi + t.qs_refine_phases >= bounds.size() - 1 && next_rows >= kRefineMinRows && (uint64_t)nq * next_rows >= kRefineMinPairs;
}
bool qs_refine_enabled(const mvfgpu_corpus* c) { return c->tune.qs_refine; }

// K2 per-query state (threshold key, candidate count, overflow flag; for the refinement the number of best candidates
// at the head of the list and the worst exact key among them), armed once and re-armed by the kernels that end a search.
int ensure_bstate(const mvfgpu_corpus* c, uint32_t nq_pad, hipStream_t s) {
    if (c->bstate_slots >= nq_pad) return MVF_OK;
    MVF_HIP_TRY(c->bstate.reserve((size_t)nq_pad * 20));
    MVF_HIP_TRY(hipMemsetAsync(c->bstate.p, 0xFF, (size_t)nq_pad * 4, s));                                                     // tau
    MVF_HIP_TRY(hipMemsetAsync(static_cast<unsigned char*>(c->bstate.p) + (size_t)nq_pad * 4, 0, (size_t)nq_pad * 16, s));  // cnt, overflow, ntop, lkey
    c->bstate_slots = nq_pad;
    return MVF_OK;
}

struct BState {
    uint32_t *tau, *cnt, *overflow, *ntop, *lkey;  // [bstate_slots] each
};
BState bstate_view(const mvfgpu_corpus* c) {
    uint32_t* tau = static_cast<uint32_t*>(c->bstate.p);
    const uint32_t n = c->bstate_slots;
    return BState{tau, tau + n, tau + 2 * n, tau + 3 * n, tau + 4 * n};
}

// The re-scoring kernels' view of a search: the candidate lists (`cap` slots per query at `cand`) and their state, the
// caller's f32 queries, the stored rows; `final`: the pass that formats the results as well.
RescoreParams rescore_params(const mvfgpu_corpus* c, const SearchCall& sc, uint64_t* cand, uint32_t cap, const BState& bs, bool final) {
    RescoreParams rp{};
    if (final) set_result_format(rp, c, sc);
    rp.cand = cand;
    rp.cnt = bs.cnt;
    rp.tau = bs.tau;
    rp.cap = cap;
    rp.k = sc.k;
    rp.queries = static_cast<const float*>(sc.d_queries);
    rp.rows = c->d_rows;
    rp.pitch = c->pitch;
    rp.dim = c->dim;
    rp.dtype = c->dtype;
    return rp;
}

// K4: per-row norms of the STORED rows, once per resident corpus (a shadow only feeds the dot products).
// float rows: |x| [n], sum x^2 [n], max sum x^2 [1]; Int8 rows: sum x^2 (i32) [n]; UInt8 rows: sum (x-128)^2 [n],
// 128 * sum (x-128) [n]
// Layout: two arrays of norm_stride(n) entries (a multiple of 256, so both are 1-KB aligned), 256 entries of padding
// (the ping-pong K2 kernel DMAs the 256 entries of a row tile at once, also for the corpus' last, partial tile), then
// the one-element maximum.
size_t norm_stride(uint64_t n) { return ((size_t)std::max<uint64_t>(n, 1) + 255u) & ~(size_t)255u; }
size_t norm_max_at(uint64_t n) { return 2 * norm_stride(n) + 256; }

int ensure_norms(const mvfgpu_corpus* c, hipStream_t s) {
    if (c->xnorm_ready) return MVF_OK;
    const uint32_t n = (uint32_t)c->n;
    const size_t nn = norm_stride(n);
    MVF_HIP_TRY(c->xnorm.reserve((norm_max_at(n) + 1) * 4));
    float* xn = static_cast<float*>(c->xnorm.p);
    float* xmax = xn + norm_max_at(n);
    if (!is_int_dtype(c->dtype)) MVF_HIP_TRY(hipMemsetAsync(xmax, 0, 4, s));
    if (c->dtype == MVF_DTYPE_FLOAT32) MVF_HIP_TRY(launch_row_norms_f32(c->d_rows, n, c->pitch, xn, xn + nn, xmax, s));
    else MVF_HIP_TRY(launch_row_norms16(c->d_rows, c->dtype, n, c->pitch, c->dim, c->xnorm.p, xn + nn, xmax, s));
    c->xnorm_ready = true;
    return MVF_OK;
}

// Queries whose candidate budget overflowed (or whose margin reached past a truncated list) are redone exactly by K1 on
// the stored rows -- DECIDED ON THE DEVICE, so the search stays asynchronous (round 1 read the flags back and
// synchronised the stream): flag_compact_kernel turns the flags into a dense list + count; then ceil(nq / R) pairs of
// REPAIR launches follow unconditionally -- K1's repair variant (every block walks its window of the list in groups of
// four queries, one pass over the rows per group) and select_final's -- each of which reads the count and exits at once
// when its window is empty.  The common case (nothing flagged) costs a few empty launches (4-5 us each on the device,
// hidden behind the scan on the host); an adversarial corpus is still answered exactly.  R (queries per pair) is what
// 256 MiB of per-block lists hold.
// nqv_want = 1: the repair passes take one query each, with the lane-group width K1 uses for ONE query (a single-query search
// whose answer must carry the bits the stored-row route gives it: search_stream_qs_path).
// The shape of the repair launches and their buffers, fixed before anything is launched: a search of one to four streamed
// queries hands the list and the count to its final select, whose block 0 compacts the flags (RescoreParams::flags) -- the
// launch of flag_compact_kernel spared.
struct RepairPlan {
    bool any = false;  // an empty corpus has nothing to repair
    K1Shape sh;        // of the repair passes over the stored rows
    uint32_t nchunks = 0, nblocks = 0, R = 0;
    uint64_t* lists = nullptr;
    uint32_t *redo_cnt = nullptr, *redo_list = nullptr;
};
int plan_repair(const mvfgpu_corpus* c, const SearchCall& sc, int nqv_want, RepairPlan* rp) {
    *rp = RepairPlan{};
    if (c->n == 0) return MVF_OK;
    const K1Shape sh = k1_shape(c, nqv_want == 1 ? 1u : 4u, sc.k);
    const uint32_t nchunks = (uint32_t)((c->n + sh.chunk_rows - 1) / sh.chunk_rows);
    if (const int frc = k1_shape_fits(sh)) return frc;
    const void* kfn = scan_kernel(c->dtype, sc.metric, sh.G, sh.nqv, /*redo=*/true);
    int occ = 1;
    {
        const int orc = scan_occupancy(c, kfn, sh.lds, &occ);
        if (orc != MVF_OK) return orc;
    }
    // Two blocks per CU at most: the repair is rare, and every block's list costs scratch for EVERY query a launch pair may
    // serve -- with fewer lists a pair serves more queries (up to 4096 within 256 MiB of lists: 512 at k = 100, all of a
    // 10,000-query batch in three pairs at k = 10), and a 1024-query search enqueues 2 (empty) pairs instead of 16
    // (0.14 ms of launches on a 10-ms search; a 10,000-query search on 1M x 128 spent 0.36 of its 5.6 ms in 40 empty pairs
    // while the cap was 256).
    // (a one-query repair -- nqv_want = 1, one search's single flagged query -- keeps K1's full grid: its lists are few)
    const uint32_t nblocks = std::min<uint32_t>(nchunks, (uint32_t)(nqv_want == 1 ? occ : std::min(occ, 2)) * (uint32_t)c->num_cus);
    const size_t per_query = (size_t)nblocks * next_pow2(sc.k) * 8;
    uint32_t R = (uint32_t)std::min<size_t>(4096, std::max<size_t>(4, ((size_t)256 << 20) / per_query));
    if (c->tune.repair_window) R = std::min<uint32_t>(R, std::max<uint32_t>(4, c->tune.repair_window));  // tests: several windows on small batches
    MVF_HIP_TRY(c->repair.reserve((size_t)R * per_query + (size_t)sc.nq * 4 + 16));
    rp->any = true;
    rp->sh = sh;
    rp->nchunks = nchunks;
    rp->nblocks = nblocks;
    rp->R = R;
    rp->lists = static_cast<uint64_t*>(c->repair.p);
    rp->redo_cnt = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(c->repair.p) + (size_t)R * per_query);
    rp->redo_list = rp->redo_cnt + 4;
    return MVF_OK;
}

// compacted != NULL: the caller's last kernel has compacted the flags into that plan's list already
int repair_flagged_queries(const mvfgpu_corpus* c, SearchCall& sc, uint32_t* overflow, int nqv_want = 4,
                           const RepairPlan* compacted = nullptr, uint64_t* ts_end = nullptr) {
    // ts_end: the last select of the last window is the last kernel of a profiled search on the streamed-shadow route
    RepairPlan own;
    if (!compacted) {
        const int prc = plan_repair(c, sc, nqv_want, &own);
        if (prc != MVF_OK) return prc;
    }
    const RepairPlan& pl = compacted ? *compacted : own;
    if (!pl.any) return MVF_OK;
    hipStream_t s = sc.stream;
    if (!compacted) {
        MVF_HIP_TRY(launch_flag_compact(overflow, sc.nq, pl.redo_list, pl.redo_cnt, feedback_mirror(c, sc), s));
        sc.launches++;
    }
    c->last_redo_cnt = pl.redo_cnt;
    for (uint32_t base = 0; base < sc.nq; base += pl.R) {
        ScanParams sp = stored_scan_params(c, sc, pl.sh, pl.nchunks, pl.lists);
        sp.redo_list = pl.redo_list;
        sp.redo_cnt = pl.redo_cnt;
        sp.redo_base = base;
        sp.redo_max = pl.R;
        MVF_HIP_TRY(scan_launch(c->dtype, sp, sc.metric, pl.sh.G, pl.sh.nqv, dim3(pl.nblocks), pl.sh.lds, s));
        SelectParams fp = final_select_params(c, sc, pl.lists, pl.nblocks);
        fp.redo_list = pl.redo_list;
        fp.redo_cnt = pl.redo_cnt;
        fp.redo_base = base;
        if (base + pl.R >= sc.nq) fp.ts_end = ts_end;
        MVF_HIP_TRY(launch_select_final(fp, std::min(pl.R, sc.nq - base), s));
        sc.launches += 2;
    }
    if (c->tune.debug_repair) {  // diagnostics only: how many queries took the repair path (synchronises)
        uint32_t n = 0;
        MVF_HIP_TRY(hipMemcpyAsync(&n, pl.redo_cnt, 4, hipMemcpyDeviceToHost, s));
        MVF_HIP_TRY(hipStreamSynchronize(s));
        if (n) fprintf(stderr, "[mvfgpu] overflow repair: %u of %u queries redone by K1\n", n, sc.nq);
    }
    return MVF_OK;
}

// K2 path: MFMA batched scan in geometric phases with per-query candidate
// compaction between them (scan_mfma.hip for Float32 rows, scan_mfma16_dma.hip and its
// siblings for Float16 / Int8 / UInt8 rows and the shadows).  Asynchronous: queries whose candidate budget overflowed are
// redone exactly by K1 in repair launches that decide on the device whether to run.
// One ROW RANGE [lo, hi) of the corpus (the whole of it, or one of the two ranges of a corpus whose int8 shadow covers a prefix
// of the rows: search_batched_path below).  allow_qs: the range may select on the int8 shadow (it lies inside it).  defer: the
// caller merges this range's lists with the other's first and runs the repair of flagged queries / the feedback itself --
// what it needs for that comes back in *dr.  profile: this range's last phase is the one the handle's timing reports.
struct BatchedDeferred {
    uint32_t* overflow = nullptr;
    bool used_bias = false, used_qs = false;
};
int search_batched_range(const mvfgpu_corpus* c, SearchCall& sc, uint64_t lo, uint64_t hi, bool allow_qs, bool defer, bool profile,
                         BatchedDeferred* dr) {
    const uint8_t metric = sc.metric;
    const void* d_queries = sc.d_queries;
    const uint32_t nq = sc.nq, k = sc.k;
    hipStream_t s = sc.stream;
    // Float32 rows: either the exact f32 MFMA kernel on the rows themselves, or -- 4x faster -- the f16 kernel on a
    // scaled-f16 SHADOW copy that only selects candidates (error bound below); the kept rows are re-scored from the
    // f32 rows and the f32 query either way, so results do not depend on which one ran.
    bool use_shadow = false, use_qs = false;
    const bool rescore_fits = (size_t)((c->dim + 7u) & ~7u) * 4 + kBatchCap * 4 <= 64 * 1024;  // query + candidates in LDS
    if (allow_qs && qs_wanted(c, k)) {  // int8 shadow: selection at the int8 MFMA rate (Float32 and Float16 corpora)
        int rc = ensure_norms(c, s);
        if (rc != MVF_OK) return rc;
        use_qs = c->shadow8_state == 1 || (c->shadow8_state == 2 && hi <= c->shadow8_rows);  // built by the caller
    }
    if (!use_qs && c->dtype == MVF_DTYPE_FLOAT32 && c->scan_path != 2 && (c->scan_path == 3 || shadow_enabled(c)) && rescore_fits) {
        MVF_HIP_TRY(ensure_shadow(c, s, c->scan_path == 3));
        use_shadow = c->shadow_state == 1;
    }
    const bool wide = c->dtype == MVF_DTYPE_FLOAT32 && !use_shadow && !use_qs;  // f32 rows: 128x128x32-float tiles
    const uint8_t kdtype = use_qs ? (uint8_t)MVF_DTYPE_INT8 : use_shadow ? (uint8_t)MVF_DTYPE_FLOAT16 : c->dtype;  // what the scan kernel reads
    const unsigned char* krows = use_qs       ? static_cast<const unsigned char*>(c->shadow8.p)
                                 : use_shadow ? static_cast<const unsigned char*>(c->shadow.p)
                                              : c->d_rows;
    const uint32_t kpitch = use_qs ? shadow8_pitch(c->dim) : use_shadow ? shadow_pitch(c->dim) : c->pitch;
    const uint32_t qpb = wide ? 128u : scan_mfma16_dma_queries_per_block(nq, c->tune.k2_tile);
    const uint32_t tile_rows = wide ? 128u : scan_mfma16_dma_tile_rows(qpb);
    const uint32_t nq_pad = (nq + qpb - 1u) / qpb * qpb;
    const uint32_t ktb = wide ? 128u : 64u;                // k-tile bytes: 32 floats / 64 bytes of the f16/int8 kernels
    const uint32_t KT = (c->dim * elem_size(kdtype) + ktb - 1u) / ktb;
    const uint32_t KPB = KT * ktb;                         // prepared query row, bytes
    const uint32_t planes = 1u;
    const uint32_t cap = use_qs ? kBatchCapQS : kBatchCap;
    const uint32_t n = (uint32_t)c->n;          // the corpus: layout of the norm arrays
    const uint64_t nr = hi - lo;                // the range: what the phases cover

    MVF_HIP_TRY(c->bq.reserve((size_t)planes * nq_pad * KPB + (size_t)nq_pad * 12 + 64));
    unsigned char* qprep = static_cast<unsigned char*>(c->bq.p);
    float* qaux0 = reinterpret_cast<float*>(qprep + (size_t)planes * nq_pad * KPB);
    float* qaux1 = qaux0 + nq_pad;
    unsigned char* zeros = reinterpret_cast<unsigned char*>(qaux1 + nq_pad);  // 64 zero bytes
    float* qdelta = reinterpret_cast<float*>(zeros + 64);                       // [nq_pad] int8-shadow selection: bound per query
    if (c->bq_zeros != zeros || c->bq_zero_bytes != c->bq.bytes) {  // nothing in this path writes them: set once per allocation and layout, not
        MVF_HIP_TRY(hipMemsetAsync(zeros, 0, 64, s));                      // once per search (a fill kernel is 4.8 us); the streaming paths, which lay
        c->bq_zeros = zeros;                                            // the buffer out differently, forget the mark
        c->bq_zero_bytes = c->bq.bytes;
    }
    {
        int rc = ensure_bstate(c, nq_pad, s);
        if (rc != MVF_OK) return rc;
    }
    const BState bs = bstate_view(c);
    uint32_t *const tau = bs.tau, *const cnt = bs.cnt, *const overflow = bs.overflow;
    MVF_HIP_TRY(c->bcand.reserve((size_t)nq_pad * cap * 8));
    const bool is_float = !is_int_dtype(c->dtype);
    // approximate selection + exact re-scoring: float L2 (GEMM-form distances) and every metric on Float16 rows
    // (single f16 query plane); the other combinations carry final keys through the phases
    const bool approx = is_float && (metric == MVF_METRIC_L2 || kdtype == MVF_DTYPE_FLOAT16 || use_qs);
    const bool need_norms = approx || metric != MVF_METRIC_INNER_PRODUCT || c->dtype == MVF_DTYPE_UINT8;
    const size_t nn = norm_stride(n);
    if (need_norms) {
        int rc = ensure_norms(c, s);
        if (rc != MVF_OK) return rc;
    }
    const float* xx2 = is_float && c->xnorm.p ? static_cast<const float*>(c->xnorm.p) + nn : nullptr;
    const float* xxmax = is_float && c->xnorm.p ? static_cast<const float*>(c->xnorm.p) + norm_max_at(n) : nullptr;
    if (use_qs)
        MVF_HIP_TRY(launch_prep_queries_i8s(static_cast<const float*>(d_queries), nq, nq_pad, c->dim, KPB, metric,
                                        static_cast<const float*>(c->qs_stats.p), xxmax, qprep, qaux0, qaux1, qdelta, s));
    else if (wide)
        MVF_HIP_TRY(launch_prep_queries(static_cast<const float*>(d_queries), nq, nq_pad, c->dim, KPB / 4,
                                    reinterpret_cast<float*>(qprep), qaux0, s));
    else
        MVF_HIP_TRY(launch_prep_queries16(d_queries, kdtype, nq, nq_pad, c->dim, KPB, qprep, qaux0, qaux1, s));

    BatchParams bp{};
    bp.qmat = reinterpret_cast<const float*>(qprep);
    bp.qnorm = qaux0;
    bp.rows = c->d_rows;
    bp.xnorm = static_cast<const float*>(c->xnorm.p);
    bp.xx2 = xx2;
    bp.xxmax = xxmax;
    bp.tomb = sc.deny;
    bp.tau = tau;
    bp.cand = static_cast<uint64_t*>(c->bcand.p);
    bp.cnt = cnt;
    bp.pitch = c->pitch;
    bp.V = c->V;
    bp.KP = KPB / 4;
    bp.KT = KT;
    bp.nq = nq;
    bp.mtiles = nq_pad / qpb;
    bp.cap = cap;

    Batch16Params hp{};
    hp.qprep = qprep;
    hp.qaux0 = qaux0;
    hp.qaux1 = qaux1;
    hp.rows = krows;
    hp.xscale = use_qs ? static_cast<const float*>(c->xscale8.p) : use_shadow ? static_cast<const float*>(c->xscale.p) : nullptr;
    hp.zeros = zeros;
    hp.xnorm_f = static_cast<const float*>(c->xnorm.p);
    hp.xnorm_i = static_cast<const int32_t*>(c->xnorm.p);
    hp.xbias_i = c->xnorm.p ? static_cast<const int32_t*>(c->xnorm.p) + nn : nullptr;
    hp.dim = c->dim;
    hp.xx2 = xx2;
    hp.xxmax = xxmax;
    hp.tomb = bp.tomb;
    hp.tau = tau;
    hp.cand = bp.cand;
    hp.cnt = cnt;
    hp.pitch = kpitch;
    hp.V = kpitch / 16;
    hp.KPB = KPB;
    hp.KT = KT;
    hp.nq = nq;
    hp.nq_pad = nq_pad;
    hp.mtiles = nq_pad / qpb;
    hp.cap = cap;
    // candidates leave the narrow-type kernels through per-block regions (no global atomics in the epilogue): T records in
    // all -- twice what the per-query lists can hold, at least the 128 MiB of round 2 -- split evenly over the blocks of
    // the launch; the LDS-DMA kernel's i32-accumulator flavours split a block's share once more per wave (raw records)
    uint64_t blk_records = 0;
    if (!wide) {
        blk_records = std::min<uint64_t>(std::max<uint64_t>((uint64_t)kBlkMaxBlocks * kBlkCap, 2ull * nq_pad * cap), 32ull << 20);
        if (c->tune.region_records)  // MVF_K2_REGION_RECORDS (tests: force the regions to overflow)
            blk_records = std::max<uint64_t>((uint64_t)kBlkMaxBlocks * kBlkWaves, c->tune.region_records);
        blk_records -= blk_records % ((uint64_t)kBlkMaxBlocks * kBlkWaves);
        {
            const void* before = c->blk.p;
            MVF_HIP_TRY(c->blk.reserve((size_t)blk_records * 16 + (size_t)kBlkMaxBlocks * kBlkWaves * 4));
            if (c->blk.p != before) c->blk_armed_cnt = nullptr;  // fresh memory
        }
        hp.blk_cand = static_cast<uint4*>(c->blk.p);
        hp.blk_cnt = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(c->blk.p) + (size_t)blk_records * 16);
        hp.blk_cap = (uint32_t)(blk_records / kBlkMaxBlocks);
    }

    CompactParams cp{};
    cp.cand = bp.cand;
    cp.cnt = cnt;
    cp.tau = tau;
    cp.overflow = overflow;
    cp.cap = cap;
    cp.metric = metric;
    set_result_format(cp, c, sc);
    cp.qnorm = wide ? qaux0 : qaux1;  // |q| (f32 path: qnorm; f16 path: second aux array)
    cp.xxmax = xxmax;
    // bound of the approximate score's error in units of (qq + xx) [L2], 1 [cosine], |q||x| [inner product]:
    // f32 accumulation of `dim` terms plus the norms, and on Float16 rows the query's rounding to f16 (2^-11 per
    // element, relative; elements that land in the f16 subnormals add < 2^-39 of it)
    cp.eps = (float)(std::max<uint32_t>(c->dim, 64) + 16) * 1.1920929e-7f;
    if (kdtype == MVF_DTYPE_FLOAT16) cp.eps += 4.8828125e-4f * 1.001f;
    if (use_shadow) cp.eps += 4.8828125e-4f * 1.001f;  // the shadow rows' own rounding (same bound, per element of x)
    cp.delta = use_qs ? qdelta : nullptr;               // int8 selection: the per-query bound from the query preparation
    // int8 selection: between the large phases the threshold is refined with exact scores of the k best (scan_mfma.h)
    uint32_t *const ntop = bs.ntop, *const lkey = bs.lkey;
    const bool refine = use_qs && qs_refine_enabled(c);
    cp.ntop = refine ? ntop : nullptr;

    mvfgpu_timing tm{};
    tm.scan_kernel = wide ? 2u : use_qs ? 6u : use_shadow ? 4u : 3u;
    mvfgpu_corpus::ProfSlot* ps = nullptr;
    if (c->profiling && profile) {
        ps = &c->prof[c->prof_next % mvfgpu_corpus::kProfSlots];
        for (auto& e : ps->e)
            if (!e) MVF_HIP_TRY(hipEventCreate(&e));
        ps->scanned = false;
    }

    // Phase p scans rows [R_p, R_{p+1}) of the range (k2_phase_bounds above)
    const uint32_t g = k2_growth_for(c, nq, k, cap);
    const std::vector<uint64_t> bounds = k2_phase_bounds(nr, cap, g);  // R_1 .. R_{P+1} = nr
    size_t bi = 0;
    uint64_t begin = 0, end = bounds[0];
    // The region counters are zero when a search starts if the search before it on this handle left them so (every scatter re-arms
    // what it has read) and they still sit at the same address: no fill kernel per search then (4.7 us: 1.6 % of a 16-query search
    // on 1M rows).  The mark is taken down while this search runs: a search that fails half way leaves it down.
    bool regions_armed = hp.blk_cnt != nullptr && c->blk_armed_cnt == hp.blk_cnt, used_bias = false;
    c->blk_armed_cnt = nullptr;
    for (;;) {
        const bool last = end >= nr;
        if (end > begin) {
            bp.row_begin = hp.row_begin = (uint32_t)(lo + begin);
            bp.row_end = hp.row_end = (uint32_t)(lo + end);
            bp.ntiles = hp.ntiles = (uint32_t)((end - begin + tile_rows - 1) / tile_rows);
            bp.direct = hp.direct = (begin == 0 && end - begin <= cap) ? 1u : 0u;
            const bool regions = hp.blk_cand && !hp.direct;
            // which kernel takes the phase
            const bool use_pp = !wide && qpb == 256u && k2_pp_wanted(c, kdtype, hp.ntiles, hp.mtiles, c->num_cus) &&
                                scan_mfma16_pp_usable(hp.mtiles, c->num_cus, KT);
            const bool use_sb = !wide && !use_pp && qpb == 64u && scan_mfma16_sb_usable(nq_pad, KT, nq);
            // per-wave regions of raw records (scan_mfma16_bias.inc): the persistent LDS-DMA kernel on i32 accumulators
            // (per-wave regions: num_cus blocks x kBlkWaves counters in blk_cnt, which holds kBlkMaxBlocks * kBlkWaves -- a part
            // with more CUs than kBlkMaxBlocks keeps round 2's per-block regions instead of reading counters past the array)
            const bool wave_regions = !wide && !use_pp && !use_sb && !c->bias_disabled && k2_bias_enabled(c) &&
                                      (uint32_t)c->num_cus <= kBlkMaxBlocks &&
                                      scan_mfma16_dma_wave_regions(kdtype, qpb, hp.direct != 0, regions, c->dim);
            hp.wave_regions = wave_regions ? 1u : 0u;
            used_bias |= wave_regions;
            const uint32_t region_blocks = wave_regions ? (uint32_t)c->num_cus : kBlkMaxBlocks;
            if (regions) hp.blk_cap = (uint32_t)(blk_records / region_blocks) & ~(kBlkWaves - 1u);
            // the region counters: zeroed once, re-armed by every scatter after it has read them
            if (regions && (!regions_armed || nq_pad > scatter_rearm_max_queries())) {
                MVF_HIP_TRY(hipMemsetAsync(hp.blk_cnt, 0, (size_t)kBlkMaxBlocks * kBlkWaves * 4, s));
                regions_armed = true;
            }
            if (ps && last) MVF_HIP_TRY(hipEventRecord(ps->e[0], s));
            if (wide) MVF_HIP_TRY(launch_scan_mfma_f32(bp, metric, s));
            else if (use_pp) MVF_HIP_TRY(launch_scan_mfma16_pp(hp, kdtype, metric, c->num_cus, s));
            else if (use_sb) MVF_HIP_TRY(launch_scan_mfma16_sb(hp, kdtype, metric, c->num_cus, s));
            else if (hp.direct && qpb >= 128u) {
                // The direct phase is a few thousand rows: 10 row tiles x 4 query tiles of 256 x 256 leave 216 CUs idle while 40 blocks
                // multiply, key and store 65536 pairs each.  In 64-query tiles (64 x 512) the same pairs spread over twice the blocks
                // at half the work each (the prepared queries and the slots by row offset do not depend on the tile shape).
                Batch16Params dp = hp;
                const uint32_t tr = scan_mfma16_dma_tile_rows(64u);
                dp.mtiles = nq_pad / 64u;
                dp.ntiles = (uint32_t)((end - begin + tr - 1) / tr);
                MVF_HIP_TRY(launch_scan_mfma16_dma(dp, kdtype, metric, c->num_cus, 64u, s));
            } else MVF_HIP_TRY(launch_scan_mfma16_dma(hp, kdtype, metric, c->num_cus, qpb, s));
            if (ps && last) {
                MVF_HIP_TRY(hipEventRecord(ps->e[1], s));
                ps->scanned = true;
                tm.scan_bytes = (end - begin) * c->dim * elem_size(kdtype);
                tm.scan_flops = 2ull * nq * (end - begin) * c->dim;
            }
            tm.scan_launches++;
            if (regions) {
                Batch16Params sp = hp;  // the scatter pass sees a wave's slice as a region of its own
                if (wave_regions) sp.blk_cap = hp.blk_cap / kBlkWaves;
                MVF_HIP_TRY(launch_scatter_cand(sp, wave_regions ? region_blocks * kBlkWaves : region_blocks, metric, kdtype, s));
            }
        }
        cp.direct_cnt = (begin == 0 && end > begin && end - begin <= cap) ? (uint32_t)(end - begin) : 0u;
        if (approx) MVF_HIP_TRY(launch_compact_margin(cp, nq, s));
        else MVF_HIP_TRY(launch_compact(cp, nq, last, s));
        if (last) break;
        if (refine && k2_refine_before(c->tune, bounds, bi, nq)) {  // worth its ~0.07 ms in front of the last (largest) phases
            const RescoreParams rp = rescore_params(c, sc, bp.cand, cap, bs, /*final=*/false);
            MVF_HIP_TRY(launch_refine_tau(rp, metric, nq, ntop, lkey, qdelta, s));
        }
        begin = end;
        end = bounds[++bi];
    }
    if (hp.blk_cnt && nq_pad <= scatter_rearm_max_queries()) c->blk_armed_cnt = hp.blk_cnt;  // every phase's scatter has been enqueued
    if (approx) {  // exact scores of the kept candidates from the caller's f32 queries, final top-k
        if (refine && nr >= kRefineMinRows) {  // once more on the final lists: the re-scoring skips what falls outside
            RescoreParams fp = rescore_params(c, sc, bp.cand, cap, bs, /*final=*/false);
            fp.write_head = 1u;  // the exact composites of the head stay where the final pass would write them
            MVF_HIP_TRY(launch_refine_tau(fp, metric, nq, ntop, lkey, qdelta, s));
        }
        RescoreParams rp = rescore_params(c, sc, bp.cand, cap, bs, /*final=*/true);
        rp.head_done = (refine && nr >= kRefineMinRows) ? ntop : nullptr;
        MVF_HIP_TRY(launch_rescore(rp, metric, nq, s));
    }
    if (ps) {
        MVF_HIP_TRY(hipEventRecord(ps->e[2], s));
        c->timing = tm;
        c->prof_next++;
    }

    if (dr) {
        dr->overflow = overflow;
        dr->used_bias |= used_bias;
        dr->used_qs |= use_qs && c->scan_path != 5 && !path_streams_i8(c);
    }
    if (defer) return MVF_OK;
    int rc = repair_flagged_queries(c, sc, overflow);
    if (rc == MVF_OK && ((use_qs && c->scan_path != 5 && !path_streams_i8(c)) || used_bias))
        rc = qs_feedback_post(c, sc, used_bias, use_qs && c->scan_path != 5 && !path_streams_i8(c));
    return rc;
}

int merge_topk_device_impl(const float* d_scores, const uint64_t* d_indices, const int32_t* d_raw, size_t ls_scores, size_t ls_indices,
                           size_t ls_raw, uint32_t nlists, uint32_t nq, uint32_t k, uint8_t metric, uint8_t data_type, float* d_out_scores,
                           uint64_t* d_out_indices, int32_t* d_out_raw, int device, void* hip_stream);

// The batched search of a corpus.  Usually ONE range, all rows.  A Float32 / Float16 corpus whose int8 selection shadow does
// not fit beside it as a whole (the 100M x 1024 Float16 corpus of BASELINE configs[4] on one GPU: 204.8 GB of rows, 102.4 GB of
// shadow) gets a shadow of the longest prefix of rows that does (ensure_shadow8) and is searched as TWO row ranges -- the
// prefix by the int8 selection, the rest by the f16 kernels on the stored rows -- whose exact top-k lists are merged like two
// shards' (the same device merge: ties by ascending position); the repair of flagged queries runs once, behind the merge, over
// the whole corpus.  100M x 1024 f16, 1024 queries: 181-184 ms -> 95.5 (profiles/r05_partial_shadow.json).
int search_batched_path(const mvfgpu_corpus* c, SearchCall& sc) {
    const uint32_t nq = sc.nq, k = sc.k;
    hipStream_t s = sc.stream;
    if (!is_filtered(c, sc)) qs_feedback_poll(c);
    if (qs_wanted_batched(c, k)) {
        int rc = ensure_norms(c, s);
        if (rc != MVF_OK) return rc;
        MVF_HIP_TRY(ensure_shadow8(c, s, c->scan_path == 5 || path_streams_i8(c), /*allow_partial=*/true));
    }
    if (!(c->shadow8_state == 2 && qs_wanted(c, k) && c->shadow8_rows < c->n))
        return search_batched_range(c, sc, 0, c->n, true, false, true, nullptr);
    {   // the per-query state (thresholds, counts, overflow flags) must not be re-allocated between the two ranges -- the second
        // would lose the first's overflow flags: sized here for the widest query tile either range may take
        const int brc = ensure_bstate(c, (nq + 255u) & ~255u, s);
        if (brc != MVF_OK) return brc;
    }
    const size_t ls = (size_t)nq * k;
    MVF_HIP_TRY(c->split_out.reserve(2 * ls * 16));
    unsigned char* t = static_cast<unsigned char*>(c->split_out.p);
    uint64_t* ti = reinterpret_cast<uint64_t*>(t);                 // [2][nq k]
    float* ts = reinterpret_cast<float*>(t + 2 * ls * 8);          // [2][nq k]
    int32_t* tr = reinterpret_cast<int32_t*>(t + 2 * ls * 12);     // [2][nq k]
    BatchedDeferred dr{};
    int rc = inner_search(sc, k, ts, ti, tr, [&](SearchCall& in) { return search_batched_range(c, in, 0, c->shadow8_rows, true, true, true, &dr); });
    if (rc != MVF_OK) return rc;
    rc = inner_search(sc, k, ts + ls, ti + ls, tr + ls,
                      [&](SearchCall& in) { return search_batched_range(c, in, c->shadow8_rows, c->n, false, true, false, &dr); });
    if (rc != MVF_OK) return rc;
    rc = merge_topk_device_impl(ts, ti, tr, ls, ls, ls, 2, nq, k, sc.metric, c->dtype, sc.d_scores, sc.d_indices, sc.d_raw, c->device, s);
    if (rc != MVF_OK) return rc;
    rc = repair_flagged_queries(c, sc, dr.overflow);
    if (rc == MVF_OK && (dr.used_qs || dr.used_bias)) rc = qs_feedback_post(c, sc, dr.used_bias, dr.used_qs);
    return rc;
}

// Scan path 4 (opt-in): one or two queries on a Float32 corpus STREAM ITS SCALED-F16 SHADOW -- half the bytes of the
// stored rows, so half the time of the HBM-bound K1 -- with the batched path's select-with-a-margin / re-score-exactly
// scheme: K1 (dt1x unit: f16 rows times xscale[r]) keeps the k' > k best approximate scores; every candidate within
// twice the error bound of the k-th is re-scored from the stored f32 rows and the f32 query; if ALL k' are inside the
// margin (rows beyond the cut may be too) the query is flagged and redone by the exact K1 (on-device conditional
// repair launches, like the batched path: asynchronous).
//   x~ = x (1 + e), |e| <= 2^-11 per element:  |q.x~ - q.x| <= 2^-11 |q||x|;  | |q - x~| - |q - x| | <= 2^-11 |x|;
//   cosine (numerator and denominator both from x~) <= 2 * 2^-11; plus the f32 accumulation, (dim + 16) 2^-23.
int search_stream_shadow_path(const mvfgpu_corpus* c, SearchCall& sc) {
    const uint8_t metric = sc.metric;
    const uint32_t nq = sc.nq, k = sc.k;
    hipStream_t s = sc.stream;
    const uint32_t cap = kBatchCap;
    const uint32_t nq_pad = (nq + 255u) & ~255u;
    const uint32_t n = (uint32_t)c->n;
    int rc = ensure_bstate(c, nq_pad, s);
    if (rc == MVF_OK) rc = ensure_norms(c, s);
    if (rc != MVF_OK) return rc;
    const BState bs = bstate_view(c);
    MVF_HIP_TRY(c->bcand.reserve((size_t)nq_pad * cap * 8));
    // |q| per query for the margins: the f16 query preparation computes it (its planes are not used here)
    const uint32_t KPB = ((c->dim * 2u + 63u) / 64u) * 64u;
    MVF_HIP_TRY(c->bq.reserve((size_t)nq_pad * KPB + (size_t)nq_pad * 8 + 64));
    c->bq_zeros = nullptr;  // another layout of the buffer: the batched path's zero bytes may be overwritten
    unsigned char* qprep = static_cast<unsigned char*>(c->bq.p);
    float* qaux0 = reinterpret_cast<float*>(qprep + (size_t)nq_pad * KPB);
    float* qaux1 = qaux0 + nq_pad;
    MVF_HIP_TRY(launch_prep_queries16(sc.d_queries, MVF_DTYPE_FLOAT16, nq, nq_pad, c->dim, KPB, qprep, qaux0, qaux1, s));

    const uint32_t ksel = std::min<uint32_t>(MVFGPU_K_PER_PASS, std::max(2u * k, k + 64u));  // k' candidates per query
    ShadowStream alt{};
    alt.rows = static_cast<const unsigned char*>(c->shadow.p);
    alt.xscale = static_cast<const float*>(c->xscale.p);
    alt.pitch = shadow_pitch(c->dim);
    alt.V = alt.pitch / 16;
    choose_group(alt.V, 1, &alt.G, &alt.J, c->tune.k1_g);
    alt.cand = static_cast<uint64_t*>(c->bcand.p);
    alt.cnt = bs.cnt;
    alt.cand_cap = cap;
    rc = inner_search(sc, ksel, nullptr, nullptr, nullptr, [&](SearchCall& in) { return search_stream_path(c, in, /*profile=*/true, &alt); });
    if (rc != MVF_OK) return rc;

    CompactParams cp{};
    cp.cand = alt.cand;
    cp.cnt = bs.cnt;
    cp.tau = bs.tau;
    cp.overflow = bs.overflow;
    cp.cap = cap;
    cp.k = k;
    cp.metric = metric;
    cp.dtype = c->dtype;
    cp.index_base = c->index_base;
    cp.ids = result_ids(c, sc);
    cp.qnorm = qaux1;
    cp.xxmax = static_cast<const float*>(c->xnorm.p) + norm_max_at(n);
    // per-element relative rounding of the shadow rows (2^-11) and f32 accumulation of `dim` terms ((dim + 16) 2^-23
    // of the sum; half of that, relative, on a square root)
    const float e11 = 4.8828125e-4f * 1.001f, eacc = (float)(std::max<uint32_t>(c->dim, 64) + 16) * 1.1920929e-7f;
    cp.eps = metric == MVF_METRIC_COSINE ? 2.0f * e11 + eacc : metric == MVF_METRIC_INNER_PRODUCT ? e11 + eacc : e11;
    cp.eps_acc = 0.5f * eacc;
    cp.l2_is_distance = 1;
    cp.truncated_at = n > ksel ? ksel : 0u;
    MVF_HIP_TRY(launch_compact_margin(cp, nq, s));

    const RescoreParams rp = rescore_params(c, sc, alt.cand, cap, bs, /*final=*/true);
    MVF_HIP_TRY(launch_rescore(rp, metric, nq, s));
    return repair_flagged_queries(c, sc, bs.overflow);
}

// One to four queries on a Float32 / Float16 corpus STREAM ITS INT8 SHADOW (dim bytes per row: a quarter / half of the
// stored rows) through K1's dt2x unit -- exact i32 dots, float keys -- with the int8 selection's proven per-query bound
// (shadow_i8.hip).  The bound is ~0.25 sigma of the score distribution -- 6-10 x k rows on the benchmark's data, more
// than K1's selection can carry as "the k' best" -- so the selection is by BLOCK: every K1 block keeps the max(k, 32)
// best approximate scores of ITS rows (n / ~1000 of them), select_final's margin mode finds the k-th best of all lists
// and gathers every entry within 2 delta of it; a list that was cut inside the bound (rows beyond the cut may be inside
// too: clustered rows, tiny corpora) or more than 2048 rows inside it flag the query, which the exact K1 then redoes.
// rescore_kernel re-scores what was gathered from the stored rows and the f32 query.
// (the 6-bit route: 128 -- its margin is twice as wide, and on short rows, whose scores are far from Gaussian, it holds a
// few per cent of ALL rows whatever k is: 28 of every 1024 rows of 3-dimensional uniform rows under Cosine)
uint32_t stream_qs_klist(uint32_t k, bool s6 = false) { return std::max(k, s6 ? 128u : 32u); }

// s6: ONE query over the 6-BIT shadow instead (shadow_6b.hip: K1's dt2y unit, the query at sixteen bits).  Its bound is twice
// the int8 route's, ~50 x k rows of the benchmark's corpus ride in the margin: the lists hold kStream6Cap kept candidates, the
// re-scoring spreads over them and the final select picks the k best before it sorts (rescore_select_wide_kernel).  The
// same launches in the same order; a flagged query is redone by K1 exactly as on the int8 route, and the repair count feeds
// the 6-bit route's own switch (s6_disabled), never qs_disabled.
constexpr uint32_t kStream6Cap = 16384;  // kept candidates per query on the 6-bit route (the list holds twice that: the exact keys go to its upper half)

int search_stream_qs_path(const mvfgpu_corpus* c, SearchCall& sc, bool s6 = false) {
    const uint8_t metric = sc.metric;
    const uint32_t nq = sc.nq, k = sc.k;
    hipStream_t s = sc.stream;
    const uint32_t cap = s6 ? 2u * kStream6Cap : kBatchCap;
    const uint32_t nq_pad = (nq + 255u) & ~255u;
    const uint32_t n = (uint32_t)c->n;
    int rc = ensure_bstate(c, nq_pad, s);
    if (rc == MVF_OK) rc = ensure_norms(c, s);
    if (rc != MVF_OK) return rc;
    const BState bs = bstate_view(c);
    MVF_HIP_TRY(c->bcand.reserve((size_t)nq_pad * cap * 8));
    const uint32_t KPB = shadow8_pitch(c->dim);
    // the queries' scale, norm and bound: K1's prologue over the shadow prepares the queries itself and stores them here
    // (block 0 of the scan; an empty corpus, which launches no scan, never gets here: qs_possible refuses n == 0)
    MVF_HIP_TRY(c->bq.reserve((size_t)nq_pad * 12 + 64));
    c->bq_zeros = nullptr;  // another layout of the buffer: the batched path's zero bytes may be overwritten
    float* qaux0 = static_cast<float*>(c->bq.p);
    float* qaux1 = qaux0 + nq_pad;
    float* qdelta = qaux1 + nq_pad;
    const size_t nn = norm_stride(n);
    const float* xn = static_cast<const float*>(c->xnorm.p);

    ShadowStream alt{};
    alt.i8 = true;
    alt.rows = static_cast<const unsigned char*>(c->shadow8.p);
    alt.xscale = static_cast<const float*>(c->xscale8.p);
    alt.qaux0 = qaux0;
    alt.qaux1 = qaux1;
    alt.qstats = static_cast<const float*>(c->qs_stats.p);
    alt.xxmax = xn + norm_max_at(n);
    alt.xrow = metric == MVF_METRIC_L2 ? xn + nn : xn;  // sum x^2 | |x| of the stored rows
    alt.pitch = KPB;
    alt.V = KPB / 16;
    if (s6) {
        alt.s6 = true;
        alt.rows = static_cast<const unsigned char*>(c->shadow6.p);
        alt.xscale = static_cast<const float*>(c->xscale6.p);
        alt.qstats = static_cast<const float*>(c->qs6_stats.p);
        alt.pitch = (uint32_t)s6_tile_bytes(c->dim);
        alt.V = s6_units(c->dim);
        if (c->shadow6_p51) {
            alt.p51 = true;
            alt.pitch = (uint32_t)s51_tile_bytes(c->dim);
            alt.V = s51_units(c->dim);
        }
    }
    alt.cand = static_cast<uint64_t*>(c->bcand.p);
    alt.cnt = bs.cnt;
    alt.cand_cap = cap;
    alt.delta = qdelta;
    alt.tau = bs.tau;
    alt.overflow = bs.overflow;
    alt.rank_k = k;
    uint64_t* ts_end = sc.whole_by_clock ? prof_ts_entry(c, c->prof_next) + 3 : nullptr;  // (this search's entry: prof_next moves below)
    rc = inner_search(sc, stream_qs_klist(k, s6), nullptr, nullptr, nullptr,
                      [&](SearchCall& in) { return search_stream_path(c, in, /*profile=*/true, &alt); });
    if (rc != MVF_OK) return rc;

    RescoreParams rp = rescore_params(c, sc, alt.cand, cap, bs, /*final=*/true);
    // Re-scored in K1's arithmetic at the width K1 takes for these queries on the stored rows, and a flagged query redone by
    // K1 at that width too -- the answer carries the bits the stored-row route gives it (Float16 rows too since round 7; they
    // went through the wave kernel's summation order before)
    const K1Shape sh = k1_shape(c, nq, k);
    // the flags are final since the margin select: block 0 of the final select turns them into the repair launches' list
    RepairPlan plan;
    rc = plan_repair(c, sc, sh.nqv, &plan);
    if (rc != MVF_OK) return rc;
    if (plan.any) {
        rp.flags = bs.overflow;
        rp.flags_nq = nq;
        rp.redo_list = plan.redo_list;
        rp.redo_cnt = plan.redo_cnt;
        rp.redo_mirror = feedback_mirror(c, sc);
    }
    MVF_HIP_TRY(launch_rescore_k1(rp, metric, nq, sh.G, sh.J, s));
    sc.launches += 2;
    rc = repair_flagged_queries(c, sc, bs.overflow, sh.nqv, &plan, ts_end);
    if (rc == MVF_OK && s6) rc = qs_feedback_post(c, sc, false, false, /*used_s6=*/true);
    else if (rc == MVF_OK && !path_streams_i8(c)) rc = qs_feedback_post(c, sc);
    return rc;
}

// ONE query on a Float32 corpus of at least this many bytes of rows streams its int8 shadow by default (scan path 0): a quarter
// of the bytes, re-scored in K1's arithmetic -- the same bits as K1 on the stored rows.  Below it the fixed cost of the route
// (the margin select, the re-scoring, the repair check: ~48 us of kernels in five launches since round 7, 58 us in
// seven before; the crossover below is round 6's and was not moved: profiles/r07_stream_fixed_cost.txt) outweighs the bytes it spares.
// Measured, 768-dim f32 cosine, top-100, device time per search (profiles/r06_stream_i8_crossover.txt): 256 MiB 0.084 ms
// against K1's 0.081; 512 MiB 0.084 against 0.123; 1 GiB 0.112 / 0.200; 4 GiB 0.234 / 0.673.
constexpr uint64_t kStreamI8MinBytes = 512ull << 20;

// The shape part of that rule, a pure function (mvfgpu_selftest_stream_rows pins it without a GPU): Float32 rows, one query,
// k <= kQsStreamMaxK, rows the int8 selection's re-scoring takes (qs_possible), at least kStreamI8MinBytes of rows.
bool stream_i8_shape(uint64_t rows, uint32_t dim, uint8_t dtype, uint32_t nq, uint32_t k) {
    if (dtype != MVF_DTYPE_FLOAT32 || nq != 1 || k == 0 || k > kQsStreamMaxK || rows == 0 || dim == 0) return false;
    if ((size_t)((dim + 7u) & ~7u) * 4 + kBatchCapQS * 4 > 64 * 1024) return false;
    return rows * (uint64_t)dim * 4u >= kStreamI8MinBytes;
}

// One to four queries stream the int8 shadow on request (scan path 6), and ONE query on scan path 0 does by default where
// stream_i8_shape holds: 10M x 768 f32, one query, 4.47 -> ~1.2 ms.  The re-scoring (launch_rescore_k1) and the repair of a
// flagged query (K1 at the one-query width) both give K1's bits, so the answer does not depend on the route -- nor on the
// handle's history (round 2 made this route automatic with the re-scoring kernel's own summation order, and the same query
// then scored differently depending on whether an earlier batched search had built the shadow; it was reverted).
// Scan path 0 takes the route only with a WHOLE shadow, held or buildable now under ensure_shadow8's free-memory rule (a
// prefix, or no room: the stored rows), and not over a shadow whose bound maxima are non-finite (search_device: every query
// would be flagged and repaired).  MVF_STREAM_I8=0 opts out; MVF_STREAM_I8=1 also takes any size once the shadow exists.
// A corpus whose queries keep needing the repair pass switches itself back (qs_disabled).  Two to four queries are served as
// fast by the 64-query MFMA tile on the same shadow (1.55-1.65 ms against 1.53-1.72:
// profiles/r02_stream_int8_shadow_1to4_queries.txt).
bool stream_qs_wanted(const mvfgpu_corpus* c, uint32_t nq, uint32_t k) {
    if (nq < 1 || nq > 4 || k > kQsStreamMaxK || !qs_wanted(c, k)) return false;
    // (a 6-bit shadow whose maxima are non-finite has seen a row holding Inf / NaN: the int8 shadow's are non-finite too and
    // every query would be flagged and repaired -- the stored rows, except where scan path 6 insists)
    if (c->shadow6_state == 1 && c->shadow6_finite == 0 && c->scan_path != 6) return false;
    if (path_streams_i8(c)) return true;
    if (c->scan_path != 0 || nq != 1 || c->tune.stream_i8 == 0) return false;
    if (c->shadow8_state != 0 && c->shadow8_state != 1) return false;
    if (c->shadow8_state == 1 && c->shadow8_finite == 0) return false;
    if (c->tune.stream_i8 == 1 && c->shadow8_state == 1) return true;
    return stream_i8_shape(c->n, c->dim, c->dtype, nq, k);
}

// ONE Float32 query on a corpus of at least kStream6MinBytes of rows streams the 6-BIT shadow instead (0.75 x the int8
// shadow's bytes, the same bits as K1 on the stored rows) -- where the margin of the 6-bit bound is predicted to hold at most
// HALF the kStream6Cap candidates the route carries: a query whose margin overflows is redone by K1 on the stored rows at four
// times the int8 route's cost, so shapes near the capacity stay on int8.
// The prediction: scores ~ Gaussian, the k-th best of `rows` at z(k / rows) sigma, the margin 2 delta = 2 c sqrt(dim) sigma wide,
// so  rows Q(z(k / rows) - 2 c sqrt(dim))  rows inside it (Q: the Gaussian tail).  c per metric from the oracle's rows
// (scripts/model_stream_6b_bound.py, 200k x 768, 8 queries: delta = 0.486 / 0.496 / 0.444 sigma for InnerProduct / Cosine /
// L2's squared distance): the headline (10M x 768, k = 100) 5 300 rows -- 6 bit; k = 204 there 9 400, 10M x 1024 at k = 100
// 9 100 -- int8.
// kStream6MinBytes, measured (scripts/probe_stream_6b_crossover.py, profiles/r10_stream_6b.txt; 768-dim cosine, top-100, device
// time per search, int8 / 6-bit): 1 GiB 0.093 / 0.103 ms, 2 GiB 0.136 / 0.138 (inside the spread), 4 GiB 0.214 / 0.189 (ranges
// disjoint), 8 GiB 0.403 / 0.321, 16 GiB 0.708 / 0.562, 10M rows 1.205 / 0.948.  One lane per row needs 1024 rows per block
// and step, so small corpora fill the chip late: the scan holds 3.4 TB/s at 1 GiB, 5.6 at 4 GiB, 6.5 at 10M rows.
constexpr uint64_t kStream6MinBytes = 4ull << 30;
constexpr double kStream6C[3] = {0.01601, 0.01754, 0.01791};  // by metric code: L2, InnerProduct, Cosine

double gauss_tail(double z) { return 0.5 * std::erfc(z / std::sqrt(2.0)); }
double gauss_tail_inv(double p) {  // z with Q(z) = p, by bisection (a pure function of p: the same on every host)
    double lo = -10.0, hi = 10.0;
    for (int i = 0; i < 100; i++) {
        const double mid = 0.5 * (lo + hi);
        if (gauss_tail(mid) > p) lo = mid;
        else hi = mid;
    }
    return 0.5 * (lo + hi);
}
double stream_6b_margin_rows(uint64_t rows, uint32_t dim, uint8_t metric, uint32_t k) {
    if (k >= rows) return (double)rows;
    const double z = gauss_tail_inv((double)k / (double)rows);
    return (double)rows * gauss_tail(z - 2.0 * kStream6C[metric <= 2 ? metric : 2] * std::sqrt((double)dim));
}
// The shape part of the rule, a pure function (mvfgpu_selftest_stream_bits pins it without a GPU); the caller has checked
// Float32 rows, one query and k <= kQsStreamMaxK (stream_i8_shape)
bool stream_6b_shape(uint64_t rows, uint32_t dim, uint8_t metric, uint32_t k) {
    if (rows * (uint64_t)dim * 4u < kStream6MinBytes) return false;
    return stream_6b_margin_rows(rows, dim, metric, k) <= kStream6Cap / 2;
}

// Who takes the 6-bit route: ONE unfiltered Float32 query of a search of its own (the windows of a join, radius and candidate
// searches, filtered searches and two to four queries stay on int8) on scan path 0 where stream_6b_shape holds -- unless
// MVF_STREAM_I8=0 (out of both shadow routes) or MVF_STREAM_6B=0 -- and on scan path 7 at any size (tests).  Only over a WHOLE
// shadow, held or buildable now (ensure_shadow6), whose bound maxima are finite; a corpus whose queries keep needing the
// repair pass switches itself back to the int8 route (s6_disabled) -- as does one the int8 route has given up on already.
bool stream_6b_wanted(const mvfgpu_corpus* c, const SearchCall& sc) {
    if (c->dtype != MVF_DTYPE_FLOAT32 || sc.nq != 1 || sc.k == 0 || sc.k > kQsStreamMaxK || c->n == 0 || sc.shared_call) return false;
    if (sc.deny != static_cast<const uint32_t*>(c->tomb.p)) return false;  // a filtered search
    if ((size_t)((c->dim + 7u) & ~7u) * 4 + kBatchCapQS * 4 > 64 * 1024) return false;  // qs_possible's row length
    if (c->s6_disabled || c->shadow6_state < 0 || (c->shadow6_state == 1 && c->shadow6_finite == 0)) return false;
    if (c->scan_path == 7) return true;
    if (c->scan_path != 0 || c->qs_disabled || !c->tune.i8_shadow || c->tune.stream_i8 == 0 || !c->tune.stream_6b) return false;
    return stream_6b_shape(c->n, c->dim, sc.metric, sc.k);
}

constexpr uint32_t kWideFinalMaxDim = 16384;  // widest Float32 row whose InnerProduct / Cosine keys the f32 MFMA kernel may finalise (use_batched_path)

// Scan path 4 applies to one or two queries on a Float32 corpus whose shadow exists (or can be built now).
bool stream_shadow_wanted(const mvfgpu_corpus* c, uint32_t nq) {
    if (c->dtype != MVF_DTYPE_FLOAT32 || nq > 2 || c->n == 0) return false;
    if (c->scan_path != 4) return false;
    return (size_t)((c->dim + 7u) & ~7u) * 4 + kBatchCap * 4 <= 64 * 1024;  // the re-scoring kernel keeps the query in LDS
}

// Batched MFMA route or K1.  Where it answers K1 for ONE Float32 query, search_device first asks stream_qs_wanted: from
// kStreamI8MinBytes of rows K1 then streams the int8 shadow instead of the stored rows (same kernel, a quarter of the bytes,
// the same bits) -- mvfgpu_selftest_route still reports route 0 there, mvfgpu_selftest_stream_rows which rows K1 reads.
bool use_batched_path(const mvfgpu_corpus* c, uint8_t metric, uint32_t nq) {
    if (c->scan_path == 1) return false;
    // Float32 / Float16: every metric (L2 = GEMM-form selection with an error margin + exact re-scoring);
    // Int8 / UInt8: every metric, exact integers (UInt8 rides the signed MFMA shifted by 128).
    bool supported = true;
    if ((metric == MVF_METRIC_L2 || c->dtype == MVF_DTYPE_FLOAT16) && !is_int_dtype(c->dtype) &&
        (size_t)((c->dim + 7u) & ~7u) * 4 + kBatchCap * 4 > 64 * 1024)
        supported = false;  // the re-scoring kernel keeps the query in LDS
    // Float32 InnerProduct / Cosine beyond the shadows' reach (dimension > 12288) are left to the exact f32 MFMA kernel, whose
    // keys are FINAL: nothing re-scores them.  Each of its sums is one long chain of accumulations over the row, and on rows whose
    // products share a sign its rounding grows with the row: 0.51-0.55 of DESIGN section 3's tolerance at 12296-16000
    // dimensions, 0.61 at 20000, 0.75 at 28000, 0.90-1.006 at 38656 (worst entry of 130 queries x 100 results on 3000 rows;
    // K1's 64 short chains stay at 0.02: tests/test_gpu_wide_rows.py group D caught it).  Wider rows go to K1.
    if (c->dtype == MVF_DTYPE_FLOAT32 && metric != MVF_METRIC_L2 && c->dim > kWideFinalMaxDim) supported = false;
    if (!supported) return false;
    if (c->scan_path == 2 || c->scan_path == 3 || (c->scan_path == 5 && !is_int_dtype(c->dtype))) return true;
    if (path_streams_i8(c) && !is_int_dtype(c->dtype)) return nq > 4;
    // K1 takes up to 4 queries per pass over the rows; K2 costs a flat padded-tile time -- since the streaming MFMA kernel
    // (scan_mfma16_sb.hip) about ONE pass over the int8 shadow / the Int8 rows for up to 64 queries, plus ~0.1 ms of phase
    // launches.  Measured crossovers (scripts/probe_small_corpora.py, profiles/r02_small_corpora_crossover.txt): Float32 /
    // Float16 rows with a shadow from 2 queries up at every size measured (1M x 768 f32, 16 queries: 0.25 ms against K1's
    // 2.4 -- until round 2 corpora under 1 GiB kept K1 up to 31 queries), Int8 / UInt8 rows from 5 (from 2 on 2 GiB and more,
    // 1 GiB when the rows are <= 256 B: the four-query pass of K1 holds 4.3-5.3 TB/s on 768-B rows and ~3 TB/s on
    // short ones, the streaming MFMA kernel 6.2 behind ~0.13 ms of fixed cost -- 50M x 768, 2 queries: 7.3 -> 6.2 ms), Float32 rows without
    // a shadow (exact f32 MFMA kernel, 128-query tiles) from 9 on >= 1 GiB and from 32 below.  Corpora under 16 MiB keep K1
    // until the batch is MFMA-sized: their searches take tens of microseconds either way, and the batched path's scratch
    // (128 MiB of candidate regions per handle) would dwarf them.
    const uint64_t bytes = c->n * (uint64_t)c->dim * elem_size(c->dtype);
    const bool shadowed = qs_wanted(c) ||  // int8 selection, else the f16 shadow (runs as Float16)
                          (c->dtype == MVF_DTYPE_FLOAT32 && (c->scan_path == 3 || shadow_enabled(c)) && c->shadow_state >= 0 &&
                           (size_t)((c->dim + 7u) & ~7u) * 4 + kBatchCap * 4 <= 64 * 1024);
    // Mid-size corpora, a pass or two of K1 (profiles/r04_small_corpora_crossover.txt, round 4: K1's four-query pass got its
    // counting merge, batched staging and a short first piece; the batched route costs 70-100 us before its first row): two to
    // four queries stay on K1 up to 512 MB of float rows (100k x 128 f32: 41 against 90 us; 300k x 768 f16: 135 against 167),
    // up to eight on <= 160 MB; Int8 / UInt8 rows up to eight queries on <= 96 MB (<= 256 MB when rows are >= 512 B) and
    // sixteen on <= 32 MB of such rows (30k x 768: 54 against 97 us).
    if (bytes >= (16ull << 20)) {
        const uint32_t row_bytes = c->dim * elem_size(c->dtype);
        if (!is_int_dtype(c->dtype)) {
            if (shadowed && nq <= 4 && bytes <= (512ull << 20)) return false;
            if (shadowed && nq <= 8 && bytes <= (160ull << 20)) return false;
        } else {
            if (nq <= 8 && bytes <= ((row_bytes >= 512u ? 256ull : 96ull) << 20)) return false;
            if (nq <= 16 && bytes <= (32ull << 20) && row_bytes >= 512u) return false;
        }
    }
    // (round 5, the same probe on the final tree: K1's passes over SHORT rows cost by the row, not by the byte -- 100k x 128 int8,
    //  13 MB: 12 / 16 queries 111 / 145 us against 97 / 96 batched; 30k x 128 f16, 7.7 MB, whose rows K1 converts: 16 / 32 queries
    //  79 / 153 us against 72 / 76)
    const uint32_t small = c->n >= 65536u ? 12u : (c->n >= 24576u && c->dtype == MVF_DTYPE_FLOAT16) ? 16u : 0u;
    const uint32_t threshold = bytes < (8ull << 20)                           ? (small ? small : 33u)  // (32 queries = 8 fused passes: 37-39 us against 73-85)
                               : bytes < (16ull << 20)                        ? (small ? small : 32u)
                               : c->dtype == MVF_DTYPE_FLOAT32 && !shadowed ? (bytes < (1ull << 30) ? 32u : 9u)
                               : is_int_dtype(c->dtype)                     ? (bytes < ((c->pitch <= 256u ? 2ull : 4ull) << 29) ? 5u : 2u)
                                                                            : 2u;
    return nq >= threshold;
}

// ---- upload pipeline: the step in front of the path ------------------------------------------------
// The host rows (an mmap'd MVF block: any alignment, stride >= row bytes) reach HBM in chunks on the copy stream while
// a second stream re-pitches, and -- on request -- computes the row norms (K4) and the f16 shadow of the chunk before:
//   copy stream   : H2D chunk i           | H2D chunk i+1            | ...
//   compute stream:   (wait ev_copy[i])  re-pitch i, norms i, shadow i |  ...
// so a corpus that will serve batched searches is ready for the first of them when the last chunk lands.
//   * rows tightly packed and a multiple of 16 B: chunks go straight to their place (no staging, no re-pitch);
//   * otherwise a chunk is copied AS IT LIES (gaps included) into one of two device staging buffers and the re-pitch
//     kernel reads it with the host stride -- only row_bytes of each row are read from the stage, the 16-B padding
//     is written as zeros (K1, the norms and the shadow all consume whole 16-B vectors).  Rows further apart than
//     twice their size go through hipMemcpy2DAsync instead (no point in moving the gaps over PCIe).
//   * source memory: pageable by default -- the runtime's own pinned bounce buffers already move a 1-D copy from
//     pageable / mmap'd memory at ~56 of the 63 GB/s PCIe Gen5 x16 offers; MVFGPU_UPLOAD_PINNED_STAGING instead
//     double-buffers through two pinned host chunks filled by a pool of memcpy threads (A/B: scripts/probe_upload.py).
struct PinnedPair {
    void* p[2] = {nullptr, nullptr};
    ~PinnedPair() {
        for (auto q : p)
            if (q) (void)hipHostFree(q);
    }
};
struct StagePair {
    unsigned char* p[2] = {nullptr, nullptr};
    ~StagePair() {
        for (auto q : p)
            if (q) (void)hipFree(q);
    }
};
struct EventSet {
    hipEvent_t e[6] = {};
    ~EventSet() {
        for (auto q : e)
            if (q) (void)hipEventDestroy(q);
    }
};

void parallel_memcpy(void* dst, const void* src, size_t bytes, unsigned threads) {
    if (threads <= 1 || bytes < ((size_t)8 << 20)) {
        std::memcpy(dst, src, bytes);
        return;
    }
    std::vector<std::thread> pool;
    const size_t part = ((bytes / threads) + 4095) & ~(size_t)4095;
    for (unsigned t = 0; t < threads; t++) {
        const size_t o = (size_t)t * part;
        if (o >= bytes) break;
        const size_t len = std::min(part, bytes - o);
        pool.emplace_back([=] { std::memcpy(static_cast<char*>(dst) + o, static_cast<const char*>(src) + o, len); });
    }
    for (auto& t : pool) t.join();
}

int upload_rows(mvfgpu_corpus* c, const void* rows, uint64_t stride, const mvfgpu_upload_options& o) {
    const uint64_t n = c->n, row_bytes = (uint64_t)c->dim * elem_size(c->dtype);
    const bool direct = stride == row_bytes && row_bytes == c->pitch;
    const bool sparse = !direct && stride > 2 * row_bytes;  // 2-D copies: do not move the gaps
    // pinned double-buffered staging is the default for uploads of 256 MiB and more (measured, 30.72 GB of pageable rows,
    // profiles/r02_upload_pipeline.txt: 50 GB/s against 10-21 GB/s handing the pageable source to the runtime)
    const uint64_t total_span = (n - 1) * stride + row_bytes;
    const bool pinned = !sparse && ((o.flags & MVFGPU_UPLOAD_PINNED_STAGING) != 0 ||
                                    ((o.flags & MVFGPU_UPLOAD_PAGEABLE) == 0 && total_span >= ((uint64_t)256 << 20)));
    const uint64_t chunk_bytes = (uint64_t)(o.chunk_mib ? o.chunk_mib : (pinned ? 64u : 256u)) << 20;
    const uint64_t chunk_rows = std::max<uint64_t>(1, chunk_bytes / stride);
    const unsigned char* src = static_cast<const unsigned char*>(rows);
    MVF_HIP_TRY(hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking));
    hipStream_t s_copy = c->own_stream, s_comp = c->up_stream;

    // what the compute stream prepares per chunk
    bool want_norms = (o.flags & (MVFGPU_UPLOAD_EAGER_NORMS | MVFGPU_UPLOAD_EAGER_SHADOW)) != 0;
    // which selection copy the batched searches of this corpus will use: the int8 shadow (Float32 and Float16 rows; the
    // default) or, with MVF_I8_SHADOW=0, the f16 shadow of Float32 rows
    bool want_shadow8 = (o.flags & MVFGPU_UPLOAD_EAGER_SHADOW) != 0 && qs_wanted(c);
    bool want_shadow = (o.flags & MVFGPU_UPLOAD_EAGER_SHADOW) != 0 && !want_shadow8 && c->dtype == MVF_DTYPE_FLOAT32 && shadow_enabled(c);
    float* xn = nullptr;
    const size_t nn = norm_stride(n);
    if (want_norms) {
        MVF_HIP_TRY(c->xnorm.reserve((norm_max_at(n) + 1) * 4));
        xn = static_cast<float*>(c->xnorm.p);
        if (!is_int_dtype(c->dtype)) MVF_HIP_TRY(hipMemsetAsync(xn + norm_max_at(n), 0, 4, s_comp));
    }
    if (want_shadow) {
        const size_t need = (size_t)n * shadow_pitch(c->dim);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < need + ((size_t)2 << 30) ||
            c->shadow.reserve(need) != hipSuccess || c->xscale.reserve(((size_t)n + 256) * 4) != hipSuccess) {
            (void)hipGetLastError();
            c->shadow.release();
            c->xscale.release();
            want_shadow = false;  // as ensure_shadow: the searches then use the exact f32 kernel
        }
    }

    if (want_shadow8) {
        const size_t need = (size_t)n * shadow8_pitch(c->dim);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < need + ((size_t)2 << 30) ||
            c->shadow8.reserve(need) != hipSuccess || c->xscale8.reserve(((size_t)n + 256) * 4) != hipSuccess ||
            c->qs_stats.reserve(16) != hipSuccess) {
            (void)hipGetLastError();
            c->shadow8.release();
            c->xscale8.release();
            want_shadow8 = false;
        } else {
            MVF_HIP_TRY(hipMemsetAsync(c->qs_stats.p, 0, 16, s_comp));  // the four bound maxima accumulate over the chunks
        }
    }

    StagePair stage;
    PinnedPair pin;
    EventSet ev;  // [0,1] copy of buffer b landed, [2,3] compute on buffer b done, [4,5] H2D out of pinned buffer b done
    for (auto& e : ev.e) MVF_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const uint64_t span_max = (std::min(chunk_rows, n) - 1) * stride + row_bytes;  // bytes of one chunk as it lies
    if (!direct && !sparse)
        for (auto& q : stage.p) {
            MVF_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q), span_max));
            MVF_HIP_TRY(poison_fill(q, span_max));
        }
    if (pinned)
        for (auto& q : pin.p) {
            MVF_HIP_TRY(hipHostMalloc(&q, span_max, hipHostMallocDefault));
            poison_fill_host(q, span_max);
        }
    if (sparse && c->pitch != row_bytes) MVF_HIP_TRY(hipMemsetAsync(c->d_rows, 0, c->rows_bytes, s_copy));  // the 16-B padding
    unsigned threads = std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
    if (c->tune.upload_threads) threads = c->tune.upload_threads;

    // (Rows handed over straight off an mmap'd .mvf: with the page cache warm the copy threads' minor faults cost nothing
    // measurable -- 52 GB/s, the same as anonymous memory; cold, the file's device sets the rate, and MADV_WILLNEED on the
    // chunks ahead of the copy changed nothing (profiles/r04_upload_from_mmap.txt), so there is no readahead code here.)
    uint64_t i = 0;
    for (uint64_t r0 = 0; r0 < n; r0 += chunk_rows, i++) {
        const int b = (int)(i & 1);
        const uint64_t h = std::min(chunk_rows, n - r0);
        const uint64_t span = (h - 1) * stride + row_bytes;
        unsigned char* place = c->d_rows + r0 * c->pitch;
        if (!direct && !sparse && i >= 2) MVF_HIP_TRY(hipEventSynchronize(ev.e[2 + b]));  // stage b: its re-pitch is done
        if (sparse) {
            MVF_HIP_TRY(hipMemcpy2DAsync(place, c->pitch, src + r0 * stride, stride, row_bytes, h, hipMemcpyHostToDevice, s_copy));
        } else {
            unsigned char* dst = direct ? place : stage.p[b];
            if (pinned) {
                if (i >= 2) MVF_HIP_TRY(hipEventSynchronize(ev.e[4 + b]));  // pinned buffer b: its H2D is done
                parallel_memcpy(pin.p[b], src + r0 * stride, span, threads);
                MVF_HIP_TRY(hipMemcpyAsync(dst, pin.p[b], span, hipMemcpyHostToDevice, s_copy));
                MVF_HIP_TRY(hipEventRecord(ev.e[4 + b], s_copy));
            } else {
                MVF_HIP_TRY(hipMemcpyAsync(dst, src + r0 * stride, span, hipMemcpyHostToDevice, s_copy));
            }
        }
        MVF_HIP_TRY(hipEventRecord(ev.e[b], s_copy));
        MVF_HIP_TRY(hipStreamWaitEvent(s_comp, ev.e[b], 0));
        if (!direct && !sparse)
            MVF_HIP_TRY(launch_repack_rows(stage.p[b], place, h, (uint32_t)row_bytes, stride, c->pitch, s_comp));
        if (want_norms) {
            if (c->dtype == MVF_DTYPE_FLOAT32)
                MVF_HIP_TRY(launch_row_norms_f32(place, (uint32_t)h, c->pitch, xn + r0, xn + nn + r0, xn + norm_max_at(n), s_comp));
            else
                MVF_HIP_TRY(launch_row_norms16(place, c->dtype, (uint32_t)h, c->pitch, c->dim, xn + r0, xn + nn + r0,
                                           xn + norm_max_at(n), s_comp));
        }
        if (want_shadow8)
            MVF_HIP_TRY(launch_shadow_i8(place, c->dtype, (uint32_t)h, c->pitch, c->dim,
                                     static_cast<unsigned char*>(c->shadow8.p) + r0 * shadow8_pitch(c->dim), shadow8_pitch(c->dim),
                                     static_cast<float*>(c->xscale8.p) + r0, static_cast<float*>(c->qs_stats.p), s_comp));
        if (want_shadow)
            MVF_HIP_TRY(launch_shadow_f16(place, (uint32_t)h, c->pitch, c->dim,
                                      static_cast<unsigned char*>(c->shadow.p) + r0 * shadow_pitch(c->dim), shadow_pitch(c->dim),
                                      static_cast<float*>(c->xscale.p) + r0, s_comp));
        MVF_HIP_TRY(hipEventRecord(ev.e[2 + b], s_comp));
    }
    MVF_HIP_TRY(hipStreamSynchronize(s_copy));
    MVF_HIP_TRY(hipStreamSynchronize(s_comp));
    if (want_norms) c->xnorm_ready = true;
    c->shadow_state = want_shadow ? 1 : c->shadow_state;
    c->shadow8_state = want_shadow8 ? 1 : c->shadow8_state;
    if (want_shadow8) c->shadow8_finite = -1;
    return MVF_OK;
}

// k beyond one pass (MVFGPU_K_PER_PASS): ceil(k / 1024) passes of the streaming kernel, pass p returning the 1024 best rows
// ranked STRICTLY BEHIND the last row of pass p - 1 -- composites (order key << 32 | row) are distinct and totally ordered,
// so "behind the floor" is exactly the set of rows not yet returned.  The floor travels on the device (select_final writes
// it, the next pass's scan reads it): no host wait.  The reference takes any k: usize (examples/similarity_search.rs:143,
// :166-168); its heap holds k + 1 entries whatever k is.
int search_large_k(const mvfgpu_corpus* c, SearchCall& sc) {
    const uint32_t k = sc.k;
    MVF_HIP_TRY(c->floor1.reserve((size_t)sc.nq * 8));
    uint64_t* fl = static_cast<uint64_t*>(c->floor1.p);
    for (uint32_t off = 0; off < k; off += MVFGPU_K_PER_PASS) {
        const uint32_t kk = std::min<uint32_t>(MVFGPU_K_PER_PASS, k - off);
        int rc = inner_search(sc, kk, sc.d_scores, sc.d_indices, sc.d_raw, [&](SearchCall& in) {
            return search_stream_path(c, in, /*profile=*/off == 0, nullptr, off ? fl : nullptr, fl, k, off);
        });
        if (rc != MVF_OK) return rc;
    }
    return MVF_OK;
}

// k beyond what passes are worth -- and any k beyond MVFGPU_K_BY_PASSES: ONE pass of the streaming kernel per 1-4 queries
// that writes every row's composite (8 bytes per row) instead of selecting, a device-wide sort of each query's composites
// (sort_topk.hip) and the formatting of the first k.  Exact, no host wait, any k (entries beyond the live rows pad); costs
// the scan + ~130 bytes of sort traffic per row, i.e. less than a second pass whenever rows are longer than that.
// Returns MVF_ERR_DEVICE with *no_room set when the buffers (16 bytes per row and query of a pass + scratch) do not fit.
int search_sorted_k(const mvfgpu_corpus* c, SearchCall& sc, bool* no_room) {
    const uint32_t nq = sc.nq, k = sc.k;
    hipStream_t s = sc.stream;
    *no_room = false;
    size_t tmp_bytes = 0;
    if (c->n > 0) MVF_HIP_TRY(sort_composites(nullptr, &tmp_bytes, nullptr, nullptr, (size_t)c->n, (size_t)k, nullptr, s, 4, (size_t)c->n));
    tmp_bytes = std::max<size_t>(tmp_bytes, 256);
    RankAll ra{};
    ra.k_out = k;
    // the dumping scan: nothing is selected, so the kernel's own list length is the smallest its LDS layout takes
    auto dump_scan = [&]() {
        return inner_search(sc, 16, sc.d_scores, sc.d_indices, sc.d_raw, [&](SearchCall& in) {
            return search_stream_path(c, in, /*profile=*/true, nullptr, nullptr, nullptr, 0, 0, &ra);
        });
    };
    // Up to 1 GiB the buffers stay with the handle; beyond it (50M rows x four queries: 3.2 GB) they come from the stream-ordered
    // allocator for this search only -- memory a later shadow build or upload may need, and no host wait either way.
    constexpr size_t kKeep = 1ull << 30;
    for (int nqv = nq >= 2 ? 4 : 1;; nqv = 1) {
        const size_t bytes = (std::max<size_t>((size_t)nqv * c->n * 8, 256) + 255) & ~(size_t)255;
        if (2 * bytes + tmp_bytes > kKeep) {
            void* scratch = nullptr;
            if (hipMallocAsync(&scratch, 2 * bytes + tmp_bytes, s) == hipSuccess) {
                MVF_HIP_TRY(poison_fill(scratch, 2 * bytes + tmp_bytes, s));
                ra.nqv = nqv;
                ra.a = static_cast<uint64_t*>(scratch);
                ra.b = reinterpret_cast<uint64_t*>(static_cast<unsigned char*>(scratch) + bytes);
                ra.tmp = static_cast<unsigned char*>(scratch) + 2 * bytes;
                ra.tmp_bytes = tmp_bytes;
                const int rc = dump_scan();
                const hipError_t ef = hipFreeAsync(scratch, s);
                if (rc != MVF_OK) return rc;
                MVF_HIP_TRY(ef);
                return MVF_OK;
            }
            (void)hipGetLastError();
        } else if (c->rank_a.reserve(bytes) == hipSuccess && c->rank_b.reserve(bytes) == hipSuccess &&
                   c->rank_tmp.reserve(tmp_bytes) == hipSuccess) {
            ra.nqv = nqv;
            break;
        } else {
            (void)hipGetLastError();
            c->rank_a.release();
            c->rank_b.release();
            c->rank_tmp.release();
        }
        if (nqv == 1) {
            if (c->shadow8_state == 2) {  // a shadow of what fitted took the room: the search the caller asked for comes first
                MVF_HIP_TRY(hipStreamSynchronize(s));  // nothing may still read it
                c->shadow8.release();
                c->xscale8.release();
                c->shadow8_state = -2;
                c->shadow8_rows = 0;
                continue;  // once more, one query per pass
            }
            *no_room = true;
            return fail(MVF_ERR_DEVICE, "no device memory for the whole-shard sort of a large-k search (16 bytes per row)");
        }
    }
    ra.a = static_cast<uint64_t*>(c->rank_a.p);
    ra.b = static_cast<uint64_t*>(c->rank_b.p);
    ra.tmp = c->rank_tmp.p;
    ra.tmp_bytes = c->rank_tmp.bytes;
    return dump_scan();
}

// Passes or the select + sort?  Measured in one process on every benchmark shape (profiles/r05_any_k.txt; round 4's library
// sort: profiles/r04_any_k.txt): the sort route wins from the second pass on nearly everywhere (10M x 768 f32, k = 16384:
// 72.5 -> 4.9 ms; four queries: 272 -> 5.9) -- a pass reads the rows again and its 1024-entry lists are heavy (doubly so four
// queries at a time), the select moves 8-byte entries only.  Passes keep what a model of the two costs gives them: one or two
// passes over a SMALL corpus (10k rows, k = 2048: 0.11 against 0.17 ms; four queries: 0.12 against 0.19), where the sort
// route's chain of a dozen short launches is the larger cost.  The model: a pass = the scan + what its lists cost (~75 us a
// full 1024-entry pass on corpora that fill the chip, a tenth of it the last, shorter one); the sort route = one dumping scan
// + ~100 us of launches (+10 per further query of the pass) + 40 bytes of traffic per row and query.
// MVF_LARGE_K forces one of them (A/B, tests).
bool large_k_by_sort(const mvfgpu_corpus* c, uint32_t nq, uint32_t k) {
    if (k > MVFGPU_K_BY_PASSES) return true;
    if (c->tune.large_k) return c->tune.large_k == 2;
    const double full = (double)(k / MVFGPU_K_PER_PASS), partial = (k % MVFGPU_K_PER_PASS) ? 1.0 : 0.0, scans = nq >= 2 ? (double)((nq + 3) / 4) : 1.0;
    const double row_bytes = std::max(128.0, (double)c->dim * elem_size(c->dtype));  // short rows scan no faster than 128-byte ones
    const double pass_us = std::max(40.0, (double)c->n * row_bytes / 5.0e6);         // 5 TB/s = 5e6 bytes per us
    const double lists_us = 75.0 * std::min(1.0, (double)c->n / 500.0e3);
    const double passes_us = scans * (nq >= 2 ? 2.0 : 1.0) * (full * (pass_us + lists_us) + partial * (pass_us + 0.15 * lists_us));
    const double sort_us = scans * (pass_us + 100.0 + 10.0 * (double)(std::min(nq, 4u) - 1)) + (double)nq * (double)c->n / 150.0e3;
    return sort_us < passes_us;
}

int check_query_args(const mvfgpu_corpus* c, uint8_t metric, const void* queries, uint8_t query_dtype,
                     uint32_t query_dim, uint32_t nq, uint32_t k, const void* out_scores, const void* out_indices) {
    if (!c) return fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    if (const int rc = check_search_scalars(metric, nq, k, queries, out_scores, out_indices)) return rc;
    const uint8_t want = is_int_dtype(c->dtype) ? c->dtype : (uint8_t)MVF_DTYPE_FLOAT32;
    if (query_dtype != want)
        return fail(MVF_ERR_BUILD, "query data type must be Float32 for Float32/Float16 spaces and the space's own type for Int8/UInt8");
    if (query_dim != c->dim) {
        g_last_error = "Dimension mismatch: expected " + std::to_string(c->dim) + ", got " + std::to_string(query_dim);
        return MVF_ERR_DIMENSION_MISMATCH;  // reference src/errors.rs:24
    }
    return MVF_OK;
}

}  // namespace

namespace mvf {
CorpusView corpus_view(const mvfgpu_corpus* c) {
    CorpusView v;
    v.device = c->device, v.num_cus = c->num_cus, v.k1_g = c->tune.k1_g;
    v.n = c->n, v.index_base = c->index_base;
    v.dim = c->dim, v.pitch = c->pitch, v.V = c->V, v.dtype = c->dtype;
    v.rows = c->d_rows;
    v.tomb = static_cast<const uint32_t*>(c->tomb.p);
    v.tomb_gen = c->tomb_gen;
    v.filter_route = c->tune.filter_route;
    v.maxsim_scratch = c->tune.maxsim_scratch;
    v.maxsim_route = c->maxsim_route ? c->maxsim_route : c->tune.maxsim_route;
    v.ids = static_cast<const uint64_t*>(c->ids.p);
    v.stream = c->own_stream;
    v.scan_path = c->scan_path;
    return v;
}
int corpus_row_norms(const mvfgpu_corpus* c, void* stream, const float** xnorm, const float** xx2, const float** xxmax) {
    const int rc = ensure_norms(c, static_cast<hipStream_t>(stream));
    if (rc != MVF_OK) return rc;
    const float* xn = static_cast<const float*>(c->xnorm.p);
    *xnorm = xn;
    *xx2 = xn + norm_stride(c->n);
    *xxmax = xn + norm_max_at(c->n);
    return MVF_OK;
}
std::mutex& corpus_host_mutex(const mvfgpu_corpus* c) { return c->host_mu; }
void k1_group(uint32_t V, int nqv, int forced, int* G, uint32_t* J) { choose_group(V, nqv, G, J, forced); }
bool corpus_ids_to_positions(const mvfgpu_corpus* c, const uint64_t* ids, uint64_t count, uint64_t* out) {
    if (c->h_ids.empty()) return false;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->id_index.empty()) {
        c->id_index.reserve(c->h_ids.size());
        for (size_t r = 0; r < c->h_ids.size(); r++) c->id_index.emplace_back(c->h_ids[r], (uint32_t)r);
        std::sort(c->id_index.begin(), c->id_index.end());
    }
    for (uint64_t i = 0; i < count; i++) {
        out[i] = ~0ull;
        if (ids[i] == ~0ull) continue;
        auto it = std::lower_bound(c->id_index.begin(), c->id_index.end(), std::make_pair(ids[i], 0u));
        if (it != c->id_index.end() && it->first == ids[i]) out[i] = c->index_base + it->second;  // duplicates: the first position holding the id
    }
    return true;
}
int corpus_pinned_mirrors(const mvfgpu_corpus* c, size_t in_bytes, size_t out_bytes, void** pin_in, void** pin_out) {
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->has_done && c->confirmed_gen != c->work_gen) MVF_HIP_TRY(hipEventSynchronize(c->ev_done[c->done_idx]));
    MVF_HIP_TRY(c->pin_q.reserve(in_bytes));
    MVF_HIP_TRY(c->pin_out.reserve(out_bytes));
    *pin_in = c->pin_q.p;
    *pin_out = c->pin_out.p;
    return MVF_OK;
}
int corpus_device_call(const mvfgpu_corpus* c, void* stream, const std::function<int()>& body) {
    return device_call(c, static_cast<hipStream_t>(stream), body);
}
int corpus_wait_newest(const mvfgpu_corpus* c) {
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->has_done) MVF_HIP_TRY(hipEventSynchronize(c->ev_done[c->done_idx]));
    return MVF_OK;
}
WriteTargets corpus_write_targets(const mvfgpu_corpus* c) {
    WriteTargets t;
    t.rows = c->d_rows;
    t.n = c->n, t.index_base = c->index_base;
    t.dim = c->dim, t.pitch = c->pitch, t.dtype = c->dtype;
    if (c->xnorm_ready) {
        float* xn = static_cast<float*>(c->xnorm.p);
        t.norms = xn;
        t.xx2 = xn + norm_stride(c->n);
        t.xxmax = xn + norm_max_at(c->n);
    }
    if (c->shadow_state == 1) {
        t.shadow16 = static_cast<unsigned char*>(c->shadow.p);
        t.pitch16 = shadow_pitch(c->dim);
        t.xscale = static_cast<float*>(c->xscale.p);
    }
    if (c->shadow8_state == 1 || c->shadow8_state == 2) {
        t.shadow8 = static_cast<unsigned char*>(c->shadow8.p);
        t.pitch8 = shadow8_pitch(c->dim);
        t.shadow8_rows = c->shadow8_state == 1 ? c->n : c->shadow8_rows;
        t.xscale8 = static_cast<float*>(c->xscale8.p);
        t.qs_stats = static_cast<float*>(c->qs_stats.p);
    }
    if (c->shadow6_state == 1) {
        t.shadow6 = static_cast<unsigned char*>(c->shadow6.p);
        t.shadow6_p51 = c->shadow6_p51;
        t.xscale6 = static_cast<float*>(c->xscale6.p);
        t.qs6_stats = static_cast<float*>(c->qs6_stats.p);
    }
    return t;
}
void corpus_rows_written(const mvfgpu_corpus* c, uint32_t refreshed) {
    // a written Inf / NaN row has made the maxima +inf on the device: the next search that asks reads them again
    if (refreshed & 4u) c->shadow8_finite = -1;
    if (refreshed & 8u) c->shadow6_finite = -1;
}
PinnedUpload& corpus_write_upload(const mvfgpu_corpus* c) { return c->write_up; }
int check_search_scalars(uint8_t metric, uint32_t nq, uint32_t k, const void* queries, const void* out_scores, const void* out_indices) {
    if (const int mrc = check_metric(metric)) return mrc;
    if (nq == 0) return fail(MVF_ERR_INVALID_ARGUMENT, "nq must be > 0");
    if (k == 0 || k > MVFGPU_MAX_K) return fail(MVF_ERR_INVALID_ARGUMENT, "k must be in 1..2^31");
    if (!queries || !out_scores || !out_indices) return fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    return MVF_OK;
}
int check_search_args(const mvfgpu_corpus* c, uint8_t metric, const void* queries, uint8_t query_dtype, uint32_t query_dim,
                      uint32_t nq, uint32_t k, const void* out_scores, const void* out_indices) {
    return check_query_args(c, metric, queries, query_dtype, query_dim, nq, k, out_scores, out_indices);
}
}  // namespace mvf

extern "C" {

int mvfgpu_device_count(int* out_count) {
    if (!out_count) return fail(MVF_ERR_INVALID_ARGUMENT, "out_count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        n = 0;
    }
    *out_count = n;
    return MVF_OK;
}

const char* mvfgpu_strerror(int status) {
    switch (status) {
    case MVF_OK: return "ok";
    case MVF_ERR_IO: return "I/O error";
    case MVF_ERR_INVALID_FORMAT: return "Invalid file format";
    case MVF_ERR_UNSUPPORTED_VERSION: return "Unsupported version";
    case MVF_ERR_SPACE_NOT_FOUND: return "Vector space not found";
    case MVF_ERR_INDEX_OUT_OF_BOUNDS: return "Index out of bounds";
    case MVF_ERR_DIMENSION_MISMATCH: return "Dimension mismatch";
    case MVF_ERR_INVALID_VECTOR_TYPE: return "Invalid vector type";
    case MVF_ERR_CORRUPTED_DATA: return "Corrupted data";
    case MVF_ERR_EXTENSION: return "Extension error";
    case MVF_ERR_BUILD: return "Build error";
    case MVF_ERR_DEVICE: return "Device error";
    case MVF_ERR_INVALID_ARGUMENT: return "Invalid argument";
    default: return "unknown status";
    }
}

const char* mvfgpu_last_error_message(void) { return g_last_error.c_str(); }

int mvfgpu_corpus_create_ex(const void* rows, uint64_t n, uint32_t dimension, uint8_t data_type, uint64_t stride_bytes,
                            int device, uint64_t index_base, const mvfgpu_upload_options* opts, mvfgpu_corpus** out) {
    if (!out) return fail(MVF_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    mvfgpu_upload_options o{};
    if (opts) {
        if (opts->struct_size < 8 || opts->struct_size > 4096) return fail(MVF_ERR_INVALID_ARGUMENT, "upload options: bad struct_size");
        std::memcpy(&o, opts, std::min<size_t>(opts->struct_size, sizeof(o)));
    }
    int rc = validate_shape(n, dimension, data_type);
    if (rc != MVF_OK) return rc;
    const uint64_t row_bytes = (uint64_t)dimension * elem_size(data_type);
    if (n > 0 && !rows) return fail(MVF_ERR_INVALID_ARGUMENT, "rows is NULL");
    if (n > 0 && stride_bytes < row_bytes)
        return fail(MVF_ERR_CORRUPTED_DATA, "Invalid stride alignment");  // cf. reference src/vectors/mem.rs:53-59
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        return fail(MVF_ERR_DEVICE, "no HIP device available (libmvf_gpu has no CPU fallback)");
    }
    if (device < 0 || device >= ndev) return fail(MVF_ERR_INVALID_ARGUMENT, "device index out of range");
    DevScope guard(device);
    if (!guard.ok) return fail(MVF_ERR_DEVICE, "hipSetDevice failed");

    auto* c = new mvfgpu_corpus();
    c->device = device;
    c->n = n;
    c->dim = dimension;
    c->dtype = data_type;
    c->index_base = index_base;
    rc = init_common(c);
    if (rc == MVF_OK) rc = alloc_rows(c);
    if (rc == MVF_OK && n > 0) rc = upload_rows(c, rows, stride_bytes, o);
    if (rc != MVF_OK) {
        mvfgpu_corpus_destroy(c);
        return rc;
    }
    *out = c;
    return MVF_OK;
}

int mvfgpu_corpus_create(const void* rows, uint64_t n, uint32_t dimension, uint8_t data_type,
                         uint64_t stride_bytes, int device, uint64_t index_base, mvfgpu_corpus** out) {
    return mvfgpu_corpus_create_ex(rows, n, dimension, data_type, stride_bytes, device, index_base, nullptr, out);
}

int mvfgpu_corpus_create_synthetic(uint64_t n, uint32_t dimension, uint8_t data_type, uint64_t seed, uint64_t row0,
                                   int device, mvfgpu_corpus** out) {
    if (!out) return fail(MVF_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    int rc = validate_shape(n, dimension, data_type);
    if (rc != MVF_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        (void)hipGetLastError();
        return fail(MVF_ERR_DEVICE, "no HIP device available (libmvf_gpu has no CPU fallback)");
    }
    if (device < 0 || device >= ndev) return fail(MVF_ERR_INVALID_ARGUMENT, "device index out of range");
    DevScope guard(device);
    if (!guard.ok) return fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    auto* c = new mvfgpu_corpus();
    c->device = device;
    c->n = n;
    c->dim = dimension;
    c->dtype = data_type;
    c->index_base = row0;
    rc = init_common(c);
    if (rc == MVF_OK) rc = alloc_rows(c);
    if (rc == MVF_OK && n > 0) {
        hipError_t e = launch_synth_rows(c->d_rows, n, dimension, c->pitch, data_type, seed, row0, c->own_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->own_stream);
        if (e != hipSuccess) rc = fail(MVF_ERR_DEVICE, std::string("synthetic fill: ") + hipGetErrorString(e));
    }
    if (rc != MVF_OK) {
        mvfgpu_corpus_destroy(c);
        return rc;
    }
    *out = c;
    return MVF_OK;
}

void mvfgpu_corpus_destroy(mvfgpu_corpus* c) {
    if (!c) return;
    {
        DevScope guard(c->device);
        (void)hipDeviceSynchronize();
        if (c->d_rows) (void)hipFree(c->d_rows);
        c->cand.release();
        c->bq.release();
        c->bstate.release();
        c->bcand.release();
        c->blk.release();
        c->blk_armed_cnt = nullptr;
        c->xnorm.release();
        c->repair.release();
        c->floor1.release();
        c->rank_a.release();
        c->rank_b.release();
        c->rank_tmp.release();
        c->shadow.release();
        c->xscale.release();
        c->tomb.release();
        c->ids.release();
        c->split_out.release();
        c->shadow8.release();
        c->xscale8.release();
        c->qs_stats.release();
        c->shadow6.release();
        c->xscale6.release();
        c->qs6_stats.release();
        c->pub51.release();
        c->h_q.release();
        c->h_s.release();
        c->h_i.release();
        c->h_r.release();
        c->pin_q.release();
        c->pin_flag.release();
        c->done_ticket.release();
        c->pin_out.release();
        c->pin_vec.release();
        c->prof_ts.release();
        c->h_v.release();
        c->write_up.release();
        if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
        if (c->up_stream) (void)hipStreamDestroy(c->up_stream);
        for (auto e : c->ev_done)
            if (e) (void)hipEventDestroy(e);
        for (auto e : c->qs_redo_ev)
            if (e) (void)hipEventDestroy(e);
        if (c->qs_redo_host) (void)hipHostFree(c->qs_redo_host);
        for (auto& ps : c->prof)
            for (auto& e : ps.e)
                if (e) (void)hipEventDestroy(e);
    }
    delete c;
}

int mvfgpu_corpus_get_info(const mvfgpu_corpus* c, mvfgpu_corpus_info* out) {
    if (!c || !out) return fail(MVF_ERR_INVALID_ARGUMENT, "NULL argument");
    mvfgpu_corpus_info inf{};
    inf.rows = c->n;
    inf.index_base = c->index_base;
    inf.dimension = c->dim;
    inf.pitch_bytes = c->pitch;
    inf.data_type = c->dtype;
    inf.device = c->device;
    inf.deleted_rows = c->deleted;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        inf.has_vector_ids = c->ids.p ? 1 : 0;
        inf.shadows = (uint8_t)((c->shadow8_state == 1 ? 1 : 0) | (c->shadow_state == 1 ? 2 : 0) | (c->shadow8_state == 2 ? 4 : 0) | (c->shadow6_state == 1 ? 8 : 0));
        inf.selection_state = (uint8_t)((c->qs_disabled ? 1 : 0) | (c->bias_disabled ? 2 : 0) | (c->s6_disabled ? 4 : 0));
        inf.device_bytes = c->tomb.bytes + c->ids.bytes + c->rows_bytes + c->cand.bytes + c->bq.bytes + c->bstate.bytes + c->bcand.bytes +
                           c->xnorm.bytes + c->repair.bytes + c->floor1.bytes + c->rank_a.bytes + c->rank_b.bytes + c->rank_tmp.bytes + c->blk.bytes + c->shadow8.bytes + c->xscale8.bytes + c->qs_stats.bytes + c->split_out.bytes + c->shadow6.bytes + c->xscale6.bytes + c->qs6_stats.bytes + c->pub51.bytes +
                           c->shadow.bytes + c->xscale.bytes + c->h_q.bytes + c->h_s.bytes + c->h_i.bytes + c->h_r.bytes + c->h_v.bytes;
    }
    return copy_out_struct(out, inf);
}

int mvfgpu_corpus_read_rows(const mvfgpu_corpus* c, uint64_t first, uint64_t count, void* out_rows) {
    if (!c || (!out_rows && count)) return fail(MVF_ERR_INVALID_ARGUMENT, "NULL argument");
    if (first + count > c->n || first + count < first) {
        g_last_error = "Index out of bounds: " + std::to_string(first + count) + " >= " + std::to_string(c->n);
        return MVF_ERR_INDEX_OUT_OF_BOUNDS;  // reference src/vectors/vector_space.rs:156-161
    }
    if (count == 0) return MVF_OK;
    DevScope guard(c->device);
    if (const int rc = corpus_wait_newest(c)) return rc;  // a row write may be the handle's newest work (update.hip)
    const uint64_t row_bytes = (uint64_t)c->dim * elem_size(c->dtype);
    MVF_HIP_TRY(hipMemcpy2D(out_rows, row_bytes, c->d_rows + first * c->pitch, c->pitch, row_bytes, count,
                        hipMemcpyDeviceToHost));
    return MVF_OK;
}

namespace {
// mvfgpu_corpus_gather_rows with c->host_mu held by the caller (mvfgpu_search_fetch fetches behind its own search)
int gather_rows_host_locked(const mvfgpu_corpus* c, const uint64_t* indices, uint64_t count, void* out_rows) {
    std::vector<uint64_t> mapped;  // with vector ids a search reports ids: translate them back to positions
    if (!c->h_ids.empty()) {
        mapped.resize(count);
        corpus_ids_to_positions(c, indices, count, mapped.data());
        for (uint64_t i = 0; i < count; i++) {
            if (indices[i] != ~0ull && mapped[i] == ~0ull) {
                g_last_error = "Index out of bounds: vector id " + std::to_string(indices[i]) + " is not in this shard";
                return MVF_ERR_INDEX_OUT_OF_BOUNDS;
            }
        }
        indices = mapped.data();
    }
    for (uint64_t i = 0; i < count; i++) {
        const uint64_t g = indices[i];
        if (g == ~0ull) continue;  // padding of a short result list: a zero row
        if (g < c->index_base || g - c->index_base >= c->n) {
            g_last_error = "Index out of bounds: " + std::to_string(g) + " >= " + std::to_string(c->index_base + c->n);
            return MVF_ERR_INDEX_OUT_OF_BOUNDS;  // reference src/vectors/vector_space.rs:102-107
        }
    }
    DevScope guard(c->device);
    if (!guard.ok) return fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    const uint32_t row_bytes = c->dim * elem_size(c->dtype);
    // small fetches (the payload rows of one result list) go through pinned host memory in place, like mvfgpu_search's
    const size_t ibytes = (size_t)count * 8, obytes = (size_t)count * row_bytes;
    const bool zc_i = ibytes <= c->tune.host_zc_query, zc_o = obytes <= c->tune.host_zc_results;
    void *di, *dout;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        if (c->has_done) MVF_HIP_TRY(hipEventSynchronize(c->ev_done[c->done_idx]));
        if (zc_i) {
            MVF_HIP_TRY(c->pin_q.reserve(ibytes));
            memcpy(c->pin_q.p, indices, ibytes);
            di = c->pin_q.p;
        } else {
            MVF_HIP_TRY(c->h_i.reserve(ibytes));
            di = c->h_i.p;
        }
        if (zc_o) {
            MVF_HIP_TRY(c->pin_out.reserve(obytes));
            dout = c->pin_out.p;
        } else {
            MVF_HIP_TRY(c->h_q.reserve(obytes));
            dout = c->h_q.p;
        }
    }
    if (!zc_i) MVF_HIP_TRY(hipMemcpyAsync(di, indices, ibytes, hipMemcpyHostToDevice, c->own_stream));
    MVF_HIP_TRY(launch_gather_rows(c->d_rows, c->n, c->pitch, row_bytes, c->index_base, static_cast<const uint64_t*>(di),
                               (uint32_t)count, static_cast<unsigned char*>(dout), c->own_stream));
    if (!zc_o) MVF_HIP_TRY(hipMemcpyAsync(out_rows, dout, obytes, hipMemcpyDeviceToHost, c->own_stream));
    MVF_HIP_TRY(hipStreamSynchronize(c->own_stream));
    if (zc_o) memcpy(out_rows, dout, obytes);
    return MVF_OK;
}
}  // namespace

int mvfgpu_corpus_gather_rows(const mvfgpu_corpus* c, const uint64_t* indices, uint64_t count, void* out_rows) {
    if (!c || (count && (!indices || !out_rows))) return fail(MVF_ERR_INVALID_ARGUMENT, "NULL argument");
    if (count == 0) return MVF_OK;
    if (count > 0xFFFFFFFFull) return fail(MVF_ERR_INVALID_ARGUMENT, "too many rows in one gather");
    std::lock_guard<std::mutex> host_lk(c->host_mu);
    return gather_rows_host_locked(c, indices, count, out_rows);
}

int mvfgpu_corpus_set_tombstones(mvfgpu_corpus* c, const uint8_t* bitmap, uint64_t first_bit, uint64_t nbits) {
    if (!c) return fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    DevScope guard(c->device);
    if (!guard.ok) return fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> lk(c->mu);
    MVF_HIP_TRY(hipDeviceSynchronize());  // searches in flight still read the old bitmap
    if (!bitmap || nbits == 0) {
        c->tomb.release();
        c->deleted = 0;
        c->tomb_gen++;
        return MVF_OK;
    }
    if (first_bit + c->n > nbits || first_bit + c->n < first_bit)
        return fail(MVF_ERR_INVALID_ARGUMENT, "tombstone bitmap covers fewer rows than the shard holds");
    const size_t words = ((size_t)c->n + 31) / 32;
    std::vector<uint32_t> w(words + 1, 0u);
    uint64_t dead = 0;
    for (uint64_t r = 0; r < c->n; r++) {  // re-base to local rows (first_bit need not be a multiple of 8)
        const uint64_t b = first_bit + r;
        if ((bitmap[b >> 3] >> (b & 7)) & 1u) {
            w[r >> 5] |= 1u << (r & 31);
            dead++;
        }
    }
    c->tomb_gen++;
    if (dead == 0) {
        c->tomb.release();
        c->deleted = 0;
        return MVF_OK;
    }
    MVF_HIP_TRY(c->tomb.reserve((words + 1) * 4));
    MVF_HIP_TRY(hipMemcpy(c->tomb.p, w.data(), (words + 1) * 4, hipMemcpyHostToDevice));
    c->deleted = dead;
    return MVF_OK;
}

int mvfgpu_corpus_set_vector_ids(mvfgpu_corpus* c, const void* ids_le, uint64_t n) {
    if (!c) return fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    DevScope guard(c->device);
    if (!guard.ok) return fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    std::lock_guard<std::mutex> lk(c->mu);
    MVF_HIP_TRY(hipDeviceSynchronize());
    c->id_index.clear();
    if (!ids_le || n == 0) {
        c->ids.release();
        c->h_ids.clear();
        return MVF_OK;
    }
    if (n != c->n) return fail(MVF_ERR_INVALID_ARGUMENT, "vector id count differs from the shard's row count");
    c->h_ids.resize(n);
    std::memcpy(c->h_ids.data(), ids_le, (size_t)n * 8);  // the block may sit at any alignment in the mapping
    MVF_HIP_TRY(c->ids.reserve((size_t)n * 8));
    MVF_HIP_TRY(hipMemcpy(c->ids.p, c->h_ids.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    return MVF_OK;
}

namespace {
int search_device(const mvfgpu_corpus* c, uint8_t metric, const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                  uint32_t k, float* d_scores, uint64_t* d_indices, int32_t* d_raw, void* hip_stream, HostFlagReq* req,
                  const FilterUse* flt = nullptr);
}

int mvfgpu_search_device(const mvfgpu_corpus* c, uint8_t metric, const void* d_queries, uint8_t query_dtype,
                         uint32_t query_dim, uint32_t nq, uint32_t k, float* d_scores, uint64_t* d_indices,
                         int32_t* d_raw, void* hip_stream) {
    return search_device(c, metric, d_queries, query_dtype, query_dim, nq, k, d_scores, d_indices, d_raw, hip_stream, nullptr);
}

namespace {
// The search itself: profiling events, the route, its kernels on `s`.  The caller holds c->mu, has ordered `s` behind the
// handle's newest work and records ev_done on every way out (search_device below; the join through corpus_device_call).
int search_locked(const mvfgpu_corpus* c, SearchCall& sc) {
    const uint8_t metric = sc.metric;
    const uint32_t nq = sc.nq, k = sc.k;
    hipStream_t s = sc.stream;
    int rc = MVF_OK;
    c->search_launches = 0;
    mvfgpu_corpus::ProfSlot* wps = nullptr;  // whole-search events: every kernel of this call on the stream
    const uint64_t prof_before = c->prof_next;
    if (c->profiling) {
        wps = &c->prof[c->prof_next % mvfgpu_corpus::kProfSlots];
        for (auto& e : wps->e)
            if (!e) MVF_HIP_TRY(hipEventCreate(&e));
        wps->whole = wps->ts_whole = false;
    }
    bool e3_recorded = false;
    if (k > MVFGPU_K_PER_PASS) {  // more results than one pass selects: the whole shard ranked by a sort, or passes of the exact streaming kernel
        uint32_t scans = 1;
        bool sorted = false;
        if (wps) MVF_HIP_TRY(hipEventRecord(wps->e[3], s));
        if (large_k_by_sort(c, nq, k)) {
            bool no_room = false;
            rc = search_sorted_k(c, sc, &no_room);
            sorted = rc == MVF_OK;
            if (!sorted && !(no_room && k <= MVFGPU_K_BY_PASSES)) return rc;
        }
        sc.launches_known = false;
        if (!sorted) {
            rc = search_large_k(c, sc);
            if (rc != MVF_OK) return rc;
            scans = (k + MVFGPU_K_PER_PASS - 1) / MVFGPU_K_PER_PASS;
        }
        if (wps && c->prof_next == prof_before + 1) {
            MVF_HIP_TRY(hipEventRecord(wps->e[4], s));
            wps->whole = true;
            c->timing.search_flops = 2ull * nq * c->n * c->dim * scans;
            if (sorted) c->timing.scan_kernel = 8u;  // the streaming kernel as a dump + the whole-shard sort
        }
        return MVF_OK;
    }
    bool shadow_stream = false, qs_stream = false, s6_stream = false;
    if ((stream_qs_wanted(c, nq, k) || stream_6b_wanted(c, sc)) && !is_filtered(c, sc)) qs_feedback_poll(c);  // may switch the int8 selection / the 6-bit stream off
    // K1 on the stored rows and the streamed int8 shadow time themselves (ProfSlot::ts_whole: from the search's first kernel, so
    // not the norms / the shadow a handle's first search builds in front of it); every other route keeps the event pair around the
    // whole call, in front of whatever it builds first.  The route is only known behind those builds: where it was expected to time
    // itself and cannot (no room for the shadow, non-finite maxima) and the batched route answers, e[3] is recorded behind them too
    if (wps && !(stream_qs_wanted(c, nq, k) || stream_6b_wanted(c, sc) || (!stream_shadow_wanted(c, nq) && !use_batched_path(c, metric, nq)))) {
        MVF_HIP_TRY(hipEventRecord(wps->e[3], s));
        e3_recorded = true;
    }
    if (stream_6b_wanted(c, sc)) {  // the 6-bit shadow first; where it cannot be had (no room, a non-finite row) the rules below decide as before
        rc = ensure_norms(c, s);
        if (rc != MVF_OK) return rc;
        hipError_t e = ensure_shadow6(c, s, c->scan_path == 7);
        if (e != hipSuccess) return fail(MVF_ERR_DEVICE, std::string("6-bit shadow build: ") + hipGetErrorString(e));
        s6_stream = c->shadow6_state == 1;
        if (s6_stream && c->shadow6_finite < 0) {  // once per shadow: its bound maxima (one small wait)
            float st[4] = {0.f, 0.f, 0.f, 0.f};
            MVF_HIP_TRY(hipMemcpyAsync(st, c->qs6_stats.p, sizeof(st), hipMemcpyDeviceToHost, s));
            MVF_HIP_TRY(hipStreamSynchronize(s));
            c->shadow6_finite = std::isfinite(st[0]) && std::isfinite(st[1]) && std::isfinite(st[2]) && std::isfinite(st[3]) ? 1 : 0;
        }
        if (s6_stream && c->shadow6_finite == 0) s6_stream = false;  // a row holds Inf / NaN
        qs_stream = s6_stream;
    }
    if (!s6_stream && stream_qs_wanted(c, nq, k)) {
        rc = ensure_norms(c, s);
        if (rc != MVF_OK) return rc;
        hipError_t e = ensure_shadow8(c, s, path_streams_i8(c));
        if (e != hipSuccess) return fail(MVF_ERR_DEVICE, std::string("int8 shadow build: ") + hipGetErrorString(e));
        qs_stream = c->shadow8_state == 1;
        if (qs_stream && c->scan_path == 0 && c->shadow8_finite < 0) {  // once per shadow: its bound maxima (one small wait)
            float st[4] = {0.f, 0.f, 0.f, 0.f};
            MVF_HIP_TRY(hipMemcpyAsync(st, c->qs_stats.p, sizeof(st), hipMemcpyDeviceToHost, s));
            MVF_HIP_TRY(hipStreamSynchronize(s));
            c->shadow8_finite = std::isfinite(st[0]) && std::isfinite(st[1]) && std::isfinite(st[2]) && std::isfinite(st[3]) ? 1 : 0;
        }
        if (qs_stream && c->scan_path == 0 && c->shadow8_finite == 0) qs_stream = false;  // a row holds Inf / NaN: the stored rows
    }
    if (!qs_stream && stream_shadow_wanted(c, nq)) {
        hipError_t e = ensure_shadow(c, s, c->scan_path == 4);
        if (e != hipSuccess) return fail(MVF_ERR_DEVICE, std::string("shadow build: ") + hipGetErrorString(e));
        shadow_stream = c->shadow_state == 1;
    }
    const bool by_clock = wps && (qs_stream || (!shadow_stream && !use_batched_path(c, metric, nq)));
    if (by_clock) {
        rc = prof_ts_ensure(c, s);
        if (rc != MVF_OK) return rc;
        sc.whole_by_clock = true;
    } else if (wps && !e3_recorded) {
        MVF_HIP_TRY(hipEventRecord(wps->e[3], s));
    }
    rc = qs_stream                           ? search_stream_qs_path(c, sc, s6_stream)
         : shadow_stream                     ? search_stream_shadow_path(c, sc)
         : use_batched_path(c, metric, nq) ? search_batched_path(c, sc)
                                           : search_stream_path(c, sc);
    if (rc != MVF_OK) return rc;
    if (sc.launches_known && (qs_stream || !(shadow_stream || use_batched_path(c, metric, nq)))) c->search_launches = sc.launches;
    if (wps && c->prof_next == prof_before + 1) {  // the path filled this slot
        if (by_clock) {
            wps->ts_whole = wps->ts_scan;  // (an empty corpus launches no scan: nothing to time)
        } else {
            MVF_HIP_TRY(hipEventRecord(wps->e[4], s));
            wps->whole = true;
        }
        c->timing.search_flops = 2ull * nq * c->n * c->dim;
    }
    return MVF_OK;
}

// mvfgpu_search_device, and -- with `req` -- the enqueue step of the host-buffer calls (search_host)
int search_device(const mvfgpu_corpus* c, uint8_t metric, const void* d_queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                  uint32_t k, float* d_scores, uint64_t* d_indices, int32_t* d_raw, void* hip_stream, HostFlagReq* req,
                  const FilterUse* flt) {
    int rc = check_query_args(c, metric, d_queries, query_dtype, query_dim, nq, k, d_scores, d_indices);
    if (rc != MVF_OK) return rc;
    DevScope guard(c->device);
    if (!guard.ok) return fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return device_call(c, s, [&]() {  // a call that holds this one search
        if (req) req->gen = c->work_gen;
        // a filter's list route (filter.hip: F2 over the admitted rows), which also answers what admits no row at all
        if (flt && (flt->by_list || flt->admitted == 0 || c->n == 0))
            return filter_list_search(corpus_view(c), *flt, metric, d_queries, nq, k, d_scores, d_indices, d_raw, s);
        // ... or its mask route: the search a plain call runs, the filter's deny mask in the tombstones' place
        SearchCall sc = new_search_call(c, metric, d_queries, nq, k, d_scores, d_indices, d_raw, s, flt ? flt->deny : nullptr);
        sc.flag_req = req;
        return search_locked(c, sc);
    });
}
}  // namespace

namespace {
// mvfgpu_search / mvfgpu_search_fetch / mvfgpu_search_filtered.  out_vectors (nullable): [nq][k] rows of the corpus in their
// stored type.  flt (nullable): the filter of a filtered search, handed down to the search enqueued here.
int search_host(const mvfgpu_corpus* c, uint8_t metric, const void* queries, uint8_t query_dtype, uint32_t query_dim, uint32_t nq,
                uint32_t k, float* out_scores, uint64_t* out_indices, int32_t* out_raw, void* out_vectors, const FilterUse* flt = nullptr) {
    int rc = check_query_args(c, metric, queries, query_dtype, query_dim, nq, k, out_scores, out_indices);
    if (rc != MVF_OK) return rc;
    DevScope guard(c->device);
    if (!guard.ok) return fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    const size_t qbytes = (size_t)nq * c->dim * (is_int_dtype(c->dtype) ? 1 : 4);
    const size_t nres = (size_t)nq * k;
    if (out_vectors && nres > 0xFFFFFFFFull) return fail(MVF_ERR_INVALID_ARGUMENT, "too many rows in one fetch");
    // Small queries / results skip the copy engine: the query is copied (by the CPU) into pinned host memory the kernels
    // read in place, and the selection kernels write the results into pinned host memory -- 10k x 128 f32, top-10:
    // 65 -> 30 us per call (profiles/r04_host_api_latency.txt); three staged hipMemcpyAsync of pageable memory cost more
    // than the search.  Larger transfers keep the device mirrors (a kernel reading megabytes over PCIe stalls its blocks).
    const size_t out_bytes = nres * 16;
    // (queries in place only where the search is short: on a large corpus every block of a pass -- a thousand and more -- would
    // stage its query over PCIe and the re-scoring waves re-read it uncached; there the pinned copy is mirrored into HBM first,
    // ~10 us in front of a search of milliseconds)
    const bool zc_q = qbytes <= c->tune.host_zc_query, zc_out = out_bytes <= c->tune.host_zc_results;
    const bool mirror_q = zc_q && c->n * (uint64_t)c->pitch > (256ull << 20);
    // The payload rows are gathered on the device BEHIND the search, on its stream, from the result indices where the
    // selection kernel left them: one submission and one wait for "the k best and their vectors" (the reference's
    // ScoredVector carries the vector, examples/similarity_search.rs:18).  A corpus that reports vector ids translates
    // them back on the host (mvfgpu_corpus_gather_rows' table), after the search: two steps, as before.
    // Only the first kv = min(k, rows) results of a query can name a row (the rest is padding): the payload staging holds
    // [nq][kv] rows -- k = 10^6 on a 10k-row corpus is 10k rows per query, not a million zero rows on the device and the host --
    // and only those rows of out_vectors ([nq][k] rows) are written.
    const uint32_t row_bytes = c->dim * elem_size(c->dtype);
    const uint32_t kv = (uint32_t)std::min<uint64_t>(k, c->n);
    const size_t nvec = (size_t)nq * kv;
    const size_t vec_bytes = nvec * row_bytes;
    const bool zc_vec = vec_bytes <= c->tune.host_zc_results;
    void *dq, *ds, *di, *dr, *dv = nullptr;
    std::lock_guard<std::mutex> host_lk(c->host_mu);
    bool fused_fetch = false;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        // wait for any in-flight user of the mirrors before (re)allocating them (nothing is in flight when the newest work
        // was seen complete through the flag: its event would only be signalled a few microseconds from now)
        if (c->has_done && c->confirmed_gen != c->work_gen) MVF_HIP_TRY(hipEventSynchronize(c->ev_done[c->done_idx]));
        fused_fetch = out_vectors && c->h_ids.empty();
        if (zc_q) {
            MVF_HIP_TRY(c->pin_q.reserve(qbytes));
            memcpy(c->pin_q.p, queries, qbytes);
            dq = c->pin_q.p;
            if (mirror_q) {
                MVF_HIP_TRY(c->h_q.reserve(qbytes));
                dq = c->h_q.p;
                MVF_HIP_TRY(hipMemcpyAsync(dq, c->pin_q.p, qbytes, hipMemcpyHostToDevice, c->own_stream));
            }
        } else {
            MVF_HIP_TRY(c->h_q.reserve(qbytes));
            dq = c->h_q.p;
            MVF_HIP_TRY(hipMemcpyAsync(dq, queries, qbytes, hipMemcpyHostToDevice, c->own_stream));
        }
        if (zc_out) {
            MVF_HIP_TRY(c->pin_out.reserve(nres * 16));
            di = c->pin_out.p;  // u64[nres] | f32[nres] | i32[nres]
            ds = static_cast<unsigned char*>(c->pin_out.p) + nres * 8;
            dr = static_cast<unsigned char*>(c->pin_out.p) + nres * 12;
        } else {
            MVF_HIP_TRY(c->h_s.reserve(nres * 4));
            MVF_HIP_TRY(c->h_i.reserve(nres * 8));
            MVF_HIP_TRY(c->h_r.reserve(nres * 4));
            ds = c->h_s.p;
            di = c->h_i.p;
            dr = c->h_r.p;
        }
        if (fused_fetch) {
            if (zc_vec) {
                MVF_HIP_TRY(c->pin_vec.reserve(vec_bytes));
                dv = c->pin_vec.p;
            } else {
                MVF_HIP_TRY(c->h_v.reserve(vec_bytes));
                dv = c->h_v.p;
            }
        }
    }
    HostFlagReq req{};
    bool want_flag = false;
    if (zc_out && c->tune.host_flag_wait && (!out_vectors || (fused_fetch && zc_vec && kv == k))) {
        std::lock_guard<std::mutex> lk(c->mu);
        if (!c->pin_flag.p) {
            MVF_HIP_TRY(c->pin_flag.reserve(64));
            *static_cast<volatile uint32_t*>(c->pin_flag.p) = 0;
            MVF_HIP_TRY(c->done_ticket.reserve(256));
            MVF_HIP_TRY(hipMemsetAsync(c->done_ticket.p, 0, 256, c->own_stream));
        }
        req.flag = static_cast<uint32_t*>(c->pin_flag.p);
        req.ticket = static_cast<uint32_t*>(c->done_ticket.p);
        req.seq = ++c->flag_seq;
        if (req.seq == 0) req.seq = ++c->flag_seq;
        req.gather_out = out_vectors && kv == k ? static_cast<unsigned char*>(dv) : nullptr;  // the select copies the payload rows as well
        want_flag = true;
    }
    rc = search_device(c, metric, dq, query_dtype, query_dim, nq, k, static_cast<float*>(ds), static_cast<uint64_t*>(di),
                       static_cast<int32_t*>(dr), c->own_stream, want_flag ? &req : nullptr, flt);
    if (rc != MVF_OK) return rc;
    if (req.armed && (!out_vectors || req.gathered)) {
        // the final select writes req.seq behind its results (and the payload rows it copied): spin on it (bounded: a long search falls back to the stream)
        const auto t0 = std::chrono::steady_clock::now();
        bool seen = false;
        for (uint32_t spins = 0;; spins++) {
            if (__atomic_load_n(req.flag, __ATOMIC_ACQUIRE) == req.seq) {
                seen = true;
                break;
            }
            if ((spins & 255u) == 255u && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(300)) break;
            __builtin_ia32_pause();
        }
        if (!seen) MVF_HIP_TRY(hipStreamSynchronize(c->own_stream));
        {
            std::lock_guard<std::mutex> lk(c->mu);
            c->confirmed_gen = req.gen;  // == work_gen unless another thread has enqueued a search meanwhile
        }
        memcpy(out_scores, ds, nres * 4);
        memcpy(out_indices, di, nres * 8);
        if (out_raw) memcpy(out_raw, dr, nres * 4);
        if (out_vectors) memcpy(out_vectors, dv, vec_bytes);
        return MVF_OK;
    }
    if (fused_fetch)  // padding entries (index UINT64_MAX) among a query's first kv results give zero rows
        MVF_HIP_TRY(launch_gather_rows(c->d_rows, c->n, c->pitch, row_bytes, c->index_base, static_cast<const uint64_t*>(di), (uint32_t)nvec,
                                   static_cast<unsigned char*>(dv), c->own_stream, k, kv));
    if (!zc_out) {
        MVF_HIP_TRY(hipMemcpyAsync(out_scores, ds, nres * 4, hipMemcpyDeviceToHost, c->own_stream));
        MVF_HIP_TRY(hipMemcpyAsync(out_indices, di, nres * 8, hipMemcpyDeviceToHost, c->own_stream));
        if (out_raw) MVF_HIP_TRY(hipMemcpyAsync(out_raw, dr, nres * 4, hipMemcpyDeviceToHost, c->own_stream));
    }
    if (fused_fetch && !zc_vec) {
        if (kv == k) MVF_HIP_TRY(hipMemcpyAsync(out_vectors, dv, vec_bytes, hipMemcpyDeviceToHost, c->own_stream));
        else MVF_HIP_TRY(hipMemcpy2DAsync(out_vectors, (size_t)k * row_bytes, dv, (size_t)kv * row_bytes, (size_t)kv * row_bytes, nq,
                                      hipMemcpyDeviceToHost, c->own_stream));
    }
    MVF_HIP_TRY(hipStreamSynchronize(c->own_stream));
    if (zc_out) {
        memcpy(out_scores, ds, nres * 4);
        memcpy(out_indices, di, nres * 8);
        if (out_raw) memcpy(out_raw, dr, nres * 4);
    }
    if (fused_fetch && zc_vec)
        for (uint32_t q = 0; q < nq; q++)
            memcpy(static_cast<unsigned char*>(out_vectors) + (size_t)q * k * row_bytes, static_cast<unsigned char*>(dv) + (size_t)q * kv * row_bytes,
                   (size_t)kv * row_bytes);
    if (out_vectors && !fused_fetch) {  // vector ids: mapped back on the host, query by query (the first kv results each)
        if (kv == k) return gather_rows_host_locked(c, out_indices, nres, out_vectors);
        for (uint32_t q = 0; q < nq; q++) {
            rc = gather_rows_host_locked(c, out_indices + (size_t)q * k, kv, static_cast<unsigned char*>(out_vectors) + (size_t)q * k * row_bytes);
            if (rc != MVF_OK) return rc;
        }
    }
    return MVF_OK;
}
}  // namespace

int mvfgpu_search(const mvfgpu_corpus* c, uint8_t metric, const void* queries, uint8_t query_dtype,
                  uint32_t query_dim, uint32_t nq, uint32_t k, float* out_scores, uint64_t* out_indices,
                  int32_t* out_raw) {
    return search_host(c, metric, queries, query_dtype, query_dim, nq, k, out_scores, out_indices, out_raw, nullptr);
}

int mvfgpu_search_fetch(const mvfgpu_corpus* c, uint8_t metric, const void* queries, uint8_t query_dtype,
                        uint32_t query_dim, uint32_t nq, uint32_t k, float* out_scores, uint64_t* out_indices,
                        int32_t* out_raw, void* out_vectors) {
    if (!out_vectors) return fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    return search_host(c, metric, queries, query_dtype, query_dim, nq, k, out_scores, out_indices, out_raw, out_vectors);
}

int mvfgpu_merge_topk_host(const float* scores, const uint64_t* indices, const int32_t* raw, uint32_t nlists,
                           uint32_t nq, uint32_t k, uint8_t metric, uint8_t data_type, float* out_scores,
                           uint64_t* out_indices, int32_t* out_raw) {
    if (!scores || !indices || !out_scores || !out_indices) return fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (const int mrc = check_metric(metric)) return mrc;
    if (nlists == 0 || nq == 0 || k == 0) return fail(MVF_ERR_INVALID_ARGUMENT, "nlists, nq and k must be > 0");
    const bool use_raw = key_is_raw(data_type, metric) && raw != nullptr;
    struct Ent {
        uint32_t key;
        uint64_t idx;
        size_t slot;
    };
    std::vector<Ent> ents;
    ents.reserve((size_t)nlists * k);
    for (uint32_t q = 0; q < nq; q++) {
        ents.clear();
        for (uint32_t l = 0; l < nlists; l++)
            for (uint32_t j = 0; j < k; j++) {
                const size_t s = ((size_t)l * nq + q) * k + j;
                if (indices[s] == ~0ull) continue;  // padding
                ents.push_back({use_raw ? key_from_raw(raw[s], metric) : key_from_score(scores[s], metric), indices[s], s});
            }
        const size_t keep = std::min<size_t>(k, ents.size());
        // ties: list order, then rank in the list (= ascending global row position for row-range shards in order)
        std::partial_sort(ents.begin(), ents.begin() + keep, ents.end(), [](const Ent& a, const Ent& b) {
            return a.key < b.key || (a.key == b.key && a.slot < b.slot);
        });
        for (uint32_t j = 0; j < k; j++) {
            const size_t o = (size_t)q * k + j;
            if (j < keep) {
                out_scores[o] = scores[ents[j].slot];
                out_indices[o] = ents[j].idx;
                if (out_raw) out_raw[o] = raw ? raw[ents[j].slot] : 0;
            } else {
                out_scores[o] = pad_score(metric);
                out_indices[o] = ~0ull;
                if (out_raw) out_raw[o] = 0;
            }
        }
    }
    return MVF_OK;
}

namespace {
int merge_topk_device_impl(const float* d_scores, const uint64_t* d_indices, const int32_t* d_raw, size_t ls_scores,
                           size_t ls_indices, size_t ls_raw, uint32_t nlists, uint32_t nq, uint32_t k, uint8_t metric,
                           uint8_t data_type, float* d_out_scores, uint64_t* d_out_indices, int32_t* d_out_raw, int device,
                           void* hip_stream) {
    if (!d_scores || !d_indices || !d_out_scores || !d_out_indices) return fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (const int mrc = check_metric(metric)) return mrc;
    if (nlists == 0 || nq == 0 || k == 0) return fail(MVF_ERR_INVALID_ARGUMENT, "nlists, nq and k must be > 0");
    const uint64_t total = (uint64_t)nlists * k;
    if (total > 0xFFFFFFFFull) return fail(MVF_ERR_INVALID_ARGUMENT, "nlists * k exceeds 2^32 - 1");
    const bool large = total > kMergeMaxEntries;  // beyond one block's LDS: a device-wide sort per query
    const uint32_t P = large ? 0u : next_pow2(std::max(2u, nlists * k));
    DevScope guard(device);
    if (!guard.ok) return fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    ShardMergeParams p{};
    p.scores = d_scores;
    p.indices = d_indices;
    p.raw = d_raw;
    p.ls_scores = ls_scores;
    p.ls_indices = ls_indices;
    p.ls_raw = ls_raw;
    p.nlists = nlists;
    p.nq = nq;
    p.k = k;
    p.P = P;
    p.metric = metric;
    p.dtype = data_type;
    p.out_scores = d_out_scores;
    p.out_indices = d_out_indices;
    p.out_raw = d_out_raw;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (!large) {
        MVF_HIP_TRY(launch_merge_shards(p, s));
        return MVF_OK;
    }
    // the sort's buffers live for this call only, in stream order (this entry point has no handle to keep them in)
    size_t tmp_bytes = 0;
    MVF_HIP_TRY(sort_composites(nullptr, &tmp_bytes, nullptr, nullptr, (size_t)total, (size_t)p.k, nullptr, s));
    tmp_bytes = std::max<size_t>(tmp_bytes, 256);
    const size_t cb = ((size_t)total * 8 + 255) & ~(size_t)255;
    void* scratch = nullptr;
    MVF_HIP_TRY(hipMallocAsync(&scratch, 2 * cb + tmp_bytes, s));
    MVF_HIP_TRY(poison_fill(scratch, 2 * cb + tmp_bytes, s));
    uint64_t *a = static_cast<uint64_t*>(scratch), *b = reinterpret_cast<uint64_t*>(static_cast<unsigned char*>(scratch) + cb);
    void* tmp = static_cast<unsigned char*>(scratch) + 2 * cb;
    hipError_t e = hipSuccess;
    for (uint32_t q = 0; q < nq && e == hipSuccess; q++) {
        uint64_t* sorted = a;
        size_t tb = tmp_bytes;
        e = launch_merge_build(p, q, a, s);
        if (e == hipSuccess) e = sort_composites(tmp, &tb, a, b, (size_t)total, (size_t)p.k, &sorted, s);
        if (e == hipSuccess) e = launch_merge_write(p, q, sorted, s);
    }
    const hipError_t ef = hipFreeAsync(scratch, s);
    MVF_HIP_TRY(e);
    MVF_HIP_TRY(ef);
    return MVF_OK;
}
}  // namespace

int mvfgpu_merge_topk_device(const float* d_scores, const uint64_t* d_indices, const int32_t* d_raw, uint32_t nlists,
                             uint32_t nq, uint32_t k, uint8_t metric, uint8_t data_type, float* d_out_scores,
                             uint64_t* d_out_indices, int32_t* d_out_raw, int device, void* hip_stream) {
    const size_t ls = (size_t)nq * k;
    return merge_topk_device_impl(d_scores, d_indices, d_raw, ls, ls, ls, nlists, nq, k, metric, data_type, d_out_scores,
                                  d_out_indices, d_out_raw, device, hip_stream);
}

int mvfgpu_merge_topk_packed_device(const void* d_packed, uint32_t nlists, uint32_t nq, uint32_t k, uint8_t metric,
                                    uint8_t data_type, float* d_out_scores, uint64_t* d_out_indices, int32_t* d_out_raw,
                                    int device, void* hip_stream) {
    if (!d_packed) return fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if ((reinterpret_cast<uintptr_t>(d_packed) & 7u) != 0) return fail(MVF_ERR_INVALID_ARGUMENT, "packed lists must be 8-byte aligned");
    // one list = { u64 indices[nq k]; f32 scores[nq k]; i32 raw[nq k] } = 16 nq k bytes (MVFGPU_PACKED_LIST_BYTES)
    const size_t n = (size_t)nq * k;
    const unsigned char* b = static_cast<const unsigned char*>(d_packed);
    return merge_topk_device_impl(reinterpret_cast<const float*>(b + 8 * n), reinterpret_cast<const uint64_t*>(b),
                                  reinterpret_cast<const int32_t*>(b + 12 * n), 4 * n, 2 * n, 4 * n, nlists, nq, k, metric,
                                  data_type, d_out_scores, d_out_indices, d_out_raw, device, hip_stream);
}

int mvfgpu_synth_queries_device(void* d_queries, uint32_t nq, uint32_t dimension, uint8_t data_type, uint64_t seed,
                                int device, void* hip_stream) {
    if (!d_queries) return fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (elem_size(data_type) == 0) return fail(MVF_ERR_BUILD, "Unsupported vector data type");
    DevScope guard(device);
    if (!guard.ok) return fail(MVF_ERR_DEVICE, "hipSetDevice failed");
    const uint8_t qd = is_int_dtype(data_type) ? data_type : (uint8_t)MVF_DTYPE_FLOAT32;
    MVF_HIP_TRY(launch_synth_packed(d_queries, (uint64_t)nq * dimension, qd, seed, static_cast<hipStream_t>(hip_stream)));
    return MVF_OK;
}

int mvfgpu_set_profiling(mvfgpu_corpus* c, int enabled) {
    if (!c) return fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    std::lock_guard<std::mutex> lk(c->mu);
    c->profiling = enabled != 0;
    c->prof_next = 0;
    c->timing = mvfgpu_timing{};
    return MVF_OK;
}

int mvfgpu_last_timing(const mvfgpu_corpus* c, mvfgpu_timing* out) {
    if (!c || !out) return fail(MVF_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    mvfgpu_timing tm = c->timing;
    if (c->last_redo_cnt) {  // the newest batched search's repair count (waits for the handle's last search)
        DevScope guard(c->device);
        if (c->has_done) MVF_HIP_TRY(hipEventSynchronize(c->ev_done[c->done_idx]));
        uint32_t n = 0;
        MVF_HIP_TRY(hipMemcpy(&n, c->last_redo_cnt, 4, hipMemcpyDeviceToHost));
        tm.repaired_queries = n;
    }
    tm.search_launches = c->search_launches;
    if (c->prof_next > 0) {
        DevScope guard(c->device);
        const uint64_t newest = c->prof_next - 1;
        const uint64_t oldest = c->prof_next > mvfgpu_corpus::kProfSlots ? c->prof_next - mvfgpu_corpus::kProfSlots : 0;
        double ssum = 0, lsum = 0, wsum = 0;
        uint32_t cnt = 0, wcnt = 0;
        std::vector<uint64_t> clk;  // the clock entries of the searches that timed themselves, behind the handle's newest call
        for (uint64_t i = oldest; i <= newest && clk.empty(); i++)
            if (c->prof[i % mvfgpu_corpus::kProfSlots].ts_scan && c->prof_ts.p) {
                if (c->has_done) MVF_HIP_TRY(hipEventSynchronize(c->ev_done[c->done_idx]));
                clk.resize((size_t)mvfgpu_corpus::kProfSlots * 4);
                MVF_HIP_TRY(hipMemcpy(clk.data(), c->prof_ts.p, clk.size() * 8, hipMemcpyDeviceToHost));
            }
        for (uint64_t i = newest + 1; i-- > oldest;) {
            const auto& ps = c->prof[i % mvfgpu_corpus::kProfSlots];
            float a = 0, b = 0, w = 0;
            if (ps.ts_scan && !clk.empty()) {
                const uint64_t* t = clk.data() + (i % mvfgpu_corpus::kProfSlots) * 4;
                if (t[1] >= t[0]) a = (float)((double)(t[1] - t[0]) / c->wall_khz);
                if (t[2] >= t[1]) b = (float)((double)(t[2] - t[1]) / c->wall_khz);
                if (ps.ts_whole && t[3] >= t[0]) {
                    w = (float)((double)(t[3] - t[0]) / c->wall_khz);
                    wsum += w;
                    wcnt++;
                }
            } else {
                MVF_HIP_TRY(hipEventSynchronize(ps.whole ? ps.e[4] : ps.e[2]));
            }
            if (ps.scanned && !ps.ts_scan) {
                MVF_HIP_TRY(hipEventElapsedTime(&a, ps.e[0], ps.e[1]));
                MVF_HIP_TRY(hipEventElapsedTime(&b, ps.e[1], ps.e[2]));
            }
            if (ps.whole) {
                if (ps.ts_scan) MVF_HIP_TRY(hipEventSynchronize(ps.e[4]));
                MVF_HIP_TRY(hipEventElapsedTime(&w, ps.e[3], ps.e[4]));
                wsum += w;
                wcnt++;
            }
            if (i == newest) {
                tm.scan_ms = a;
                tm.select_ms = b;
                tm.total_ms = a + b;
                tm.search_ms = w;
            }
            ssum += a;
            lsum += b;
            cnt++;
        }
        tm.samples = cnt;
        tm.scan_ms_avg = cnt ? (float)(ssum / cnt) : 0.f;
        tm.select_ms_avg = cnt ? (float)(lsum / cnt) : 0.f;
        tm.search_ms_avg = wcnt ? (float)(wsum / wcnt) : 0.f;
    }
    return copy_out_struct(out, tm);
}

int mvfgpu_debug_stream_lo_lines(const mvfgpu_corpus* c, uint64_t* out_fetched, uint64_t* out_total) {
    if (!c || !out_fetched || !out_total) return fail(MVF_ERR_INVALID_ARGUMENT, "NULL argument");
    std::lock_guard<std::mutex> lk(c->mu);
    *out_fetched = *out_total = 0;
    if (!c->pub51.p || c->pub51_blocks == 0) return MVF_OK;  // the newest 6-bit-route search did not read the 5+1 layout
    DevScope guard(c->device);
    if (c->has_done) MVF_HIP_TRY(hipEventSynchronize(c->ev_done[c->done_idx]));
    std::vector<uint32_t> st((size_t)c->pub51_blocks * 4);
    MVF_HIP_TRY(hipMemcpy(st.data(), static_cast<const unsigned char*>(c->pub51.p) + (size_t)kPub51Blocks * 8, st.size() * 4, hipMemcpyDeviceToHost));
    for (uint32_t b = 0; b < c->pub51_blocks; b++)
        if (st[(size_t)b * 4] == c->pub51_seq) *out_fetched += st[(size_t)b * 4 + 1], *out_total += st[(size_t)b * 4 + 2];
    return MVF_OK;
}

int mvfgpu_set_scan_path(mvfgpu_corpus* c, int path) {
    if (!c) return fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    if (path < 0 || path > 7) return fail(MVF_ERR_INVALID_ARGUMENT, "path must be 0..7");
    std::lock_guard<std::mutex> lk(c->mu);
    c->scan_path = path;
    return MVF_OK;
}

int mvfgpu_set_maxsim_route(mvfgpu_corpus* c, int route) {
    if (!c) return fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    if (route < 0 || route > 2) return fail(MVF_ERR_INVALID_ARGUMENT, "route must be 0, 1 or 2");
    std::lock_guard<std::mutex> lk(c->mu);
    c->maxsim_route = route;
    return MVF_OK;
}

int mvfgpu_corpus_reload_tuning(mvfgpu_corpus* c) {
    if (!c) return fail(MVF_ERR_INVALID_ARGUMENT, "corpus is NULL");
    // host_mu first (search_host's order): the host-buffer searches read c->tune under it, without c->mu.  Device-pointer
    // searches (mvfgpu_search_device) read the switches unlocked: do not call this beside them (include/mvf_gpu.h).
    std::lock_guard<std::mutex> host_lk(c->host_mu);
    std::lock_guard<std::mutex> lk(c->mu);
    c->tune = mvf::read_tuning();
    choose_group(c->V, 1, &c->G, &c->J, c->tune.k1_g);
    return MVF_OK;
}

int mvfgpu_selftest_poison(void) { return mvf::debug_poison_byte(); }

uint32_t mvfgpu_abi_version(void) { return MVFGPU_ABI_VERSION; }

int mvfgpu_selftest_feedback(const uint32_t* samples, uint32_t n_samples, uint32_t* out_state) {
    if ((!samples && n_samples) || !out_state) return fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    uint32_t seen = 0, redone = 0;
    bool bias_off = false, qs_off = false;
    for (uint32_t i = 0; i < n_samples; i++)
        feedback_consume(seen, redone, bias_off, qs_off, samples[4 * i], samples[4 * i + 1], samples[4 * i + 2] != 0, samples[4 * i + 3] != 0);
    out_state[0] = seen;
    out_state[1] = redone;
    out_state[2] = bias_off;
    out_state[3] = qs_off;
    return MVF_OK;
}

int mvfgpu_selftest_schedule(uint64_t rows, uint32_t nq, uint32_t k, int int8_selection, uint64_t* out_bounds, uint32_t max_bounds,
                             uint32_t* out_n_bounds, uint32_t* out_growth, uint32_t* out_refined_mask) {
    if (!out_bounds || !out_n_bounds || !out_growth || !out_refined_mask) return fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (rows == 0 || nq == 0 || k == 0 || k > MVFGPU_K_PER_PASS) return fail(MVF_ERR_INVALID_ARGUMENT, "empty corpus / batch, or k beyond one pass");
    const Tuning t{};  // the DEFAULT tuning, not the environment
    const uint32_t cap = int8_selection ? kBatchCapQS : kBatchCap;
    const uint32_t g = k2_growth_for(t, nq, k, cap);
    const std::vector<uint64_t> bounds = k2_phase_bounds(rows, cap, g);
    if (bounds.size() > max_bounds) return fail(MVF_ERR_INVALID_ARGUMENT, "more phases than the buffer holds");
    uint32_t mask = 0;
    for (size_t i = 0; i < bounds.size(); i++) {
        out_bounds[i] = bounds[i];
        if (int8_selection && i < 32 && k2_refine_before(t, bounds, i, nq)) mask |= 1u << i;
    }
    *out_n_bounds = (uint32_t)bounds.size();
    *out_growth = g;
    *out_refined_mask = mask;
    return MVF_OK;
}

int mvfgpu_selftest_route(uint64_t rows, uint32_t dimension, uint8_t data_type, uint8_t metric, uint32_t nq, uint32_t k, uint32_t* out_route) {
    if (!out_route) return fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (elem_size(data_type) == 0 || dimension == 0 || nq == 0 || k == 0 || k > MVFGPU_MAX_K)
        return fail(MVF_ERR_INVALID_ARGUMENT, "unsupported type or empty dimension / batch / k");
    if (const int mrc = check_metric(metric)) return mrc;
    // a handle that owns nothing on a device: the route is a function of these fields and the DEFAULT tuning (not the environment)
    std::unique_ptr<mvfgpu_corpus> c(new mvfgpu_corpus());
    c->n = rows;
    c->dim = dimension;
    c->dtype = data_type;
    c->pitch = (dimension * elem_size(data_type) + 15u) & ~15u;
    c->V = c->pitch / 16;
    c->tune = Tuning{};
    if (k > MVFGPU_K_PER_PASS) *out_route = large_k_by_sort(c.get(), nq, k) ? 3u : 2u;
    else *out_route = use_batched_path(c.get(), metric, nq) ? 1u : 0u;
    return MVF_OK;
}

int mvfgpu_selftest_filter_route(uint64_t rows, uint32_t dimension, uint8_t data_type, uint32_t nq, uint32_t k, uint64_t admitted,
                                 uint32_t* out_route) {
    if (!out_route) return fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (elem_size(data_type) == 0 || dimension == 0 || nq == 0 || k == 0 || k > MVFGPU_MAX_K)
        return fail(MVF_ERR_INVALID_ARGUMENT, "unsupported type or empty dimension / batch / k");
    if (admitted > rows) return fail(MVF_ERR_INVALID_ARGUMENT, "more rows admitted than the corpus holds");
    *out_route = filter_route_rule(rows, dimension, data_type, nq, k, admitted);
    return MVF_OK;
}

int mvfgpu_selftest_stream_rows(uint64_t rows, uint32_t dimension, uint8_t data_type, uint8_t metric, uint32_t nq, uint32_t k,
                                uint32_t* out_rows) {
    if (!out_rows) return fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (elem_size(data_type) == 0 || dimension == 0 || nq == 0 || k == 0 || k > MVFGPU_MAX_K)
        return fail(MVF_ERR_INVALID_ARGUMENT, "unsupported type or empty dimension / batch / k");
    if (const int mrc = check_metric(metric)) return mrc;
    *out_rows = stream_i8_shape(rows, dimension, data_type, nq, k) ? 1u : 0u;
    return MVF_OK;
}

int mvfgpu_selftest_stream_bits(uint64_t rows, uint32_t dimension, uint8_t data_type, uint8_t metric, uint32_t nq, uint32_t k,
                                uint32_t* out_bits) {
    if (!out_bits) return fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (elem_size(data_type) == 0 || dimension == 0 || nq == 0 || k == 0 || k > MVFGPU_MAX_K)
        return fail(MVF_ERR_INVALID_ARGUMENT, "unsupported type or empty dimension / batch / k");
    if (const int mrc = check_metric(metric)) return mrc;
    *out_bits = !stream_i8_shape(rows, dimension, data_type, nq, k) ? 0u : stream_6b_shape(rows, dimension, metric, k) ? 6u : 8u;
    return MVF_OK;
}

}  // extern "C"

namespace mvf {
// Mask or list (DESIGN.md section 5 "F0 / F1 / F2"; every figure below: scripts/probe_filtered.py, profiles/r09_filtered.txt,
// 10M x 768 f32 cosine and 50M x 768 int8 dot at k = 100).  Both routes are bound by the bytes of rows they read, so the rule
// compares those: the list route reads the admitted rows' pitch once per group of queries F2 serves together; the mask route
// reads what the plain search of this shape reads under the default tuning -- K1 the stored rows once per four queries (ONE
// Float32 query from kStreamI8MinBytes on: the int8 shadow), the batched route one pass over the int8 shadow / the Int8 rows
// per kFilterMaskTile queries (1024 queries cost 6.9 / 5.9 times one query's pass on the two shapes), a large k at least
// K1's passes.  The metric is left out: it moves the plain route only for Float32 rows beyond kWideFinalMaxDim dimensions
// (taken as InnerProduct here).
//   * kFilterListCost: a byte gathered through the list costs this many streamed ones.  F2 holds 2.4-4.9 TB/s on lists of a
//     million rows and more against the 6.6-7.0 TB/s of the one-query streamed passes, and the measured crossovers put the
//     factor at 1.4 (int8, one query) .. 2.7 (f32, 16 queries): 2 decides every measured point but one the way the times do.
//   * kFilterRepairDensity: a BATCHED search under a mask that admits few rows -- as under tombstones of that weight --
//     flags nearly every query for the exact repair pass, K1 over the stored rows four queries at a time: 1024 queries
//     take 0.6-3.1 s instead of 8-36 ms at every density measured from 1e-4 to 0.05, 256 queries 0.15-1.4 s from 0.015 to
//     0.05 (and still 146 ms at 0.07 on the f32 shape); at 0.07 and above, and for 64 queries at every density, it does not
//     happen.  The list route takes 9-160 ms there.  So more than 64 queries take the list up to a density of 1/16.
//     Measured at k = 100 on these two shapes only.
constexpr uint64_t kFilterListCost = 2, kFilterMaskTile = 128, kFilterRepairDensity = 16;
uint32_t filter_route_rule(uint64_t rows, uint32_t dim, uint8_t dtype, uint32_t nq, uint32_t k, uint64_t admitted) {
    if (rows == 0 || admitted >= rows) return 1u;
    std::unique_ptr<mvfgpu_corpus> c(new mvfgpu_corpus());  // owns nothing on a device (mvfgpu_selftest_route's stub)
    c->n = rows;
    c->dim = dim;
    c->dtype = dtype;
    c->pitch = (dim * elem_size(dtype) + 15u) & ~15u;
    c->V = c->pitch / 16;
    c->tune = Tuning{};
    int G = 64;
    uint32_t J = 1;
    choose_group(c->V, 1, &G, &J);
    const uint32_t qg = filter_group_queries(cand_query_bytes(dtype, G, J));
    const uint64_t pitch8 = ((uint64_t)dim + 15u) & ~15ull;  // a row of the int8 shadow, about
    typedef unsigned __int128 u128;
    const u128 list_bytes = (u128)admitted * c->pitch * ((nq + qg - 1) / qg);
    u128 mask_bytes;
    if (k > MVFGPU_K_PER_PASS) {
        mask_bytes = (u128)rows * c->pitch * ((nq + 3) / 4);
    } else if (use_batched_path(c.get(), MVF_METRIC_INNER_PRODUCT, nq)) {
        if (nq > 64 && (u128)admitted * kFilterRepairDensity <= rows) return 2u;
        mask_bytes = (u128)rows * pitch8 * ((nq + kFilterMaskTile - 1) / kFilterMaskTile);
    } else if (stream_i8_shape(rows, dim, dtype, nq, k)) {
        mask_bytes = (u128)rows * pitch8;
    } else {
        mask_bytes = (u128)rows * c->pitch * ((nq + 3) / 4);
    }
    return list_bytes * kFilterListCost <= mask_bytes ? 2u : 1u;
}

int search_positions_locked(const mvfgpu_corpus* c, uint8_t metric, const void* d_queries, uint32_t nq, uint32_t k, float* d_scores,
                            uint64_t* d_indices, int32_t* d_raw, void* stream) {
    SearchCall sc = new_search_call(c, metric, d_queries, nq, k, d_scores, d_indices, d_raw, static_cast<hipStream_t>(stream));
    sc.positions_only = true;
    sc.shared_call = true;  // corpus_device_call's body may run any number of searches
    return search_locked(c, sc);
}
int search_filtered_host(const mvfgpu_corpus* c, const FilterUse& flt, uint8_t metric, const void* queries, uint8_t query_dtype,
                         uint32_t query_dim, uint32_t nq, uint32_t k, float* out_scores, uint64_t* out_indices, int32_t* out_raw) {
    return search_host(c, metric, queries, query_dtype, query_dim, nq, k, out_scores, out_indices, out_raw, nullptr, &flt);
}
int search_filtered_device(const mvfgpu_corpus* c, const FilterUse& flt, uint8_t metric, const void* d_queries, uint8_t query_dtype,
                           uint32_t query_dim, uint32_t nq, uint32_t k, float* d_scores, uint64_t* d_indices, int32_t* d_raw,
                           void* hip_stream) {
    return search_device(c, metric, d_queries, query_dtype, query_dim, nq, k, d_scores, d_indices, d_raw, hip_stream, nullptr, &flt);
}
}  // namespace mvf
