// scan_radius.h — launch interface of the radius search kernels (scan_radius.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mvf {

// R1: the streaming radius scan.  K1's row layout, lane groups and per-row arithmetic; instead of a running top-k every
// row whose order key is <= bound[q] (and that is not deleted) is COUNTED, and -- when `lists` is set -- appended to the
// query's device list as (key << 32 | row) in arrival order.  The counter keeps counting past `cap`: counts are exact,
// the list holds the first `cap` arrivals.
struct RadiusParams {
    const unsigned char* rows;  // device rows, `pitch` bytes apart, zero padded to the pitch
    const void* queries;        // device [nq_total][dim]: f32, or the space's int type
    const uint32_t* tomb;       // deletion bitmap over local rows; NULL = none
    const uint32_t* bound;      // [nq_total] the largest order key that matches (mvf_common.h keys)
    uint32_t* counts;           // [nq_total] matches per query; zeroed by the host before the launch
    uint64_t* lists;            // [nq_total][cap] composites; NULL = count only (the lists are never touched)
    uint32_t cap;
    uint32_t n, pitch, dim, V, J;
    uint32_t q0;                // first query of pass 0 (pass blockIdx.y serves q0 + NQ * blockIdx.y ..)
    uint32_t nq_total;
};

// R2: one block (1024 threads) per query orders the query's list best first (bitonic in LDS) and writes the first
// min(count, cap, kout) entries of row q of the outputs ([nq][kout]); queries with count > cap are left to the host.
struct RadiusPackParams {
    const uint64_t* lists;      // [nq][cap]
    const uint32_t* counts;     // [nq]
    uint32_t cap;               // a power of two
    uint32_t kout;              // entries per output row (<= cap)
    uint8_t metric, dtype;
    uint64_t index_base;
    const uint64_t* ids;        // vector ids per local row; NULL = index_base + row
    float* out_scores;
    uint64_t* out_indices;
    int32_t* out_raw;
};

// R3: exact re-scoring of the candidates a thresholded pass of the batched f32 MFMA kernel selected (radius.hip): one block
// per query; G lanes per candidate row with R1's order of the sums (the same G as R1 for this batch: the same keys); a row
// whose exact key is <= bound[q] is counted and appended like R1's matches.  Float32 rows only.
struct RadiusRescoreParams {
    const uint64_t* cand;       // [nq][ccap] candidate composites (approximate keys), first min(ccnt[q], ccap) valid
    const uint32_t* ccnt;
    uint32_t ccap;
    const unsigned char* rows;
    const float* queries;       // device [nq][dim]
    uint32_t dim, pitch, V, J;
    const uint32_t* bound;
    uint32_t* counts;           // [nq] zeroed by the host
    uint64_t* lists;            // [nq][cap]; NULL = count only
    uint32_t cap;
};

// nqv: queries per pass over the rows, 1 or 4; grid.y passes
hipError_t radius_scan_launch(uint8_t dtype, int metric, int G, int nqv, const RadiusParams& p, dim3 grid, size_t lds,
                              hipStream_t s);
const void* radius_scan_kernel_ptr(uint8_t dtype, int metric, int G, int nqv);
size_t radius_scan_lds_bytes(uint8_t dtype, int G, uint32_t J, int nqv);
hipError_t radius_pack_launch(const RadiusPackParams& p, uint32_t nq, hipStream_t s);
hipError_t radius_rescore_launch(int metric, int G, const RadiusRescoreParams& p, uint32_t nq, size_t lds, hipStream_t s);

}  // namespace mvf
