// scan_join.h — launch interface of the k-NN join kernels (scan_join.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mvf {

// J0: rows [first, first + nq) of a corpus -> a contiguous [nq][dim] block of queries in the type a search takes:
// Float32 rows as stored (without the pitch padding), Float16 rows widened exactly, Int8 / UInt8 rows as stored.
struct JoinStageParams {
    const unsigned char* rows;  // the query corpus' resident rows
    uint32_t pitch, V, dim;     // bytes per stored row, 16-byte vectors per row, elements per row
    uint8_t dtype;
    uint64_t first;             // local row of the window's first query
    void* queries;              // out: [nq][dim] f32, or the space's int type
};

// J1: query q's k' ordered entries of a search that reports POSITIONS -> its k entries of the join.  The entry whose
// position is the query row's own global position is left out (exclude set); where there is none among the k', or exclude
// is not set, the first k stay.  A deleted query row gets all padding.
struct JoinFinishParams {
    const float* in_scores;      // [nq][kin]
    const uint64_t* in_indices;  // [nq][kin] global positions of the searched corpus, UINT64_MAX = padding
    const int32_t* in_raw;       // [nq][kin]; read only where out_raw is set
    uint32_t kin, k;             // kin = k + 1 (exclusion possible) or k
    uint32_t exclude;
    uint8_t metric;
    uint64_t q_pos0;             // global position of the window's first query row
    uint64_t q_row0;             // its local row in the query corpus
    const uint32_t* q_tomb;      // the query corpus' deletion bitmap; NULL = none
    uint64_t c_index_base;
    const uint64_t* c_ids;       // the searched corpus' vector ids per local row; NULL = positions are reported
    float* out_scores;           // [nq][k]
    uint64_t* out_indices;
    int32_t* out_raw;            // nullable
};

hipError_t join_stage_launch(const JoinStageParams& p, uint32_t nq, hipStream_t s);
hipError_t join_finish_launch(const JoinFinishParams& p, uint32_t nq, hipStream_t s);

}  // namespace mvf
