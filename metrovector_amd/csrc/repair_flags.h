// repair_flags.h — the flags of queries whose candidate budget overflowed (overflow[q] != 0) as a dense list for the repair
// launches (api.hip: repair_flagged_queries), by ONE block: a launch of its own behind a batched search
// (aux_kernels.hip: flag_compact_kernel), block 0 of the final select behind one to four streamed queries (scan_mfma.hip:
// rescore_select_kernel), whose flags are final once the margin select has run.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mvf {

// Every thread of the block calls it.  The flags are cleared; order within the list is irrelevant.  n_s: one word of LDS.
// host_mirror: pinned host memory or NULL -- the repair feedback reads the count there two searches later, behind an event.
__device__ __forceinline__ void compact_flags(uint32_t* overflow, uint32_t nq, uint32_t* redo_list, uint32_t* redo_cnt,
                                              uint32_t* host_mirror, uint32_t* n_s) {
    if (threadIdx.x == 0) *n_s = 0;
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < nq; q += blockDim.x) {
        if (overflow[q]) {
            redo_list[atomicAdd(n_s, 1u)] = q;
            overflow[q] = 0;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        *redo_cnt = *n_s;
        if (host_mirror) *host_mirror = *n_s;
    }
}

}  // namespace mvf
