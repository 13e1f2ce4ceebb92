// scan_candidates.hip — C0 (a query's candidate list -> its distinct live local rows, ascending) of the candidate search
// (candidates.hip, DESIGN.md §5 "C0 / C1 — candidate search").  C1, K1's scores of those rows, is the gathered-row kernel
// (scan_gather.hip).
//
// C0 maps every entry to a local row (UINT64_MAX, positions outside the shard and deleted rows become dead), sorts the list
// and keeps the first of every run of equal rows: exact counts, distinct rows for the selection, and the gathers of C1 in
// ascending row order.  Lists of up to kCandLdsSort entries are sorted in one block's LDS, longer ones by sort_composites.
//
// Algorithmic HBM bytes: 12 bytes per list entry.

#include "scan_candidates.h"
#include "aux_kernels.h"
#include "bitonic.h"
#include "mvf_common.h"

#include <algorithm>

namespace mvf {
namespace {

constexpr uint32_t kDeadRow = 0xFFFFFFFFu;  // no local row is this large (a shard holds at most 2^32 - 65536 rows)

__device__ __forceinline__ uint32_t local_row(uint64_t g, const CandPrepParams& p) {
    if (g == ~0ull || g < p.index_base || g - p.index_base >= p.n) return kDeadRow;
    const uint32_t r = (uint32_t)(g - p.index_base);
    if (p.tomb && ((p.tomb[r >> 5] >> (r & 31)) & 1u)) return kDeadRow;
    return r;
}

// The first of every run of equal rows of an ascending list (dead entries last) -> out, in order; block of 1024 threads.
// get(i): the list's row i.  wsum: 16 words of LDS.
template <class Get>
__device__ __forceinline__ void compact_rows(Get get, uint32_t m, uint32_t* out, uint32_t* cnt, uint64_t* cnt64, uint32_t* wsum) {
    const uint32_t kept = block_compact_1024(
        0u, m, 0u, wsum, [&](uint32_t i) { return get(i) != kDeadRow && (i == 0 || get(i - 1) != get(i)); },
        [&](uint32_t i, uint32_t slot) { out[slot] = get(i); });
    if (threadIdx.x == 0) {
        *cnt = kept;
        if (cnt64) *cnt64 = kept;
    }
}

// C0, lists of up to kCandLdsSort entries: grid (nq), block 1024, dynamic LDS next_pow2(m) * 8
__global__ void __launch_bounds__(1024) cand_prep_kernel(CandPrepParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* buf = reinterpret_cast<uint64_t*>(smem);
    __shared__ uint32_t wsum[16];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t P = next_pow2(p.m < 2 ? 2u : p.m);
    const uint64_t* c = p.cand + (size_t)q * p.m;
    for (uint32_t i = tid; i < P; i += 1024) buf[i] = i < p.m ? (uint64_t)local_row(c[i], p) : (uint64_t)kDeadRow;
    __syncthreads();
    bitonic_sort_u64_1024(buf, P, (int)tid);
    compact_rows([&](uint32_t i) { return (uint32_t)buf[i]; }, p.m, p.rows + (size_t)q * p.m, p.counts + q,
                 p.out_counts ? p.out_counts + q : nullptr, wsum);
}

// C0, longer lists, step 1: rank entries (list position << 32 | local row) for sort_composites, which orders them by row
__global__ void __launch_bounds__(256) cand_map_kernel(CandPrepParams p) {
    const uint32_t q = blockIdx.y;
    const uint64_t* c = p.cand + (size_t)q * p.m;
    uint64_t* e = p.ent + (size_t)q * p.m;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < p.m; i += gridDim.x * 256) e[i] = ((uint64_t)i << 32) | local_row(c[i], p);
}

// C0, longer lists, step 2: the sorted entries -> distinct rows; grid (nq), block 1024
__global__ void __launch_bounds__(1024) cand_compact_kernel(CandPrepParams p, const uint64_t* sorted) {
    __shared__ uint32_t wsum[16];
    const uint32_t q = blockIdx.x;
    const uint64_t* e = sorted + (size_t)q * p.m;
    compact_rows([&](uint32_t i) { return (uint32_t)e[i]; }, p.m, p.rows + (size_t)q * p.m, p.counts + q,
                 p.out_counts ? p.out_counts + q : nullptr, wsum);
}

}  // namespace

hipError_t cand_prep_launch(const CandPrepParams& p, uint32_t nq, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    if (p.m > kCandLdsSort) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cand_prep_kernel, dim3(nq), dim3(1024), (size_t)next_pow2(p.m < 2 ? 2u : p.m) * 8u, s, p);
    return hipGetLastError();
}

hipError_t cand_map_launch(const CandPrepParams& p, uint32_t nq, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    const uint32_t bx = std::min<uint32_t>((p.m + 255u) / 256u, 1024u);
    hipLaunchKernelGGL(cand_map_kernel, dim3(bx, nq), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t cand_compact_launch(const CandPrepParams& p, const uint64_t* sorted, uint32_t nq, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(cand_compact_kernel, dim3(nq), dim3(1024), 0, s, p, sorted);
    return hipGetLastError();
}

}  // namespace mvf
