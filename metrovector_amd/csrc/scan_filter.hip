// scan_filter.hip — F0 (allow bits -> deny mask + block counts) and F1 (the ascending list of admitted rows) of the filtered
// search (filter.hip, DESIGN.md §5 "F0 / F1 / F2 — filtered search").  F2, K1's scores of the listed rows for groups of queries, is the
// gathered-row kernel (scan_gather.hip).
//
// F0 re-bases the caller's bits to local rows -- a word of the mask is a funnel of two adjacent words of the upload, shifted by
// 0 .. 31 -- and combines them with the handle's tombstones: deny = ~allow | tomb, zero at and beyond the last row, which is
// the layout every scan kernel already takes as its deletion bitmap.  A block covers kFilterBlockRows rows and leaves their
// admitted count.  F1 scans those counts and scatters every block's admitted rows in ascending order with the block compaction
// (mvf_common.h: block_compact_1024; a ballot per wave, the waves' counts through LDS) -- no sort.

#include "scan_filter.h"
#include "aux_kernels.h"
#include "mvf_common.h"
#include "scan_candidates.h"

#include <algorithm>

namespace mvf {
namespace {

// F0: grid (filter_blocks(n)), block 1024; thread t of block b owns word b * 1024 + t of the mask
__global__ void __launch_bounds__(1024) filter_mask_kernel(FilterMaskParams p) {
    __shared__ uint32_t wsum[16];
    const uint64_t nw = (p.n + 31) / 32;
    const uint64_t w = (uint64_t)blockIdx.x * 1024u + threadIdx.x;
    uint32_t admitted = 0;
    if (w < nw) {
        const uint32_t lo = p.allow[w];
        // (a shift of 0 takes the word as it lies: `hi << 32` is undefined, and the device form's last word has no neighbour)
        const uint32_t allow = p.shift ? (lo >> p.shift) | (p.allow[w + 1] << (32u - p.shift)) : lo;
        const uint64_t left = p.n - w * 32u;
        const uint32_t valid = left >= 32u ? 0xFFFFFFFFu : (1u << (uint32_t)left) - 1u;
        const uint32_t deny = (~allow | (p.tomb ? p.tomb[w] : 0u)) & valid;
        p.deny[w] = deny;
        admitted = (uint32_t)__builtin_popcount(~deny & valid);
    } else if (w == nw) {
        p.deny[w] = 0u;
    }
    const uint32_t tot = block_sum_1024(admitted, wsum);
    if (threadIdx.x == 0) p.block_cnt[blockIdx.x] = tot;
}

// F1, step 1: one block of 1024 threads; block_off[b] = the counts in front of block b, *total = all of them
__global__ void __launch_bounds__(1024) filter_scan_kernel(const uint32_t* block_cnt, uint32_t nb, uint64_t* block_off, uint64_t* total) {
    __shared__ uint64_t wtot[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t per = (nb + 1023u) / 1024u;
    const uint32_t b0 = tid * per, b1 = min(nb, b0 + per);
    uint64_t mine = 0;
    for (uint32_t b = b0; b < b1; b++) mine += block_cnt[b];
    uint64_t incl = mine;  // inclusive scan inside the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t o = __shfl_up(incl, off, 64);
        if ((int)lane >= off) incl += o;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint64_t base = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < 16; w++) {
        base += w < wave ? wtot[w] : 0ull;
        all += wtot[w];
    }
    uint64_t run = base + incl - mine;
    for (uint32_t b = b0; b < b1; b++) {
        block_off[b] = run;
        run += block_cnt[b];
    }
    if (tid == 0) *total = all;
}

// F1, step 2: grid (filter_blocks(n)), block 1024; block b scatters the admitted rows of [b, b + 1) * kFilterBlockRows
__global__ void __launch_bounds__(1024) filter_compact_kernel(const uint32_t* deny, uint64_t n, const uint64_t* block_off, uint32_t* list) {
    __shared__ uint32_t wsum[16];
    const uint64_t r0 = (uint64_t)blockIdx.x * kFilterBlockRows;
    block_compact_1024(
        r0, min(r0 + kFilterBlockRows, n), block_off[blockIdx.x], wsum, [&](uint64_t r) { return !((deny[r >> 5] >> (r & 31u)) & 1u); },
        [&](uint64_t r, uint64_t slot) { list[slot] = (uint32_t)r; });
}

}  // namespace

hipError_t filter_mask_launch(const FilterMaskParams& p, hipStream_t s) {
    hipLaunchKernelGGL(filter_mask_kernel, dim3(filter_blocks(p.n)), dim3(1024), 0, s, p);
    return hipGetLastError();
}

hipError_t filter_scan_launch(const uint32_t* block_cnt, uint32_t nb, uint64_t* block_off, uint64_t* total, hipStream_t s) {
    hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(1024), 0, s, block_cnt, nb, block_off, total);
    return hipGetLastError();
}

hipError_t filter_compact_launch(const uint32_t* deny, uint64_t n, const uint64_t* block_off, uint32_t* list, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(filter_compact_kernel, dim3((uint32_t)((n + kFilterBlockRows - 1) / kFilterBlockRows)), dim3(1024), 0, s, deny, n,
                       block_off, list);
    return hipGetLastError();
}

uint32_t filter_group_queries(uint32_t qbytes) { return (size_t)qbytes * kFilterGroup <= kCandQueryLdsMax ? kFilterGroup : 1u; }

}  // namespace mvf
