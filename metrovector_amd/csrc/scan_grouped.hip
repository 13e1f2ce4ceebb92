// scan_grouped.hip — G1 of the grouped search: the per_key best entries of every key's segment of a scored, key-ordered list
// (DESIGN.md §5 "G0 / G1 — grouped search"), and the column gather.
//
// G0 (scan_gather.hip's kernel) leaves query q's rank entries in the partition's order: key by key, ascending position inside
// a key.  G1 works on COMPOSITES (key' << 32 | local row; key' is the rank entry's low word, so a live NaN is 0xFFFFFFFE and
// ~0 is free for padding): smaller = better, ties to the lower position.  Tiles of kGroupTile entries get one block each,
// whatever the segments are -- a tile of ten-row keys holds a hundred of them, a key of a million rows a thousand tiles:
//
//   group_tile_kernel : the tile's composites in LDS; every entry knows its segment (bounds) and with it its RUN, the part of
//       the segment inside the tile, and the run's tier (group_run_tier).  Tiers 0 / 1 are decided per entry.  Tier 2 runs
//       -- at most 7 long ones inside the tile and the two that cross its ends -- go round the block's four waves: a wave
//       keeps the run's 64 best, sorted, one per lane, and takes 64 entries at a time (sort across the lanes, then the
//       bitonic half-cleaner against the reversed list and a 6-step merge).  A run of a segment inside the tile ends there;
//       a crossing segment's run leaves its list in `partial`.
//   group_merge_kernel : one block per tile boundary; it acts where a segment crosses that boundary and began in the tile
//       in front of it, merges the lists of all the segment's runs (four waves, every fourth list each, then one merge of the
//       four) and writes the best per_key.
//
// Survivors are written to the row-indexed array the tail sorts (rank entries; every other row dead), so entries reach the
// tail in ascending position, which sort_composites' tie rule needs.  Plain C++ and vector memory operations only.

#include "scan_grouped.h"

#include <algorithm>

namespace mvf {
namespace {

constexpr uint32_t kMaxRuns = 16;  // tier-2 runs of a tile: <= kGroupTile / (kGroupRankMax + 1) inside + 2 crossing

__device__ __forceinline__ uint64_t comp_of_entry(uint64_t e) { return (e << 32) | (e >> 32); }  // and back

// a survivor to its row's place of the row-indexed array (the row is a held row's, below n; the test keeps a corrupt entry
// from being written anywhere else)
__device__ __forceinline__ void put_survivor(uint64_t* out, uint32_t n, uint64_t comp) {
    const uint32_t row = (uint32_t)comp;
    if (row < n) out[row] = comp_of_entry(comp);
}

// ascending across the wave's 64 lanes
__device__ __forceinline__ uint64_t wave_sort64(uint64_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (uint32_t s = size >> 1; s >= 1; s >>= 1) {
            const uint64_t w = __shfl_xor((unsigned long long)v, (int)s, 64);
            const bool keep_min = ((lane & s) == 0) == ((lane & size) == 0);
            v = (w < v) == keep_min ? w : v;
        }
    }
    return v;
}

// a, b ascending across the lanes -> the 64 smallest of both, ascending
__device__ __forceinline__ uint64_t wave_merge64(uint64_t a, uint64_t b, uint32_t lane) {
    const uint64_t r = __shfl((unsigned long long)b, (int)(63u - lane), 64);
    uint64_t v = r < a ? r : a;  // bitonic, and the 64 smallest
#pragma unroll
    for (uint32_t s = 32; s >= 1; s >>= 1) {
        const uint64_t w = __shfl_xor((unsigned long long)v, (int)s, 64);
        const bool keep_min = (lane & s) == 0;
        v = (w < v) == keep_min ? w : v;
    }
    return v;
}

__global__ void __launch_bounds__(256) group_bounds_kernel(const uint64_t* offsets, uint64_t n_keys, uint32_t live, uint2* bounds) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= live) return;
    uint64_t lo = 0, hi = n_keys;  // the last j with offsets[j] <= i; offsets[0] = 0
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid;
        else hi = mid;
    }
    bounds[i] = make_uint2((uint32_t)offsets[lo], (uint32_t)offsets[lo + 1]);
}

__global__ void __launch_bounds__(256) group_dead_fill_kernel(uint64_t* out, uint32_t n) {
    uint64_t* o = out + (size_t)blockIdx.y * n;
    for (uint32_t r = blockIdx.x * 256u + threadIdx.x; r < n; r += gridDim.x * 256u) o[r] = rank_entry(0u, r, true);
}

// grid (tiles, nq), block 256
__global__ void __launch_bounds__(256) group_tile_kernel(GroupParams p) {
    __shared__ uint64_t comp[kGroupTile];
    __shared__ uint32_t run_lo[kMaxRuns], run_hi[kMaxRuns], run_kind[kMaxRuns];  // kind 0: inside; 1 / 2: partial list 0 / 1
    __shared__ uint32_t nruns;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t q = blockIdx.y, tile0 = blockIdx.x * kGroupTile;
    const uint32_t cnt = min(kGroupTile, p.live - tile0);  // >= 1: the grid covers live
    const uint64_t* scored = p.scored + (size_t)q * p.live + tile0;
    uint64_t* out = p.out + (size_t)q * p.n;
    if (tid == 0) nruns = 0;
    uint64_t mine[4];
    uint32_t lo[4], hi[4], tier[4];
#pragma unroll
    for (int x = 0; x < 4; x++) {
        const uint32_t i = tid + (uint32_t)x * 256u;
        tier[x] = 3u;  // no entry
        if (i < cnt) {
            mine[x] = comp_of_entry(scored[i]);
            comp[i] = mine[x];
            const uint2 b = p.bounds[tile0 + i];
            const bool crossing = b.x < tile0 || b.y > tile0 + cnt;
            lo[x] = max(b.x, tile0) - tile0;
            hi[x] = min(b.y, tile0 + cnt) - tile0;
            tier[x] = group_run_tier(hi[x] - lo[x], p.per_key, crossing);
        }
    }
    __syncthreads();
#pragma unroll
    for (int x = 0; x < 4; x++) {
        const uint32_t i = tid + (uint32_t)x * 256u;
        if (tier[x] == 0u) {
            put_survivor(out, p.n, mine[x]);
        } else if (tier[x] == 1u) {
            uint32_t rank = 0;
            for (uint32_t j = lo[x]; j < hi[x]; j++) rank += comp[j] < mine[x] ? 1u : 0u;
            if (rank < p.per_key) put_survivor(out, p.n, mine[x]);
        } else if (tier[x] == 2u && i == lo[x]) {  // the run's first entry lists the run
            const uint2 b = p.bounds[tile0 + i];
            const uint32_t slot = atomicAdd(&nruns, 1u);
            if (slot < kMaxRuns) {
                run_lo[slot] = lo[x];
                run_hi[slot] = hi[x];
                run_kind[slot] = b.x < tile0 ? 1u : b.y > tile0 + cnt ? 2u : 0u;
            }
        }
    }
    __syncthreads();
    const uint32_t nr = min(nruns, kMaxRuns);
    for (uint32_t r = wave; r < nr; r += 4) {  // wave-uniform: every lane reaches the exchanges
        const uint32_t rl = run_lo[r], rh = run_hi[r], kind = run_kind[r];
        uint64_t best = kPadComposite;
        for (uint32_t j0 = rl; j0 < rh; j0 += 64) {
            const uint32_t j = j0 + lane;
            const uint64_t v = wave_sort64(j < rh ? comp[j] : kPadComposite, lane);
            best = j0 == rl ? v : wave_merge64(best, v, lane);
        }
        if (kind == 0u) {
            if (lane < p.per_key && best != kPadComposite) put_survivor(out, p.n, best);
        } else {
            p.partial[(((size_t)q * gridDim.x + blockIdx.x) * 2u + (kind - 1u)) * 64u + lane] = best;
        }
    }
}

// grid (tiles - 1, nq), block 256: block b looks at the boundary in front of tile b + 1
__global__ void __launch_bounds__(256) group_merge_kernel(GroupParams p, uint32_t tiles) {
    __shared__ uint64_t lists[4][64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t q = blockIdx.y, ft = blockIdx.x, e = (ft + 1u) * kGroupTile;  // e < live: tile ft + 1 exists
    const uint2 b = p.bounds[e];
    if (b.x >= e || b.x < ft * kGroupTile) return;  // (block-uniform) nothing crosses here, or it began further in front
    const uint32_t nitems = min((b.y - 1u) / kGroupTile, tiles - 1u) - ft + 1u;  // the segment's runs: tile ft's list 1, then lists 0
    const uint64_t* part = p.partial + (size_t)q * tiles * 128u;
    auto item = [&](uint32_t j) { return part[((size_t)(ft + j) * 2u + (j == 0u ? 1u : 0u)) * 64u + lane]; };
    uint64_t best = kPadComposite;
    uint32_t j = wave;
    uint64_t next = j < nitems ? item(j) : kPadComposite;
    while (j < nitems) {  // wave-uniform; the next list is on its way while this one is merged
        const uint64_t cur = next;
        j += 4;
        next = j < nitems ? item(j) : kPadComposite;
        best = wave_merge64(best, cur, lane);
    }
    lists[wave][lane] = best;
    __syncthreads();
    if (wave != 0) return;
    for (uint32_t w = 1; w < 4; w++) best = wave_merge64(best, lists[w][lane], lane);
    if (lane < p.per_key && best != kPadComposite) put_survivor(p.out + (size_t)q * p.n, p.n, best);
}

__global__ void __launch_bounds__(256) column_gather_kernel(const void* values, bool is_u64, const uint64_t* rows, uint64_t count,
                                                            uint64_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint64_t r = rows[i];
    out[i] = r == ~0ull ? 0ull : is_u64 ? static_cast<const uint64_t*>(values)[r] : (uint64_t)static_cast<const uint32_t*>(values)[r];
}

}  // namespace

hipError_t group_bounds_launch(const uint64_t* offsets, uint64_t n_keys, uint32_t live, uint2* bounds, hipStream_t s) {
    if (live == 0 || n_keys == 0) return hipSuccess;
    hipLaunchKernelGGL(group_bounds_kernel, dim3((live + 255u) / 256u), dim3(256), 0, s, offsets, n_keys, live, bounds);
    return hipGetLastError();
}

hipError_t group_dead_fill_launch(uint64_t* out, uint32_t n, uint32_t nq, hipStream_t s) {
    if (n == 0 || nq == 0) return hipSuccess;
    const uint32_t blocks = std::min<uint32_t>((n + 255u) / 256u, 4096u);
    hipLaunchKernelGGL(group_dead_fill_kernel, dim3(blocks, nq), dim3(256), 0, s, out, n);
    return hipGetLastError();
}

hipError_t group_best_launch(const GroupParams& p, hipStream_t s) {
    if (p.live == 0 || p.nq == 0) return hipSuccess;
    if (p.per_key < 1 || p.per_key > 64) return hipErrorInvalidValue;
    const uint32_t tiles = group_tiles(p.live);
    hipLaunchKernelGGL(group_tile_kernel, dim3(tiles, p.nq), dim3(256), 0, s, p);
    if (tiles > 1) hipLaunchKernelGGL(group_merge_kernel, dim3(tiles - 1, p.nq), dim3(256), 0, s, p, tiles);
    return hipGetLastError();
}

hipError_t column_gather_launch(const void* values, bool is_u64, const uint64_t* rows, uint64_t count, uint64_t* out, hipStream_t s) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(column_gather_kernel, dim3((uint32_t)((count + 255u) / 256u)), dim3(256), 0, s, values, is_u64, rows, count, out);
    return hipGetLastError();
}

}  // namespace mvf
