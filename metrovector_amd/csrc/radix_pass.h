// radix_pass.h — one stable pass of an LSD radix sort of 64-bit words: histogram, digit scan, scatter.  Stated once for the two
// device-wide sorts: the rank entries of sort_topk.hip (digit from the key half, 8 or 11 bits wide, a batch of lists) and the
// (key, row) pairs of scan_partition.hip (digit from the whole 64-bit key, 8 bits, a row moved with every key).  The
// instantiations and their launch sequences stay in those two files.
//
// A tile is kRsTile words, one block of 256 threads each.  bh[d * NB + tile] counts the tile's words with digit d; the scatter
// wants them summed over the tiles in front (rs_scan_kernel, which leaves the digits' totals in tot) or sums them itself.
// blockIdx.y picks the list of a batch: list l at in / out + l stride, its counts at bh + l bh_stride and tot + l 2048.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mvf {

constexpr int kRsItems = 8, kRsTile = 256 * kRsItems;  // words per thread / per block tile

// Where a word's digit comes from (the kernels mask the width).  A rank entry's key is its low half: the 11-bit digit at
// shift 22 is bits 22..31 of that half, never the position's low bit.
struct RsEntryDigit {
    static __device__ __forceinline__ uint32_t at(uint64_t e, int shift) { return (uint32_t)e >> shift; }
};
struct RsKeyDigit {
    static __device__ __forceinline__ uint32_t at(uint64_t key, int shift) { return (uint32_t)(key >> shift); }
};

// Exclusive scan of one value per thread of a 256-thread block (thread 0 walks the 256 partial sums: a microsecond, once per
// block); *total, where wanted, receives their sum from thread 0.  part: 256 words of LDS, free again after the next barrier.
__device__ __forceinline__ uint32_t block_scan_256(uint32_t v, uint32_t* part, uint32_t* total = nullptr) {
    part[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int t = 0; t < 256; t++) {
            const uint32_t x = part[t];
            part[t] = run;
            run += x;
        }
        if (total) *total = run;
    }
    __syncthreads();
    return part[threadIdx.x];
}

namespace {  // the kernels are each including file's own, like the ones it defines itself

template <int BITS, class Digit>
__global__ void __launch_bounds__(256) rs_hist_kernel(const uint64_t* in, size_t m, int shift, uint32_t* bh, uint32_t NB, size_t stride,
                                                       size_t bh_stride) {
    constexpr int NBIN = 1 << BITS;
    __shared__ uint32_t lh[NBIN];
    in += (size_t)blockIdx.y * stride, bh += (size_t)blockIdx.y * bh_stride;
    for (int i = threadIdx.x; i < NBIN; i += 256) lh[i] = 0;
    __syncthreads();
    const size_t t0 = (size_t)blockIdx.x * kRsTile;
#pragma unroll
    for (int r = 0; r < kRsItems; r++) {
        const size_t i = t0 + (size_t)r * 256 + threadIdx.x;
        if (i < m) atomicAdd(&lh[Digit::at(in[i], shift) & (NBIN - 1)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NBIN; i += 256) bh[(size_t)i * NB + blockIdx.x] = lh[i];
}

// block d: exclusive scan of digit d's per-tile counts in place, the digit's total to tot[d]
__global__ void __launch_bounds__(256) rs_scan_kernel(uint32_t* bh, uint32_t NB, uint32_t* tot, size_t bh_stride) {
    __shared__ uint32_t part[256];
    bh += (size_t)blockIdx.y * bh_stride, tot += (size_t)blockIdx.y * 2048;
    uint32_t* row = bh + (size_t)blockIdx.x * NB;
    const uint32_t per = (NB + 255) / 256, lo = threadIdx.x * per;
    uint32_t s = 0;
    for (uint32_t i = lo; i < lo + per && i < NB; i++) s += row[i];
    uint32_t run = block_scan_256(s, part, &tot[blockIdx.x]);
    for (uint32_t i = lo; i < lo + per && i < NB; i++) {
        const uint32_t v = row[i];
        row[i] = run;
        run += v;
    }
}

// Block b scatters its tile in order.  Wave w owns the tile's words [w TW, (w + 1) TW) and walks them in rounds of 64: a
// lane's rank among the words of its digit = the wave's running count of the digit (LDS) + its rank among the round's lanes
// with that digit (one ballot per digit bit).  Waves in order, rounds in order, lanes in order: stable.
// SCANNED: bh holds the tiles' counts already scanned per digit and tot the digits' totals (rs_scan_kernel); otherwise (few
// tiles) the block sums the raw counts of the tiles in front of it, and of all tiles, itself.
// PAYLOAD: pay_in[i] travels with in[i] to pay_out (one list, not batched); otherwise the two pointers are not read.
template <int BITS, bool SCANNED, class Digit, bool PAYLOAD>
__global__ void __launch_bounds__(256) rs_scatter_kernel(const uint64_t* in, uint64_t* out, const uint32_t* pay_in, uint32_t* pay_out, size_t m,
                                                          int shift, const uint32_t* bh, const uint32_t* tot, uint32_t NB, size_t stride,
                                                          size_t bh_stride) {
    constexpr int NBIN = 1 << BITS, PER = NBIN / 256;
    in += (size_t)blockIdx.y * stride, out += (size_t)blockIdx.y * stride, bh += (size_t)blockIdx.y * bh_stride, tot += (size_t)blockIdx.y * 2048;
    __shared__ uint32_t dbase[NBIN];     // digit d's first output slot + what the tiles in front of this one hold of it
    __shared__ uint32_t cw[4][NBIN];     // per wave: running count per digit, then the wave's offset inside the block's share
    __shared__ uint32_t part[256];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    {
        // digit totals and this tile's share: thread t owns digits [t PER, (t + 1) PER)
        uint32_t mine = 0;
        for (int x = 0; x < PER; x++) {
            const int d = tid * PER + x;
            uint32_t total, before;
            if (SCANNED) {
                total = tot[d];
                before = bh[(size_t)d * NB + blockIdx.x];
            } else {
                total = before = 0;
                for (uint32_t b = 0; b < NB; b++) {
                    const uint32_t v = bh[(size_t)d * NB + b];
                    total += v;
                    before += b < blockIdx.x ? v : 0u;
                }
            }
            cw[0][d] = total;
            dbase[d] = before;
            mine += total;
        }
        uint32_t run = block_scan_256(mine, part);
        for (int x = 0; x < PER; x++) {
            const int d = tid * PER + x;
            const uint32_t total = cw[0][d];
            dbase[d] += run;
            run += total;
        }
        __syncthreads();
        for (int w = 0; w < 4; w++)
            for (int x = 0; x < PER; x++) cw[w][tid * PER + x] = 0;
        __syncthreads();
    }
    constexpr int TW = kRsTile / 4, ROUNDS = TW / 64;
    const size_t w0 = (size_t)blockIdx.x * kRsTile + (size_t)wave * TW;
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint64_t el[ROUNDS];
    uint32_t ep[PAYLOAD ? ROUNDS : 1], lr[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; r++) {
        const size_t i = w0 + (size_t)r * 64 + lane;
        const bool valid = i < m;
        el[r] = valid ? in[i] : 0ull;
        if constexpr (PAYLOAD) ep[r] = valid ? pay_in[i] : 0u;
        const uint32_t d = Digit::at(el[r], shift) & (NBIN - 1);
        unsigned long long peers = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
        for (int b = 0; b < BITS; b++) {
            const unsigned long long bm = __builtin_amdgcn_ballot_w64((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? bm : ~bm;
        }
        const uint32_t rank = (uint32_t)__builtin_popcountll(peers & lt);
        const uint32_t base = valid ? cw[wave][d] : 0u;  // a wave's LDS operations execute in order: every peer reads before the leader writes
        if (valid && rank == 0) cw[wave][d] = base + (uint32_t)__builtin_popcountll(peers);
        lr[r] = base + rank;
    }
    __syncthreads();
    for (int x = 0; x < PER; x++) {  // the waves' offsets inside the block's share of the thread's digits
        const int d = tid * PER + x;
        uint32_t run = 0;
        for (int w = 0; w < 4; w++) {
            const uint32_t v = cw[w][d];
            cw[w][d] = run;
            run += v;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ROUNDS; r++) {
        const size_t i = w0 + (size_t)r * 64 + lane;
        if (i < m) {
            const uint32_t d = Digit::at(el[r], shift) & (NBIN - 1);
            const size_t o = (size_t)dbase[d] + cw[wave][d] + lr[r];
            out[o] = el[r];
            if constexpr (PAYLOAD) pay_out[o] = ep[r];
        }
    }
}

}  // namespace
}  // namespace mvf
