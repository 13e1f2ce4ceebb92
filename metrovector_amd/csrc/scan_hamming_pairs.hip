// scan_hamming_pairs.hip — HJ and HJP, the Hamming pair join: every two live rows of one corpus within r bits of each other,
// counted exactly, with each row's degree, and listed in ascending (i, j) order (scan_hamming_pairs.h; DESIGN.md §5 "HJ / HJP").
//
// The arithmetic is H2's (scan_hamming_mfma.hip, "Operands"): d(q, x) = popcount(q) + sum over the bits of x (1 - 2 q), FP4
// factors 0, +1, -1 on v_mfma_scale_f32_16x16x128_f8f6f4 with both scales 2^0, exact f32 accumulators; and the radius sits in
// the accumulators' start value as in HR2 (scan_hamming_radius.hip), popcount(q) - r - 1 with r clamped to 8 x dim, so a pair
// matches iff its accumulator ends negative.  What is new is where the two operands come from and how the work is cut.
//
// HJ, a 1-D grid over the launched (column tile, span) pairs (ham_pairs_decode), 256 threads.
//   Fused preparation.  Both operands are rows of the same resident corpus.  The block's "queries" are the QT consecutive rows of
//   its column tile, and it expands them itself, from the packed bytes straight into LDS in HQ's fragment order
//   [chunk][step][column tile of 16][lane] x 16 bytes: item i of that order is one 4-byte word of one row, read from global
//   memory, masked to `dim`, and spread into four FP4 words.  One thread per column counts the row's bits and leaves the start
//   value beside the fragments.  A column whose row is deleted or behind the corpus' end is idle: start 1.0, +1.0 factors
//   everywhere (the bits of an all-zero row), so it can never end negative.  Nothing prepared ever exists in HBM.
//   The span.  As in H2 a wave owns 64 rows (four A fragments) per iteration against all QT columns, rows from global memory
//   straight to registers (load_chunk), the next chunk's 16 bytes in flight under this chunk's MFMAs.  In the span that holds
//   the tile itself the iterations in front of the tile's first row are skipped: their rows pair with no column of the tile.
//   Behind the MFMAs a lane takes the min over its 16 values per column and makes one compare; the wave enters the rare path
//   for a column tile of 16 only where some lane's min is negative.  There a match is a negative accumulator whose row lies
//   inside the span, ABOVE the column's position -- which drops the lower triangle and the diagonal -- and is not deleted.
//   Column side of the degrees: per-lane counts, through LDS at the block's end, one global atomic per (block, column).  Row
//   side: one ballot per accumulator element gives the 16 lanes that share a row their row's matches in this column tile; the
//   sums ride in one byte per row (QT <= 128) and, behind the last column tile, the lane whose index names the row adds them with
//   ONE global atomic per (row, column tile).  The total is the sum of the column counts: one u64 atomic per block.
//   Listing: a match appends i << 32 | j and d to the call's list, the slot from a returning u64 atomic on the fill counter; a
//   lane that draws a slot at or behind the cap stops appending for the rest of the block (the list is then not used at all).
//
// HJP.  With total <= cap the list holds every pair once, so arrival order does not matter: stable LSD radix passes
// (radix_pass.h; RsKeyDigit on the whole key, 8-bit digits, d as the payload) over the bytes of i and of j that the row count
// leaves non-zero, then a writer turns positions into reported names.

#include "scan_hamming_pairs.h"

#include "hamming_select.h"
#include "radix_pass.h"

namespace mvf {
namespace {

constexpr int NT = (int)kHamPairsThreads;
constexpr int F = (int)kHamPairsWaveRows / 16;  // A fragments of a wave

extern __shared__ __align__(16) unsigned char ham_pairs_smem[];

__device__ __forceinline__ bool row_deleted(const uint32_t* tomb, uint32_t r) { return tomb && ((tomb[r >> 5] >> (r & 31u)) & 1u); }

template <int NC>
HAM_KERNEL __launch_bounds__(NT) void hamming_pairs_kernel(const HammingPairsParams rp) {
    constexpr uint32_t QT = (uint32_t)NC * 16u;
    const HammingParams& p = rp.p;
    const uint32_t tid = threadIdx.x;
    uint64_t tile, span;
    ham_pairs_decode(rp.block_base + blockIdx.x, rp.spans, rp.tiles_per_span, &tile, &span);
    const uint64_t col0 = tile * QT;  // the tile's first row
    const uint32_t items = rp.chunks * 4u * (uint32_t)NC * 64u;
    const uint32_t bits = 8u * p.dim, rc = rp.radius < bits ? rp.radius : bits;
    const float back = (float)(rc + 1u);  // d = accumulator + back

    u32x4* staged = reinterpret_cast<u32x4*>(ham_pairs_smem);
    float* start = reinterpret_cast<float*>(staged + items);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(start + QT);
    uint32_t* block_total = cnt + QT;
    const u32x4 tail = step_mask(p.V - 1u, p.dim);
    {
        // the tile's rows as B fragments (HQ's item order and HQ's expansion)
        for (uint32_t i = tid; i < items; i += NT) {
            const uint32_t lane = i % 64u, c = (i / 64u) % (uint32_t)NC, m = (i / (64u * NC)) % 4u, t = i / (256u * NC);
            const uint64_t row = col0 + c * 16u + (lane & 15u);
            const uint32_t at = t * 64u + (lane >> 4) * 16u + m * 4u;
            uint32_t w = 0;
            if (row < p.n && at < p.dim && !row_deleted(p.tomb, (uint32_t)row)) {
                w = *reinterpret_cast<const uint32_t*>(p.rows + row * p.pitch + at);  // (at < dim <= pitch, pitch a multiple of 16)
                if (p.dim - at < 4u) w &= (1u << (8u * (p.dim - at))) - 1u;
            }
            u32x4 out;
            out.x = 0x22222222u | ((w & 0x11111111u) << 3);
            out.y = 0x22222222u | (((w >> 1) & 0x11111111u) << 3);
            out.z = 0x22222222u | (((w >> 2) & 0x11111111u) << 3);
            out.w = 0x22222222u | (((w >> 3) & 0x11111111u) << 3);
            staged[i] = out;
        }
        if (tid < QT) {
            const uint64_t row = col0 + tid;
            float s = 1.0f;  // an idle column
            if (row < p.n && !row_deleted(p.tomb, (uint32_t)row)) {
                const u32x4* src = reinterpret_cast<const u32x4*>(p.rows + row * p.pitch);
                uint32_t ones = 0;
                for (uint32_t v = 0; v < p.V; v++) {
                    u32x4 x = src[v];
                    if (v == p.V - 1u) x.x &= tail.x, x.y &= tail.y, x.z &= tail.z, x.w &= tail.w;
                    ones += __builtin_popcount(x.x) + __builtin_popcount(x.y) + __builtin_popcount(x.z) + __builtin_popcount(x.w);
                }
                s = (float)ones - back;  // exact: -4097 .. 4095
            }
            start[tid] = s;
            cnt[tid] = 0;
        }
        if (tid == 0) block_total[0] = 0;
        __syncthreads();
    }

    const uint32_t lane = tid & 63u, wave = tid >> 6, r16 = lane & 15u, g = lane >> 4;
    uint32_t hits[NC], closed = 0;  // matches per column tile of 16; set: the list is full
#pragma unroll
    for (int c = 0; c < NC; c++) hits[c] = 0;
    uint64_t lo = span * rp.span_rows;
    const uint64_t hi = lo + rp.span_rows < p.n ? lo + rp.span_rows : p.n;
    {
        const uint64_t skip = col0 / kHamPairsStepRows * kHamPairsStepRows;  // whole iterations in front of the tile's first row
        if (skip > lo) lo = skip;
    }

    for (uint64_t wrow = lo + (uint64_t)wave * kHamPairsWaveRows; wrow < hi; wrow += (uint64_t)kHamPairsStepRows) {
        v4f acc[F][NC];
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const float s = start[c * 16 + (int)r16];
#pragma unroll
            for (int f = 0; f < F; f++) acc[f][c] = v4f{s, s, s, s};
        }
        uint32_t cur[F][4], nxt[F][4];
        load_chunk(cur, p, wrow + r16, hi, 0u, g, tail);
#pragma unroll 1
        for (uint32_t ch = 0; ch < rp.chunks; ch++) {
            if (ch + 1u < rp.chunks) load_chunk(nxt, p, wrow + r16, hi, ch + 1u, g, tail);  // in flight under this chunk's MFMAs
            const u32x4* bq = staged + (size_t)ch * 4u * NC * 64u + lane;
#pragma unroll
            for (int m = 0; m < 4; m++) {
                v8i av[F];
#pragma unroll
                for (int f = 0; f < F; f++) av[f] = fp4_row_operand(cur[f][m]);
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    const u32x4 b = bq[(m * NC + c) * 64];
                    const v8i bv = v8i{(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
#pragma unroll
                    for (int f = 0; f < F; f++)
                        acc[f][c] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av[f], bv, acc[f][c], 4, 4, 0, 127, 0, 127);
                }
            }
#pragma unroll
            for (int f = 0; f < F; f++)
#pragma unroll
                for (int j = 0; j < 4; j++) cur[f][j] = nxt[f][j];
        }
        // element i of acc[f][c]: row 16 f + 4 g + i of the wave's rows against column 16 c + r16 of the tile, as d - r - 1
        uint32_t rowsum[F];  // byte i of rowsum[f]: matches of row 16 f + 4 g + i in this column tile (every lane of the row's 16)
#pragma unroll
        for (int f = 0; f < F; f++) rowsum[f] = 0;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            float least = acc[0][c][0];
#pragma unroll
            for (int f = 0; f < F; f++)
#pragma unroll
                for (int i = 0; i < 4; i++) least = __builtin_fminf(least, acc[f][c][i]);
            if (__builtin_amdgcn_ballot_w64(least < 0.0f)) {  // the rare path, entered by the whole wave
                const uint64_t col = col0 + (uint32_t)c * 16u + r16;
#pragma unroll
                for (int f = 0; f < F; f++)
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const uint64_t r64 = wrow + (uint64_t)(f * 16 + i) + g * 4u;
                        bool match = acc[f][c][i] < 0.0f && r64 < hi && r64 > col;
                        if (match) match = !row_deleted(p.tomb, (uint32_t)r64);
                        if (match) {
                            hits[c]++;
                            if (rp.list && !closed) {
                                const uint64_t slot = __hip_atomic_fetch_add(&rp.counters[1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                if (slot < rp.cap) {
                                    rp.list[slot] = (col << 32) | r64;
                                    rp.dist[slot] = (uint32_t)(acc[f][c][i] + back);
                                } else {
                                    closed = 1u;
                                }
                            }
                        }
                        if (rp.degrees) {
                            const unsigned long long who = __builtin_amdgcn_ballot_w64(match);
                            rowsum[f] += (uint32_t)__builtin_popcount((uint32_t)(who >> (g * 16u)) & 0xFFFFu) << (8 * i);
                        }
                    }
            }
        }
        if (rp.degrees) {
            // lane r16 of a k-group names row 16 (r16 / 4) + 4 g + r16 % 4 of the wave's rows
            const uint32_t word = r16 < 4u ? rowsum[0] : r16 < 8u ? rowsum[1] : r16 < 12u ? rowsum[2] : rowsum[3];
            const uint32_t add = (word >> (8u * (r16 & 3u))) & 0xFFu;
            if (add) {  // (a match lies inside the span, so the row does)
                const uint64_t r64 = wrow + (uint64_t)((r16 >> 2) * 16u + (r16 & 3u)) + g * 4u;
                __hip_atomic_fetch_add(&rp.degrees[r64], add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    // the lanes' column counts: through LDS, then one global atomic per column that matched in this block, and one for the total
#pragma unroll
    for (int c = 0; c < NC; c++)
        if (hits[c]) __hip_atomic_fetch_add(&cnt[c * 16 + (int)r16], hits[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    if (tid < QT && cnt[tid]) {  // (a column that matched holds a live row of the corpus)
        if (rp.degrees) __hip_atomic_fetch_add(&rp.degrees[col0 + tid], cnt[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(block_total, cnt[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // <= QT x span_rows
    }
    __syncthreads();
    if (tid == 0 && block_total[0])
        __hip_atomic_fetch_add(&rp.counters[0], (uint64_t)block_total[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// HJP's writer: sorted composites and distances -> the reported pair list
__global__ void __launch_bounds__(256) hamming_pairs_write_kernel(const HammingParams p, const uint64_t* list, const uint32_t* dist, uint64_t m,
                                                                  uint64_t* out_first, uint64_t* out_second, int32_t* out_raw) {
    const uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= m) return;
    const uint64_t comp = list[e];  // (read before the writes: the outputs may be the list's own arrays)
    const uint32_t d = dist[e];
    const uint32_t i = (uint32_t)(comp >> 32), j = (uint32_t)comp;
    out_first[e] = p.ids ? p.ids[i] : p.index_base + i;
    out_second[e] = p.ids ? p.ids[j] : p.index_base + j;
    if (out_raw) out_raw[e] = (int32_t)d;
}

}  // namespace

hipError_t hamming_pairs_scan_launch(const HammingPairsForm& f, const HammingPairsParams& r, hipStream_t s) {
    if (f.blocks == 0) return hipSuccess;
    const void* fn = f.query_tile == 128u ? reinterpret_cast<const void*>(&hamming_pairs_kernel<8>)
                   : f.query_tile == 64u ? reinterpret_cast<const void*>(&hamming_pairs_kernel<4>)
                   : f.query_tile == 32u ? reinterpret_cast<const void*>(&hamming_pairs_kernel<2>)
                   : f.query_tile == 16u ? reinterpret_cast<const void*>(&hamming_pairs_kernel<1>) : nullptr;
    if (!fn || f.lds_bytes > kHamPairsLds || r.chunks != f.chunks || r.span_rows != f.span_rows || r.tiles_per_span != f.tiles_per_span ||
        r.spans != f.spans || (r.list && (!r.dist || !r.cap)))
        return hipErrorInvalidValue;
    if (f.lds_bytes > 48u * 1024u) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.lds_bytes);
        if (e != hipSuccess) return e;
    }
    HammingPairsParams arg = r;
    void* args[] = {&arg};
    for (uint64_t b0 = 0; b0 < f.blocks; b0 += kHamPairsGrid) {
        arg.block_base = b0;
        const uint64_t nb = f.blocks - b0 < kHamPairsGrid ? f.blocks - b0 : kHamPairsGrid;
        if (const hipError_t e = hipLaunchKernel(fn, dim3((uint32_t)nb), dim3(kHamPairsThreads), args, f.lds_bytes, s)) return e;
    }
    return hipSuccess;
}

hipError_t hamming_pairs_order_launch(const HammingParams& p, uint64_t* list_a, uint32_t* dist_a, uint64_t* list_b, uint32_t* dist_b, uint64_t m,
                                      uint32_t* bh, uint32_t* tot, uint64_t* out_first, uint64_t* out_second, int32_t* out_raw, hipStream_t s) {
    if (m == 0) return hipSuccess;
    static_assert(kRsTile == 2048, "ham_pairs_sort_tiles() counts the shared pass's tiles");
    if (m > kHamPairsMaxPairs || p.n < 2u) return hipErrorInvalidValue;
    const uint32_t NB = ham_pairs_sort_tiles(m);
    int bytes = 1;  // of a row position
    while (bytes < 4 && ((p.n - 1u) >> (8 * bytes))) bytes++;
    uint64_t *kin = list_a, *kout = list_b;
    uint32_t *din = dist_a, *dout = dist_b;
    for (int half = 0; half < 2; half++)  // j's bytes, then i's: an even number of passes
        for (int b = 0; b < bytes; b++) {
            const int shift = 32 * half + 8 * b;
            hipLaunchKernelGGL((rs_hist_kernel<8, RsKeyDigit>), dim3(NB), dim3(256), 0, s, kin, (size_t)m, shift, bh, NB, 0, 0);
            hipLaunchKernelGGL(rs_scan_kernel, dim3(256), dim3(256), 0, s, bh, NB, tot, 0);
            hipLaunchKernelGGL((rs_scatter_kernel<8, true, RsKeyDigit, true>), dim3(NB), dim3(256), 0, s, kin, kout, din, dout, (size_t)m, shift, bh,
                               tot, NB, 0, 0);
            uint64_t* tk = kin;
            kin = kout, kout = tk;
            uint32_t* td = din;
            din = dout, dout = td;
        }
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(hamming_pairs_write_kernel, dim3((uint32_t)((m + 255u) / 256u)), dim3(256), 0, s, p, kin, din, m, out_first, out_second, out_raw);
    return hipGetLastError();
}

}  // namespace mvf
