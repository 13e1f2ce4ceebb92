// scan_hamming_radius.hip — HR2 and HRP, the Hamming radius search: every row within r bits of each query, counted exactly and
// listed best first (scan_hamming_radius.h; DESIGN.md §5 "HR2 / HRP").  HQ (scan_hamming_mfma.hip) prepares the queries.
//
// The arithmetic is H2's (scan_hamming_mfma.hip, "Operands"): d(q, x) = popcount(q) + sum over the bits of x (1 - 2 q), FP4
// factors 0, +1, -1, v_mfma_scale_f32_16x16x128_f8f6f4 with both scales 2^0, f32 accumulators that hold every partial sum
// exactly.  What differs is everything behind the MFMAs.  A radius is known before the first row is read and never moves, so the
// scan keeps no selection state: no thresholds in LDS, no candidate buffers, no sort area, no settle and no barrier in the row
// loop.  A block's LDS is its staged query tile and one u32 count per query, so a tile of 16 queries is a few KiB and many
// blocks share a CU; the slices are not merged, so nothing caps their number (hamming_radius_form).
//
// HR2, grid (row slices x query tiles), 256 threads.  A wave owns 64 rows (four A fragments) per iteration against the tile's
// QT = 16 NC queries; rows go from global memory straight to registers (load_chunk), the next chunk's 16 bytes in flight under
// this chunk's MFMAs.  A lane holds the distances of 16 rows to ONE query per column tile, so it keeps that query's radius in
// the accumulators' start value, popcount(q) - r - 1 with r clamped to 8 x dim (an exact f32 of magnitude <= 4097): the
// accumulator ends as d - r - 1 and a row matches iff it is negative.  Per (row, query) behind the MFMAs that is a min over the
// lane's 16 values and one compare.  Only where one is negative are the row bound and the tombstone bit read (as offer does),
// the lane's count for the column tile bumped, and -- where entries are asked for -- the composite d << 32 | row appended to the
// query's list in the global scratch, the slot from a returning atomic on fill[q].  A lane that draws a slot at or beyond the
// cap stops appending for that query: a dense query costs the cap plus one atomic per lane, not one per match.  At the slice's
// end the lanes' counts meet in LDS and ONE global atomic per (block, query) with a non-zero count goes to counts[q].
//
// HRP, one block of 1024 threads per query: writes out_counts; where the count is within the cap the list holds every match:
// sorted in LDS (composites are unique, so arrival order does not matter), its first min(count, kout) entries written as H1
// writes them, H1's padding behind.  A query beyond the cap is left to the host (hamming_radius.hip).

#include "scan_hamming_radius.h"

#include "bitonic.h"
#include "hamming_select.h"

namespace mvf {
namespace {

constexpr int NT = (int)kHamRadiusThreads;
constexpr int F = (int)kHamRadiusWaveRows / 16;  // A fragments of a wave

extern __shared__ __align__(16) unsigned char ham_radius_smem[];

// what the start value takes off a query's popcount: the radius clamped to the row's bits, and one -- d = accumulator + this
__device__ __forceinline__ float radius_back(uint32_t radius, uint32_t dim) { return (float)((radius < 8u * dim ? radius : 8u * dim) + 1u); }

template <int NC>
HAM_KERNEL __launch_bounds__(NT) void hamming_radius_kernel(const HammingRadiusParams rp) {
    constexpr uint32_t QT = (uint32_t)NC * 16u;
    const HammingMfmaParams& a = rp.a;
    const HammingParams& p = a.p;
    const uint32_t tid = threadIdx.x, slice = blockIdx.x, tile = blockIdx.y, q0 = tile * QT;
    const uint32_t qn = p.nq - q0 < QT ? p.nq - q0 : QT;
    const uint32_t items = a.chunks * 4u * (uint32_t)NC * 64u;

    u32x4* staged = reinterpret_cast<u32x4*>(ham_radius_smem);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(staged + items);
    {
        const u32x4* src = reinterpret_cast<const u32x4*>(a.prepared) + (size_t)tile * items;
        for (uint32_t i = tid; i < items; i += NT) staged[i] = src[i];
        if (tid < QT) cnt[tid] = 0;
        __syncthreads();
    }

    const uint32_t lane = tid & 63u, wave = tid >> 6, r16 = lane & 15u, g = lane >> 4;
    // the lane's queries: the radius folded into the start; an idle column (an all-zero prepared query: every term >= 0) starts at 1
    float start[NC];
    uint32_t hits[NC], closed = 0;  // matches per column tile; bit c: the query's list is full
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const uint32_t q = (uint32_t)c * 16u + r16;
        start[c] = q < qn ? a.starts[q0 + q] - radius_back(rp.radii[q0 + q], p.dim) : 1.0f;
        hits[c] = 0;
    }
    const u32x4 tail = step_mask(p.V - 1u, p.dim);
    const uint64_t lo = (uint64_t)slice * p.slice_rows;
    const uint64_t hi = lo + p.slice_rows < p.n ? lo + p.slice_rows : p.n;

    for (uint64_t wrow = lo + (uint64_t)wave * kHamRadiusWaveRows; wrow < hi; wrow += (uint64_t)(NT / 64) * kHamRadiusWaveRows) {
        v4f acc[F][NC];
#pragma unroll
        for (int c = 0; c < NC; c++) {
            // (opaque per iteration: the start values are loop-invariant, and hoisted they would hold a second register per
            // accumulator for the whole slice -- the 128-query tile then spills)
            float s = start[c];
            asm volatile("" : "+v"(s));
#pragma unroll
            for (int f = 0; f < F; f++) acc[f][c] = v4f{s, s, s, s};
        }
        uint32_t cur[F][4], nxt[F][4];
        load_chunk(cur, p, wrow + r16, hi, 0u, g, tail);
#pragma unroll 1
        for (uint32_t ch = 0; ch < a.chunks; ch++) {
            if (ch + 1u < a.chunks) load_chunk(nxt, p, wrow + r16, hi, ch + 1u, g, tail);  // in flight under this chunk's MFMAs
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
        // element i of acc[f][c]: row 16 f + 4 g + i of the wave's rows against query 16 c + r16 of the tile, as d - r - 1
#pragma unroll
        for (int c = 0; c < NC; c++) {
            float least = acc[0][c][0];
#pragma unroll
            for (int f = 0; f < F; f++)
#pragma unroll
                for (int i = 0; i < 4; i++) least = __builtin_fminf(least, acc[f][c][i]);
            if (least < 0.0f) {  // the rare path
                const uint32_t q = q0 + (uint32_t)c * 16u + r16;
                const float back = radius_back(rp.radii[q], p.dim);  // (least < 0: the query is one of the window's)
#pragma unroll
                for (int f = 0; f < F; f++)
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const uint64_t r64 = wrow + (uint64_t)(f * 16 + i) + g * 4u;
                        if (acc[f][c][i] < 0.0f && r64 < hi) {
                            const uint32_t r = (uint32_t)r64;
                            if (p.tomb && ((p.tomb[r >> 5] >> (r & 31u)) & 1u)) continue;
                            hits[c]++;
                            if (rp.lists && !((closed >> c) & 1u)) {
                                const uint32_t slot = __hip_atomic_fetch_add(&rp.fill[q], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                if (slot < rp.cap)
                                    rp.lists[(size_t)q * rp.cap + slot] = ((uint64_t)(uint32_t)(acc[f][c][i] + back) << 32) | r;
                                else
                                    closed |= 1u << c;
                            }
                        }
                    }
            }
        }
    }
    // the lanes' counts: through LDS, then one global atomic per query of the tile that matched in this slice
#pragma unroll
    for (int c = 0; c < NC; c++)
        if (hits[c]) __hip_atomic_fetch_add(&cnt[c * 16 + (int)r16], hits[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    if (tid < qn && cnt[tid]) __hip_atomic_fetch_add(&rp.counts[q0 + tid], cnt[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// HRP: grid (nq), block 1024, dynamic LDS cap x 8 bytes (none where kout = 0)
HAM_KERNEL __launch_bounds__(1024) void hamming_radius_pack_kernel(const HammingRadiusParams rp) {
    const HammingParams& p = rp.a.p;
    uint64_t* buf = reinterpret_cast<uint64_t*>(ham_radius_smem);
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t m = rp.counts[q];
    if (tid == 0) rp.out_counts[q] = m;
    if (rp.kout == 0 || m > rp.cap) return;  // counts only; or the list lost arrivals: the host completes this query by a top-k search
    const uint32_t P = m < 2u ? 2u : next_pow2(m);
    const uint64_t* list = rp.lists + (size_t)q * rp.cap;
    for (uint32_t i = tid; i < P; i += 1024u) buf[i] = i < m ? list[i] : kPadComposite;
    __syncthreads();
    bitonic_sort_u64_1024(buf, P, (int)tid);
    for (uint32_t i = tid; i < rp.kout; i += 1024u) {
        const size_t o = (size_t)q * rp.kout + i;
        if (i < m) {
            const uint64_t comp = buf[i];
            const uint32_t r = (uint32_t)comp;
            const int32_t d = (int32_t)(comp >> 32);
            p.out_scores[o] = (float)d;  // exact: d <= 4096
            p.out_indices[o] = p.ids ? p.ids[r] : p.index_base + r;
            if (p.out_raw) p.out_raw[o] = d;
        } else {  // the Hamming search's padding
            p.out_scores[o] = pad_score(MVF_METRIC_L2);
            p.out_indices[o] = ~0ull;
            if (p.out_raw) p.out_raw[o] = 0;
        }
    }
}

}  // namespace

hipError_t hamming_radius_launch(const HammingRadiusForm& f, const HammingRadiusParams& r, hipStream_t s, hipEvent_t* marks) {
    if (r.a.p.nq == 0) return hipSuccess;
    HammingRadiusParams arg = r;
    void* args[] = {&arg};
    auto mark = [&](int i) { return marks ? hipEventRecord(marks[i], s) : hipSuccess; };
    if (const hipError_t e = mark(0)) return e;
    const void* fn = f.query_tile == 128u ? reinterpret_cast<const void*>(&hamming_radius_kernel<8>)
                   : f.query_tile == 64u ? reinterpret_cast<const void*>(&hamming_radius_kernel<4>)
                   : f.query_tile == 32u ? reinterpret_cast<const void*>(&hamming_radius_kernel<2>)
                   : f.query_tile == 16u ? reinterpret_cast<const void*>(&hamming_radius_kernel<1>) : nullptr;
    if (!fn || f.lds_bytes > kHamRadiusLds || r.cap != kHamRadiusListCap || r.kout > kHamRadiusMaxOut || (r.kout && !r.lists))
        return hipErrorInvalidValue;
    if (f.row_slices)
        if (const hipError_t e = hamming_prepare_launch(r.a, s)) return e;  // HQ
    if (const hipError_t e = mark(1)) return e;
    if (f.row_slices) {  // HR2
        if (f.lds_bytes > 48u * 1024u) {
            const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.lds_bytes);
            if (e != hipSuccess) return e;
        }
        if (const hipError_t e = hipLaunchKernel(fn, dim3(f.row_slices, f.tiles), dim3(kHamRadiusThreads), args, f.lds_bytes, s)) return e;
    }
    if (const hipError_t e = mark(2)) return e;
    {  // HRP
        const void* pfn = reinterpret_cast<const void*>(&hamming_radius_pack_kernel);
        const size_t lds = r.kout ? (size_t)r.cap * 8u : 0u;
        if (lds > 48u * 1024u) {
            const hipError_t e = hipFuncSetAttribute(pfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        if (const hipError_t e = hipLaunchKernel(pfn, dim3(r.a.p.nq), dim3(1024), args, lds, s)) return e;
    }
    return mark(3);
}

}  // namespace mvf
