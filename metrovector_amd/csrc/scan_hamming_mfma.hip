// scan_hamming_mfma.hip — HQ and H2, the Hamming search's batch route on the matrix unit (scan_hamming_mfma.h; DESIGN.md §5
// "HQ / H2").
//
// With a row x as 0/1 values and a query q as q' = 1 - 2q in {+1, -1},  d(q, x) = popcount(q) + sum over the bits of x q':
// an integer GEMM whose partial sums stay below 2^24 in magnitude, so f32 accumulators hold them exactly in any order, and
// whose factors 0, +1, -1 are exact in FP4 (E2M1: 0x0, 0x2, 0xA).  v_mfma_scale_f32_16x16x128_f8f6f4 with both operands FP4
// and both scales 2^0 multiplies 16 rows x 16 queries x 128 bits.
//
// Operands.  Lane l of a wave serves index l % 16 (a row of the A fragment, a query of the B fragment) and k-group l / 16 on
// both sides, and holds 32 FP4 values -- 128 bits, four VGPRs -- of its k-group.  The order of the bits inside an instruction
// is free as long as rows and queries share it; the one chosen makes the rows' side cheapest:
//   a lane loads the 16 bytes at offset 64 t + 16 g of its row (g its k-group; a wave reads whole 64-byte lines of 16 rows), and
//   step m = 0 .. 3 of chunk t takes the lane's word m, w: VGPR j of the operand holds bit 4 n + j of w in nibble n,
//   (w >> (j - 1)) & 0x22222222 (j = 0: (w << 1) & ...) -- 0x2 = 1.0 where the bit is set, 0 elsewhere.
// HQ writes the queries' side in the same order -- 0x22222222 | ((w >> j) & 0x11111111) << 3: -1.0 where the bit is set, +1.0
// elsewhere -- as [tile][chunk][step][query column tile][lane] x 16 bytes, the order in which H2's lanes read B fragments: a
// block stages its tile with straight 16-byte copies and a wave's ds_read_b128 of one fragment covers 1 KiB without a bank
// conflict.  Bits behind `dimension` are +1.0 on the queries' side and 0 on the rows'.
//
// H2, grid (row slices x query tiles), 256 threads: the tile's prepared queries stay in LDS for the whole slice; a wave owns 64
// rows (four A fragments) of the block's 256 per iteration against all QT queries, accumulators started from popcount(q); the
// chunk loop is outermost, so an expanded A operand is used QT / 16 times and a B fragment four times.  Behind it a lane holds
// four rows' distances to one query per tile, converts them (exact) and offers them as H0 does -- composite below the query's
// threshold, tombstone clear -- to the query's buffer in the global scratch cand[slice][tile][query][buf], the slot from an
// LDS counter.  A buffer that could not take another iteration is read into the LDS sort area, sorted, cut to k and written
// back (same block, behind a barrier); at the slice's end every buffer is, and the lists go where H0 leaves them.

#include "scan_hamming_mfma.h"

#include "bitonic.h"
#include "hamming_select.h"

namespace mvf {
namespace {

constexpr int NT = (int)kHamMfmaThreads;
constexpr int F = (int)kHamMfmaWaveRows / 16;  // A fragments of a wave

// HQ: one thread per 16-byte item of the prepared queries; the first item of a query also counts its bits.  Queries behind
// the window's last fill their tile as all-zero queries: nothing H2 stages is unwritten.
HAM_KERNEL __launch_bounds__(256) void hamming_prepare_kernel(const HammingMfmaParams a) {
    const HammingParams& p = a.p;
    const uint32_t QT = p.query_tile, NC = QT / 16u;
    const uint32_t per_tile = a.chunks * 4u * NC * 64u;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.tiles * per_tile) return;
    const uint32_t tile = i / per_tile, r = i % per_tile;
    const uint32_t lane = r % 64u, c = (r / 64u) % NC, m = (r / (64u * NC)) % 4u, t = r / (256u * NC);
    const uint32_t slot = tile * QT + c * 16u + (lane & 15u), g = lane >> 4;
    const uint32_t at = t * 64u + g * 16u + m * 4u;
    const unsigned char* src = p.queries + (size_t)slot * p.dim;
    uint32_t w = 0;
    if (slot < p.nq) {
#pragma unroll
        for (uint32_t b = 0; b < 4; b++)
            if (at + b < p.dim) w |= (uint32_t)src[at + b] << (8u * b);
    }
    u32x4 out;
    out.x = 0x22222222u | ((w & 0x11111111u) << 3);
    out.y = 0x22222222u | (((w >> 1) & 0x11111111u) << 3);
    out.z = 0x22222222u | (((w >> 2) & 0x11111111u) << 3);
    out.w = 0x22222222u | (((w >> 3) & 0x11111111u) << 3);
    reinterpret_cast<u32x4*>(a.prepared)[i] = out;
    if (t == 0 && m == 0 && g == 0) {
        uint32_t bits = 0;
        if (slot < p.nq)
            for (uint32_t b = 0; b < p.dim; b++) bits += __builtin_popcount((uint32_t)src[b]);
        a.starts[slot] = (float)bits;  // exact: at most 4096
    }
}

extern __shared__ __align__(16) unsigned char ham_mfma_smem[];

// A block's LDS: the staged queries and the starts beside the selection's part (hamming_select.h: offer, settle, load_chunk).
struct MfmaLds : SelectLds {
    const u32x4* qs;
    float* start;
};

template <int NC>
HAM_KERNEL __launch_bounds__(NT) void hamming_mfma_kernel(const HammingMfmaParams a) {
    constexpr uint32_t QT = (uint32_t)NC * 16u;
    const HammingParams& p = a.p;
    const uint32_t tid = threadIdx.x, slice = blockIdx.x, tile = blockIdx.y, q0 = tile * QT;
    const uint32_t qn = p.nq - q0 < QT ? p.nq - q0 : QT;
    const uint32_t items = a.chunks * 4u * (uint32_t)NC * 64u;

    u32x4* staged = reinterpret_cast<u32x4*>(ham_mfma_smem);
    MfmaLds t;
    t.qs = staged;
    t.sort = reinterpret_cast<uint64_t*>(staged + items);
    t.thr = t.sort + p.buf;
    t.start = reinterpret_cast<float*>(t.thr + QT);
    t.cnt = reinterpret_cast<uint32_t*>(t.start + QT);
    t.flag = t.cnt + QT;
    {
        const u32x4* src = reinterpret_cast<const u32x4*>(a.prepared) + (size_t)tile * items;
        for (uint32_t i = tid; i < items; i += NT) staged[i] = src[i];
        if (tid < QT) {
            t.thr[tid] = kPadComposite;
            t.start[tid] = a.starts[q0 + tid];
            t.cnt[tid] = 0;
        }
        if (tid == 0) t.flag[0] = 0;
        __syncthreads();
    }

    const uint32_t lane = tid & 63u, wave = tid >> 6, r16 = lane & 15u, g = lane >> 4;
    const u32x4 tail = step_mask(p.V - 1u, p.dim);
    const uint64_t lo = (uint64_t)slice * p.slice_rows;
    const uint64_t hi = lo + p.slice_rows < p.n ? lo + p.slice_rows : p.n;
    uint64_t* cand = a.cand + ((size_t)slice * a.tiles + tile) * QT * p.buf;

    for (uint64_t base = lo; base < hi; base += kHamStepRows) {
        const uint64_t wrow = base + (uint64_t)wave * kHamMfmaWaveRows;
        if (wrow < hi) {  // (wave-uniform)
            v4f acc[F][NC];
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const float s = t.start[c * 16 + (int)r16];
#pragma unroll
                for (int f = 0; f < F; f++) acc[f][c] = v4f{s, s, s, s};
            }
            uint32_t cur[F][4], nxt[F][4];
            load_chunk(cur, p, wrow + r16, hi, 0u, g, tail);
#pragma unroll 1
            for (uint32_t ch = 0; ch < a.chunks; ch++) {
                if (ch + 1u < a.chunks) load_chunk(nxt, p, wrow + r16, hi, ch + 1u, g, tail);  // in flight under this chunk's MFMAs
                const u32x4* bq = t.qs + (size_t)ch * 4u * NC * 64u + lane;
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
            // element i of acc[f][c]: row 16 f + 4 g + i of the wave's rows against query 16 c + r16 of the tile
#pragma unroll
            // A threshold moves only in settle, so its distance part is read once per query: the least of the lane's 16 distances
            // to the query decides in one comparison whether any of them can enter (after the first iterations, hardly ever).
            for (int c = 0; c < NC; c++) {
                const uint32_t q = (uint32_t)c * 16u + r16;
                const float bound = q < qn ? (float)(uint32_t)(t.thr[q] >> 32) : -1.0f;  // (kPadComposite: 2^32, above every distance)
                float least = acc[0][c][0];
#pragma unroll
                for (int f = 0; f < F; f++)
#pragma unroll
                    for (int i = 0; i < 4; i++) least = __builtin_fminf(least, acc[f][c][i]);
                if (least <= bound) {
#pragma unroll
                    for (int f = 0; f < F; f++)
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const uint64_t r = wrow + (uint64_t)(f * 16 + i) + g * 4u;
                            if (r < hi && acc[f][c][i] <= bound) offer(t, p, cand, q, (uint32_t)acc[f][c][i], (uint32_t)r);
                        }
                }
            }
        }
        settle<NT>(t, p, cand, qn, false);
    }
    settle<NT>(t, p, cand, qn, true);
    store_lists<NT>(cand, t.cnt, p, q0, qn, slice);
}

}  // namespace

hipError_t hamming_prepare_launch(const HammingMfmaParams& a, hipStream_t s) {
    HammingMfmaParams arg = a;
    void* args[] = {&arg};
    const uint32_t items = a.tiles * a.p.query_tile * a.chunks * 16u;
    if (items == 0) return hipSuccess;
    return hipLaunchKernel(reinterpret_cast<const void*>(&hamming_prepare_kernel), dim3((items + 255u) / 256u), dim3(256), args, 0, s);
}

hipError_t hamming_mfma_launch(const HammingMfmaForm& f, const HammingMfmaParams& a, hipStream_t s, hipEvent_t* marks) {
    if (a.p.nq == 0) return hipSuccess;
    HammingMfmaParams arg = a;
    void* args[] = {&arg};
    auto mark = [&](int i) { return marks ? hipEventRecord(marks[i], s) : hipSuccess; };
    if (const hipError_t e = mark(0)) return e;
    if (f.row_slices) {
        const void* fn = f.query_tile == 128u ? reinterpret_cast<const void*>(&hamming_mfma_kernel<8>)
                       : f.query_tile == 64u ? reinterpret_cast<const void*>(&hamming_mfma_kernel<4>) : nullptr;
        if (!fn || f.lds_bytes > 160u * 1024u || (uint64_t)f.row_slices * f.kcap > kHamMergeMax || f.scratch_bytes > kHamMfmaScratch)
            return hipErrorInvalidValue;
        if (const hipError_t e = hamming_prepare_launch(a, s)) return e;  // HQ
        // H2
        if (f.lds_bytes > 48u * 1024u) {
            const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.lds_bytes);
            if (e != hipSuccess) return e;
        }
        if (const hipError_t e = hipLaunchKernel(fn, dim3(f.row_slices, f.tiles), dim3(f.threads), args, f.lds_bytes, s)) return e;
    }
    if (const hipError_t e = mark(1)) return e;
    if (const hipError_t e = hamming_merge_launch(a.p, s)) return e;  // H1
    return mark(2);
}

}  // namespace mvf
