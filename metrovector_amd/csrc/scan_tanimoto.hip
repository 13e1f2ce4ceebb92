// scan_tanimoto.hip — TQ and T2, the Tanimoto search: UInt8 queries against bit-packed UInt8 rows, ordered by Jaccard similarity,
// on the FP4 matrix unit (scan_tanimoto.h; DESIGN.md §5 "TQ / T2").
//
// With a = popcount(q), b = popcount(x), c = popcount(q & x) and u = a + b - c,  T(q, x) = c / u  (0 where u = 0).  c is an
// integer GEMM of 0/1 values against 0/1 values, exact in FP4 (E2M1: 0x0, 0x2) and in f32 accumulators in any order (c <= 4096);
// b is the same GEMM against a query of all ones.  v_mfma_scale_f32_16x16x128_f8f6f4 with both operands FP4 and both scales 2^0
// multiplies 16 rows x 16 queries x 128 bits.
//
// Operands: H2's (scan_hamming_mfma.hip, "Operands"), rows and queries.  A lane loads the 16 bytes at offset 64 t + 16 g of its
// row and step m of chunk t takes the lane's word m through fp4_row_operand; TQ writes the queries' side in the same bit order --
// ((w >> j) & 0x11111111) << 1: 1.0 where the bit is set, 0 elsewhere -- as [tile][chunk][step][query column tile][lane] x 16
// bytes, and a = popcount(q) as f32.  Bits behind `dimension` and query slots behind the window's last are zeros.
//
// T2, grid (row slices x query tiles), 256 threads: the tile's prepared queries stay in LDS for the whole slice; a wave owns 64
// rows (four A fragments) of the block's 256 per iteration against all QT = 16 NC queries, accumulators started at 0.  Per
// (step, A fragment) one more MFMA multiplies the fragment by the constant B operand 0x22222222 x 4 -- every query column all
// ones, no LDS read: its accumulator holds b of the lane's four rows in the very C layout the c accumulators use, so the row
// popcount takes no cross-lane reduction and no per-handle array.
//
// Selection.  key = kTaniBias - bits(T) with T the correctly rounded f32 quotient (include/mvf_gpu_tanimoto.h: strictly monotone
// and injective on the exact rationals), smaller is better, so offer / settle / store_lists (hamming_select.h) carry "largest T
// first, ties by ascending position" unchanged and H1 turns the keys back (HammingParams::float_key).  In front of the division a
// pair is tested against the query's k-th best kept as the pair (c_t, u_t): it can enter only if c u_t >= c_t u -- both
// products at most 2^24, exact in u32.  The pair is refreshed behind settle from the threshold's own row (refresh_pairs); an
// unset threshold is the pair (0, 1), which admits everything.

#include "scan_tanimoto.h"

#include "bitonic.h"
#include "hamming_select.h"

namespace mvf {
namespace {

constexpr int NT = (int)kTaniThreads;
constexpr int F = (int)kTaniWaveRows / 16;  // A fragments of a wave
constexpr uint32_t kU24 = 0xFFFFFFu;        // c and u are at most 4096: the mask tells the compiler, which then multiplies in 24 bits

// the word at byte `at` of a query of `dim` bytes, zeros behind its end (queries are not aligned)
__device__ __forceinline__ uint32_t query_word(const unsigned char* q, uint32_t at, uint32_t dim) {
    uint32_t w = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; b++)
        if (at + b < dim) w |= (uint32_t)q[at + b] << (8u * b);
    return w;
}

// TQ: one thread per 16-byte item of the prepared queries; the first item of a query also counts its bits.  Queries behind
// the window's last fill their tile as all-zero queries: nothing T2 stages is unwritten.
HAM_KERNEL __launch_bounds__(256) void tanimoto_prepare_kernel(const TanimotoParams a) {
    const HammingParams& p = a.p;
    const uint32_t QT = p.query_tile, NC = QT / 16u;
    const uint32_t per_tile = a.chunks * 4u * NC * 64u;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.tiles * per_tile) return;
    const uint32_t tile = i / per_tile, r = i % per_tile;
    const uint32_t lane = r % 64u, c = (r / 64u) % NC, m = (r / (64u * NC)) % 4u, t = r / (256u * NC);
    const uint32_t slot = tile * QT + c * 16u + (lane & 15u), g = lane >> 4;
    const unsigned char* src = p.queries + (size_t)slot * p.dim;
    const uint32_t w = slot < p.nq ? query_word(src, t * 64u + g * 16u + m * 4u, p.dim) : 0u;
    u32x4 out;
    out.x = (w & 0x11111111u) << 1;
    out.y = ((w >> 1) & 0x11111111u) << 1;
    out.z = ((w >> 2) & 0x11111111u) << 1;
    out.w = ((w >> 3) & 0x11111111u) << 1;
    reinterpret_cast<u32x4*>(a.prepared)[i] = out;
    if (t == 0 && m == 0 && g == 0) {
        uint32_t bits = 0;
        if (slot < p.nq)
            for (uint32_t b = 0; b < p.dim; b++) bits += __builtin_popcount((uint32_t)src[b]);
        a.pops[slot] = (float)bits;  // exact: at most 4096
    }
}

extern __shared__ __align__(16) unsigned char tani_smem[];

// A block's LDS: the staged queries, their popcounts and their thresholds as pairs beside the selection's part
// (hamming_select.h: offer, settle, load_chunk).
struct TaniLds : SelectLds {
    const u32x4* qs;
    uint64_t* seen;      // the threshold composite (ct, ut) belong to
    uint32_t *ct, *ut;   // c and u of the query's k-th best; (0, 1) while the threshold is unset
    float* pop;          // a
};

// Behind settle: the pairs of the queries whose threshold moved, recomputed from the threshold's row -- a thread per word of
// (query, row), summed in LDS.  Block-uniform; hardly ever entered once the thresholds stand.
__device__ __forceinline__ void refresh_pairs(const TaniLds& t, const HammingParams& p, uint32_t q0, uint32_t qn) {
    const uint32_t tid = threadIdx.x;
    const bool moved = tid < qn && t.thr[tid] != t.seen[tid];
    if (moved) t.flag[1] = 1u;
    __syncthreads();
    if (!t.flag[1]) return;
    if (moved) t.ct[tid] = 0u, t.ut[tid] = 0u;
    __syncthreads();
    if (tid == 0) t.flag[1] = 0u;  // (read by everyone in front of the barrier)
    const uint32_t W = p.V * 4u;
    for (uint32_t i = tid; i < qn * W; i += NT) {
        const uint32_t q = i / W, wd = i % W;
        const uint64_t thr = t.thr[q];
        if (thr == t.seen[q]) continue;
        const uint32_t have = wd * 4u >= p.dim ? 0u : (p.dim - wd * 4u >= 4u ? 4u : p.dim - wd * 4u);
        if (have == 0u) continue;
        const uint32_t mask = have == 4u ? 0xFFFFFFFFu : ((1u << (8u * have)) - 1u);
        const uint32_t x = reinterpret_cast<const uint32_t*>(p.rows + (uint64_t)(uint32_t)thr * p.pitch)[wd] & mask;
        const uint32_t w = query_word(p.queries + (size_t)(q0 + q) * p.dim, wd * 4u, p.dim);
        __hip_atomic_fetch_add(&t.ct[q], (uint32_t)__builtin_popcount(x & w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&t.ut[q], (uint32_t)__builtin_popcount(x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    if (moved) {
        t.ut[tid] = (uint32_t)t.pop[tid] + t.ut[tid] - t.ct[tid];  // u = a + b - c
        t.seen[tid] = t.thr[tid];
    }
    __syncthreads();
}

template <int NC>
HAM_KERNEL __launch_bounds__(NT) void tanimoto_scan_kernel(const TanimotoParams a) {
    constexpr uint32_t QT = (uint32_t)NC * 16u;
    const HammingParams& p = a.p;
    const uint32_t tid = threadIdx.x, slice = blockIdx.x, tile = blockIdx.y, q0 = tile * QT;
    const uint32_t qn = p.nq - q0 < QT ? p.nq - q0 : QT;
    const uint32_t items = a.chunks * 4u * (uint32_t)NC * 64u;

    u32x4* staged = reinterpret_cast<u32x4*>(tani_smem);
    TaniLds t;
    t.qs = staged;
    t.sort = reinterpret_cast<uint64_t*>(staged + items);
    t.thr = t.sort + p.buf;
    t.seen = t.thr + QT;
    t.ct = reinterpret_cast<uint32_t*>(t.seen + QT);
    t.ut = t.ct + QT;
    t.pop = reinterpret_cast<float*>(t.ut + QT);
    t.cnt = reinterpret_cast<uint32_t*>(t.pop + QT);
    t.flag = t.cnt + QT;
    {
        const u32x4* src = reinterpret_cast<const u32x4*>(a.prepared) + (size_t)tile * items;
        for (uint32_t i = tid; i < items; i += NT) staged[i] = src[i];
        if (tid < QT) {
            t.thr[tid] = kPadComposite;
            t.seen[tid] = kPadComposite;
            t.ct[tid] = 0u, t.ut[tid] = 1u;
            t.pop[tid] = a.pops[q0 + tid];
            t.cnt[tid] = 0;
        }
        if (tid == 0) t.flag[0] = 0, t.flag[1] = 0;
        __syncthreads();
    }

    const uint32_t lane = tid & 63u, wave = tid >> 6, r16 = lane & 15u, g = lane >> 4;
    const u32x4 tail = step_mask(p.V - 1u, p.dim);
    const uint64_t lo = (uint64_t)slice * p.slice_rows;
    const uint64_t hi = lo + p.slice_rows < p.n ? lo + p.slice_rows : p.n;
    uint64_t* cand = a.cand + ((size_t)slice * a.tiles + tile) * QT * p.buf;
    const v8i ones = v8i{0x22222222, 0x22222222, 0x22222222, 0x22222222, 0, 0, 0, 0};  // B: 1.0 in every query column

    for (uint64_t base = lo; base < hi; base += kHamStepRows) {
        const uint64_t wrow = base + (uint64_t)wave * kTaniWaveRows;
        if (wrow < hi) {  // (wave-uniform)
            v4f acc[F][NC], rowpop[F];
#pragma unroll
            for (int f = 0; f < F; f++) {
                rowpop[f] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int c = 0; c < NC; c++) acc[f][c] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
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
                    for (int f = 0; f < F; f++) {
                        av[f] = fp4_row_operand(cur[f][m]);
                        rowpop[f] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av[f], ones, rowpop[f], 4, 4, 0, 127, 0, 127);
                    }
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
            // element i of acc[f][c]: c of row 16 f + 4 g + i of the wave's rows against query 16 c + r16 of the tile; element i of
            // rowpop[f]: b of that row (the same in every column).  A threshold moves only in settle, so its pair is read once
            // per query; only the pairs that pass the test without division are divided and offered.
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const uint32_t q = (uint32_t)c * 16u + r16;
                if (q >= qn) continue;
                const uint32_t ct = t.ct[q] & kU24, ut = t.ut[q] & kU24;
                const float ab = t.pop[q];
                uint32_t pass = 0;
#pragma unroll
                for (int f = 0; f < F; f++)
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const uint32_t cc = (uint32_t)acc[f][c][i], u = (uint32_t)(ab + rowpop[f][i] - acc[f][c][i]);  // exact, <= 4096
                        pass |= ((cc & kU24) * ut >= ct * (u & kU24) ? 1u : 0u) << (f * 4 + i);  // 24-bit factors: one full-rate multiply each
                    }
                if (pass) {
#pragma unroll
                    for (int f = 0; f < F; f++)
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const uint64_t r = wrow + (uint64_t)(f * 16 + i) + g * 4u;
                            if (r < hi && ((pass >> (f * 4 + i)) & 1u)) {
                                const float u = ab + rowpop[f][i] - acc[f][c][i];
                                const float score = u > 0.0f ? __fdiv_rn(acc[f][c][i], u) : 0.0f;
                                offer(t, p, cand, q, (uint32_t)kTaniBias - __float_as_uint(score), (uint32_t)r);
                            }
                        }
                }
            }
        }
        settle<NT>(t, p, cand, qn, false);
        refresh_pairs(t, p, q0, qn);
    }
    settle<NT>(t, p, cand, qn, true);
    store_lists<NT>(cand, t.cnt, p, q0, qn, slice);
}

const void* scan_kernel(uint32_t query_tile) {
    switch (query_tile) {
        case 16: return reinterpret_cast<const void*>(&tanimoto_scan_kernel<1>);
        case 32: return reinterpret_cast<const void*>(&tanimoto_scan_kernel<2>);
        case 64: return reinterpret_cast<const void*>(&tanimoto_scan_kernel<4>);
        case 128: return reinterpret_cast<const void*>(&tanimoto_scan_kernel<8>);
        default: return nullptr;
    }
}

}  // namespace

hipError_t tanimoto_launch(const TanimotoForm& f, const TanimotoParams& a, hipStream_t s, hipEvent_t* marks) {
    if (a.p.nq == 0) return hipSuccess;
    TanimotoParams arg = a;
    void* args[] = {&arg};
    auto mark = [&](int i) { return marks ? hipEventRecord(marks[i], s) : hipSuccess; };
    if (const hipError_t e = mark(0)) return e;
    const void* fn = scan_kernel(f.query_tile);
    if (f.row_slices && (!fn || f.lds_bytes > kTaniLds || (uint64_t)f.row_slices * f.kcap > kHamMergeMax || f.scratch_bytes > kHamMfmaScratch))
        return hipErrorInvalidValue;
    if (f.row_slices) {  // TQ
        const uint32_t items = f.tiles * f.query_tile * (tani_query_bytes(f.chunks) / 16u);
        const void* qfn = reinterpret_cast<const void*>(&tanimoto_prepare_kernel);
        if (const hipError_t e = hipLaunchKernel(qfn, dim3((items + 255u) / 256u), dim3(256), args, 0, s)) return e;
    }
    if (const hipError_t e = mark(1)) return e;
    if (f.row_slices) {  // T2
        if (f.lds_bytes > 48u * 1024u) {
            const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.lds_bytes);
            if (e != hipSuccess) return e;
        }
        if (const hipError_t e = hipLaunchKernel(fn, dim3(f.row_slices, f.tiles), dim3(kTaniThreads), args, f.lds_bytes, s)) return e;
    }
    if (const hipError_t e = mark(2)) return e;
    if (const hipError_t e = hamming_merge_launch(a.p, s)) return e;  // H1
    return mark(3);
}

}  // namespace mvf
