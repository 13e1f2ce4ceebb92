// scan_signbits.hip — SQ and S2, the sign-bit search: Int8 queries against bit-packed UInt8 rows on the int8 matrix unit
// (scan_signbits.h; DESIGN.md §5 "SQ / S2").
//
// Element e = 8 i + b of a row x is bit b of its byte i, and  s(q, x) = sum_e q[e] * (x_e ? +1 : -1) = 2 t - sum(q)  with
// t = sum over the set bits of q[e]: an integer GEMM of 0/1 values against int8 whose i32 sums are exact in any order.
// v_mfma_i32_16x16x64_i8 multiplies 16 rows x 16 queries x 64 elements; 2 t - sum(q) is one integer operation per (row, query)
// behind it.  (2 q is not staged: it leaves int8.)
//
// Operands.  Lane l of a wave serves index l % 16 (a row of the A fragment, a query of the B fragment) and k-group g = l / 16 on
// both sides, and holds 16 int8 -- four VGPRs -- of its k-group.  The order of the elements inside an instruction is free as long
// as rows and queries share it; the one chosen makes the rows' side cheapest and keeps the rows out of LDS:
//   a lane loads the 16 bytes at offset 64 t + 16 g of its row (a wave reads whole 64-byte lines of 16 rows), and word m = 0 .. 3
//   of them, w, expands to eight VGPRs: register j = (w >> j) & 0x01010101, bit j of each of the word's four bytes as an int8
//   0/1.  Registers 0 .. 3 are the A operand of one MFMA (half h = 0), registers 4 .. 7 of a second (h = 1).
// SQ writes the queries' side in the same order: for MFMA (chunk t, word m, half h) lane (column c16, group g) gets register jj
// holding the four int8 q[8 (64 t + 16 g + 4 m + n) + 4 h + jj], n = 0 .. 3 -- as [tile][chunk][m][h][column tile][lane] x 16
// bytes, the order in which S2's lanes read B fragments: a block stages its tile with straight 16-byte copies and a wave's
// ds_read_b128 of one fragment covers 1 KiB without a bank conflict.  Elements behind `dimension` and query slots behind the
// window's last are zeros on the queries' side; bits behind `dimension` are zeros on the rows'.
//
// S2, grid (row slices x query tiles), 256 threads: the tile's prepared queries stay in LDS for the whole slice; a wave owns 64
// rows (four A fragments) of the block's 256 per iteration against all QT = 16 NC queries, i32 accumulators started at 0; the
// chunk loop is outermost, so an expanded A operand is used NC times and a B fragment four times, and the next chunk's 16 bytes
// are in flight under this chunk's MFMAs.  Behind it a lane holds four rows' t to one query per column tile and offers
// key = kSignBias - s as H2 offers its distances (hamming_select.h): smaller is better, so H0's exact "below the threshold" rule
// carries "largest s first, ties by ascending position"; H1 turns the keys back (HammingParams::score_bias).

#include "scan_signbits.h"

#include "bitonic.h"
#include "hamming_select.h"

namespace mvf {
namespace {

constexpr int NT = (int)kSignThreads;
constexpr int F = (int)kSignWaveRows / 16;  // A fragments of a wave

typedef int v4i __attribute__((ext_vector_type(4)));

// SQ: one thread per 16-byte item of the prepared queries; the first item of a query also sums its elements.
HAM_KERNEL __launch_bounds__(256) void signbits_prepare_kernel(const SignbitsParams a) {
    const HammingParams& p = a.p;
    const uint32_t QT = p.query_tile, NC = QT / 16u;
    const uint32_t per_tile = a.chunks * 8u * NC * 64u;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.tiles * per_tile) return;
    const uint32_t tile = i / per_tile, r = i % per_tile;
    const uint32_t lane = r % 64u, c = (r / 64u) % NC, h = (r / (64u * NC)) % 2u, m = (r / (128u * NC)) % 4u, t = r / (512u * NC);
    const uint32_t slot = tile * QT + c * 16u + (lane & 15u), g = lane >> 4;
    const uint32_t at = t * 64u + g * 16u + m * 4u;  // the row byte whose bits register byte 0 meets
    const signed char* src = reinterpret_cast<const signed char*>(p.queries) + (size_t)slot * p.dim * 8u;
    uint32_t out[4] = {0, 0, 0, 0};
    if (slot < p.nq) {
#pragma unroll
        for (uint32_t n = 0; n < 4; n++)
            if (at + n < p.dim) {
#pragma unroll
                for (uint32_t jj = 0; jj < 4; jj++) out[jj] |= (uint32_t)(unsigned char)src[8u * (at + n) + 4u * h + jj] << (8u * n);
            }
    }
    reinterpret_cast<u32x4*>(a.prepared)[i] = u32x4{out[0], out[1], out[2], out[3]};
    if (t == 0 && m == 0 && h == 0 && g == 0) {
        int32_t sum = 0;
        if (slot < p.nq)
            for (uint32_t e = 0; e < p.dim * 8u; e++) sum += (int32_t)src[e];
        a.sums[slot] = sum;
    }
}

extern __shared__ __align__(16) unsigned char sign_smem[];

// A block's LDS: the staged queries and their sums beside the selection's part (hamming_select.h: offer, settle, load_chunk).
struct SignLds : SelectLds {
    const u32x4* qs;
    int32_t* sum;
};

template <int NC>
HAM_KERNEL __launch_bounds__(NT) void signbits_scan_kernel(const SignbitsParams a) {
    constexpr uint32_t QT = (uint32_t)NC * 16u;
    const HammingParams& p = a.p;
    const uint32_t tid = threadIdx.x, slice = blockIdx.x, tile = blockIdx.y, q0 = tile * QT;
    const uint32_t qn = p.nq - q0 < QT ? p.nq - q0 : QT;
    const uint32_t items = a.chunks * 8u * (uint32_t)NC * 64u;

    u32x4* staged = reinterpret_cast<u32x4*>(sign_smem);
    SignLds t;
    t.qs = staged;
    t.sort = reinterpret_cast<uint64_t*>(staged + items);
    t.thr = t.sort + p.buf;
    t.sum = reinterpret_cast<int32_t*>(t.thr + QT);
    t.cnt = reinterpret_cast<uint32_t*>(t.sum + QT);
    t.flag = t.cnt + QT;
    {
        const u32x4* src = reinterpret_cast<const u32x4*>(a.prepared) + (size_t)tile * items;
        for (uint32_t i = tid; i < items; i += NT) staged[i] = src[i];
        if (tid < QT) {
            t.thr[tid] = kPadComposite;
            t.sum[tid] = a.sums[q0 + tid];
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
        const uint64_t wrow = base + (uint64_t)wave * kSignWaveRows;
        if (wrow < hi) {  // (wave-uniform)
            v4i acc[F][NC];
#pragma unroll
            for (int f = 0; f < F; f++)
#pragma unroll
                for (int c = 0; c < NC; c++) acc[f][c] = v4i{0, 0, 0, 0};
            uint32_t cur[F][4], nxt[F][4];
            load_chunk<F>(cur, p, wrow + r16, hi, 0u, g, tail);
#pragma unroll 1
            for (uint32_t ch = 0; ch < a.chunks; ch++) {
                if (ch + 1u < a.chunks) load_chunk<F>(nxt, p, wrow + r16, hi, ch + 1u, g, tail);  // in flight under this chunk's MFMAs
                const u32x4* bq = t.qs + (size_t)ch * 8u * NC * 64u + lane;
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    v4i av[F][2];
#pragma unroll
                    for (int f = 0; f < F; f++) {
                        const uint32_t w = cur[f][m];
                        av[f][0] = v4i{(int)(w & 0x01010101u), (int)((w >> 1) & 0x01010101u), (int)((w >> 2) & 0x01010101u),
                                       (int)((w >> 3) & 0x01010101u)};
                        av[f][1] = v4i{(int)((w >> 4) & 0x01010101u), (int)((w >> 5) & 0x01010101u), (int)((w >> 6) & 0x01010101u),
                                       (int)((w >> 7) & 0x01010101u)};
                    }
#pragma unroll
                    for (int h = 0; h < 2; h++)
#pragma unroll
                        for (int c = 0; c < NC; c++) {
                            const u32x4 b = bq[((m * 2 + h) * NC + c) * 64];
                            const v4i bv = v4i{(int)b.x, (int)b.y, (int)b.z, (int)b.w};
#pragma unroll
                            for (int f = 0; f < F; f++) acc[f][c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[f][h], bv, acc[f][c], 0, 0, 0);
                        }
                }
#pragma unroll
                for (int f = 0; f < F; f++)
#pragma unroll
                    for (int j = 0; j < 4; j++) cur[f][j] = nxt[f][j];
            }
            // element i of acc[f][c]: t of row 16 f + 4 g + i of the wave's rows against query 16 c + r16 of the tile.
            // A threshold moves only in settle, so its key part is read once per query: the largest of the lane's 16 sums decides
            // in one comparison whether any of them can enter (after the first iterations, hardly ever).
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const uint32_t q = (uint32_t)c * 16u + r16;
                if (q >= qn) continue;
                const uint32_t bound = (uint32_t)(t.thr[q] >> 32);  // (kPadComposite: 2^32 - 1, above every key)
                const int32_t bias = kSignBias + t.sum[q];           // key = kSignBias - (2 t - sum)
                int32_t most = acc[0][c][0];
#pragma unroll
                for (int f = 0; f < F; f++)
#pragma unroll
                    for (int i = 0; i < 4; i++) most = acc[f][c][i] > most ? acc[f][c][i] : most;
                if ((uint32_t)(bias - 2 * most) <= bound) {
#pragma unroll
                    for (int f = 0; f < F; f++)
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const uint64_t r = wrow + (uint64_t)(f * 16 + i) + g * 4u;
                            const uint32_t key = (uint32_t)(bias - 2 * acc[f][c][i]);
                            if (r < hi && key <= bound) offer(t, p, cand, q, key, (uint32_t)r);
                        }
                }
            }
        }
        settle<NT>(t, p, cand, qn, false);
    }
    settle<NT>(t, p, cand, qn, true);
    store_lists<NT>(cand, t.cnt, p, q0, qn, slice);
}

const void* scan_kernel(uint32_t query_tile) {
    switch (query_tile) {
        case 16: return reinterpret_cast<const void*>(&signbits_scan_kernel<1>);
        case 32: return reinterpret_cast<const void*>(&signbits_scan_kernel<2>);
        case 64: return reinterpret_cast<const void*>(&signbits_scan_kernel<4>);
        case 128: return reinterpret_cast<const void*>(&signbits_scan_kernel<8>);
        default: return nullptr;
    }
}

}  // namespace

hipError_t signbits_launch(const SignbitsForm& f, const SignbitsParams& a, hipStream_t s, hipEvent_t* marks) {
    if (a.p.nq == 0) return hipSuccess;
    SignbitsParams arg = a;
    void* args[] = {&arg};
    auto mark = [&](int i) { return marks ? hipEventRecord(marks[i], s) : hipSuccess; };
    if (const hipError_t e = mark(0)) return e;
    const void* fn = scan_kernel(f.query_tile);
    if (f.row_slices && (!fn || f.lds_bytes > kSignLds || (uint64_t)f.row_slices * f.kcap > kHamMergeMax || f.scratch_bytes > kHamMfmaScratch))
        return hipErrorInvalidValue;
    if (f.row_slices) {  // SQ
        const uint32_t items = f.tiles * f.query_tile * (sign_query_bytes(f.chunks) / 16u);
        const void* qfn = reinterpret_cast<const void*>(&signbits_prepare_kernel);
        if (const hipError_t e = hipLaunchKernel(qfn, dim3((items + 255u) / 256u), dim3(256), args, 0, s)) return e;
    }
    if (const hipError_t e = mark(1)) return e;
    if (f.row_slices) {  // S2
        if (f.lds_bytes > 48u * 1024u) {
            const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.lds_bytes);
            if (e != hipSuccess) return e;
        }
        if (const hipError_t e = hipLaunchKernel(fn, dim3(f.row_slices, f.tiles), dim3(kSignThreads), args, f.lds_bytes, s)) return e;
    }
    if (const hipError_t e = mark(2)) return e;
    if (const hipError_t e = hamming_merge_launch(a.p, s)) return e;  // H1
    return mark(3);
}

}  // namespace mvf
