// scan_hamming_gather.hip — HG, the filtered Hamming search's list route on the matrix unit (scan_hamming_gather.h; DESIGN.md §5
// "HG"): H2's arithmetic (scan_hamming_mfma.hip, "Operands") over the rows an ascending list names, so that only admitted rows
// leave HBM.
//
// HG, grid (list slices x query tiles), 256 threads: the tile's prepared queries (HQ's, unchanged) and their starts stay in LDS
// for the whole slice.  One iteration takes 256 list entries; a wave owns 64 of them, four 16-row A fragments, against all QT
// queries.  Lane l first loads the four positions list[e0 + 16 f + l % 16], then per 64-byte chunk the 16 bytes at
// rows + pos * pitch + 64 ch + 16 (l / 16) of each: the four k-groups of a row still read one whole 64-byte line, but the 16
// rows of a fragment are wherever the list says.  The position-then-row load is a dependent pair H2 does not have, so two
// things stay in flight under a chunk's MFMAs: the next chunk's row bytes and the NEXT iteration's four positions.  Entries
// behind the slice's end carry the position "no row": a zero operand, never offered.
//
// Behind the chunks a lane holds four entries' distances to one query per tile (element i of acc[f][c]: entry 16 f + 4 g + i of
// the wave's); it offers what beats the query's threshold as H2 does, with the composite d << 32 | ROW POSITION -- read back
// from the list, which the cache still holds -- so ties go by position and H1 and the id mapping serve unchanged.  No
// tombstone is tested: the list holds admitted live rows only (p.tomb is NULL).

#include "scan_hamming_gather.h"

#include "bitonic.h"
#include "hamming_select.h"

namespace mvf {
namespace {

constexpr int NT = (int)kHamMfmaThreads;
constexpr int F = (int)kHamMfmaWaveRows / 16;  // A fragments of a wave
constexpr uint32_t kNoRow = 0xFFFFFFFFu;       // at or above every shard's row count: load_chunk gives zeros

extern __shared__ __align__(16) unsigned char ham_gather_smem[];

struct GatherLds : SelectLds {
    const u32x4* qs;
    float* start;
};

// the lane's four positions of the 64 entries at e0 (its own: e0 + 16 f + l % 16), kNoRow behind the slice's end
__device__ __forceinline__ void load_positions(uint32_t (&pos)[F], const uint32_t* list, uint32_t e, uint32_t hi) {
#pragma unroll
    for (int f = 0; f < F; f++) pos[f] = e + (uint32_t)(f * 16) < hi ? list[e + (uint32_t)(f * 16)] : kNoRow;
}

template <int NC>
HAM_KERNEL __launch_bounds__(NT) void hamming_gather_kernel(const HammingGatherParams gp) {
    constexpr uint32_t QT = (uint32_t)NC * 16u;
    const HammingMfmaParams& a = gp.a;
    const HammingParams& p = a.p;
    const uint32_t tid = threadIdx.x, slice = blockIdx.x, tile = blockIdx.y, q0 = tile * QT;
    const uint32_t qn = p.nq - q0 < QT ? p.nq - q0 : QT;
    const uint32_t items = a.chunks * 4u * (uint32_t)NC * 64u;

    u32x4* staged = reinterpret_cast<u32x4*>(ham_gather_smem);
    GatherLds t;
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
    const uint32_t lo = slice * gp.slice_entries;
    const uint32_t hi = gp.m - lo < gp.slice_entries ? gp.m : lo + gp.slice_entries;
    uint64_t* cand = a.cand + ((size_t)slice * a.tiles + tile) * QT * p.buf;

    uint32_t pos[F], npos[F];
    load_positions(pos, gp.list, lo + wave * kHamMfmaWaveRows + r16, hi);
    for (uint32_t base = lo; base < hi; base += kHamStepRows) {
        const uint32_t wbase = base + wave * kHamMfmaWaveRows;
        load_positions(npos, gp.list, wbase + kHamStepRows + r16, hi);  // in flight under this iteration's chunks
        if (wbase < hi) {  // (wave-uniform)
            v4f acc[F][NC];
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const float s = t.start[c * 16 + (int)r16];
#pragma unroll
                for (int f = 0; f < F; f++) acc[f][c] = v4f{s, s, s, s};
            }
            uint32_t cur[F][1][4], nxt[F][1][4];
#pragma unroll
            for (int f = 0; f < F; f++) load_chunk(cur[f], p, pos[f], p.n, 0u, g, tail);
#pragma unroll 1
            for (uint32_t ch = 0; ch < a.chunks; ch++) {
                if (ch + 1u < a.chunks) {  // in flight under this chunk's MFMAs
#pragma unroll
                    for (int f = 0; f < F; f++) load_chunk(nxt[f], p, pos[f], p.n, ch + 1u, g, tail);
                }
                const u32x4* bq = t.qs + (size_t)ch * 4u * NC * 64u + lane;
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    v8i av[F];
#pragma unroll
                    for (int f = 0; f < F; f++) av[f] = fp4_row_operand(cur[f][0][m]);
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
                    for (int j = 0; j < 4; j++) cur[f][0][j] = nxt[f][0][j];
            }
            // H2's pre-test: the least of the lane's 16 distances to the query decides whether any of them can enter
#pragma unroll
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
                            const uint32_t e = wbase + (uint32_t)(f * 16 + i) + g * 4u;
                            if (e < hi && acc[f][c][i] <= bound) offer(t, p, cand, q, (uint32_t)acc[f][c][i], gp.list[e]);
                        }
                }
            }
        }
        settle<NT>(t, p, cand, qn, false);
#pragma unroll
        for (int f = 0; f < F; f++) pos[f] = npos[f];
    }
    settle<NT>(t, p, cand, qn, true);
    store_lists<NT>(cand, t.cnt, p, q0, qn, slice);
}

}  // namespace

hipError_t hamming_gather_launch(const HammingGatherForm& f, const HammingGatherParams& g, hipStream_t s, hipEvent_t* marks) {
    if (g.a.p.nq == 0) return hipSuccess;
    HammingGatherParams arg = g;
    void* args[] = {&arg};
    auto mark = [&](int i) { return marks ? hipEventRecord(marks[i], s) : hipSuccess; };
    const void* fn = f.query_tile == 128u ? reinterpret_cast<const void*>(&hamming_gather_kernel<8>)
                   : f.query_tile == 64u ? reinterpret_cast<const void*>(&hamming_gather_kernel<4>)
                   : f.query_tile == 32u ? reinterpret_cast<const void*>(&hamming_gather_kernel<2>)
                   : f.query_tile == 16u ? reinterpret_cast<const void*>(&hamming_gather_kernel<1>) : nullptr;
    if (!fn || !f.list_slices || !g.list || f.lds_bytes > 160u * 1024u || (uint64_t)f.list_slices * f.kcap > kHamMergeMax ||
        f.scratch_bytes > kHamMfmaScratch || (uint64_t)f.list_slices * f.slice_entries < g.m ||
        (uint64_t)(f.list_slices - 1u) * f.slice_entries >= g.m || g.slice_entries != f.slice_entries || g.a.p.tomb)
        return hipErrorInvalidValue;
    if (const hipError_t e = mark(0)) return e;
    if (const hipError_t e = hamming_prepare_launch(g.a, s)) return e;  // HQ
    if (const hipError_t e = mark(1)) return e;
    if (f.lds_bytes > 48u * 1024u) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.lds_bytes);
        if (e != hipSuccess) return e;
    }
    if (const hipError_t e = hipLaunchKernel(fn, dim3(f.list_slices, f.tiles), dim3(kHamMfmaThreads), args, f.lds_bytes, s)) return e;  // HG
    if (const hipError_t e = mark(2)) return e;
    if (const hipError_t e = hamming_merge_launch(g.a.p, s)) return e;  // H1
    return mark(3);
}

}  // namespace mvf
