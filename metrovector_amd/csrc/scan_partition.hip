// scan_partition.hip — the kernels of the partition index and of the partitioned search (partition.hip; DESIGN.md §3
// "Partitioned search", §5 "B0 / B1 / B2 / S1 — partitioned search").
//
// Build.  B0 lays the live rows' (key, local row) pairs down in ascending position: a count per block (and the OR / AND of the
// live keys, which tell the bits the keys differ in), F1's scan of the counts (scan_filter.hip), then the block compaction
// (mvf_common.h: block_compact_1024).  B1 is a stable LSD radix sort of the pairs by 8-bit digits of the 64-bit key -- the
// radix pass of radix_pass.h, the digit taken from the whole key and the row moved as its payload (every 64-bit value is a
// legal key here; sort_topk.hip's rank entries reserve two) -- which the host runs only for the digits the keys differ in.
// The pairs arrive in position order and the sort is stable, so the rows of a key stay in ascending position.  B2 flags the
// entries whose key differs from the one in front, compacts the flagged ones the same way and writes the key table.
//
// Search.  S1 is the gathered-row kernel (scan_gather.hip) for one query and one chunk per block: the block's list is a
// segment of rows_by_key, its query lies anywhere in the caller's buffer.  The same staging loop, K1's per-row arithmetic
// (k1_rowscore.h) with the handle's one-query lane group, four rows in flight per wave, the same sorted list out: K1's
// one-query bits.  Two small kernels move queries (the large tier's, made contiguous per key) and result rows (from the order
// they were computed in to the caller's, padding rows included).
//
// Algorithmic HBM bytes of S1: the segment's rows' pitch + 4 bytes per row, the query once per block.

#include "scan_partition.h"
#include "bitonic.h"
#include "k1_rowscore.h"
#include "mvf_common.h"
#include "radix_pass.h"
#include "scan_gather.h"

namespace mvf {
namespace {

__device__ __forceinline__ bool row_live(const uint32_t* tomb, uint64_t r) { return !tomb || !((tomb[r >> 5] >> (r & 31u)) & 1u); }
__device__ __forceinline__ uint64_t key_at(const void* values, bool is_u64, uint64_t r) {
    return is_u64 ? static_cast<const uint64_t*>(values)[r] : (uint64_t) static_cast<const uint32_t*>(values)[r];
}

// B0, count: grid (part_blocks(n)), block 1024
__global__ void __launch_bounds__(1024) part_count_kernel(const void* values, bool is_u64, uint64_t n, const uint32_t* tomb,
                                                          uint32_t* block_cnt, uint64_t* bits) {
    __shared__ uint32_t wsum[16];
    const uint32_t tid = threadIdx.x;
    const uint64_t r0 = (uint64_t)blockIdx.x * kPartBlockRows;
    uint32_t cnt = 0;
    uint64_t any = 0, all = ~0ull;
    for (uint32_t t0 = 0; t0 < kPartBlockRows; t0 += 1024u) {
        const uint64_t r = r0 + t0 + tid;
        if (r < n && row_live(tomb, r)) {
            const uint64_t key = key_at(values, is_u64, r);
            any |= key, all &= key;
            cnt++;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        any |= __shfl_xor(any, off, 64);
        all &= __shfl_xor(all, off, 64);
    }
    const bool wave_has_live = __builtin_amdgcn_ballot_w64(cnt != 0) != 0;
    if ((tid & 63u) == 0 && wave_has_live) {
        atomicOr(reinterpret_cast<unsigned long long*>(&bits[0]), (unsigned long long)any);
        atomicAnd(reinterpret_cast<unsigned long long*>(&bits[1]), (unsigned long long)all);
    }
    const uint32_t tot = block_sum_1024(cnt, wsum);
    if (tid == 0) block_cnt[blockIdx.x] = tot;
}

// B0, compact: grid (part_blocks(n)), block 1024
__global__ void __launch_bounds__(1024) part_compact_kernel(const void* values, bool is_u64, uint64_t n, const uint32_t* tomb,
                                                            const uint64_t* block_off, uint64_t* keys, uint32_t* rows) {
    __shared__ uint32_t wsum[16];
    const uint64_t r0 = (uint64_t)blockIdx.x * kPartBlockRows;
    block_compact_1024(
        r0, min(r0 + kPartBlockRows, n), block_off[blockIdx.x], wsum, [&](uint64_t r) { return row_live(tomb, r); },
        [&](uint64_t r, uint64_t slot) {
            keys[slot] = key_at(values, is_u64, r);
            rows[slot] = (uint32_t)r;
        });
}

// ---- B2: the key table.  grid (part_blocks(m)), block 1024
__device__ __forceinline__ bool is_head(const uint64_t* keys, uint64_t m, uint64_t i) { return i < m && (i == 0 || keys[i] != keys[i - 1]); }

__global__ void __launch_bounds__(1024) part_heads_count_kernel(const uint64_t* keys, uint64_t m, uint32_t* block_cnt) {
    __shared__ uint32_t wsum[16];
    const uint32_t tid = threadIdx.x;
    const uint64_t i0 = (uint64_t)blockIdx.x * kPartBlockRows;
    uint32_t cnt = 0;
    for (uint32_t t0 = 0; t0 < kPartBlockRows; t0 += 1024u) cnt += is_head(keys, m, i0 + t0 + tid) ? 1u : 0u;
    const uint32_t tot = block_sum_1024(cnt, wsum);
    if (tid == 0) block_cnt[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(1024) part_heads_write_kernel(const uint64_t* keys, uint64_t m, const uint64_t* block_off, uint64_t* table_keys,
                                                                uint64_t* table_off) {
    __shared__ uint32_t wsum[16];
    const uint64_t i0 = (uint64_t)blockIdx.x * kPartBlockRows, i1 = min(i0 + kPartBlockRows, m);
    const uint64_t heads = block_compact_1024(
        i0, i1, block_off[blockIdx.x], wsum, [&](uint64_t i) { return is_head(keys, m, i); },
        [&](uint64_t i, uint64_t slot) {
            table_keys[slot] = keys[i];
            table_off[slot] = i;
        });
    if (i1 == m && threadIdx.x == 0) table_off[heads] = m;  // the block of the last entry: `heads` counts every head, n_keys
}

// ---- S1.  grid (n small-tier queries), block 256; dynamic LDS kGatherChunk * 8 (composites) + kGatherChunk * 4 (rows) + 16
// (qq partials) + the padded query.
template <int DT, int METRIC, int G>
__global__ void __launch_bounds__(256) segment_score_kernel(SegmentScoreParams p) {
    using Tr = k1::Traits<DT>;
    using Acc = typename Tr::Acc;
    using QT = typename Tr::Q;
    constexpr int EPV = 16 / Tr::ES;
    constexpr int RPG = 64 / G;
    constexpr int U = 4;
    constexpr bool NEED_XX = k1::kNeedXX<DT, METRIC>;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* buf = reinterpret_cast<uint64_t*>(smem);                               // [kGatherChunk] composites
    uint32_t* rowbuf = reinterpret_cast<uint32_t*>(smem + kGatherChunk * 8);         // [kGatherChunk] the segment's rows
    Acc* red = reinterpret_cast<Acc*>(smem + kGatherChunk * 8 + kGatherChunk * 4);   // [4] qq partials
    unsigned char* qs = smem + kGatherChunk * 8 + kGatherChunk * 4 + 16;             // [J G vectors] the query
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane % G, rsel = lane / G;
    const PartQuery pq = p.plan[blockIdx.x];
    const uint32_t nr = min(pq.count, kGatherChunk);  // the plan sends longer segments to the large tier
    uint64_t* lout = p.lists + (size_t)blockIdx.x * p.kcap;

    // ---- the query: K1's staging loop (zero padded to J G vectors) and sum of squares (k1::stage_queries' lines); the rows
    const uint32_t VP = p.J * G;
    const QT* src = reinterpret_cast<const QT*>(p.queries) + (size_t)pq.query * p.dim;
    {
        Acc qq_part = 0;
        for (uint32_t e = tid; e < VP * EPV; e += 256) {
            const QT v = e < p.dim ? src[e] : (QT)0;
            reinterpret_cast<QT*>(qs)[e] = v;
            if constexpr (Tr::INT) qq_part += (int32_t)v * (int32_t)v;
            else qq_part = fmaf(v, v, qq_part);
        }
        const Acc s = k1::group_sum<64>(qq_part);
        if (lane == 0) red[wave] = s;
    }
    const uint32_t* list = p.rows_by_key + pq.offset;
    for (uint32_t i = tid; i < nr; i += 256) rowbuf[i] = list[i];
    __syncthreads();
    const Acc qq = red[0] + red[1] + red[2] + red[3];

    auto qload = [&](uint32_t v, int half) __attribute__((always_inline)) {  // float types: 4 query elements from LDS
        return *reinterpret_cast<const float4*>(qs + (size_t)v * (EPV * 4) + half * 16);
    };

    const uint32_t ngroups = (nr + RPG - 1) / RPG;
    for (uint32_t g0 = (uint32_t)wave * U; g0 < ngroups; g0 += 4 * U) {  // wave-uniform: every lane reaches the shuffles
        uint32_t idx[U];
        bool rv[U];
        const unsigned char* rp[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            idx[u] = (g0 + u) * RPG + rsel;
            rv[u] = idx[u] < nr;
            rp[u] = p.rows + (size_t)(rv[u] ? rowbuf[idx[u]] : 0u) * p.pitch;
        }
        Acc acc[U], xx[U];
#pragma unroll
        for (int u = 0; u < U; u++) acc[u] = 0, xx[u] = 0;
        for (uint32_t j = 0; j < p.J; j++) {
            const uint32_t v = j * G + sub;
            const bool vv = v < p.V;
            k1::u32x4 x[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                x[u] = k1::u32x4{0, 0, 0, 0};
                if (vv && rv[u]) x[u] = __builtin_nontemporal_load(reinterpret_cast<const k1::u32x4*>(rp[u] + (size_t)v * 16));
            }
            if constexpr (DT == MVF_DTYPE_FLOAT32) {
#pragma unroll
                for (int u = 0; u < U; u++)
                    if constexpr (NEED_XX) xx[u] = k1::xx4(xx[u], x[u]);
                const float4 qv = qload(v, 0);
#pragma unroll
                for (int u = 0; u < U; u++) acc[u] = k1::acc4<METRIC>(acc[u], qv, x[u]);
            } else if constexpr (DT == MVF_DTYPE_FLOAT16) {
#pragma unroll
                for (int u = 0; u < U; u++) {
                    float xf[8];
                    k1::widen_f16(x[u], xf);
                    if constexpr (NEED_XX) xx[u] = k1::xx8_f16(xx[u], xf);
                    const float4 qa = qload(v, 0), qb = qload(v, 1);
                    acc[u] = k1::acc8_f16<METRIC>(acc[u], qa, qb, xf);
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; u++)
                    if constexpr (NEED_XX) xx[u] = k1::dot16_int<DT == MVF_DTYPE_INT8>(xx[u], uint4{x[u].x, x[u].y, x[u].z, x[u].w}, x[u]);
                const uint4 qv = *reinterpret_cast<const uint4*>(qs + (size_t)v * 16);
#pragma unroll
                for (int u = 0; u < U; u++) acc[u] = k1::dot16_int<DT == MVF_DTYPE_INT8>(acc[u], qv, x[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            Acc xxs = 0;
            if constexpr (NEED_XX) xxs = k1::group_sum<G>(xx[u]);
            const uint32_t key = k1::make_key<DT, METRIC>(k1::group_sum<G>(acc[u]), xxs, qq);
            if (sub == 0 && rv[u]) buf[idx[u]] = ((uint64_t)key << 32) | rowbuf[idx[u]];
        }
    }
    // ---- the segment's best min(kcap, nr), sorted
    __syncthreads();
    const uint32_t P = next_pow2(nr < 2 ? 2u : nr);
    for (uint32_t i = nr + tid; i < P; i += 256) buf[i] = kPadComposite;
    __syncthreads();
    bitonic_sort_u64_reg<256, kGatherChunk / 256>(buf, P, tid);
    for (uint32_t i = tid; i < p.kcap; i += 256) lout[i] = i < nr ? buf[i] : kPadComposite;
}

template <int DT>
const void* pick_segment_kernel(int metric, int G) {
    return k1::for_metric(metric, [&](auto m) {
        return k1::for_group(G, [&](auto g) -> const void* {
            return reinterpret_cast<const void*>(&segment_score_kernel<DT, decltype(m)::value, decltype(g)::value>);
        });
    });
}

// grid (n), block 256
__global__ void __launch_bounds__(256) part_gather_queries_kernel(const unsigned char* queries, const PartQuery* plan, uint32_t qrow, bool words,
                                                                  unsigned char* dst) {
    const unsigned char* src = queries + (size_t)plan[blockIdx.x].query * qrow;
    unsigned char* out = dst + (size_t)blockIdx.x * qrow;
    if (words) {
        for (uint32_t i = threadIdx.x; i < qrow / 4; i += 256) reinterpret_cast<uint32_t*>(out)[i] = reinterpret_cast<const uint32_t*>(src)[i];
    } else {
        for (uint32_t i = threadIdx.x; i < qrow; i += 256) out[i] = src[i];
    }
}

// grid (nq), block 256
__global__ void __launch_bounds__(256) part_scatter_kernel(PartScatterParams p) {
    const uint32_t i = blockIdx.x;
    const size_t o = (size_t)p.plan[i].query * p.k;
    if (i < p.n_scored) {
        const size_t c = (size_t)i * p.k;
        for (uint32_t j = threadIdx.x; j < p.k; j += 256) {
            p.out_scores[o + j] = p.c_scores[c + j];
            p.out_indices[o + j] = p.c_indices[c + j];
            if (p.out_raw) p.out_raw[o + j] = p.c_raw[c + j];
        }
    } else {
        const float pad = pad_score(p.metric);
        for (uint32_t j = threadIdx.x; j < p.k; j += 256) {
            p.out_scores[o + j] = pad;
            p.out_indices[o + j] = ~0ull;
            if (p.out_raw) p.out_raw[o + j] = 0;
        }
    }
}

}  // namespace

hipError_t part_count_launch(const void* values, bool is_u64, uint64_t n, const uint32_t* tomb, uint32_t* block_cnt, uint64_t* bits,
                             hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(part_count_kernel, dim3(part_blocks(n)), dim3(1024), 0, s, values, is_u64, n, tomb, block_cnt, bits);
    return hipGetLastError();
}

hipError_t part_compact_launch(const void* values, bool is_u64, uint64_t n, const uint32_t* tomb, const uint64_t* block_off, uint64_t* keys,
                               uint32_t* rows, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(part_compact_kernel, dim3(part_blocks(n)), dim3(1024), 0, s, values, is_u64, n, tomb, block_off, keys, rows);
    return hipGetLastError();
}

hipError_t part_sort_pass_launch(const uint64_t* keys_in, const uint32_t* rows_in, uint64_t* keys_out, uint32_t* rows_out, uint64_t m, int shift,
                                 uint32_t* bh, uint32_t* tot, hipStream_t s) {
    if (m == 0) return hipSuccess;
    static_assert(kPartSortTile == kRsTile, "part_sort_tiles() counts the shared pass's tiles");
    const uint32_t NB = part_sort_tiles(m);  // one list: no batch, strides 0
    hipLaunchKernelGGL((rs_hist_kernel<8, RsKeyDigit>), dim3(NB), dim3(256), 0, s, keys_in, m, shift, bh, NB, 0, 0);
    hipLaunchKernelGGL(rs_scan_kernel, dim3(256), dim3(256), 0, s, bh, NB, tot, 0);
    hipLaunchKernelGGL((rs_scatter_kernel<8, true, RsKeyDigit, true>), dim3(NB), dim3(256), 0, s, keys_in, keys_out, rows_in, rows_out, m, shift, bh,
                       tot, NB, 0, 0);
    return hipGetLastError();
}

hipError_t part_heads_count_launch(const uint64_t* keys, uint64_t m, uint32_t* block_cnt, hipStream_t s) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(part_heads_count_kernel, dim3(part_blocks(m)), dim3(1024), 0, s, keys, m, block_cnt);
    return hipGetLastError();
}

hipError_t part_heads_write_launch(const uint64_t* keys, uint64_t m, const uint64_t* block_off, uint64_t* table_keys, uint64_t* table_off,
                                   hipStream_t s) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(part_heads_write_kernel, dim3(part_blocks(m)), dim3(1024), 0, s, keys, m, block_off, table_keys, table_off);
    return hipGetLastError();
}

hipError_t segment_score_launch(uint8_t dtype, int metric, int G, const SegmentScoreParams& p, hipStream_t s) {
    if (p.n == 0) return hipSuccess;
    const uint32_t qbytes = cand_query_bytes(dtype, G, p.J);
    if (qbytes > kCandQueryLdsMax) return hipErrorInvalidValue;  // the plan sends such queries to the large tier
    const void* fn = nullptr;
    switch (dtype) {
        case MVF_DTYPE_FLOAT32: fn = pick_segment_kernel<MVF_DTYPE_FLOAT32>(metric, G); break;
        case MVF_DTYPE_FLOAT16: fn = pick_segment_kernel<MVF_DTYPE_FLOAT16>(metric, G); break;
        case MVF_DTYPE_INT8: fn = pick_segment_kernel<MVF_DTYPE_INT8>(metric, G); break;
        case MVF_DTYPE_UINT8: fn = pick_segment_kernel<MVF_DTYPE_UINT8>(metric, G); break;
        default: break;
    }
    if (!fn) return hipErrorInvalidValue;
    const size_t lds = (size_t)kGatherChunk * 8u + kGatherChunk * 4u + 16u + qbytes;
    SegmentScoreParams arg = p;
    void* args[] = {&arg};
    return hipLaunchKernel(fn, dim3(p.n), dim3(256), args, lds, s);
}

hipError_t part_gather_queries_launch(const void* queries, const PartQuery* plan, uint32_t n, uint32_t qrow, void* dst, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const bool words = ((reinterpret_cast<uintptr_t>(queries) | reinterpret_cast<uintptr_t>(dst) | qrow) & 3u) == 0;
    hipLaunchKernelGGL(part_gather_queries_kernel, dim3(n), dim3(256), 0, s, static_cast<const unsigned char*>(queries), plan, qrow, words,
                       static_cast<unsigned char*>(dst));
    return hipGetLastError();
}

hipError_t part_scatter_launch(const PartScatterParams& p, hipStream_t s) {
    if (p.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(part_scatter_kernel, dim3(p.nq), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace mvf
