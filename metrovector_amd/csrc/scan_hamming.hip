// scan_hamming.hip — H0 and H1, the Hamming search over bit-packed UInt8 rows (scan_hamming.h; DESIGN.md §5 "H0 / H1").
//
// H0, grid (row slices x query tiles), 256 threads.  A block stages its tile's queries in LDS as zero-padded u32 words,
// walks its slice of rows once and keeps, per query, an LDS buffer of composites (distance << 32 | local row) and the
// composite of the current k-th best as a threshold.  A row enters a query's buffer when its composite is below the
// threshold -- an exact comparison: a tie at the k-th distance enters only with a lower position -- and it is not deleted.
// Whenever a buffer could not take another iteration's rows, the block sorts it, cuts it to k and lowers the threshold.
//   register form   G = next_pow2(pitch / 16) <= 16 lanes per row, each with its 16-byte step in 4 VGPRs and U rows in
//                   flight; per query 4 x (v_xor_b32, v_bcnt_u32_b32 with the sum as its addend).
//   streaming form  G = 32 or 64 lanes walk a row in 16-byte steps, one i32 sum per query of the tile.
// Both combine a group's sums by the transposing butterfly: QB queries at a time, every step hands half of a lane's sums
// to its partner (ds_swizzle; the 32-lane step a ds_bpermute), so that lane j of the group ends with the row's distance to
// query j of the batch and tests and appends it itself.
// H1, one block of 1024 threads per query: the slices' sorted lists merged by sorting them in LDS, 16384 entries a round,
// and the results written.

#include "scan_hamming.h"

#include "bitonic.h"
#include "hamming_select.h"

namespace mvf {
namespace {

constexpr int NT = (int)kHamThreads;

template <int S>
__device__ __forceinline__ uint32_t lane_xor(uint32_t v) {
    if constexpr (S >= 32) return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((threadIdx.x & 63u) ^ (uint32_t)S) << 2), (int)v);
    else return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (S << 10) | 0x1F);  // bit mode: and 0x1F, or 0, xor S
}

// The sums acc[0 .. QB) of the G lanes of a group (G a power of two, QB <= G) -> in lane `sub` the group's total of
// acc[sub % QB].  Steps of QB lanes and more add whole arrays; below that a lane keeps the half of its sums its bit of
// `sub` names and receives the partner's part of them: G/QB-fold adds first, then QB - 1.
template <int G, int QB, int S>
__device__ __forceinline__ void butterfly_step(uint32_t (&acc)[QB], uint32_t sub) {
    if constexpr (S >= 1) {
        if constexpr (S < G && S >= QB) {
#pragma unroll
            for (int i = 0; i < QB; i++) acc[i] += lane_xor<S>(acc[i]);
        } else if constexpr (S < G) {
            const bool hi = (sub & (uint32_t)S) != 0;
#pragma unroll
            for (int i = 0; i < S; i++) {
                const uint32_t send = hi ? acc[i] : acc[i + S], keep = hi ? acc[i + S] : acc[i];
                acc[i] = keep + lane_xor<S>(send);
            }
        }
        butterfly_step<G, QB, S / 2>(acc, sub);
    }
}

__device__ __forceinline__ uint32_t xor_bits(const u32x4& a, const u32x4& b, uint32_t acc) {
    acc = __builtin_popcount(a.x ^ b.x) + acc;
    acc = __builtin_popcount(a.y ^ b.y) + acc;
    acc = __builtin_popcount(a.z ^ b.z) + acc;
    return __builtin_popcount(a.w ^ b.w) + acc;
}

// A block's LDS: the queries' buffers, thresholds, words, counts and the flag "a buffer is nearly full".
struct TileLds {
    uint64_t *bufs, *thr;
    uint32_t *qw, *cnt, *flag;
};
__device__ __forceinline__ TileLds tile_lds(unsigned char* smem, uint32_t QT, uint32_t B, uint32_t qwords) {
    TileLds t;
    t.bufs = reinterpret_cast<uint64_t*>(smem);
    t.thr = t.bufs + (size_t)QT * B;
    t.qw = reinterpret_cast<uint32_t*>(t.thr + (QT > 2u ? QT : 2u));
    t.cnt = t.qw + (size_t)QT * qwords;
    t.flag = t.cnt + QT;
    return t;
}

// The tile's queries as zero-padded words (qwords per query), the buffers empty, every threshold at "everything".
__device__ __forceinline__ void stage_tile(const TileLds& t, const HammingParams& p, uint32_t QT, uint32_t q0, uint32_t qn, uint32_t qwords) {
    for (uint32_t i = threadIdx.x; i < QT * qwords; i += NT) {
        const uint32_t q = i / qwords, at = (i % qwords) * 4u;
        uint32_t word = 0;
        if (q < qn) {
            const unsigned char* src = p.queries + (size_t)(q0 + q) * p.dim;
#pragma unroll
            for (uint32_t b = 0; b < 4; b++)
                if (at + b < p.dim) word |= (uint32_t)src[at + b] << (8u * b);
        }
        t.qw[i] = word;
    }
    if (threadIdx.x < QT) {
        t.thr[threadIdx.x] = kPadComposite;
        t.cnt[threadIdx.x] = 0;
    }
    if (threadIdx.x == 0) t.flag[0] = 0;
    __syncthreads();
}

// A live row whose composite beats the query's threshold joins its buffer.  The slot comes from an LDS counter: between two
// checks a buffer receives each row once at most, so it cannot run over; the order inside it is settled by the sort.
template <uint32_t STEP>
__device__ __forceinline__ void offer(const TileLds& t, const HammingParams& p, uint32_t q, uint32_t d, uint32_t r) {
    const uint64_t comp = ((uint64_t)d << 32) | r;
    if (comp < t.thr[q] && !(p.tomb && ((p.tomb[r >> 5] >> (r & 31u)) & 1u))) {
        const uint32_t slot = __hip_atomic_fetch_add(&t.cnt[q], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (slot < p.buf) t.bufs[(size_t)q * p.buf + slot] = comp;
        if (slot + 1u + STEP > p.buf) t.flag[0] = 1u;
    }
}

// Behind an iteration: every buffer that could not take STEP more entries (all of them at the end of the slice) is sorted,
// cut to k and its threshold lowered to its k-th composite.
template <uint32_t STEP>
__device__ __forceinline__ void settle(const TileLds& t, const HammingParams& p, uint32_t qn, bool last) {
    const int tid = (int)threadIdx.x;
    __syncthreads();
    const uint32_t full = t.flag[0];
    __syncthreads();
    if (!full && !last) return;
    for (uint32_t q = 0; q < qn; q++) {
        uint32_t c = t.cnt[q];
        if (!last && c + STEP <= p.buf) continue;
        c = c < p.buf ? c : p.buf;
        uint64_t* buf = t.bufs + (size_t)q * p.buf;
        const uint32_t keep = sort_cut<NT>(buf, c, p.k, tid);
        if (tid == 0) {
            t.cnt[q] = keep;
            t.thr[q] = keep >= p.k ? buf[p.k - 1u] : kPadComposite;
        }
    }
    if (tid == 0) t.flag[0] = 0;
    __syncthreads();
}

extern __shared__ __align__(16) unsigned char ham_smem[];

template <int G, int QB>
HAM_KERNEL __launch_bounds__(NT) void hamming_reg_kernel(const HammingParams p) {
    constexpr int U = G >= 4 ? 4 : G, RPP = NT / G;
    constexpr uint32_t STEP = (uint32_t)(RPP * U), QWORDS = (uint32_t)G * 4u;
    static_assert(STEP <= kHamStepRows, "hamming_form sizes a query's buffer for kHamStepRows rows between two checks");
    const uint32_t QT = p.query_tile, slice = blockIdx.x, q0 = blockIdx.y * QT;
    const uint32_t qn = p.nq - q0 < QT ? p.nq - q0 : QT;
    const TileLds t = tile_lds(ham_smem, QT, p.buf, QWORDS);
    stage_tile(t, p, QT, q0, qn, QWORDS);

    const uint32_t sub = threadIdx.x % G, grp = threadIdx.x / G;
    const bool holds = sub < p.V;             // lanes behind the row's last step hold zeros
    const u32x4 mask = step_mask(sub, p.dim);  // the pitch padding behind `dim` is never relied on
    const uint64_t lo = (uint64_t)slice * p.slice_rows;
    const uint64_t hi = lo + p.slice_rows < p.n ? lo + p.slice_rows : p.n;
    const u32x4* qsteps = reinterpret_cast<const u32x4*>(t.qw) + sub;

    for (uint64_t base = lo; base < hi; base += STEP) {
        u32x4 w[U];
        bool rv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t r = base + (uint64_t)(u * RPP) + grp;
            rv[u] = r < hi;
            w[u] = u32x4{0, 0, 0, 0};
            if (rv[u] && holds) w[u] = *(reinterpret_cast<const u32x4*>(p.rows + r * p.pitch) + sub);
            w[u].x &= mask.x, w[u].y &= mask.y, w[u].z &= mask.z, w[u].w &= mask.w;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t r = (uint32_t)(base + (uint64_t)(u * RPP) + grp);
#pragma unroll 1
            for (uint32_t qb = 0; qb < QT; qb += QB) {
                uint32_t acc[QB];
#pragma unroll
                for (int i = 0; i < QB; i++) acc[i] = xor_bits(w[u], qsteps[(size_t)(qb + i) * G], 0u);
                butterfly_step<G, QB, 32>(acc, sub);
                const uint32_t q = qb + (sub & (uint32_t)(QB - 1));
                if (sub < (uint32_t)QB && rv[u] && q < qn) offer<STEP>(t, p, q, acc[0], r);
            }
        }
        settle<STEP>(t, p, qn, false);
    }
    settle<STEP>(t, p, qn, true);
    store_lists<NT>(t.bufs, t.cnt, p, q0, qn, slice);
}

template <int G, int QT>
HAM_KERNEL __launch_bounds__(NT) void hamming_stream_kernel(const HammingParams p) {
    constexpr int RPP = NT / G;
    constexpr uint32_t STEP = kHamStepRows;
    static_assert(STEP % RPP == 0, "an iteration is whole passes");
    const uint32_t slice = blockIdx.x, q0 = blockIdx.y * QT;
    const uint32_t qn = p.nq - q0 < (uint32_t)QT ? p.nq - q0 : (uint32_t)QT;
    const uint32_t qwords = p.pitch / 4u;
    const TileLds t = tile_lds(ham_smem, QT, p.buf, qwords);
    stage_tile(t, p, QT, q0, qn, qwords);

    const uint32_t sub = threadIdx.x % G, grp = threadIdx.x / G;
    const u32x4 tail = step_mask(p.V - 1u, p.dim);
    const uint64_t lo = (uint64_t)slice * p.slice_rows;
    const uint64_t hi = lo + p.slice_rows < p.n ? lo + p.slice_rows : p.n;
    const u32x4* qsteps = reinterpret_cast<const u32x4*>(t.qw);

    for (uint64_t base = lo; base < hi; base += STEP) {
#pragma unroll 1
        for (uint32_t pass = 0; pass < STEP; pass += RPP) {
            const uint64_t r = base + pass + grp;
            const bool rv = r < hi;
            uint32_t acc[QT];  // 32-bit sums: a row holds up to 264 200 bits
#pragma unroll
            for (int i = 0; i < QT; i++) acc[i] = 0;
            if (rv) {
                const u32x4* row = reinterpret_cast<const u32x4*>(p.rows + r * p.pitch);
                for (uint32_t step = sub; step < p.V; step += G) {
                    u32x4 w = row[step];
                    if (step == p.V - 1u) w.x &= tail.x, w.y &= tail.y, w.z &= tail.z, w.w &= tail.w;
#pragma unroll
                    for (int i = 0; i < QT; i++) acc[i] = xor_bits(w, qsteps[(size_t)i * p.V + step], acc[i]);
                }
            }
            butterfly_step<G, QT, 32>(acc, sub);
            const uint32_t q = sub & (uint32_t)(QT - 1);
            if (sub < (uint32_t)QT && rv && q < qn) offer<STEP>(t, p, q, acc[0], (uint32_t)r);
        }
        settle<STEP>(t, p, qn, false);
    }
    settle<STEP>(t, p, qn, true);
    store_lists<NT>(t.bufs, t.cnt, p, q0, qn, slice);
}

// H1
HAM_KERNEL __launch_bounds__(1024) void hamming_merge_kernel(const HammingParams p) {
    uint64_t* buf = reinterpret_cast<uint64_t*>(ham_smem);
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t total = p.row_slices * p.kcap;
    const uint64_t* lists = p.lists + (size_t)q * total;
    uint32_t have = 0, at = 0;
    // The k best lie at or below every slice's own k-th composite, so at or below the smallest of those: where the entries up to
    // it fit the LDS (a few per slice on spread-out data), they alone are sorted, in one round.
    __shared__ uint64_t bound;
    __shared__ uint32_t kept;
    if (total > kHamMergeLds) {
        if (tid == 0) bound = kPadComposite, kept = 0;
        __syncthreads();
        uint64_t m = kPadComposite;
        for (uint32_t s = tid; s < p.row_slices; s += 1024u) {
            const uint64_t e = lists[(size_t)s * p.kcap + p.k - 1u];
            m = e < m ? e : m;
        }
        if (m != kPadComposite) __hip_atomic_fetch_min(&bound, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        const uint64_t b = bound;
        uint32_t mine = 0;
        for (uint32_t i = tid; i < total; i += 1024u) mine += lists[i] <= b && lists[i] != kPadComposite ? 1u : 0u;
        if (mine) __hip_atomic_fetch_add(&kept, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        const uint32_t n = kept;
        __syncthreads();
        if (n <= kHamMergeLds) {  // (block-uniform)
            if (tid == 0) kept = 0;
            __syncthreads();
            for (uint32_t i = tid; i < total; i += 1024u) {
                const uint64_t e = lists[i];
                if (e <= b && e != kPadComposite) buf[__hip_atomic_fetch_add(&kept, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)] = e;
            }
            const uint32_t P = n < 2u ? 2u : next_pow2(n);
            for (uint32_t i = n + tid; i < P; i += 1024u) buf[i] = kPadComposite;
            __syncthreads();
            bitonic_sort_u64_1024(buf, P, (int)tid);
            have = n < p.k ? n : p.k;
            at = total;
        }
    }
    for (; at < total;) {  // (block-uniform)
        const uint32_t take = total - at < kHamMergeLds - have ? total - at : kHamMergeLds - have;
        const uint32_t P = have + take < 2u ? 2u : next_pow2(have + take);
        for (uint32_t i = tid; i < take; i += 1024u) buf[have + i] = lists[at + i];
        for (uint32_t i = have + take + tid; i < P; i += 1024u) buf[i] = kPadComposite;
        __syncthreads();
        bitonic_sort_u64_1024(buf, P, (int)tid);
        have = have + take < p.k ? have + take : p.k;
        at += take;
    }
    for (uint32_t i = tid; i < p.k; i += 1024u) {
        const uint64_t comp = i < have ? buf[i] : kPadComposite;
        const size_t o = (size_t)q * p.k + i;
        if (comp == kPadComposite) {  // mvfgpu_search's padding under L2; under InnerProduct for a biased key
            p.out_scores[o] = pad_score(p.score_bias ? MVF_METRIC_INNER_PRODUCT : MVF_METRIC_L2);
            p.out_indices[o] = ~0ull;
            if (p.out_raw) p.out_raw[o] = 0;
        } else if (p.float_key) {  // (out_raw is NULL)
            p.out_scores[o] = __uint_as_float((uint32_t)p.score_bias - (uint32_t)(comp >> 32));
            p.out_indices[o] = p.ids ? p.ids[(uint32_t)comp] : p.index_base + (uint32_t)comp;
        } else {
            const uint32_t r = (uint32_t)comp;
            const int32_t d = p.score_bias ? p.score_bias - (int32_t)(comp >> 32) : (int32_t)(comp >> 32);
            p.out_scores[o] = (float)d;  // exact: |d| < 2^24
            p.out_indices[o] = p.ids ? p.ids[r] : p.index_base + r;
            if (p.out_raw) p.out_raw[o] = d;
        }
    }
}

template <int G>
const void* reg_kernel(uint32_t qb) {
    switch (qb) {
        case 1: return reinterpret_cast<const void*>(&hamming_reg_kernel<G, 1>);
        case 2: if constexpr (G >= 2) return reinterpret_cast<const void*>(&hamming_reg_kernel<G, 2>); break;
        case 4: if constexpr (G >= 4) return reinterpret_cast<const void*>(&hamming_reg_kernel<G, 4>); break;
        case 8: if constexpr (G >= 8) return reinterpret_cast<const void*>(&hamming_reg_kernel<G, 8>); break;
        case 16: if constexpr (G >= 16) return reinterpret_cast<const void*>(&hamming_reg_kernel<G, 16>); break;
        default: break;
    }
    return nullptr;
}

template <int G>
const void* stream_kernel(uint32_t qt) {
    switch (qt) {
        case 1: return reinterpret_cast<const void*>(&hamming_stream_kernel<G, 1>);
        case 2: return reinterpret_cast<const void*>(&hamming_stream_kernel<G, 2>);
        case 4: return reinterpret_cast<const void*>(&hamming_stream_kernel<G, 4>);
        case 8: return reinterpret_cast<const void*>(&hamming_stream_kernel<G, 8>);
        default: return nullptr;
    }
}

const void* scan_kernel(const HammingForm& f) {
    if (f.form == 0) {
        switch (f.lanes) {
            case 1: return reg_kernel<1>(f.batch);
            case 2: return reg_kernel<2>(f.batch);
            case 4: return reg_kernel<4>(f.batch);
            case 8: return reg_kernel<8>(f.batch);
            case 16: return reg_kernel<16>(f.batch);
            default: return nullptr;
        }
    }
    return f.lanes == 32 ? stream_kernel<32>(f.query_tile) : f.lanes == 64 ? stream_kernel<64>(f.query_tile) : nullptr;
}

}  // namespace

hipError_t hamming_launch(const HammingForm& f, const HammingParams& p, hipStream_t s, hipEvent_t* marks) {
    if (p.nq == 0) return hipSuccess;
    HammingParams arg = p;
    void* args[] = {&arg};
    auto mark = [&](int i) { return marks ? hipEventRecord(marks[i], s) : hipSuccess; };
    if (const hipError_t e = mark(0)) return e;
    if (f.row_slices) {  // H0
        const void* fn = scan_kernel(f);
        if (!fn || f.lds_bytes > 160u * 1024u || (uint64_t)f.row_slices * f.kcap > kHamMergeMax) return hipErrorInvalidValue;
        if (f.lds_bytes > 48u * 1024u) {
            const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.lds_bytes);
            if (e != hipSuccess) return e;
        }
        const dim3 grid(f.row_slices, (p.nq + f.query_tile - 1u) / f.query_tile);
        const hipError_t e = hipLaunchKernel(fn, grid, dim3(kHamThreads), args, f.lds_bytes, s);
        if (e != hipSuccess) return e;
    }
    if (const hipError_t e = mark(1)) return e;
    if (const hipError_t e = hamming_merge_launch(arg, s)) return e;
    return mark(2);
}

hipError_t hamming_merge_launch(const HammingParams& p, hipStream_t s) {
    HammingParams arg = p;
    void* args[] = {&arg};
    const uint32_t total = p.row_slices * p.kcap;
    const uint32_t held = total < kHamMergeLds ? (total < 2u ? 2u : next_pow2(total)) : kHamMergeLds;
    const size_t lds = (size_t)held * 8u;
    const void* mfn = reinterpret_cast<const void*>(&hamming_merge_kernel);
    if (lds > 48u * 1024u) {
        const hipError_t e = hipFuncSetAttribute(mfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    return hipLaunchKernel(mfn, dim3(p.nq), dim3(1024), args, lds, s);
}

}  // namespace mvf
