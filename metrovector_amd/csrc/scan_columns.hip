// scan_columns.hip — P0, the predicate kernel of the column filters (columns.hip, DESIGN.md §5 "P0 — column predicates").
//
// One launch evaluates every clause of a call over the handle's device columns, combines them (all / any), takes the base
// filter's admitted rows and writes the ALLOW words over local rows that F0 (scan_filter.hip) consumes with shift 0.  A wave
// covers kWhereStepRows = 256 consecutive rows per step: lane l owns rows 4 l .. 4 l + 3 and reads them with one 16-byte load
// per UInt32 column and two per UInt64 column; the lanes' 4-bit results are OR-ed across the eight lanes of a word with three
// lane exchanges, and the first lane of each group stores the word -- once, with a plain store: steps start at multiples of
// 256 rows, so no two waves share a word and nothing is read back.  Set clauses search the call's sorted values in LDS.

#include "scan_columns.h"

#include <algorithm>

namespace mvf {
namespace {

// is v among set[0 .. cnt), ascending and distinct?
__device__ __forceinline__ bool in_sorted_set(const uint64_t* set, uint32_t cnt, uint64_t v) {
    uint32_t lo = 0, hi = cnt;  // the first entry >= v
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (set[mid] < v) lo = mid + 1u;
        else hi = mid;
    }
    return lo < cnt && set[lo] == v;
}

// the values of rows r0 .. r0 + 3 of a column, zero-extended; rows at and beyond n are not read (0)
__device__ __forceinline__ void load_rows4(const WhereClause& c, uint64_t r0, uint64_t n, uint64_t v[4]) {
    const bool whole = r0 + 4u <= n;
    if (c.is_u64) {
        const uint64_t* p = static_cast<const uint64_t*>(c.values) + r0;
        if (whole) {
            const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(p);
            const ulonglong2 b = *reinterpret_cast<const ulonglong2*>(p + 2);
            v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) v[j] = r0 + j < n ? p[j] : 0ull;
        }
    } else {
        const uint32_t* p = static_cast<const uint32_t*>(c.values) + r0;
        if (whole) {
            const uint4 a = *reinterpret_cast<const uint4*>(p);
            v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) v[j] = r0 + j < n ? p[j] : 0u;
        }
    }
}

// P0: grid (where_blocks), block 256 = four waves; wave g of the grid takes steps g, g + waves, ...
__global__ void __launch_bounds__(256) where_kernel(WhereParams p) {
    extern __shared__ uint64_t sets[];
    for (uint32_t i = threadIdx.x; i < p.n_sets; i += 256u) sets[i] = p.sets[i];
    if (p.n_sets) __syncthreads();  // block-uniform
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t nw = (p.n + 31u) / 32u;
    const uint64_t steps = (p.n + kWhereStepRows - 1u) / kWhereStepRows;
    for (uint64_t s = (uint64_t)blockIdx.x * 4u + wave; s < steps; s += (uint64_t)gridDim.x * 4u) {  // wave-uniform
        const uint64_t r0 = s * kWhereStepRows + lane * 4u;
        uint32_t acc = p.any ? 0u : 0xFu;
        for (uint32_t c = 0; c < p.n_clauses; c++) {
            const WhereClause& cl = p.clause[c];
            uint64_t v[4];
            load_rows4(cl, r0, p.n, v);
            uint32_t nib = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const bool hit = cl.is_set ? in_sorted_set(sets + cl.set_first, cl.set_count, v[j]) : (v[j] >= cl.lo && v[j] <= cl.hi);
                nib |= (uint32_t)(hit != (cl.negate != 0)) << j;
            }
            acc = p.any ? acc | nib : acc & nib;
        }
        acc &= r0 + 4u <= p.n ? 0xFu : r0 < p.n ? (1u << (uint32_t)(p.n - r0)) - 1u : 0u;  // bits at and beyond n are zero
        uint32_t word = acc << (4u * (lane & 7u));
        word |= __shfl_xor(word, 1, 64);
        word |= __shfl_xor(word, 2, 64);
        word |= __shfl_xor(word, 4, 64);
        const uint64_t w = s * (kWhereStepRows / 32u) + (lane >> 3);
        if ((lane & 7u) == 0u && w < nw) {
            if (p.base_deny) word &= ~p.base_deny[w];
            p.allow[w] = word;
        }
    }
}

}  // namespace

hipError_t where_launch(const WhereParams& p, int num_cus, hipStream_t s) {
    if (p.n == 0) return hipSuccess;
    const uint64_t steps = (p.n + kWhereStepRows - 1u) / kWhereStepRows;
    const uint64_t blocks = std::min<uint64_t>((steps + 3u) / 4u, (uint64_t)std::max(num_cus, 1) * 8u);
    hipLaunchKernelGGL(where_kernel, dim3((uint32_t)blocks), dim3(256), (size_t)p.n_sets * 8u, s, p);
    return hipGetLastError();
}

}  // namespace mvf
