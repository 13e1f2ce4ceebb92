// hamming_select.h — what the Hamming scans share on the device (scan_hamming.hip: H0; scan_hamming_mfma.hip: HQ / H2): the
// kernel attribute, a row's 16-byte step and its mask, the sort that cuts a query's buffer to k, and the slices' lists; and what
// H2 shares with the sign-bit scan (scan_signbits.hip: S2): a row chunk's load and the candidate buffers in the global scratch;
// and what H2 shares with the radius scan (scan_hamming_radius.hip: HR2): a row word's FP4 operand.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bitonic.h"
#include "scan_hamming.h"

namespace mvf {

// A guard, not a tuning: the kernels are integer work whose answers are compared byte for byte, and they are compiled with the
// packed-f32 VALU forms (v_pk_*_f32) switched off so that no compiler version lowers H1's one float conversion or a 64-bit
// move to them.  Effect with the current compiler: none on the arithmetic -- the ISA holds no v_pk_* instruction with or
// without the attribute -- but a callee without the attribute is not inlined into a kernel with it, so __syncthreads is a call here (a few dozen cycles beside each barrier) and the
// helpers below use builtins and a plain word struct instead of the HIP vector types.  It can be removed without changing a result.
#if defined(__HIP_DEVICE_COMPILE__)
#define HAM_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
#else
#define HAM_KERNEL __global__
#endif

// a 16-byte step as four words (a plain aggregate: loads and LDS reads of it are one 128-bit access)
struct alignas(16) u32x4 {
    uint32_t x, y, z, w;
};

// the u32 words of 16-byte step `step` that lie inside `dim` bytes: all ones, the tail's low bytes, or zero
__device__ __forceinline__ u32x4 step_mask(uint32_t step, uint32_t dim) {
    uint32_t m[4];
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) {
        const uint32_t at = step * 16u + w * 4u;
        const uint32_t have = at >= dim ? 0u : (dim - at >= 4u ? 4u : dim - at);
        m[w] = have == 4u ? 0xFFFFFFFFu : ((1u << (8u * have)) - 1u);
    }
    return u32x4{m[0], m[1], m[2], m[3]};
}

// One query's buffer settled by the whole block: buf[0 .. c) in any order -> its entries ascending in LDS, kPadComposite behind
// them up to a power of two.  Returns what the query keeps, min(c, k); the caller's thread 0 stores it and the new threshold,
// buf[k - 1] where the buffer held k.
// REG (H2; NT = 256): the network runs in registers where 8 entries a thread hold the buffer -- a step inside a wave is a lane
// exchange, and 512 entries take 6 barrier steps instead of 45.
template <int NT, bool REG = false>
__device__ __forceinline__ uint32_t sort_cut(uint64_t* buf, uint32_t c, uint32_t k, int tid) {
    const uint32_t P = c < 2u ? 2u : next_pow2(c);
    for (uint32_t i = c + (uint32_t)tid; i < P; i += NT) buf[i] = kPadComposite;
    __syncthreads();
    if (REG && P <= 2u * NT) bitonic_sort_u64_reg<NT, 2>(buf, P, tid);
    else if (REG && P <= 8u * NT) bitonic_sort_u64_reg<NT, 8>(buf, P, tid);
    else bitonic_sort_u64<NT>(buf, P, tid);
    return c < k ? c : k;
}

// a tile's sorted lists -- query q's cnt[q] entries at bufs + q * p.buf -- to lists[q][slice][kcap]
template <int NT>
__device__ __forceinline__ void store_lists(const uint64_t* bufs, const uint32_t* cnt, const HammingParams& p, uint32_t q0, uint32_t qn,
                                            uint32_t slice) {
    for (uint32_t i = threadIdx.x; i < qn * p.kcap; i += NT) {
        const uint32_t q = i / p.kcap, e = i % p.kcap;
        p.lists[((size_t)(q0 + q) * p.row_slices + slice) * p.kcap + e] = e < cnt[q] ? bufs[(size_t)q * p.buf + e] : kPadComposite;
    }
}

// ---- what the matrix-unit scans share (scan_hamming_mfma.hip: H2; scan_signbits.hip: S2) ----

// The selection part of such a block's LDS: the sort area, the queries' thresholds and counts, the flag "a buffer is nearly full".
struct SelectLds {
    uint64_t *sort, *thr;
    uint32_t *cnt, *flag;
};

// A live row whose composite (key << 32 | row, smaller is better) beats the query's threshold joins the query's buffer in the
// global scratch cand[query][buf] of the block (H0's rule and H0's bookkeeping: between two checks a buffer receives each row
// once at most, so it cannot run over).
__device__ __forceinline__ void offer(const SelectLds& t, const HammingParams& p, uint64_t* cand, uint32_t q, uint32_t key, uint32_t r) {
    const uint64_t comp = ((uint64_t)key << 32) | r;
    if (comp < t.thr[q] && !(p.tomb && ((p.tomb[r >> 5] >> (r & 31u)) & 1u))) {
        const uint32_t slot = __hip_atomic_fetch_add(&t.cnt[q], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (slot < p.buf) cand[(size_t)q * p.buf + slot] = comp;
        if (slot + 1u + kHamStepRows > p.buf) t.flag[0] = 1u;
    }
}

// Behind an iteration: every buffer that could not take kHamStepRows more entries (all of them at the end of the slice) goes
// through the sort area: sorted, cut to k, written back, its threshold lowered to its k-th composite.
template <int NT>
__device__ __forceinline__ void settle(const SelectLds& t, const HammingParams& p, uint64_t* cand, uint32_t qn, bool last) {
    const int tid = (int)threadIdx.x;
    __syncthreads();
    const uint32_t full = t.flag[0];
    __syncthreads();
    if (!full && !last) return;
    for (uint32_t q = 0; q < qn; q++) {
        uint32_t c = t.cnt[q];
        if (!last && c + kHamStepRows <= p.buf) continue;
        c = c < p.buf ? c : p.buf;
        uint64_t* own = cand + (size_t)q * p.buf;
        for (uint32_t i = (uint32_t)tid; i < c; i += NT) t.sort[i] = own[i];
        const uint32_t keep = sort_cut<NT, true>(t.sort, c, p.k, tid);
        for (uint32_t i = (uint32_t)tid; i < keep; i += NT) own[i] = t.sort[i];
        if (tid == 0) {
            t.cnt[q] = keep;
            t.thr[q] = keep >= p.k ? t.sort[p.k - 1u] : kPadComposite;
        }
        __syncthreads();  // the sort area is the next query's
    }
    if (tid == 0) t.flag[0] = 0;
    __syncthreads();
}

// the lane's 16 bytes of chunk t of its F rows (row0, row0 + 16, ...; g the lane's k-group): zeros behind the slice's end and
// behind the pitch, the row's last step masked to `dim` (the pitch padding is never relied on)
template <int F>
__device__ __forceinline__ void load_chunk(uint32_t (&w)[F][4], const HammingParams& p, uint64_t row0, uint64_t hi, uint32_t t, uint32_t g,
                                           const u32x4& tail) {
    const uint32_t step = t * 4u + g;
#pragma unroll
    for (int f = 0; f < F; f++) {
        const uint64_t r = row0 + (uint64_t)(f * 16);
        u32x4 v{0, 0, 0, 0};
        if (r < hi && step < p.V) v = *(reinterpret_cast<const u32x4*>(p.rows + r * p.pitch) + step);
        if (step == p.V - 1u) v.x &= tail.x, v.y &= tail.y, v.z &= tail.z, v.w &= tail.w;
        w[f][0] = v.x, w[f][1] = v.y, w[f][2] = v.z, w[f][3] = v.w;
    }
}

// ---- what the FP4 scans share (scan_hamming_mfma.hip: H2; scan_hamming_radius.hip: HR2) ----

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));

// A row's word w as the A operand of one v_mfma_scale_f32_16x16x128_f8f6f4 step (scan_hamming_mfma.hip, "Operands"): VGPR j holds
// bit 4 n + j of w in nibble n as FP4 0x2 = 1.0 where the bit is set, 0 elsewhere; an FP4 operand fills four of the eight VGPRs.
__device__ __forceinline__ v8i fp4_row_operand(uint32_t w) {
    return v8i{(int)((w << 1) & 0x22222222u), (int)(w & 0x22222222u), (int)((w >> 1) & 0x22222222u), (int)((w >> 2) & 0x22222222u), 0, 0, 0, 0};
}

}  // namespace mvf
