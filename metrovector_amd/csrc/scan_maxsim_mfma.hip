// scan_maxsim_mfma.hip — the kernels of the multi-vector search's MFMA selection route (DESIGN.md §3 "Multi-vector search: the
// MFMA route", §5 "A0 / P0"; maxsim.hip is the host side, scan_maxsim.hip holds M0 / M1, which the route runs unchanged).
//
// A0 has M0's outer shape -- a block of 256 threads per kMaxsimRows positions of the key-ordered list, an LDS minimum per (query
// row, key of the block), one global atomicMin per (query row, run of the block) -- but takes its dot products from the matrix
// unit: wave w holds positions 32 w .. 32 w + 31 as operand B (the rows as stored) and 32 (set, token) query rows per accumulator
// as operand A (the prepared tokens, read where they lie: they are small and stay in the cache).  A step covers 32 bytes of a
// row: the lanes of half h = lane >> 5 load 16-byte vector 2 s + h of their row and of their query row.  Float16 rows: that is
// the operand of one mfma_f32_32x32x16_f16 as it stands.  Float32 rows: four mfma_f32_32x32x2f32, the e-th on element e of both
// vectors -- k = 8 s + e and 8 s + 4 + e meet in it; a sum does not care which products share an instruction as long as both
// operands are permuted alike.  MT accumulators share a row load.  In the C/D layout the lane's column lane & 31 is its list
// position and its 16 registers are query rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the tile.
// The scores are APPROXIMATIONS of K1's (another order of the f32 sum; the query rounded to f16 on Float16 rows); the bound of
// their error is maxsim_margin (scan_maxsim.h).  Where its premises fail for a (query row, position) -- a dot product, a norm or
// a denominator that is not finite, too large or too small -- the position's key is FORCED: a candidate whatever its sum.
// P0 turns the approximate sums, their kth best and the bound into the candidate keys of every set and those into the block
// table M0's candidate form takes.
//
// Algorithmic HBM bytes of A0: the held rows' pitch once per chunk of tokens and per MT x 32 query rows of the window (a block
// reads its own 128 rows again for the next MT tiles: from the cache where they fit) + 8 bytes per held row and block.

#include "scan_maxsim.h"

#include <hip/hip_fp16.h>

#include <algorithm>

namespace mvf {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr float kMfmaTooLarge = 1e37f;  // a dot product or denominator from here on leaves the bound's premises
constexpr float kMfmaTooSmall = 1e-30f; // .. and a non-zero denominator below this

__device__ __forceinline__ bool finite_f32(float x) { return (f32_bits(x) & 0x7F800000u) != 0x7F800000u; }

// a value of another lane of the caller's row of 16 lanes; a lane whose source lies outside the row keeps `old`
template <int CTRL>
__device__ __forceinline__ uint32_t row_dpp(uint32_t old, uint32_t src) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)src, CTRL, 0xF, 0xF, false);
}
constexpr int kRowShl = 0x100, kRowShr = 0x110;  // row_shl:n / row_shr:n are these + n: the neighbour n lanes to one side / the other

// grid (ceil(m / kMaxsimRows)), block 256
template <int DT, int METRIC, int MT>
__global__ void __launch_bounds__(256) maxsim_mfma_kernel(MaxsimMfmaParams p) {
    constexpr bool F16 = DT == MVF_DTYPE_FLOAT16;
    constexpr int PB = MT == 4 ? 2 : 4;  // steps of a batch: PB row vectors in flight, PB x MT query vectors
    __shared__ uint32_t lmin[32 * kMaxsimRows];  // [query row of the tile][key of the block] the block's minima
    __shared__ float q_undo[32], q_norm[32];     // the tile's query rows: undo scale, |q|
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, j = lane & 31u, h = lane >> 5;
    const uint32_t c0 = blockIdx.x * kMaxsimRows, nr = min(kMaxsimRows, p.m - c0);  // >= 1: the grid covers m
    const uint32_t R = p.sets * p.tc, tiles = (R + 31u) / 32u;                       // the launch's query rows
    const uint32_t pos = wave * 32u + j;
    const bool valid = pos < nr;
    const uint32_t at = c0 + (valid ? pos : 0u);
    const uint32_t row = p.list[at], ord0 = p.ord[c0];
    const uint32_t ordl = min(p.ord[at] - ord0, kMaxsimRows - 1u);  // every key holds a row: at most pos
    const uint32_t nseg = min(p.ord[c0 + nr - 1u] - ord0, kMaxsimRows - 1u) + 1u;
    const unsigned char* rp = p.rows + (size_t)row * p.pitch;
    float xn = 0.0f;
    if constexpr (METRIC == MVF_METRIC_COSINE) xn = p.xnorm[row];
    const uint32_t steps = (p.V + 1u) / 2u;

    // the elements behind `dim` inside a row's last vector are zero: the upload and the synthetic generator both write them
    auto load_b = [&](uint32_t s) __attribute__((always_inline)) {
        const uint32_t v = 2u * s + h;
        u32x4 x = u32x4{0, 0, 0, 0};  // vector V of an odd V is not the row's
        if (v < p.V) x = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(rp + (size_t)v * 16u));
        return x;
    };

    for (uint32_t tile0 = 0; tile0 < tiles; tile0 += MT) {
        // the lane's query row of every tile: row i of the launch is token t0 + i % tc of set i / tc
        const unsigned char* ap[MT];
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const uint32_t i = min((tile0 + mt) * 32u + j, R - 1u);  // a row behind the last scores the last again
            const uint32_t src = (i / p.tc) * p.n_tokens + p.t0 + i % p.tc;
            ap[mt] = p.qprep + (size_t)src * p.kp_bytes + h * 16u;
        }
        f32x16 acc[MT];
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[mt][r] = 0.0f;

        // PB steps at a time: the rows' vectors of the NEXT batch are in flight while this one's products run (a row is a random
        // gather: nothing but loads in flight hides its latency), the query rows' vectors of this batch come from the cache
        u32x4 cur[PB], nxt[PB];
#pragma unroll
        for (int i = 0; i < PB; i++) cur[i] = load_b((uint32_t)i);
        for (uint32_t s0 = 0; s0 < steps; s0 += PB) {
            u32x4 xa[PB][MT];
#pragma unroll
            for (int i = 0; i < PB; i++) {
                const uint32_t sa = min(s0 + (uint32_t)i, steps - 1u);  // a step behind the last reads the last again, unused
#pragma unroll
                for (int mt = 0; mt < MT; mt++) xa[i][mt] = *reinterpret_cast<const u32x4*>(ap[mt] + (size_t)sa * 32u);
            }
            if (s0 + PB < steps) {  // uniform
#pragma unroll
                for (int i = 0; i < PB; i++) nxt[i] = load_b(s0 + PB + (uint32_t)i);
            }
#pragma unroll
            for (int i = 0; i < PB; i++) {
                if (s0 + (uint32_t)i >= steps) break;  // uniform
#pragma unroll
                for (int mt = 0; mt < MT; mt++) {
                    if constexpr (F16) {
                        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, xa[i][mt]), __builtin_bit_cast(f16x8, cur[i]), acc[mt], 0, 0, 0);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; e++)
                            acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(xa[i][mt][e]), __uint_as_float(cur[i][e]), acc[mt], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < PB; i++) cur[i] = nxt[i];
        }

        // ---- the epilogue, tile after tile through one table
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const uint32_t tile = tile0 + mt;
            if (tile >= tiles) break;  // uniform
            __syncthreads();           // the table's last readers are through
            for (uint32_t i = tid; i < 32u * kMaxsimRows; i += 256u) lmin[i] = kNanKey;
            if (tid < 32u) {
                const uint32_t i = min(tile * 32u + tid, R - 1u);
                const uint32_t src = (i / p.tc) * p.n_tokens + p.t0 + i % p.tc;
                q_undo[tid] = p.undo ? p.undo[src] : 1.0f;
                q_norm[tid] = p.qnorm[src];
            }
            __syncthreads();
            // The 16 lanes of a row hold 16 neighbouring list positions, their key ordinals in runs: the keys of a run meet in
            // the run's lane at one end (log steps towards that end; equal ordinals 1, 2, 4, 8 lanes apart lie in one run),
            // and only that lane -- the one whose neighbour on the other side is outside the run or the row -- goes to LDS:
            // 32 lanes on one address cost the LDS 32 turns.  A minimum takes its operands in any order.
            const uint32_t ordk = valid ? ordl : 0xFFFFFFF0u;
            const bool same1 = row_dpp<kRowShl + 1>(0xFFFFFFFFu, ordk) == ordk, same2 = row_dpp<kRowShl + 2>(0xFFFFFFFFu, ordk) == ordk,
                       same4 = row_dpp<kRowShl + 4>(0xFFFFFFFFu, ordk) == ordk, same8 = row_dpp<kRowShl + 8>(0xFFFFFFFFu, ordk) == ordk;
            const bool leader = valid && row_dpp<kRowShr + 1>(0xFFFFFFFFu, ordk) != ordk;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const uint32_t il = (uint32_t)(r & 3) + 8u * (uint32_t)(r >> 2) + 4u * h, i = tile * 32u + il;
                const float dot = acc[mt][r] * q_undo[il];
                bool bad = !(fabsf(dot) < kMfmaTooLarge);  // NaN included
                float sc = dot;
                if constexpr (METRIC == MVF_METRIC_COSINE) {
                    const float qn = q_norm[il], den = qn * xn;
                    if (qn == 0.0f || xn == 0.0f) sc = 0.0f;  // K1's rule; a sum of squares is 0 in every order or in none
                    else if (!(den >= kMfmaTooSmall && den < kMfmaTooLarge)) sc = 0.0f, bad = true;
                    else sc = dot / den;
                }
                const bool live = valid && i < R;
                uint32_t key = live ? key_from_score(sc, METRIC) : kNanKey;
                if (live && bad && ord0 + ordl < p.n_keys) p.force[(size_t)(i / p.tc) * p.n_keys + ord0 + ordl] = 1;
                uint32_t o = row_dpp<kRowShl + 1>(key, key);
                key = same1 ? min(key, o) : key;
                o = row_dpp<kRowShl + 2>(key, key);
                key = same2 ? min(key, o) : key;
                o = row_dpp<kRowShl + 4>(key, key);
                key = same4 ? min(key, o) : key;
                o = row_dpp<kRowShl + 8>(key, key);
                key = same8 ? min(key, o) : key;
                if (leader && i < R) atomicMin(&lmin[il * kMaxsimRows + ordl], key);
            }
            __syncthreads();
            // one atomicMin per (query row, run of the block)
            for (uint32_t e = tid; e < 32u * nseg; e += 256u) {
                const uint32_t il = e / nseg, sg = e % nseg, i = tile * 32u + il;
                if (i < R && ord0 + sg < p.n_keys) atomicMin(&p.best[(size_t)i * p.n_keys + ord0 + sg], lmin[il * kMaxsimRows + sg]);
            }
        }
    }
}

// grid (ceil(n_keys / 256), sets), block 256
__global__ void __launch_bounds__(256) maxsim_mask_kernel(MaxsimMaskParams p) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, set = blockIdx.y;
    if (g >= p.n_keys) return;
    const size_t at = (size_t)set * p.n_keys + g;
    const bool flag = p.flag[at] != 0;
    if (p.dead) {
        if (!flag) p.rank[at] = rank_entry(kNanKey, g, true);
    } else if (flag || !finite_f32(p.sum[at])) {
        p.rank[at] = rank_entry(kNanKey, g, false);
    }
}

// grid (sets), block 64: delta[set]
__global__ void __launch_bounds__(64) maxsim_delta_kernel(MaxsimPickParams p) {
    if (threadIdx.x == 0)
        p.delta[blockIdx.x] = maxsim_margin(p.dtype, p.metric, p.dim, p.qnorm + (size_t)blockIdx.x * p.n_tokens, p.n_tokens, p.xxmax[0]);
}

// grid (ceil(n_keys / 256), sets), block 256
__global__ void __launch_bounds__(256) maxsim_pick_keys_kernel(MaxsimPickParams p) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, set = blockIdx.y;
    bool cand = false;
    if (g < p.n_keys) {
        const size_t at = (size_t)set * p.n_keys + g;
        const uint32_t te = (uint32_t)p.sorted[(size_t)set * p.n_keys + p.kth];  // the key half: 0xFFFFFFFE a live NaN entry
        const float theta = score_from_key(te, p.metric), S = p.sum[at];
        const double d = p.delta[set];
        cand = p.flag[at] != 0 || te >= 0xFFFFFFFEu || !finite_f32(theta) || !finite_f32(S) || !(d < 1e300);
        if (!cand) {
            double thr = (double)theta - 2.0 * d;
            thr -= fabs(thr) * 0x1p-52;  // the subtraction's own rounding: downwards
            cand = (double)S >= thr;
        }
        p.flag[at] = cand ? 1 : 0;
    }
    if (p.stats) {
        const uint32_t n = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cand));
        if ((threadIdx.x & 63u) == 0 && n) atomicAdd(&p.stats[set], n);
    }
}

// grid (ceil(n_blocks / 256), sets), block 256
__global__ void __launch_bounds__(256) maxsim_pick_blocks_kernel(MaxsimPickParams p, uint32_t n_blocks) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x, set = blockIdx.y;
    bool any = false;
    if (b < n_blocks) {
        const uint32_t c0 = b * kMaxsimRows, n = min(kMaxsimRows, p.m - c0);
        const uint32_t first = p.ord[c0], last = min(p.ord[c0 + n - 1u], p.n_keys - 1u);
        const unsigned char* flag = p.flag + (size_t)set * p.n_keys;
        for (uint32_t o = first; o <= last && !any; o++) any = flag[o] != 0;
        p.blocks[(size_t)set * n_blocks + b] = MaxsimCandBlock{set, any ? n : 0u};
    }
    if (p.stats) {
        const uint32_t n = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(any));
        if ((threadIdx.x & 63u) == 0 && n) atomicAdd(&p.stats[p.sets + set], n);
    }
}

template <int DT, int METRIC>
const void* pick_mfma(uint32_t tiles) {
    if (tiles >= 4) return reinterpret_cast<const void*>(&maxsim_mfma_kernel<DT, METRIC, 4>);
    if (tiles >= 2) return reinterpret_cast<const void*>(&maxsim_mfma_kernel<DT, METRIC, 2>);
    return reinterpret_cast<const void*>(&maxsim_mfma_kernel<DT, METRIC, 1>);
}

}  // namespace

hipError_t maxsim_mfma_score_launch(uint8_t dtype, int metric, const MaxsimMfmaParams& p, hipStream_t s) {
    if (p.sets == 0 || p.m == 0 || p.tc == 0) return hipSuccess;
    if (!maxsim_mfma_eligible(dtype, (uint8_t)metric) || p.t0 + p.tc > p.n_tokens || p.kp_bytes < (p.V + 1u) / 2u * 32u ||
        (uint64_t)p.sets * p.tc > 0xFFFFFFFFull || (dtype == MVF_DTYPE_FLOAT16 && !p.undo) || !p.force)
        return hipErrorInvalidValue;
    const uint32_t tiles = (p.sets * p.tc + 31u) / 32u;
    const bool cosine = metric == MVF_METRIC_COSINE;
    const void* fn = dtype == MVF_DTYPE_FLOAT16
                         ? (cosine ? pick_mfma<MVF_DTYPE_FLOAT16, MVF_METRIC_COSINE>(tiles) : pick_mfma<MVF_DTYPE_FLOAT16, MVF_METRIC_INNER_PRODUCT>(tiles))
                         : (cosine ? pick_mfma<MVF_DTYPE_FLOAT32, MVF_METRIC_COSINE>(tiles) : pick_mfma<MVF_DTYPE_FLOAT32, MVF_METRIC_INNER_PRODUCT>(tiles));
    MaxsimMfmaParams arg = p;
    void* args[] = {&arg};
    return hipLaunchKernel(fn, dim3((p.m + kMaxsimRows - 1) / kMaxsimRows), dim3(256), args, 0, s);
}

hipError_t maxsim_mask_launch(const MaxsimMaskParams& p, hipStream_t s) {
    if (p.n_keys == 0 || p.sets == 0) return hipSuccess;
    hipLaunchKernelGGL(maxsim_mask_kernel, dim3((p.n_keys + 255u) / 256u, p.sets), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t maxsim_pick_launch(const MaxsimPickParams& p, hipStream_t s) {
    if (p.n_keys == 0 || p.sets == 0 || p.m == 0) return hipSuccess;
    if (p.kth >= p.n_keys || p.sets > 65535u || !p.delta) return hipErrorInvalidValue;
    const uint32_t n_blocks = (p.m + kMaxsimRows - 1) / kMaxsimRows;
    hipLaunchKernelGGL(maxsim_delta_kernel, dim3(p.sets), dim3(64), 0, s, p);
    hipLaunchKernelGGL(maxsim_pick_keys_kernel, dim3((p.n_keys + 255u) / 256u, p.sets), dim3(256), 0, s, p);
    hipLaunchKernelGGL(maxsim_pick_blocks_kernel, dim3((n_blocks + 255u) / 256u, p.sets), dim3(256), 0, s, p, n_blocks);
    return hipGetLastError();
}

}  // namespace mvf
