// scan_hamming_maxsim.hip — B0 and the integer sums, the kernels of the binary MaxSim (scan_hamming_maxsim.h; hamming_maxsim.hip is
// the host side; DESIGN.md §3 "Binary MaxSim", §5 "B0").
//
// B0 has A0's outer shape (scan_maxsim_mfma.hip) -- a block of 256 threads per kMaxsimRows positions of the key-ordered list, an LDS
// minimum per (query row, key of the block), one global atomicMin per (query row, run of the block) -- and H2's arithmetic
// (scan_hamming_mfma.hip, "Operands"): d(q, x) = popcount(q) + sum over the bits of x (1 - 2q) on
// v_mfma_scale_f32_16x16x128_f8f6f4 with exact FP4 factors 0, +1, -1 and both scales 2^0; every partial sum is an integer below
// 2^24 in magnitude, so the f32 accumulators hold it exactly in any order.
//
// The operands change sides against H2: the prepared query rows are operand A, read where HQ left them (tiles of 16 rows; a
// wave's read of one step of one tile is 1 KiB, and the window's tokens stay in the cache), and the rows are operand B.  The FP4
// layouts of A and B are the same, lane l serving index l % 16 and k-group l / 16, so nothing is rearranged; but in C/D the
// lane's column l % 16 is now a LIST POSITION and its four registers are query rows 4 (l / 16) + i of the tile: the 16 lanes of a
// DPP row hold 16 neighbouring positions of one query row, which is what A0's epilogue wants.
// Wave w owns positions 32 w .. 32 w + 31 of its block as F = 2 fragments.  A lane loads the 16 bytes at offset 64 ch + 16 (l / 16)
// of its position's row, masks the row's last step to `dimension`, and expands word m for step m (fp4_row_operand).  MT = 4
// accumulator tiles share an expanded operand: a pass scores 64 query rows against the block's 128 positions.  Rows of one chunk
// (pitch <= 64) are loaded ONCE per launch and stay in registers over every pass; wider rows are loaded again per pass, chunk
// after chunk with the next chunk in flight.
//
// Algorithmic HBM bytes of B0: the held rows' pitch once per chunk of tokens (REG) or per pass (wider rows; from the cache where
// a block's 128 rows fit) + 8 bytes per held row and block.

#include "scan_hamming_maxsim.h"

#include "hamming_select.h"

namespace mvf {
namespace {

constexpr int MT = (int)kBinMaxsimPassTiles, F = (int)kBinMaxsimFrags, QP = MT * (int)kBinMaxsimTile;  // QP: query rows of a pass

// a value of another lane of the caller's row of 16 lanes; a lane whose source lies outside the row keeps `old`
template <int CTRL>
__device__ __forceinline__ uint32_t row_dpp(uint32_t old, uint32_t src) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)src, CTRL, 0xF, 0xF, false);
}
constexpr int kRowShl = 0x100, kRowShr = 0x110;  // row_shl:n / row_shr:n are these + n

// grid (ceil(words / 256)), block 256
__global__ void __launch_bounds__(256) hamming_maxsim_clear_kernel(uint32_t* best, size_t words) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i < words) best[i] = 0xFFFFFFFFu;
}

// grid (ceil(m / kMaxsimRows)), block 256
template <bool REG>
__global__ void __launch_bounds__(256) hamming_maxsim_kernel(HammingMaxsimParams p) {
    __shared__ uint32_t lmin[QP * kMaxsimRows];  // [query row of the pass][key of the block] the block's minima
    __shared__ uint32_t q_src[QP];               // the pass's query rows: their place among the window's prepared rows
    __shared__ float q_start[QP];                // .. and popcount(q)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r16 = lane & 15u, g = lane >> 4;
    const uint32_t c0 = blockIdx.x * kMaxsimRows, nr = min(kMaxsimRows, p.m - c0);  // >= 1: the grid covers m
    const uint32_t R = p.sets * p.tc, tiles = (R + kBinMaxsimTile - 1u) / kBinMaxsimTile;  // the launch's query rows
    const uint32_t ord0 = p.ord[c0];
    const uint32_t nseg = min(p.ord[c0 + nr - 1u] - ord0, kMaxsimRows - 1u) + 1u;
    uint32_t seg_sh = 0;  // the runs of the block padded to a power of two: the flush splits its index by a shift
    while ((1u << seg_sh) < nseg) seg_sh++;
    const u32x4 tail = step_mask(p.V - 1u, p.dim);

    // the lane's position of every fragment.  The 16 lanes of a row hold 16 neighbouring list positions, their key ordinals in
    // runs: the minima of a run meet in the run's lane at one end (log steps towards that end; equal ordinals 1, 2, 4, 8 lanes
    // apart lie in one run), and only that lane goes to LDS (A0's epilogue)
    const unsigned char* rp[F];
    uint32_t ordl[F];
    bool valid[F], same1[F], same2[F], same4[F], same8[F], leader[F];
#pragma unroll
    for (int f = 0; f < F; f++) {
        const uint32_t pos = wave * 32u + (uint32_t)f * 16u + r16;
        valid[f] = pos < nr;
        const uint32_t at = c0 + (valid[f] ? pos : 0u);  // a dead position scores the block's first row, and keeps nothing
        rp[f] = p.rows + (size_t)p.list[at] * p.pitch;
        ordl[f] = min(p.ord[at] - ord0, kMaxsimRows - 1u);  // every key holds a row: at most pos
        const uint32_t ordk = valid[f] ? ordl[f] : 0xFFFFFFF0u;
        same1[f] = row_dpp<kRowShl + 1>(0xFFFFFFFFu, ordk) == ordk;
        same2[f] = row_dpp<kRowShl + 2>(0xFFFFFFFFu, ordk) == ordk;
        same4[f] = row_dpp<kRowShl + 4>(0xFFFFFFFFu, ordk) == ordk;
        same8[f] = row_dpp<kRowShl + 8>(0xFFFFFFFFu, ordk) == ordk;
        leader[f] = valid[f] && row_dpp<kRowShr + 1>(0xFFFFFFFFu, ordk) != ordk;
    }
    // the lane's 16 bytes of chunk ch of its F rows: zeros behind the pitch, the row's last step masked to `dim`
    auto load_words = [&](uint32_t ch, uint32_t (&w)[F][4]) __attribute__((always_inline)) {
        const uint32_t step = ch * 4u + g;
#pragma unroll
        for (int f = 0; f < F; f++) {
            u32x4 v{0, 0, 0, 0};
            if (step < p.V) v = *(reinterpret_cast<const u32x4*>(rp[f]) + step);
            if (step == p.V - 1u) v.x &= tail.x, v.y &= tail.y, v.z &= tail.z, v.w &= tail.w;
            w[f][0] = v.x, w[f][1] = v.y, w[f][2] = v.z, w[f][3] = v.w;
        }
    };
    uint32_t cur[F][4], nxt[F][4] = {};
    if constexpr (REG) load_words(0u, cur);

    const u32x4* prepared = reinterpret_cast<const u32x4*>(p.prepared);
    for (uint32_t tile0 = 0; tile0 < tiles; tile0 += MT) {
        // the pass's table and its query rows: row i of the launch is token t0 + i % tc of set i / tc
        for (uint32_t i = tid; i < (uint32_t)QP * kMaxsimRows; i += 256u) lmin[i] = 0xFFFFFFFFu;
        if (tid < (uint32_t)QP) {
            const uint32_t i = min(tile0 * kBinMaxsimTile + tid, R - 1u);  // a row behind the last scores the last again, unkept
            const uint32_t src = (i / p.tc) * p.n_tokens + p.t0 + i % p.tc;
            q_src[tid] = src;
            q_start[tid] = p.starts[src];
        }
        __syncthreads();
        const u32x4* ap[MT];  // the lane's A items of every tile: [tile of 16 prepared rows][chunk][step][lane]
        v4f acc[F][MT];
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const uint32_t src = q_src[mt * 16 + (int)r16];
            ap[mt] = prepared + (size_t)(src >> 4) * p.chunks * 256u + g * 16u + (src & 15u);
            const float* st = q_start + mt * 16 + (int)g * 4;
#pragma unroll
            for (int f = 0; f < F; f++) acc[f][mt] = v4f{st[0], st[1], st[2], st[3]};
        }
        if constexpr (!REG) load_words(0u, cur);
#pragma unroll 1
        for (uint32_t ch = 0; ch < p.chunks; ch++) {
            if constexpr (!REG)
                if (ch + 1u < p.chunks) load_words(ch + 1u, nxt);  // in flight under this chunk's MFMAs
#pragma unroll
            for (int m = 0; m < 4; m++) {
                v8i bv[F];
#pragma unroll
                for (int f = 0; f < F; f++) bv[f] = fp4_row_operand(cur[f][m]);
#pragma unroll
                for (int mt = 0; mt < MT; mt++) {
                    const u32x4 a = ap[mt][(ch * 4u + (uint32_t)m) * 64u];
                    const v8i av = v8i{(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
#pragma unroll
                    for (int f = 0; f < F; f++)
                        acc[f][mt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv[f], acc[f][mt], 4, 4, 0, 127, 0, 127);
                }
            }
            if constexpr (!REG) {
#pragma unroll
                for (int f = 0; f < F; f++)
#pragma unroll
                    for (int j = 0; j < 4; j++) cur[f][j] = nxt[f][j];
            }
        }
        // element i of acc[f][mt]: query row 16 mt + 4 g + i of the pass against position 32 wave + 16 f + r16 of the block;
        // the key is the distance itself
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int f = 0; f < F; f++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint32_t il = (uint32_t)(mt * 16 + i) + 4u * g;
                    const bool in = tile0 * kBinMaxsimTile + il < R;
                    uint32_t key = valid[f] && in ? (uint32_t)acc[f][mt][i] : 0xFFFFFFFFu;
                    uint32_t o = row_dpp<kRowShl + 1>(key, key);
                    key = same1[f] ? min(key, o) : key;
                    o = row_dpp<kRowShl + 2>(key, key);
                    key = same2[f] ? min(key, o) : key;
                    o = row_dpp<kRowShl + 4>(key, key);
                    key = same4[f] ? min(key, o) : key;
                    o = row_dpp<kRowShl + 8>(key, key);
                    key = same8[f] ? min(key, o) : key;
                    if (leader[f] && in) atomicMin(&lmin[il * kMaxsimRows + ordl[f]], key);
                }
        __syncthreads();
        // one atomicMin per (query row, run of the block)
        for (uint32_t e = tid; e < ((uint32_t)QP << seg_sh); e += 256u) {
            const uint32_t il = e >> seg_sh, sg = e & ((1u << seg_sh) - 1u), i = tile0 * kBinMaxsimTile + il;
            if (sg < nseg && i < R && ord0 + sg < p.n_keys) atomicMin(&p.best[(size_t)i * p.n_keys + ord0 + sg], lmin[il * kMaxsimRows + sg]);
        }
        __syncthreads();  // the table's readers are through
    }
}

// grid (ceil(n_keys / 256), sets), block 256
__global__ void __launch_bounds__(256) hamming_maxsim_sum_kernel(HammingMaxsimSumParams p) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, set = blockIdx.y;
    if (g >= p.n_keys) return;
    uint32_t* best = p.best + (size_t)set * p.tc * p.n_keys + g;
    float* sum = p.sum + (size_t)set * p.n_keys + g;
    uint32_t S = p.first ? 0u : (uint32_t)*sum;
    for (uint32_t t = 0; t < p.tc; t++) {
        S += best[(size_t)t * p.n_keys];
        best[(size_t)t * p.n_keys] = 0xFFFFFFFFu;
    }
    *sum = (float)S;  // exact: S <= 2^22
    if (p.last) p.rank[(size_t)set * p.n_keys + g] = rank_entry(S, g, false);
}

}  // namespace

hipError_t hamming_maxsim_clear_launch(uint32_t* best, size_t words, hipStream_t s) {
    if (words == 0) return hipSuccess;
    if ((words + 255u) / 256u > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hamming_maxsim_clear_kernel, dim3((uint32_t)((words + 255u) / 256u)), dim3(256), 0, s, best, words);
    return hipGetLastError();
}

hipError_t hamming_maxsim_score_launch(const HammingMaxsimParams& p, hipStream_t s) {
    if (p.sets == 0 || p.m == 0 || p.tc == 0) return hipSuccess;
    if (p.t0 + p.tc > p.n_tokens || (uint64_t)p.sets * p.tc > 0xFFFFFFFFull || p.dim == 0 || p.dim > kBinMaxsimMaxDim ||
        p.V != (p.dim + 15u) / 16u || p.pitch < p.V * 16u || p.chunks != (p.V + 3u) / 4u)
        return hipErrorInvalidValue;
    const void* fn = p.chunks == 1u ? reinterpret_cast<const void*>(&hamming_maxsim_kernel<true>) : reinterpret_cast<const void*>(&hamming_maxsim_kernel<false>);
    HammingMaxsimParams arg = p;
    void* args[] = {&arg};
    return hipLaunchKernel(fn, dim3((p.m + kMaxsimRows - 1) / kMaxsimRows), dim3(256), args, 0, s);
}

hipError_t hamming_maxsim_sum_launch(const HammingMaxsimSumParams& p, hipStream_t s) {
    if (p.n_keys == 0 || p.sets == 0) return hipSuccess;
    if (p.sets > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hamming_maxsim_sum_kernel, dim3((p.n_keys + 255u) / 256u, p.sets), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace mvf
