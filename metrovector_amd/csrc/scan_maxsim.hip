// scan_maxsim.hip — the kernels of the multi-vector search (DESIGN.md §3 "Multi-vector search", §5 "M0 / M1 — multi-vector
// search"; maxsim.hip is the host side).
//
// M0 walks the partition's key-ordered row list in blocks of kMaxsimRows positions.  The chunk's tokens are staged as K1
// stages one query (zero padded to J G vectors; sums of squares in K1's order), each G-lane group of K1's one-query shape
// scores a row against the tokens, kMaxsimTokenGroup at a time, with K1's per-row arithmetic (k1_rowscore.h): for every
// (token, row) the vectors advance j = 0 .. J-1, so the bits are K1's whatever the chunk.  Rows of up to kMaxsimRegSteps steps
// are loaded ONCE (non-temporal 16-byte loads) and stay in registers over the whole chunk; longer rows are read again per token
// group, through the cache.  The G partial sums of a step's (token, row) pairs meet in k1::group_sum's pairs and order, scattered
// over the group's lanes (scatter_sum): one lane per pair makes the key.  What is kept is the smallest u32 order key per (token,
// key): an LDS minimum per (token, key of the block) first, then one atomicMin per (token, run of the block) into
// best[token][key ordinal].  A minimum does not depend on the order of its operands: the result is deterministic.
// M1 adds the chunk's reconstructed scores to the running f32 sum of every key, in token order.
// The candidate form (mvfgpu_search_maxsim_candidates; DESIGN.md §5 "E0"): E0 expands the host plan's segments into one
// concatenated (row, slot ordinal) list per window of query sets, every set's part padded to whole blocks, and M0's CAND
// instantiations walk it with the block's set taken from a block table; M1 and the writer take the sets' candidate counts.
//
// Algorithmic HBM bytes of M0: the held rows' pitch once per chunk of tokens and query set (+ 8 bytes per held row and block).

#include "scan_maxsim.h"
#include "k1_rowscore.h"

#include <algorithm>
#include <type_traits>

namespace mvf {
namespace {

__global__ void __launch_bounds__(256) maxsim_ordinals_kernel(const uint64_t* offsets, uint64_t n_keys, uint32_t live, uint32_t* ord) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= live) return;
    uint64_t lo = 0, hi = n_keys;  // the last j with offsets[j] <= i; offsets[0] = 0
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid;
        else hi = mid;
    }
    ord[i] = (uint32_t)lo;
}

#include "scan_maxsim_score.inc"  // scatter_sum, M0 (maxsim_score_kernel), maxsim_score_of, pick_kernel, score_launch

// grid (ceil(n_keys / 256), sets), block 256
__global__ void __launch_bounds__(256) maxsim_sum_kernel(MaxsimSumParams p) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x, set = blockIdx.y;
    if (g >= p.n_keys) return;
    if (p.cand && g >= p.cand[set].count) {  // no candidate of this set: behind every key, a NaN sum's included
        if (p.last) p.rank[(size_t)set * p.n_keys + g] = rank_entry(kNanKey, g, true);
        return;
    }
    const bool raw_key = key_is_raw(p.dtype, p.metric);
    const uint32_t* best = p.best + (size_t)set * p.tc * p.n_keys + g;
    float* sum = p.sum + (size_t)set * p.n_keys + g;
    float S = p.first ? 0.0f : *sum;
    for (uint32_t t = 0; t < p.tc; t++) {
        const float b = maxsim_score_of(best[(size_t)t * p.n_keys], p.metric, raw_key);
        S = (p.first && t == 0) ? b : __fadd_rn(S, b);
    }
    *sum = S;
    if (p.last) p.rank[(size_t)set * p.n_keys + g] = rank_entry(key_from_score(S, p.metric), g, false);
}

// grid (blocks over k, sets), block 256
__global__ void __launch_bounds__(256) maxsim_write_kernel(MaxsimWriteParams p) {
    const uint32_t set = blockIdx.y;
    const uint32_t held = p.cand ? p.cand[set].count : p.n_keys;
    const uint64_t* keys = p.cand ? p.keys + p.cand[set].seg0 : p.keys;
    if (p.out_counts && blockIdx.x == 0 && threadIdx.x == 0) p.out_counts[set] = min(p.k, held);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < p.k; i += (size_t)gridDim.x * 256) {
        const size_t o = (size_t)set * p.k + i;
        if (i < held) {
            const uint32_t g = (uint32_t)(p.sorted[(size_t)set * p.n_keys + i] >> 32);
            const float S = p.sum[(size_t)set * p.n_keys + g];
            p.out_scores[o] = S != S ? unord_f32(kNanKey) : S;  // the NaN every result carries
            p.out_keys[o] = keys[g];
        } else {
            p.out_scores[o] = pad_score(p.metric);
            p.out_keys[o] = ~0ull;
        }
    }
}

// E0; grid (n_blocks), block kMaxsimRows
__global__ void __launch_bounds__(kMaxsimRows) maxsim_expand_kernel(MaxsimExpandParams p) {
    const MaxsimCandBlock b = p.blocks[blockIdx.x];
    const MaxsimCandSet st = p.sets[b.set];
    const uint32_t pos = blockIdx.x * kMaxsimRows + threadIdx.x;
    const uint32_t i = pos - st.list0;  // the position among the set's rows
    uint32_t row = 0, slot = st.count ? st.count - 1u : 0u;
    if (i < st.rows) {
        const MaxsimCandSeg* seg = p.segs + st.seg0;
        uint32_t lo = 0, hi = st.count;  // the last j with before[j] <= i; before[0] = 0
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (seg[mid].before <= i) lo = mid;
            else hi = mid;
        }
        row = p.rows_by_key[(size_t)seg[lo].offset + (i - seg[lo].before)];
        slot = lo;
    }
    p.list[pos] = row;
    p.ord[pos] = slot;
}

}  // namespace

hipError_t maxsim_ordinals_launch(const uint64_t* offsets, uint64_t n_keys, uint32_t live, uint32_t* ord, hipStream_t s) {
    if (live == 0 || n_keys == 0) return hipSuccess;
    hipLaunchKernelGGL(maxsim_ordinals_kernel, dim3((live + 255u) / 256u), dim3(256), 0, s, offsets, n_keys, live, ord);
    return hipGetLastError();
}

hipError_t maxsim_score_launch(uint8_t dtype, int metric, int G, const MaxsimScoreParams& p, hipStream_t s) {
    return score_launch<false>(dtype, metric, G, p, s);
}

hipError_t maxsim_score_candidates_launch(uint8_t dtype, int metric, int G, const MaxsimScoreParams& p, hipStream_t s) {
    return score_launch<true>(dtype, metric, G, p, s);
}

hipError_t maxsim_expand_launch(const MaxsimExpandParams& p, hipStream_t s) {
    if (p.n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(maxsim_expand_kernel, dim3(p.n_blocks), dim3(kMaxsimRows), 0, s, p);
    return hipGetLastError();
}

hipError_t maxsim_sum_launch(const MaxsimSumParams& p, hipStream_t s) {
    if (p.n_keys == 0 || p.sets == 0) return hipSuccess;
    hipLaunchKernelGGL(maxsim_sum_kernel, dim3((p.n_keys + 255u) / 256u, p.sets), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t maxsim_write_launch(const MaxsimWriteParams& p, hipStream_t s) {
    if (p.sets == 0 || p.k == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)std::min<size_t>(((size_t)p.k + 255u) / 256u, 1024u);
    hipLaunchKernelGGL(maxsim_write_kernel, dim3(blocks, p.sets), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace mvf
