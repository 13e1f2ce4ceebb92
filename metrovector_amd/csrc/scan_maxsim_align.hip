// scan_maxsim_align.hip — the kernels of the MaxSim alignments (mvfgpu_maxsim_align; DESIGN.md §3 "Alignments", §5 "M0-arg and the
// alignment writer"; maxsim.hip is the host side): M0-arg, the instantiations of M0's template (scan_maxsim_score.inc) that keep
// the row with the order key, and the writer.  A translation unit of its own, so that the build does not wait for M0's twice.
//
// Algorithmic HBM bytes of M0-arg: M0's -- the candidates' rows once per chunk of tokens and query set.

#include "scan_maxsim.h"
#include "k1_rowscore.h"

#include <algorithm>
#include <type_traits>

namespace mvf {
namespace {

#include "scan_maxsim_score.inc"

// grid (blocks over sets x m x tc), block 256
__global__ void __launch_bounds__(256) maxsim_align_write_kernel(MaxsimAlignWriteParams p) {
    const size_t total = (size_t)p.sets * p.m * p.tc;
    const bool raw_key = key_is_raw(p.dtype, p.metric);
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const uint32_t t = (uint32_t)(e % p.tc);
        const size_t entry = e / p.tc;  // set * m + i
        const uint32_t set = (uint32_t)(entry / p.m);
        const size_t o = entry * p.n_tokens + p.t0 + t;
        const uint32_t slot = p.best64 ? p.slots[entry] : 0xFFFFFFFFu;
        uint64_t comp = kPadComposite;
        if (slot < p.n_keys) comp = p.best64[((size_t)set * p.tc + t) * p.n_keys + slot];
        if (comp == kPadComposite) {
            p.out_scores[o] = pad_score(p.metric);
            p.out_rows[o] = ~0ull;
            if (p.out_raw) p.out_raw[o] = 0;
            continue;
        }
        const uint32_t key = (uint32_t)(comp >> 32), row = (uint32_t)comp;
        p.out_scores[o] = maxsim_score_of(key, p.metric, raw_key);
        p.out_rows[o] = p.ids ? p.ids[row] : p.index_base + row;
        if (p.out_raw) p.out_raw[o] = raw_key ? raw_from_key(key, p.metric) : 0;
    }
}

}  // namespace

hipError_t maxsim_score_arg_launch(uint8_t dtype, int metric, int G, const MaxsimScoreParams& p, hipStream_t s) {
    return score_launch<true, true>(dtype, metric, G, p, s);
}

hipError_t maxsim_align_write_launch(const MaxsimAlignWriteParams& p, hipStream_t s) {
    const size_t total = (size_t)p.sets * p.m * p.tc;
    if (total == 0) return hipSuccess;
    if (p.t0 + p.tc > p.n_tokens || (p.best64 && !p.slots)) return hipErrorInvalidValue;
    const uint32_t blocks = (uint32_t)std::min<size_t>((total + 255u) / 256u, 65536u);
    hipLaunchKernelGGL(maxsim_align_write_kernel, dim3(blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace mvf
