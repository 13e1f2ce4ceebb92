// mmr_walk.h — the arithmetic of the diversified re-ranking's greedy walk (DESIGN.md §3 "Diversified re-ranking"), stated once
// for D0 (scan_mmr.hip) and the host walk (mmr.hip: mvfgpu_selftest_mmr_walk):
//   * value(score): larger is better for every metric -- the score itself under InnerProduct and Cosine, its exact negation
//     under L2;
//   * objective(a, rel, b, red) = (a rel) - (b red): two f32 multiplications and one f32 subtraction, each rounded to nearest
//     and never contracted into an fma (hipcc contracts a x - b y by default: the device takes the _rn intrinsics, the host
//     compiles the three operations with contraction switched off);
//   * order_key(obj): ascending u32 = best first, as key_from_score orders values -- -0.0 == +0.0, NaN last;
//   * reported(obj): the objective as written out -- every NaN the one quiet NaN;
//   * score_of_key: the f32 score (and the exact integer) a search writes for an order key (aux_kernels.hip: write_result).
#pragma once

#include <math.h>

#include "mvf_common.h"

namespace mvf {
namespace mmr {

MVF_HD float value(float score, uint8_t metric) { return metric == MVF_METRIC_L2 ? -score : score; }

MVF_HD float objective(float a, float rel, float b, float red) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(__fmul_rn(a, rel), __fmul_rn(b, red));
#else
#pragma clang fp contract(off)
    const float x = a * rel;
    const float y = b * red;
    return x - y;
#endif
}

// a rel alone: the objective reported for pick 0
MVF_HD float relevance_term(float a, float rel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, rel);
#else
    return a * rel;
#endif
}

MVF_HD uint32_t order_key(float obj) { return ord_f32(-obj); }

// the objective as it is reported: a NaN is the quiet NaN 0x7FC00000 whatever produced it (as a NaN score is: unord_f32) --
// which operand's NaN an operation hands on, and the sign of a NaN made from 0 x inf, differ between processors
MVF_HD float reported(float obj) { return obj != obj ? bits_f32(0x7FC00000u) : obj; }

// fmaxf that ignores a NaN on either side, as the device's (the host's fmaxf does the same; written out so that both sides
// run the same lines)
MVF_HD float max_ignoring_nan(float red, float sim) {
    if (sim != sim) return red;
    if (red != red) return sim;
    return red < sim ? sim : red;
}

MVF_HD float score_of_key(uint32_t key, uint8_t dtype, uint8_t metric, int32_t* raw) {
    if (key_is_raw(dtype, metric)) {
        *raw = raw_from_key(key, metric);
        return metric == MVF_METRIC_L2 ? sqrtf((float)*raw) : (float)*raw;
    }
    *raw = 0;
    return score_from_key(key, metric);
}

}  // namespace mmr
}  // namespace mvf
