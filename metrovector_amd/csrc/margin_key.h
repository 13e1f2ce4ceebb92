// margin_key.h — the threshold of the shadow routes' margin, stated once: the key 2 delta behind the key `kth`.
// select_final_kernel's margin mode (aux_kernels.hip) keeps every listed row whose key is <= margin_key(k-th best key);
// the 5+1 scan (scan_stream.inc, S51) skips the low bit of a row only if even its best possible key is > margin_key(a key
// at or behind the k-th best).  The expression is one float subtraction (L2: addition) of the same 2 delta, monotone in the
// key it starts from: a worse `kth` never gives a better threshold, so the scan's threshold lies at or behind the select's.
#pragma once

#include "mvf_common.h"

namespace mvf {

MVF_HD uint32_t margin_key(uint32_t kth, float delta, uint8_t metric) {
    const float vk = score_from_key(kth, metric), d = 2.0f * delta;
    return key_from_score(metric == MVF_METRIC_L2 ? vk + d : vk - d, metric);
}

}  // namespace mvf
