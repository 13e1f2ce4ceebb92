// query_16s.h — the query side of the 6-bit selection (shadow_6b.hip): the prologue of K1's 6-bit-shadow unit
// (scan_stream.inc, S6) quantises the caller's f32 query to SIXTEEN bits, held as two int8 planes.
#pragma once

#include "mvf_common.h"

namespace mvf {

constexpr float kQ16Max = 16256.0f;  // 127 * 128: the largest |Q| whose high plane is an int8

// One 256-thread block quantises ONE f32 query of `dim` elements into `nelem` >= dim values Q = rint(q / s_q),
// s_q = max|q| / 16256, split as Q = 128 hi + lo with lo in [-64, 63] and hi in [-127, 127] (zero padded; dst_lo / dst_hi:
// LDS or global, natural element order).  Thread t takes the elements t, t + 256, ... in both passes; the sums meet as in
// query_i8s.h (xor butterfly, then red[]).  red: 16 words of LDS.  Three block barriers.
//   *sq_out = s_q, *qn_out = |q| (f32 norm of the ORIGINAL query), *qsum_out = sum Q (exact), in every thread;
//   *qpos_out (where asked for: the 5+1 unit) = P = sum max(Q, 0) (exact), in every thread: the most the low bits of a row's
//   codes can add to Q.y (shadow_5p1.h: y = 2 hi + lo, 0 <= Q.lo <= P);
//   *delta_out (thread 0 only, where want_delta) = the proven bound of |approximate score - exact score| over ALL rows,
//   query_i8s.h's three forms with the 6-bit shadow's maxima in stats[0..3], the 16-bit query's MEASURED |eq| and |Q|, and
//   6e-7 where the int8 route has 4e-7: the approximate dot product is float(128 hi.y + lo.y - 32 sum Q), an exact integer
//   rounded ONCE (2^-24), times s_r, times s_q (2^-24 each) -- three roundings of a value of at most |q||x| (1 + 1/31)
//   where the int8 route has two.
// A non-finite query gets s_q = 0 and delta = +inf: every row is kept, the query overflows its budget and K1 repairs it.
__device__ __forceinline__ void prep_query_16s(const float* q, uint32_t dim, uint32_t nelem, int metric, const float* stats,
                                               const float* xxmax, int8_t* dst_lo, int8_t* dst_hi, float* red, bool want_delta,
                                               float* sq_out, float* qn_out, int32_t* qsum_out, float* delta_out, int32_t* qpos_out = nullptr) {
    const uint32_t tid = threadIdx.x;
    float mx = 0.f, ss = 0.f;
    bool bad = false;
    for (uint32_t c = tid; c < dim; c += 256) {
        const float v = q[c];
        bad |= !(fabsf(v) < 3.0e38f);
        mx = fmaxf(mx, fabsf(v));
        ss = fmaf(v, v, ss);
    }
    for (int off = 32; off > 0; off >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        ss += __shfl_xor(ss, off, 64);
    }
    const bool wbad = __builtin_amdgcn_ballot_w64(bad) != 0;
    if ((tid & 63) == 0) {
        red[tid >> 6] = mx;
        red[4 + (tid >> 6)] = ss;
        red[8 + (tid >> 6)] = wbad ? 1.f : 0.f;
    }
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    ss = red[4] + red[5] + red[6] + red[7];
    bad = (red[8] + red[9] + red[10] + red[11]) > 0.f || !(ss < 3.0e38f);
    __syncthreads();
    const float sq = (bad || !(mx > 0.f)) ? 0.f : mx / kQ16Max;
    float q2 = 0.f, e2 = 0.f;
    int32_t qsum = 0, qpos = 0;
    for (uint32_t c = tid; c < nelem; c += 256) {
        const float v = c < dim ? q[c] : 0.f;
        const float t = sq > 0.f ? v / sq : 0.f;
        float r16 = rintf(t);
        r16 = fminf(fmaxf(r16, -kQ16Max), kQ16Max);  // |t| <= 16256 (1 + 2^-23): the clamp never bites beyond rounding
        const float e = t - r16;
        q2 = fmaf(r16, r16, q2);
        e2 = fmaf(e, e, e2);
        const int Q = (int)r16, lo = ((Q + 64) & 127) - 64;
        qsum += Q;
        if (qpos_out) qpos += Q > 0 ? Q : 0;
        dst_lo[c] = (int8_t)lo;
        dst_hi[c] = (int8_t)((Q - lo) >> 7);
    }
    for (int off = 32; off > 0; off >>= 1) {
        q2 += __shfl_xor(q2, off, 64);
        e2 += __shfl_xor(e2, off, 64);
        qsum += __shfl_xor(qsum, off, 64);
        if (qpos_out) qpos += __shfl_xor(qpos, off, 64);
    }
    if ((tid & 63) == 0) {
        red[tid >> 6] = q2;
        red[4 + (tid >> 6)] = e2;
        reinterpret_cast<int32_t*>(red)[12 + (tid >> 6)] = qsum;
        if (qpos_out) reinterpret_cast<int32_t*>(red)[8 + (tid >> 6)] = qpos;
    }
    __syncthreads();
    const int32_t* rsum = reinterpret_cast<const int32_t*>(red) + 12;
    *sq_out = sq;
    *qn_out = sqrtf(ss);
    *qsum_out = rsum[0] + rsum[1] + rsum[2] + rsum[3];
    if (qpos_out) *qpos_out = rsum[-4] + rsum[-3] + rsum[-2] + rsum[-1];
    if (want_delta && tid == 0) {
        const float qn = sqrtf(ss);
        q2 = red[0] + red[1] + red[2] + red[3];
        e2 = red[4] + red[5] + red[6] + red[7];
        const float inf = __uint_as_float(0x7F800000u);
        const float eq = sqrtf(e2) * 1.0005f + 1e-3f, qqn = sqrtf(q2) * 1.0005f;
        float d;
        if (bad) d = inf;
        else if (metric == MVF_METRIC_COSINE) d = qn > 0.f ? sq * (eq * stats[2] + qqn * stats[3]) / qn * 1.0001f + 6e-7f : 0.f;
        else {
            const float xm = sqrtf(xxmax[0]);
            d = sq * (eq * stats[0] + qqn * stats[1]) * 1.0001f + 6e-7f * qn * xm;
            if (metric == MVF_METRIC_L2) d = 2.0f * d + 4e-7f * (ss + xxmax[0]);
        }
        *delta_out = d;
    }
}

}  // namespace mvf
