// query_i8s.h — the query side of the int8 selection (shadow_i8.hip), as ONE device function: the stand-alone preparation
// kernel of the batched route and the prologue of K1's int8-shadow unit (scan_stream.inc, QSK) both call it, so a query gets
// the same scale, the same int8 bytes and the same bound whichever route prepares it.
#pragma once

#include "mvf_common.h"

namespace mvf {

// One 256-thread block quantises ONE f32 query (q == NULL: all zeros) of `dim` elements into `nelem` >= dim int8 values at
// dst (zero padded; LDS or global): q8 = rint(q / s_q), s_q = max|q| / 127.  Thread t takes the elements t, t + 256, ... in
// both passes, a wave's partial sums meet in an xor butterfly and the four waves' in red[] -- the order every sum below is
// defined by.  red: 12 floats of LDS; a block that calls this several times in a row alternates between two such areas (the
// last read of one call is not fenced from the first write of the next).  Three block barriers.
//   *sq_out = s_q, *qn_out = |q| (f32 norm of the ORIGINAL query), in every thread;
//   *delta_out (thread 0 only, where want_delta) = the proven bound of |approximate score - exact score| over ALL rows:
//     InnerProduct  s_q (|eq| A + |q8| B) + 4e-7 |q| max|x|
//     Cosine        s_q (|eq| Ac + |q8| Bc) / |q| + 4e-7
//     L2 (on the GEMM-form squared distance qq + xx - 2 q.x)   2 x the InnerProduct bound + 4e-7 (qq + max xx)
//   (A, B, Ac, Bc = stats[0..3]; the 4e-7 terms cover the f32 evaluation of acc * s_r * s_q and of the norms.)
// A non-finite query gets s_q = 0 and delta = +inf: every row is kept, the query overflows its budget and K1 repairs it.
__device__ __forceinline__ void prep_query_i8s(const float* q, uint32_t dim, uint32_t nelem, int metric, const float* stats,
                                               const float* xxmax, int8_t* dst, float* red, bool want_delta, float* sq_out,
                                               float* qn_out, float* delta_out) {
    const uint32_t tid = threadIdx.x;
    float mx = 0.f, ss = 0.f;
    bool bad = false;
    if (q)
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
    const float sq = (bad || !(mx > 0.f)) ? 0.f : mx / 127.0f;
    float q2 = 0.f, e2 = 0.f;
    for (uint32_t c = tid; c < nelem; c += 256) {
        const float v = (q && c < dim) ? q[c] : 0.f;
        const float t = sq > 0.f ? v / sq : 0.f;
        float r8 = rintf(t);
        r8 = fminf(fmaxf(r8, -127.f), 127.f);
        const float e = t - r8;
        q2 = fmaf(r8, r8, q2);
        e2 = fmaf(e, e, e2);
        dst[c] = (int8_t)(int)r8;
    }
    for (int off = 32; off > 0; off >>= 1) {
        q2 += __shfl_xor(q2, off, 64);
        e2 += __shfl_xor(e2, off, 64);
    }
    if ((tid & 63) == 0) {
        red[tid >> 6] = q2;
        red[4 + (tid >> 6)] = e2;
    }
    __syncthreads();
    const float qn = sqrtf(ss);
    *sq_out = sq;
    *qn_out = qn;
    if (want_delta && tid == 0) {
        q2 = red[0] + red[1] + red[2] + red[3];
        e2 = red[4] + red[5] + red[6] + red[7];
        const float inf = __uint_as_float(0x7F800000u);
        const float eq = sqrtf(e2) * 1.0005f + 1e-3f, q8n = sqrtf(q2) * 1.0005f;
        float d;
        if (!q) d = 0.f;
        else if (bad) d = inf;
        else if (metric == MVF_METRIC_COSINE) d = qn > 0.f ? sq * (eq * stats[2] + q8n * stats[3]) / qn * 1.0001f + 4e-7f : 0.f;
        else {
            const float xm = sqrtf(xxmax[0]);
            d = sq * (eq * stats[0] + q8n * stats[1]) * 1.0001f + 4e-7f * qn * xm;
            if (metric == MVF_METRIC_L2) d = 2.0f * d + 4e-7f * (ss + xxmax[0]);
        }
        *delta_out = d;
    }
}

}  // namespace mvf
