// shadow_i8.hip — the INT8 SHADOW of a Float32 / Float16 corpus and its queries (selection only).
//
// Under the power limit that bounds the MFMA loops on this part the int8 MFMA delivers ~1.9 POP/s where
// the f16 one holds ~1.05 PFLOP/s, and only ~k rows per query need more than a coarse score.  So the batched path may
// SELECT on an int8 copy of the rows -- per-row scale s_r = max|x| / 127, x8 = rint(x / s_r) -- with int8 queries
// (s_q = max|q| / 127), keep every candidate inside a PROVEN error bound of the k-th best, and re-score the kept rows
// exactly from the stored rows and the caller's f32 query (compact_margin_kernel / rescore_kernel, as for the f16
// shadow): results are those of the exact paths.
//
// The bound.  With x = s_r (x8 + ex), q = s_q (q8 + eq), |ex|, |eq| <= 1/2 per element (rounding; nothing clamps):
//     q.x = s_r s_q [ x8.q8  +  x8.eq  +  ex.q8  +  ex.eq ]
// and by Cauchy-Schwarz  |q.x - s_r s_q x8.q8| <= s_r s_q [ (|x8| + |ex|) |eq| + |ex| |q8| ]  (2-norms; |ex| and |eq|
// are MEASURED, ~0.29 sqrt(dim), not bounded by sqrt(dim)/2).  Per row the kernel below stores nothing but x8 and
// s_r; what the margins need is the corpus-wide maximum of s_r (|x8| + |ex|) and of s_r |ex| -- plain (InnerProduct,
// L2 = qq + xx - 2 q.x) and divided by |x| (Cosine) -- four floats, accumulated with atomicMax while the shadow is
// built.  Per query: delta = s_q (|eq| A + |q8| B) (+ the f32 evaluation of the approximate score), see
// prep_queries_i8s_kernel.  On the benchmark's uniform rows that is 0.23 sigma of the score distribution at dim 768
// (0.27 at 1024): 5-8 x k candidates per query reach the re-scoring (the f16 shadow: a handful beyond k).
// A row holding Inf / NaN (or whose sum x^2 overflows) makes the maxima +inf: every query is then answered by K1's
// repair launches, exactly as with the f16 shadow.

#include "scan_mfma.h"

#include "mvf_common.h"
#include "query_i8s.h"
#include "row_builders.h"

#include <hip/hip_fp16.h>

namespace mvf {
namespace {

// One wave per row.  SRC = MVF_DTYPE_FLOAT32 / MVF_DTYPE_FLOAT16 rows at `pitch`; out: int8 rows at pitch8 (dim rounded
// up to 16, zero padded), xscale8[r] = s_r, stats[0..3] = max s_r(|x8|+|ex|), max s_r|ex|, the same two over |x|.
// The row's body is row_builders.h's shadow_i8_row, shared with the list-driven refresh of a row write (scan_update.hip).
template <int SRC>
__global__ void __launch_bounds__(256) shadow_i8_kernel(const unsigned char* rows, uint32_t n, uint32_t pitch, uint32_t dim,
                                                         unsigned char* rows8, uint32_t pitch8, float* xscale8, float* stats) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, nwaves = (gridDim.x * 256u) >> 6;
    ShadowMaxima m;
    for (uint32_t r = wave; r < n; r += nwaves) shadow_i8_row<SRC>(rows, pitch, dim, rows8, pitch8, xscale8, r, lane, m);
    fold_shadow_maxima(stats, lane, m);
}

// Queries for the int8 shadow, one block per (padded) query row: query_i8s.h does the arithmetic -- the int8 values, zero
// padded to KPB bytes per row, qaux0 = s_q (the scale the epilogue undoes), qaux1 = |q|, delta[q] = the proven bound.
// The batched route's preparation; one to four streamed queries are prepared by K1's own prologue (scan_stream.inc).
__global__ void __launch_bounds__(256) prep_queries_i8s_kernel(const float* q, uint32_t nq, uint32_t dim, uint32_t KPB, int metric,
                                                                const float* stats, const float* xxmax, unsigned char* qprep,
                                                                float* qaux0, float* qaux1, float* delta) {
    const uint32_t row = blockIdx.x;
    __shared__ float red[12];
    float sq, qn, d = 0.f;
    prep_query_i8s(row < nq ? q + (size_t)row * dim : nullptr, dim, KPB, metric, stats, xxmax,
                   reinterpret_cast<int8_t*>(qprep) + (size_t)row * KPB, red, true, &sq, &qn, &d);
    if (threadIdx.x == 0) {
        qaux0[row] = sq;
        qaux1[row] = qn;
        delta[row] = d;
    }
}

}  // namespace

hipError_t launch_shadow_i8(const unsigned char* rows, int src_dtype, uint32_t n, uint32_t pitch, uint32_t dim, unsigned char* rows8,
                            uint32_t pitch8, float* xscale8, float* stats, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n + 3) / 4, 256u * 8u);
    if (src_dtype == MVF_DTYPE_FLOAT32)
        hipLaunchKernelGGL(shadow_i8_kernel<MVF_DTYPE_FLOAT32>, dim3(blocks), dim3(256), 0, s, rows, n, pitch, dim, rows8, pitch8, xscale8, stats);
    else
        hipLaunchKernelGGL(shadow_i8_kernel<MVF_DTYPE_FLOAT16>, dim3(blocks), dim3(256), 0, s, rows, n, pitch, dim, rows8, pitch8, xscale8, stats);
    return hipGetLastError();
}

hipError_t launch_prep_queries_i8s(const float* q, uint32_t nq, uint32_t nq_pad, uint32_t dim, uint32_t KPB, int metric,
                                   const float* stats, const float* xxmax, unsigned char* qprep, float* qaux0, float* qaux1,
                                   float* delta, hipStream_t s) {
    hipLaunchKernelGGL(prep_queries_i8s_kernel, dim3(nq_pad), dim3(256), 0, s, q, nq, dim, KPB, metric, stats, xxmax, qprep, qaux0,
                       qaux1, delta);
    return hipGetLastError();
}

}  // namespace mvf
