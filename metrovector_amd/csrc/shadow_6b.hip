// shadow_6b.hip — the 6-BIT SHADOW of a Float32 corpus (selection only; ONE streamed query: api.hip, search_stream_qs_path).
//
// K1 over the int8 shadow runs at the part's read ceiling (profiles/r07_stream_fixed_cost.txt), so the only lever left on a
// one-query search of a large corpus is the bytes the scan reads: six bits per element instead of eight, 0.75 x.  Per row
// s_r = max|x| / 31, x6 = rint(x / s_r) in [-31, 31], stored as the code x6 + 32 in the tiled layout of shadow_6b.h.
//
// The bound is shadow_i8.hip's, with x6 for x8.  What changes is the QUERY.  With int8 queries the two terms of
//     |q.x - s_r s_q x6.Q| <= s_r s_q [ (|x6| + |ex|) |eq| + |ex| |Q| ]        (x = s_r (x6 + ex), q = s_q (Q + eq))
// are equal on the benchmark's rows -- half the margin pays for the query's rounding -- and at six bits the margin would hold
// ~11 000 rows of 10M x 768 at k = 100.  K1 is HBM-bound with the query in LDS and its VALU mostly idle, so its 6-bit unit
// takes the query at SIXTEEN bits (query_16s.h: Q = 128 hi + lo, two int8 planes, two exact i32 dot products per row):
// |eq| stays ~0.29 sqrt(dim) while |Q| grows 128-fold, the first term all but vanishes, and
//     delta = s_q (|eq| A + |Q| B) ~ |q| max_r s_r |ex|        (A, B: the corpus-wide maxima below; Cosine: over |x|)
// is 0.495 sigma of the score distribution on those rows (int8 rows and query: 0.229; 6-bit rows, int8 query: 0.604):
// ~5 300 rows inside 2 delta of the 100-th best of 10M.  The candidate path behind the scan is sized for that (api.hip:
// kStream6Cap), and stream_6b_shape keeps shapes whose margin is predicted to hold more than half of it on the int8 shadow.
//
// The scan's arithmetic.  The codes y = x6 + 32 are non-negative bytes, both query planes int8: acc_hi = hi.y and
// acc_lo = lo.y are exact i32 sums (v_dot4_i32_i8), and  Q.x6 = 128 acc_hi + acc_lo - 32 sum Q  is formed exactly in 64-bit
// integers, once per row, from the per-query constant 32 sum Q; ONE rounding takes it to f32.  The keys are the int8 unit's:
// dot s_r s_q; Cosine / (|q||x|); L2 in GEMM form.  The f32 evaluation term of delta is widened from 4e-7 to 6e-7 for the
// third rounding (query_16s.h).
// A row holding Inf / NaN makes the maxima +inf, as in shadow_i8.hip: the route then leaves such a corpus to the stored rows.

#include "../../include/mvf_gpu.h"
#include "../../include/mvf_gpu_stream_5p1.h"

#include "internal.h"
#include "mvf_common.h"
#include "row_builders.h"
#include "scan_mfma.h"
#include "shadow_6b.h"
#include "shadow_5p1.h"

namespace mvf {
namespace {

// One wave per row, lane l taking element 64 u + l of unit u.  rows: Float32 at `pitch`; out: the tiled shadow (shadow_6b.h),
// xscale6[r] = s_r, stats[0..3] = max s_r(|x6|+|ex|), max s_r|ex|, the same two over |x| -- shadow_i8_kernel's four, from the
// measured |x6| and |ex|.  Every byte of the rows [0, n) is written (padding elements as the code of zero).
// P51: the same codes in the 5+1 layout (shadow_5p1.h) -- a lane quantises the elements 128 U + l and 128 U + 64 + l of unit U
// in the 6-bit kernel's order (the sums behind the bound maxima see the same operands in the same sequence: identical maxima).
// The row's body is row_builders.h's shadow_6b_row, shared with the list-driven refresh of a row write (scan_update.hip).
template <bool P51>
__global__ void __launch_bounds__(256) shadow_6b_kernel(const unsigned char* rows, uint32_t n, uint32_t pitch, uint32_t dim,
                                                         unsigned char* rows6, float* xscale6, float* stats) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, nwaves = (gridDim.x * 256u) >> 6;
    ShadowMaxima m;
    for (uint32_t r = wave; r < n; r += nwaves) shadow_6b_row<P51>(rows, pitch, dim, rows6, xscale6, r, lane, m);
    fold_shadow_maxima(stats, lane, m);
}

}  // namespace

// rows6: s6_bytes(n, dim) bytes (p51: s51_bytes(n, dim), the 5+1 layout); the rows of the last tile behind row n - 1 are
// zeroed here, in front of the kernel
hipError_t launch_shadow_6b(const unsigned char* rows, uint32_t n, uint32_t pitch, uint32_t dim, unsigned char* rows6, float* xscale6,
                            float* stats, hipStream_t s, bool p51) {
    if (n == 0) return hipSuccess;
    const size_t tile = p51 ? s51_tile_bytes(dim) : s6_tile_bytes(dim);
    if (n % kS6TileRows) {
        hipError_t e = hipMemsetAsync(rows6 + (size_t)(n / kS6TileRows) * tile, 0, tile, s);
        if (e != hipSuccess) return e;
    }
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n + 3) / 4, 256u * 8u);
    if (p51) hipLaunchKernelGGL(shadow_6b_kernel<true>, dim3(blocks), dim3(256), 0, s, rows, n, pitch, dim, rows6, xscale6, stats);
    else hipLaunchKernelGGL(shadow_6b_kernel<false>, dim3(blocks), dim3(256), 0, s, rows, n, pitch, dim, rows6, xscale6, stats);
    return hipGetLastError();
}

}  // namespace mvf

extern "C" {

uint64_t mvfgpu_selftest_shadow6_bytes(uint64_t rows, uint32_t dimension) { return dimension ? (uint64_t)mvf::s6_bytes(rows, dimension) : 0; }

int mvfgpu_selftest_shadow6_pack(const int8_t* codes, uint64_t rows, uint32_t dimension, uint8_t* out, uint64_t out_bytes) {
    if (!codes || !out || dimension == 0) return mvf::set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer or empty dimension");
    if (out_bytes < mvf::s6_bytes(rows, dimension)) return mvf::set_fail(MVF_ERR_INVALID_ARGUMENT, "the output holds fewer bytes than the shadow of these rows");
    for (uint64_t i = 0; i < rows * (uint64_t)dimension; i++)
        if (codes[i] < -mvf::kS6Max || codes[i] > mvf::kS6Max) return mvf::set_fail(MVF_ERR_INVALID_ARGUMENT, "a 6-bit code lies in [-31, 31]");
    memset(out, 0, mvf::s6_bytes(rows, dimension));
    for (uint64_t r = 0; r < rows; r++) mvf::s6_pack_row(codes + r * dimension, dimension, r, out);
    return MVF_OK;
}

int mvfgpu_selftest_shadow6_unpack(const uint8_t* shadow, uint64_t shadow_bytes, uint64_t rows, uint32_t dimension, int8_t* out_codes) {
    if (!shadow || !out_codes || dimension == 0) return mvf::set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer or empty dimension");
    if (shadow_bytes < mvf::s6_bytes(rows, dimension)) return mvf::set_fail(MVF_ERR_INVALID_ARGUMENT, "fewer bytes than the shadow of these rows");
    for (uint64_t r = 0; r < rows; r++) mvf::s6_unpack_row(shadow, dimension, r, out_codes + r * dimension);
    return MVF_OK;
}

uint64_t mvfgpu_selftest_shadow51_bytes(uint64_t rows, uint32_t dimension) { return dimension ? (uint64_t)mvf::s51_bytes(rows, dimension) : 0; }

int mvfgpu_selftest_shadow51_pack(const int8_t* codes, uint64_t rows, uint32_t dimension, uint8_t* out, uint64_t out_bytes) {
    if (!codes || !out || dimension == 0) return mvf::set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer or empty dimension");
    if (out_bytes < mvf::s51_bytes(rows, dimension)) return mvf::set_fail(MVF_ERR_INVALID_ARGUMENT, "the output holds fewer bytes than the shadow of these rows");
    for (uint64_t i = 0; i < rows * (uint64_t)dimension; i++)
        if (codes[i] < -mvf::kS6Max || codes[i] > mvf::kS6Max) return mvf::set_fail(MVF_ERR_INVALID_ARGUMENT, "a 6-bit code lies in [-31, 31]");
    memset(out, 0, mvf::s51_bytes(rows, dimension));
    for (uint64_t r = 0; r < rows; r++) mvf::s51_pack_row(codes + r * dimension, dimension, r, out);
    return MVF_OK;
}

int mvfgpu_selftest_shadow51_unpack(const uint8_t* shadow, uint64_t shadow_bytes, uint64_t rows, uint32_t dimension, int8_t* out_codes) {
    if (!shadow || !out_codes || dimension == 0) return mvf::set_fail(MVF_ERR_INVALID_ARGUMENT, "NULL buffer or empty dimension");
    if (shadow_bytes < mvf::s51_bytes(rows, dimension)) return mvf::set_fail(MVF_ERR_INVALID_ARGUMENT, "fewer bytes than the shadow of these rows");
    for (uint64_t r = 0; r < rows; r++) mvf::s51_unpack_row(shadow, dimension, r, out_codes + r * dimension);
    return MVF_OK;
}

}  // extern "C"
