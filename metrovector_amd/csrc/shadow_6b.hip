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
#include "scan_mfma.h"
#include "shadow_6b.h"
#include "shadow_5p1.h"

namespace mvf {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void atomic_max_nonneg6(float* dst, float v) {  // v >= 0 or +inf; NaN -> +inf
    if (!(v == v)) v = __uint_as_float(0x7F800000u);
    atomicMax(reinterpret_cast<unsigned int*>(dst), __float_as_uint(v));
}

// One wave per row, lane l taking element 64 u + l of unit u.  rows: Float32 at `pitch`; out: the tiled shadow (shadow_6b.h),
// xscale6[r] = s_r, stats[0..3] = max s_r(|x6|+|ex|), max s_r|ex|, the same two over |x| -- shadow_i8_kernel's four, from the
// measured |x6| and |ex|.  Every byte of the rows [0, n) is written (padding elements as the code of zero).
// P51: the same codes in the 5+1 layout (shadow_5p1.h) -- a lane quantises the elements 128 U + l and 128 U + 64 + l of unit U
// in the 6-bit kernel's order (the sums behind the bound maxima see the same operands in the same sequence: identical maxima).
template <bool P51>
__global__ void __launch_bounds__(256) shadow_6b_kernel(const unsigned char* rows, uint32_t n, uint32_t pitch, uint32_t dim,
                                                         unsigned char* rows6, float* xscale6, float* stats) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, nwaves = (gridDim.x * 256u) >> 6;
    const uint32_t units = s6_units(dim);
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f;
    for (uint32_t r = wave; r < n; r += nwaves) {
        const float* rp = reinterpret_cast<const float*>(rows + (size_t)r * pitch);
        float mx = 0.f, ss = 0.f;
        bool bad = false;
        for (uint32_t c = lane; c < dim; c += 64) {
            const float v = rp[c];
            bad |= !(fabsf(v) < 3.0e38f);
            mx = fmaxf(mx, fabsf(v));
            ss = fmaf(v, v, ss);
        }
        for (int off = 32; off > 0; off >>= 1) {
            mx = fmaxf(mx, __shfl_xor(mx, off, 64));
            ss += __shfl_xor(ss, off, 64);
        }
        bad = __builtin_amdgcn_ballot_w64(bad) != 0 || !(ss < 3.0e38f);
        const float sr = bad ? 0.f : mx / (float)kS6Max;
        float x2 = 0.f, e2 = 0.f;
        // the code of element c (padding: the code of zero); x2 / e2 take its terms
        auto quantise = [&](uint32_t c) __attribute__((always_inline)) -> uint32_t {
            const float x = c < dim ? rp[c] : 0.f;
            float t = sr > 0.f ? x / sr : 0.f;       // IEEE division: x = sr (t / (1 + eps)), |eps| <= 2^-24
            float q = rintf(t);
            q = fminf(fmaxf(q, -(float)kS6Max), (float)kS6Max);  // |t| <= 31 (1 + 2^-23): the clamp never bites beyond rounding
            const float e = t - q;
            x2 = fmaf(q, q, x2);
            e2 = fmaf(e, e, e2);
            return (uint32_t)((int)q + kS6Bias);
        };
        auto word_of = [&](uint32_t byte) __attribute__((always_inline)) -> uint32_t {  // the bytes of lanes l .. l + 3
            return byte | ((uint32_t)__shfl_down((int)byte, 1, 64) << 8) | ((uint32_t)__shfl_down((int)byte, 2, 64) << 16) |
                   ((uint32_t)__shfl_down((int)byte, 3, 64) << 24);
        };
        if constexpr (P51) {
            for (uint32_t u = 0; u < s51_units(dim); u++) {
                const uint32_t y0 = quantise(u * 128 + lane), y1 = quantise(u * 128 + 64 + lane);
                const uint32_t hi0 = y0 >> 1, hi1 = y1 >> 1, b = lane & 15u, pl = lane >> 4;
                // the 15 spare bits of byte b of the five planes: hi of the elements 80 + b, 96 + b, 112 + b (lanes 16 + b, 32 + b, 48 + b)
                const uint32_t sp = (uint32_t)__shfl((int)hi1, 16 + (int)b, 64) | ((uint32_t)__shfl((int)hi1, 32 + (int)b, 64) << 5) |
                                    ((uint32_t)__shfl((int)hi1, 48 + (int)b, 64) << 10);
                const uint32_t w = word_of(hi0 | (((sp >> (3u * pl)) & 7u) << 5));     // planes 0..3: element 16 pl + b
                const uint32_t w4 = word_of(hi1 | (((sp >> 12) & 7u) << 5));            // plane 4 (lanes 0..15): element 64 + b
                if ((lane & 3u) == 0) *reinterpret_cast<uint32_t*>(rows6 + s51_hi_offset(r, dim, u, pl) + b) = w;
                if (lane < 16 && (lane & 3u) == 0) *reinterpret_cast<uint32_t*>(rows6 + s51_hi_offset(r, dim, u, 4) + b) = w4;
                const unsigned long long l0 = __builtin_amdgcn_ballot_w64((y0 & 1u) != 0), l1 = __builtin_amdgcn_ballot_w64((y1 & 1u) != 0);
#pragma unroll
                for (uint32_t ph = 0; ph < 2; ph++) {  // lane l makes bit 64 ph + l of the lo plane
                    const uint32_t B = 64u * ph + lane, d = B >> 5, beta = B & 31u, i = 32u * d + 4u * (beta & 7u) + (beta >> 3);
                    const unsigned long long bits = __builtin_amdgcn_ballot_w64((((i < 64 ? l0 : l1) >> (i & 63u)) & 1ull) != 0);
                    if (lane == 0) *reinterpret_cast<unsigned long long*>(rows6 + s51_lo_offset(r, dim, u) + 8u * ph) = bits;
                }
            }
        } else
        for (uint32_t u = 0; u < units; u++) {
            const uint32_t y = quantise(u * 64 + lane);
            // lanes 0..47 hold the low six bits of byte (lane & 15) of plane lane / 16; its top two come from lane 48 + (lane & 15)
            const uint32_t yd = (uint32_t)__shfl((int)y, 48 + (int)(lane & 15u), 64);
            const uint32_t w = word_of(y | (((yd >> (2u * (lane >> 4))) & 3u) << 6));
            if (lane < 48 && (lane & 3u) == 0)
                *reinterpret_cast<uint32_t*>(rows6 + s6_offset(r, dim, u, lane >> 4) + (lane & 15u)) = w;
        }
        for (int off = 32; off > 0; off >>= 1) {
            x2 += __shfl_xor(x2, off, 64);
            e2 += __shfl_xor(e2, off, 64);
        }
        if (lane == 0) {
            xscale6[r] = sr;
            const float inf = __uint_as_float(0x7F800000u);
            // measured norms, inflated for the f32 sums above and the (1 + eps) of the division
            const float ex = sqrtf(e2) * 1.0005f + 1e-3f, xa = sqrtf(x2) * 1.0005f + ex;
            const float a = bad ? inf : sr * xa, b = bad ? inf : sr * ex;
            const float xn = sqrtf(ss);
            m0 = fmaxf(m0, a);
            m1 = fmaxf(m1, b);
            if (bad) m2 = m3 = inf;
            else if (xn > 0.f) {
                m2 = fmaxf(m2, a / xn * 1.000001f);
                m3 = fmaxf(m3, b / xn * 1.000001f);
            }
        }
    }
    if (lane == 0) {
        atomic_max_nonneg6(stats + 0, m0);
        atomic_max_nonneg6(stats + 1, m1);
        atomic_max_nonneg6(stats + 2, m2);
        atomic_max_nonneg6(stats + 3, m3);
    }
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
