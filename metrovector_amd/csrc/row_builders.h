// row_builders.h — the per-row bodies of everything the library derives from a row's bytes: the row norms (K4), the scaled-f16
// shadow, the int8 shadow and the 6-bit shadow in either layout.  One wave per row; every output is addressed from the row
// number alone, and no row's output depends on another row.  Each body is stated ONCE here and driven twice: by the range
// kernels that build the state of a whole corpus (r = wave, wave + nwaves, ...: scan_mfma.hip, scan_mfma16_prep.hip,
// shadow_i8.hip, shadow_6b.hip) and by the list kernels that refresh it behind a row write (r = list[i]: scan_update.hip,
// DESIGN.md §5 "W0 / W1").  The corpus-wide maxima travel through the caller's accumulators and are folded with atomicMax by
// both drivers (fold_* below): a maximum is raised by a refreshed row and never lowered.
#pragma once

#include "mvf_common.h"
#include "shadow_5p1.h"
#include "shadow_6b.h"

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

namespace mvf {

typedef uint32_t rb_u32x4 __attribute__((ext_vector_type(4)));
typedef float rb_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void rb_atomic_max_nonneg(float* dst, float v) {  // v >= 0 or +inf; NaN -> +inf
    if (!(v == v)) v = __uint_as_float(0x7F800000u);
    atomicMax(reinterpret_cast<unsigned int*>(dst), __float_as_uint(v));
}

// ---- K4: row norms -----------------------------------------------------------------------------------------------
// Float32 rows: xnorm[r] = sqrt(sum x^2), xx2[r] = sum x^2; mx = the wave's largest sum so far (lane 0's is the one folded)
__device__ __forceinline__ void norms_f32_row(const unsigned char* rows, uint32_t pitch, uint32_t V, uint32_t r, uint32_t lane,
                                              float* xnorm, float* xx2, float& mx) {
    const unsigned char* rp = rows + (size_t)r * pitch;
    float s = 0.f;
    for (uint32_t v = lane; v < V; v += 64) {
        const rb_f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const rb_f32x4*>(rp + (size_t)v * 16));
        s = fmaf(x[0], x[0], s);
        s = fmaf(x[1], x[1], s);
        s = fmaf(x[2], x[2], s);
        s = fmaf(x[3], x[3], s);
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) {
        xnorm[r] = sqrtf(s);
        xx2[r] = s;
        if (s > mx) mx = s;  // NaN never wins: the margin uses finite rows only
    }
}

// Float16 rows: the same three
__device__ __forceinline__ void norms_f16_row(const unsigned char* rows, uint32_t pitch, uint32_t V, uint32_t r, uint32_t lane,
                                              float* xnorm, float* xx2, float& mx) {
    const unsigned char* rp = rows + (size_t)r * pitch;
    float s = 0.f;
    for (uint32_t v = lane; v < V; v += 64) {
        const rb_u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const rb_u32x4*>(rp + (size_t)v * 16));
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const float a = __half2float(__ushort_as_half((unsigned short)(x[w] & 0xFFFFu)));
            const float b2 = __half2float(__ushort_as_half((unsigned short)(x[w] >> 16)));
            s = fmaf(a, a, s);
            s = fmaf(b2, b2, s);
        }
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) {
        xnorm[r] = sqrtf(s);
        xx2[r] = s;
        if (s > mx) mx = s;
    }
}

// the fold of the float norms' maximum: non-negative floats order as uints
__device__ __forceinline__ void fold_norm_max(float* xxmax, uint32_t lane, float mx) {
    if (lane == 0 && mx > 0.f) atomicMax(reinterpret_cast<unsigned int*>(xxmax), __float_as_uint(mx));
}

// Int8 rows: xx[r] = sum x^2 (i32)
__device__ __forceinline__ void norms_i8_row(const unsigned char* rows, uint32_t pitch, uint32_t V, uint32_t r, uint32_t lane,
                                             int32_t* xx) {
    const unsigned char* rp = rows + (size_t)r * pitch;
    int s = 0;
    for (uint32_t v = lane; v < V; v += 64) {
        const rb_u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const rb_u32x4*>(rp + (size_t)v * 16));
#pragma unroll
        for (int w = 0; w < 4; w++) s = __builtin_amdgcn_sdot4((int)x[w], (int)x[w], s, false);
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) xx[r] = s;
}

// UInt8 rows: xx[r] = sum (x-128)^2, xbias[r] = 128 * sum (x-128), over the row's REAL elements
__device__ __forceinline__ void norms_u8_row(const unsigned char* rows, uint32_t pitch, uint32_t V, uint32_t dim, uint32_t r,
                                             uint32_t lane, int32_t* xx, int32_t* xbias) {
    const unsigned char* rp = rows + (size_t)r * pitch;
    int s2 = 0, s1 = 0;
    for (uint32_t v = lane; v < V; v += 64) {
        const rb_u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const rb_u32x4*>(rp + (size_t)v * 16));
#pragma unroll
        for (int w = 0; w < 4; w++) {
            // bytes past `dim` inside the last vector are zero padding: keep them 0 in the signed domain too
            const uint32_t e0 = v * 16 + w * 4;
            uint32_t mask = e0 + 4 <= dim ? 0xFFFFFFFFu : e0 >= dim ? 0u : (0xFFFFFFFFu >> (8 * (4 - (dim - e0))));
            const uint32_t xs = (x[w] ^ 0x80808080u) & mask;
            s2 = __builtin_amdgcn_sdot4((int)xs, (int)xs, s2, false);
            s1 = __builtin_amdgcn_sdot4((int)xs, 0x01010101, s1, false);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        s2 += __shfl_xor(s2, off, 64);
        s1 += __shfl_xor(s1, off, 64);
    }
    if (lane == 0) {
        xx[r] = s2;
        xbias[r] = 128 * s1;
    }
}

// ---- the scaled-f16 shadow of a Float32 row (scan_mfma16_prep.hip, shadow_f16_kernel) -----------------------------
__device__ __forceinline__ void shadow_f16_row(const unsigned char* rows32, uint32_t pitch32, unsigned char* rows16,
                                               uint32_t pitch16, float* xscale, uint32_t r, uint32_t lane) {
    const uint32_t V32 = pitch32 / 16, V16 = pitch16 / 16;
    const unsigned char* rp = rows32 + (size_t)r * pitch32;
    float mx = 0.f;
    for (uint32_t v = lane; v < V32; v += 64) {
        const rb_u32x4 x = *reinterpret_cast<const rb_u32x4*>(rp + (size_t)v * 16);
#pragma unroll
        for (int w = 0; w < 4; w++) mx = fmaxf(mx, fabsf(__uint_as_float(x[w])));
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    int sh = 0;
    if (mx > 0.f && mx < 3.0e38f) {
        int ex;
        (void)frexpf(mx, &ex);  // mx = m * 2^ex, m in [0.5, 1)
        sh = 15 - ex;
    }
    unsigned char* op = rows16 + (size_t)r * pitch16;
    for (uint32_t v = lane; v < V16; v += 64) {  // one 16-B f16 vector = two f32 vectors
        rb_u32x4 o;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t v32 = 2 * v + h;
            rb_u32x4 x = rb_u32x4{0, 0, 0, 0};
            if (v32 < V32) x = *reinterpret_cast<const rb_u32x4*>(rp + (size_t)v32 * 16);  // f32 padding is zero
#pragma unroll
            for (int w = 0; w < 2; w++) {
                const unsigned short lo = __half_as_ushort(__float2half_rn(ldexpf(__uint_as_float(x[2 * w]), sh)));
                const unsigned short hi = __half_as_ushort(__float2half_rn(ldexpf(__uint_as_float(x[2 * w + 1]), sh)));
                o[2 * h + w] = (uint32_t)lo | ((uint32_t)hi << 16);
            }
        }
        *reinterpret_cast<rb_u32x4*>(op + (size_t)v * 16) = o;
    }
    if (lane == 0) xscale[r] = ldexpf(1.0f, -sh);
}

// ---- the bound maxima of the int8 and the 6-bit shadow -------------------------------------------------------------
// lane 0's running maxima of a wave: max s_r(|xq|+|ex|), max s_r|ex|, the same two over |x| (shadow_i8.hip)
struct ShadowMaxima {
    float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f;
};
// one row's terms, from the measured sums x2 = sum xq^2, e2 = sum ex^2 and ss = sum x^2 (lane 0)
__device__ __forceinline__ void shadow_maxima_row(ShadowMaxima& m, bool bad, float sr, float x2, float e2, float ss) {
    const float inf = __uint_as_float(0x7F800000u);
    // measured norms, inflated for the f32 sums above and the (1 + eps) of the division
    const float ex = sqrtf(e2) * 1.0005f + 1e-3f, xa = sqrtf(x2) * 1.0005f + ex;
    const float a = bad ? inf : sr * xa, b = bad ? inf : sr * ex;
    const float xn = sqrtf(ss);
    m.m0 = fmaxf(m.m0, a);
    m.m1 = fmaxf(m.m1, b);
    if (bad) m.m2 = m.m3 = inf;
    else if (xn > 0.f) {
        m.m2 = fmaxf(m.m2, a / xn * 1.000001f);
        m.m3 = fmaxf(m.m3, b / xn * 1.000001f);
    }
}
__device__ __forceinline__ void fold_shadow_maxima(float* stats, uint32_t lane, const ShadowMaxima& m) {
    if (lane == 0) {
        rb_atomic_max_nonneg(stats + 0, m.m0);
        rb_atomic_max_nonneg(stats + 1, m.m1);
        rb_atomic_max_nonneg(stats + 2, m.m2);
        rb_atomic_max_nonneg(stats + 3, m.m3);
    }
}

// ---- the int8 shadow of a Float32 / Float16 row (shadow_i8.hip) ------------------------------------------------------
template <int SRC>
__device__ __forceinline__ void shadow_i8_row(const unsigned char* rows, uint32_t pitch, uint32_t dim, unsigned char* rows8,
                                              uint32_t pitch8, float* xscale8, uint32_t r, uint32_t lane, ShadowMaxima& m) {
    const uint32_t V8 = pitch8 / 16;
    auto elem = [&](const unsigned char* rp, uint32_t c) __attribute__((always_inline)) -> float {
        if (c >= dim) return 0.f;
        if (SRC == MVF_DTYPE_FLOAT32) return reinterpret_cast<const float*>(rp)[c];
        return __half2float(reinterpret_cast<const __half*>(rp)[c]);
    };
    const unsigned char* rp = rows + (size_t)r * pitch;
    float mx = 0.f, ss = 0.f;
    bool bad = false;
    for (uint32_t c = lane; c < dim; c += 64) {
        const float v = elem(rp, c);
        bad |= !(fabsf(v) < 3.0e38f);
        mx = fmaxf(mx, fabsf(v));
        ss = fmaf(v, v, ss);
    }
    for (int off = 32; off > 0; off >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        ss += __shfl_xor(ss, off, 64);
    }
    bad = __builtin_amdgcn_ballot_w64(bad) != 0 || !(ss < 3.0e38f);
    const float sr = bad ? 0.f : mx / 127.0f;
    float x2 = 0.f, e2 = 0.f;
    for (uint32_t v8 = lane; v8 < V8; v8 += 64) {
        uint32_t w[4] = {0, 0, 0, 0};
        float xs[16];
        if (v8 * 16 + 16 <= dim) {  // whole vectors: 16-byte loads (the row pitch is a multiple of 16)
            if (SRC == MVF_DTYPE_FLOAT32) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const rb_u32x4 x = *reinterpret_cast<const rb_u32x4*>(rp + (size_t)v8 * 64 + k * 16);
#pragma unroll
                    for (int i = 0; i < 4; i++) xs[4 * k + i] = __uint_as_float(x[i]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const rb_u32x4 x = *reinterpret_cast<const rb_u32x4*>(rp + (size_t)v8 * 32 + k * 16);
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        xs[8 * k + 2 * i] = __half2float(__ushort_as_half((unsigned short)(x[i] & 0xFFFFu)));
                        xs[8 * k + 2 * i + 1] = __half2float(__ushort_as_half((unsigned short)(x[i] >> 16)));
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) xs[i] = elem(rp, v8 * 16 + i);
        }
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const float x = xs[i];
            float t = sr > 0.f ? x / sr : 0.f;     // IEEE division: x = sr (t / (1 + eps)), |eps| <= 2^-24
            float q = rintf(t);
            q = fminf(fmaxf(q, -127.f), 127.f);     // |t| <= 127 (1 + 2^-23): the clamp never bites beyond rounding
            const float e = t - q;
            x2 = fmaf(q, q, x2);
            e2 = fmaf(e, e, e2);
            w[i >> 2] |= (uint32_t)(uint8_t)(int8_t)(int)q << (8 * (i & 3));
        }
        *reinterpret_cast<rb_u32x4*>(rows8 + (size_t)r * pitch8 + (size_t)v8 * 16) = rb_u32x4{w[0], w[1], w[2], w[3]};
    }
    for (int off = 32; off > 0; off >>= 1) {
        x2 += __shfl_xor(x2, off, 64);
        e2 += __shfl_xor(e2, off, 64);
    }
    if (lane == 0) {
        xscale8[r] = sr;
        shadow_maxima_row(m, bad, sr, x2, e2, ss);
    }
}

// ---- the 6-bit shadow of a Float32 row (shadow_6b.hip), P51: in the 5+1 layout (shadow_5p1.h) ---------------------------
// A row owns its 16-byte slots of each plane of its tile (s6_offset, s51_hi_offset, s51_lo_offset): no read-modify-write.
template <bool P51>
__device__ __forceinline__ void shadow_6b_row(const unsigned char* rows, uint32_t pitch, uint32_t dim, unsigned char* rows6,
                                              float* xscale6, uint32_t r, uint32_t lane, ShadowMaxima& m) {
    const uint32_t units = s6_units(dim);
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
        shadow_maxima_row(m, bad, sr, x2, e2, ss);
    }
}

}  // namespace mvf
