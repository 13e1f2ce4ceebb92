// scan_radius.hip — R1 (the streaming radius scan) and R2 (ordering + packing of the per-query match lists).
//
// R1 reads the rows exactly as K1 does (scan_stream.inc): G lanes per row, each lane owning the 16-B vectors
// v = j*G + sub, U = 4 row groups in flight per wave, non-temporal 16-B loads, the query staged in LDS (f32 / packed
// int8), Float16 widened exactly, sdot4 / udot4 for Int8 / UInt8 rows.  The per-lane accumulation order, the G-lane
// pairing of the partial sums and the score -> key arithmetic are K1's, so for the same lane-group width the keys are
// bit-identical to those the top-k path ranks.  The epilogue differs: there is no running threshold, the bound is
// fixed per query, and every row whose key is <= the bound -- and whose tombstone bit is clear, read only for such
// rows -- is counted with ONE returning atomic per wave, query and row group that has a match (ballot + mbcnt give
// every matching lane its slot).  A query's list holds `cap` composites; the counter keeps counting past it.
//
// Algorithmic HBM bytes: rows * pitch per pass (+ 8 bytes per match).

#include "scan_radius.h"
#include "bitonic.h"
#include "k1_rowscore.h"
#include "mvf_common.h"

#include <hip/hip_fp16.h>

#include <type_traits>

namespace mvf {
namespace {

template <int DT> struct RTraits;
template <> struct RTraits<MVF_DTYPE_FLOAT32> { static constexpr int ES = 4; static constexpr bool INT = false; using Q = float; using Acc = float; };
template <> struct RTraits<MVF_DTYPE_FLOAT16> { static constexpr int ES = 2; static constexpr bool INT = false; using Q = float; using Acc = float; };
template <> struct RTraits<MVF_DTYPE_INT8> { static constexpr int ES = 1; static constexpr bool INT = true; using Q = int8_t; using Acc = int32_t; };
template <> struct RTraits<MVF_DTYPE_UINT8> { static constexpr int ES = 1; static constexpr bool INT = true; using Q = uint8_t; using Acc = int32_t; };

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int G, typename T>
__device__ __forceinline__ T rgroup_sum(T v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Wave-aggregated append: every lane with `hit` gets a slot of the query's list; one returning atomic per wave.
// Must be reached by the whole wave (the ballot).
__device__ __forceinline__ void radius_append(bool hit, uint64_t comp, uint32_t* cnt, uint64_t* list, uint32_t cap, int lane) {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
    if (m == 0) return;
    const int lead = __builtin_ctzll(m);
    uint32_t base = 0;
    if (lane == lead) base = atomicAdd(cnt, (uint32_t)__builtin_popcountll(m));
    if (!list) return;  // counting only: the list is never touched
    base = __shfl(base, lead, 64);
    const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (hit && slot < cap) list[slot] = comp;
}

template <int DT, int METRIC, int G, int NQ>
__global__ void __launch_bounds__(256) radius_scan_kernel(RadiusParams p) {
    using Tr = RTraits<DT>;
    using Acc = typename Tr::Acc;
    constexpr int ES = Tr::ES;
    constexpr int EPV = 16 / ES;
    constexpr int RPG = 64 / G;
    constexpr int U = 4;
    constexpr int QB = Tr::INT ? 16 : EPV * 4;
    constexpr bool NEED_XX = (METRIC == MVF_METRIC_COSINE) || (Tr::INT && METRIC == MVF_METRIC_L2);

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane % G, rsel = lane / G;

    const uint32_t VP = p.J * G;
    unsigned char* qs = smem;
    const uint32_t qstride = VP * QB;
    Acc* red = reinterpret_cast<Acc*>(smem + ((NQ * qstride + 15u) & ~15u));  // [NQ][4] qq partials

    const uint32_t q0 = p.q0 + blockIdx.y * NQ;
    bool qvalid[NQ];
    uint32_t bnd[NQ];
    // ---- stage the queries in LDS, zero padded; the sums of squares in K1's order
    Acc qq_part[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        qq_part[q] = 0;
        qvalid[q] = q0 + q < p.nq_total;
        bnd[q] = qvalid[q] ? p.bound[q0 + q] : 0u;
    }
    {
        const uint32_t nelem = VP * EPV;
        using QT = typename std::conditional<Tr::INT, typename Tr::Q, float>::type;
        const QT* src[NQ];
        QT* dst[NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const uint32_t qi = qvalid[q] ? q0 + q : p.nq_total - 1;  // padding lanes repeat the last query (never counted)
            src[q] = reinterpret_cast<const QT*>(p.queries) + (size_t)qi * p.dim;
            dst[q] = reinterpret_cast<QT*>(qs + q * qstride);
        }
        for (uint32_t e = tid; e < nelem; e += 256) {
            QT v[NQ];
#pragma unroll
            for (int q = 0; q < NQ; q++) v[q] = e < p.dim ? src[q][e] : (QT)0;
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                dst[q][e] = v[q];
                if constexpr (Tr::INT) qq_part[q] += (int32_t)v[q] * (int32_t)v[q];
                else qq_part[q] = fmaf(v[q], v[q], qq_part[q]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        Acc s = rgroup_sum<64>(qq_part[q]);
        if (lane == 0) red[q * 4 + wave] = s;
    }
    __syncthreads();
    Acc qq[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) qq[q] = red[q * 4 + 0] + red[q * 4 + 1] + red[q * 4 + 2] + red[q * 4 + 3];

    auto make_key = [&](Acc s, Acc xxs, Acc qqv) __attribute__((always_inline)) -> uint32_t {
        if constexpr (Tr::INT) {
            if constexpr (METRIC == MVF_METRIC_L2) return key_from_raw(qqv + xxs - 2 * s, METRIC);
            else if constexpr (METRIC == MVF_METRIC_INNER_PRODUCT) return key_from_raw(s, METRIC);
            else {
                const float den = sqrtf((float)qqv) * sqrtf((float)xxs);
                return key_from_score(den > 0.0f ? (float)s / den : 0.0f, METRIC);
            }
        } else {
            float sc;
            if constexpr (METRIC == MVF_METRIC_L2) sc = sqrtf(s);
            else if constexpr (METRIC == MVF_METRIC_INNER_PRODUCT) sc = s;
            else {
                const float den = sqrtf(qqv) * sqrtf(xxs);
                sc = den > 0.0f ? s / den : 0.0f;
            }
            return key_from_score(sc, METRIC);
        }
    };
    auto live = [&](uint32_t r) __attribute__((always_inline)) -> bool {
        return !(p.tomb && ((p.tomb[r >> 5] >> (r & 31)) & 1u));
    };

    const uint32_t ngroups = (p.n + RPG - 1) / RPG;
    const uint32_t wstride = gridDim.x * 4u * U;
    for (uint32_t g0 = (blockIdx.x * 4u + wave) * U; g0 < ngroups; g0 += wstride) {
        uint32_t r[U];
        bool rv[U];
        const unsigned char* rp[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            r[u] = (g0 + u) * RPG + rsel;
            rv[u] = r[u] < p.n;
            rp[u] = p.rows + (size_t)(rv[u] ? r[u] : 0u) * p.pitch;
        }
        Acc acc[U][NQ];
        Acc xx[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            xx[u] = 0;
#pragma unroll
            for (int q = 0; q < NQ; q++) acc[u][q] = 0;
        }
        for (uint32_t j = 0; j < p.J; j++) {
            const uint32_t v = j * G + sub;
            const bool vv = v < p.V;
            u32x4 x[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                x[u] = u32x4{0, 0, 0, 0};
                if (vv && rv[u]) x[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(rp[u] + (size_t)v * 16));
            }
            if constexpr (DT == MVF_DTYPE_FLOAT32) {
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    const float4 qv = *reinterpret_cast<const float4*>(qs + q * qstride + v * 16);
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        const float x0 = __uint_as_float(x[u].x), x1 = __uint_as_float(x[u].y),
                                    x2 = __uint_as_float(x[u].z), x3 = __uint_as_float(x[u].w);
                        if constexpr (METRIC == MVF_METRIC_L2) {
                            float t0 = qv.x - x0, t1 = qv.y - x1, t2 = qv.z - x2, t3 = qv.w - x3;
                            acc[u][q] = fmaf(t0, t0, acc[u][q]);
                            acc[u][q] = fmaf(t1, t1, acc[u][q]);
                            acc[u][q] = fmaf(t2, t2, acc[u][q]);
                            acc[u][q] = fmaf(t3, t3, acc[u][q]);
                        } else {
                            acc[u][q] = fmaf(qv.x, x0, acc[u][q]);
                            acc[u][q] = fmaf(qv.y, x1, acc[u][q]);
                            acc[u][q] = fmaf(qv.z, x2, acc[u][q]);
                            acc[u][q] = fmaf(qv.w, x3, acc[u][q]);
                        }
                    }
                }
                if constexpr (NEED_XX) {
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        const float x0 = __uint_as_float(x[u].x), x1 = __uint_as_float(x[u].y),
                                    x2 = __uint_as_float(x[u].z), x3 = __uint_as_float(x[u].w);
                        xx[u] = fmaf(x0, x0, xx[u]);
                        xx[u] = fmaf(x1, x1, xx[u]);
                        xx[u] = fmaf(x2, x2, xx[u]);
                        xx[u] = fmaf(x3, x3, xx[u]);
                    }
                }
            } else if constexpr (DT == MVF_DTYPE_FLOAT16) {
                float xf[U][8];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t w[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        xf[u][2 * i] = __half2float(__ushort_as_half((unsigned short)(w[i] & 0xFFFFu)));
                        xf[u][2 * i + 1] = __half2float(__ushort_as_half((unsigned short)(w[i] >> 16)));
                    }
                }
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    const float4 qa = *reinterpret_cast<const float4*>(qs + q * qstride + v * 32);
                    const float4 qb = *reinterpret_cast<const float4*>(qs + q * qstride + v * 32 + 16);
                    const float qf[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
#pragma unroll
                    for (int u = 0; u < U; u++) {
#pragma unroll
                        for (int i = 0; i < 8; i++) {
                            if constexpr (METRIC == MVF_METRIC_L2) {
                                float t = qf[i] - xf[u][i];
                                acc[u][q] = fmaf(t, t, acc[u][q]);
                            } else {
                                acc[u][q] = fmaf(qf[i], xf[u][i], acc[u][q]);
                            }
                        }
                    }
                }
                if constexpr (NEED_XX) {
#pragma unroll
                    for (int u = 0; u < U; u++)
#pragma unroll
                        for (int i = 0; i < 8; i++) xx[u] = fmaf(xf[u][i], xf[u][i], xx[u]);
                }
            } else {  // Int8 / UInt8: exact i32
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    const uint4 qv = *reinterpret_cast<const uint4*>(qs + q * qstride + v * 16);
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        if constexpr (DT == MVF_DTYPE_INT8) {
                            acc[u][q] = __builtin_amdgcn_sdot4((int)qv.x, (int)x[u].x, acc[u][q], false);
                            acc[u][q] = __builtin_amdgcn_sdot4((int)qv.y, (int)x[u].y, acc[u][q], false);
                            acc[u][q] = __builtin_amdgcn_sdot4((int)qv.z, (int)x[u].z, acc[u][q], false);
                            acc[u][q] = __builtin_amdgcn_sdot4((int)qv.w, (int)x[u].w, acc[u][q], false);
                        } else {
                            acc[u][q] = (int32_t)__builtin_amdgcn_udot4(qv.x, x[u].x, (uint32_t)acc[u][q], false);
                            acc[u][q] = (int32_t)__builtin_amdgcn_udot4(qv.y, x[u].y, (uint32_t)acc[u][q], false);
                            acc[u][q] = (int32_t)__builtin_amdgcn_udot4(qv.z, x[u].z, (uint32_t)acc[u][q], false);
                            acc[u][q] = (int32_t)__builtin_amdgcn_udot4(qv.w, x[u].w, (uint32_t)acc[u][q], false);
                        }
                    }
                }
                if constexpr (NEED_XX) {
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        if constexpr (DT == MVF_DTYPE_INT8) {
                            xx[u] = __builtin_amdgcn_sdot4((int)x[u].x, (int)x[u].x, xx[u], false);
                            xx[u] = __builtin_amdgcn_sdot4((int)x[u].y, (int)x[u].y, xx[u], false);
                            xx[u] = __builtin_amdgcn_sdot4((int)x[u].z, (int)x[u].z, xx[u], false);
                            xx[u] = __builtin_amdgcn_sdot4((int)x[u].w, (int)x[u].w, xx[u], false);
                        } else {
                            xx[u] = (int32_t)__builtin_amdgcn_udot4(x[u].x, x[u].x, (uint32_t)xx[u], false);
                            xx[u] = (int32_t)__builtin_amdgcn_udot4(x[u].y, x[u].y, (uint32_t)xx[u], false);
                            xx[u] = (int32_t)__builtin_amdgcn_udot4(x[u].z, x[u].z, (uint32_t)xx[u], false);
                            xx[u] = (int32_t)__builtin_amdgcn_udot4(x[u].w, x[u].w, (uint32_t)xx[u], false);
                        }
                    }
                }
            }
        }

        // ---- finish the rows: G-lane sums, key, the bound, the tombstone bit (matches only), the append
        if constexpr (NQ == 1 && G >= 4) {
            // K1's reduce-scatter over the four rows of a group: lane `sub` ends with the total of row u = (h0, h1) and
            // computes one key; the pairing of the partial sums is the butterfly's (bit-identical totals)
            const bool h0 = (sub & (G / 2)) != 0, h1 = (sub & (G / 4)) != 0;
            const int ul = (h0 ? 2 : 0) + (h1 ? 1 : 0);
            Acc v2[2], s1;
#pragma unroll
            for (int i = 0; i < 2; i++) v2[i] = (h0 ? acc[i + 2][0] : acc[i][0]) + __shfl_xor(h0 ? acc[i][0] : acc[i + 2][0], G / 2, 64);
            s1 = (h1 ? v2[1] : v2[0]) + __shfl_xor(h1 ? v2[0] : v2[1], G / 4, 64);
#pragma unroll
            for (int off = G / 8; off > 0; off >>= 1) s1 += __shfl_xor(s1, off, 64);
            Acc xx1 = 0;
            if constexpr (NEED_XX) {
                Acc x2[2];
#pragma unroll
                for (int i = 0; i < 2; i++) x2[i] = (h0 ? xx[i + 2] : xx[i]) + __shfl_xor(h0 ? xx[i] : xx[i + 2], G / 2, 64);
                xx1 = (h1 ? x2[1] : x2[0]) + __shfl_xor(h1 ? x2[0] : x2[1], G / 4, 64);
#pragma unroll
                for (int off = G / 8; off > 0; off >>= 1) xx1 += __shfl_xor(xx1, off, 64);
            }
            const uint32_t rl = (g0 + ul) * RPG + rsel;
            const uint32_t key = make_key(s1, xx1, qq[0]);
            const bool hit = (sub & (G / 4 - 1)) == 0 && rl < p.n && qvalid[0] && key <= bnd[0] && live(rl);
            radius_append(hit, ((uint64_t)key << 32) | rl, p.counts + q0, p.lists ? p.lists + (size_t)q0 * p.cap : nullptr, p.cap, lane);
        } else {
#pragma unroll
            for (int u = 0; u < U; u++) {
                Acc xxs = 0;
                if constexpr (NEED_XX) xxs = rgroup_sum<G>(xx[u]);
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    const Acc s = rgroup_sum<G>(acc[u][q]);
                    const uint32_t key = make_key(s, xxs, qq[q]);
                    const bool hit = sub == 0 && rv[u] && qvalid[q] && key <= bnd[q] && live(r[u]);
                    radius_append(hit, ((uint64_t)key << 32) | r[u], p.counts + q0 + q,
                                  p.lists ? p.lists + (size_t)(q0 + q) * p.cap : nullptr, p.cap, lane);
                }
            }
        }
    }
}

// R2: grid (nq), block 1024, dynamic LDS cap * 8 bytes
__global__ void __launch_bounds__(1024) radius_pack_kernel(RadiusPackParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* buf = reinterpret_cast<uint64_t*>(smem);
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t cnt = p.counts[q];
    if (cnt > p.cap) return;  // the list lost arrivals: the host completes this query through the top-k identity
    const uint32_t m = cnt, P = next_pow2(m ? m : 1u);
    const uint64_t* list = p.lists + (size_t)q * p.cap;
    for (uint32_t i = tid; i < P; i += 1024) buf[i] = i < m ? list[i] : kPadComposite;
    __syncthreads();
    bitonic_sort_u64<1024>(buf, P, (int)tid);
    const uint32_t w = min(m, p.kout);
    const bool raw_keys = key_is_raw(p.dtype, p.metric);
    for (uint32_t i = tid; i < w; i += 1024) {
        const uint64_t comp = buf[i];
        const uint32_t key = (uint32_t)(comp >> 32), row = (uint32_t)comp;
        const size_t o = (size_t)q * p.kout + i;
        float s;
        int32_t raw = 0;
        if (raw_keys) {
            raw = raw_from_key(key, p.metric);
            s = p.metric == MVF_METRIC_L2 ? sqrtf((float)raw) : (float)raw;
        } else {
            s = score_from_key(key, p.metric);
        }
        p.out_scores[o] = s;
        p.out_indices[o] = p.ids ? p.ids[row] : p.index_base + row;
        p.out_raw[o] = raw;
    }
}

// R3: grid (nq), block 256, dynamic LDS radius_scan_lds_bytes(Float32, G, J, 1).  The per-row arithmetic is K1's, from
// k1_rowscore.h (shared with the int8-shadow stream's re-scoring); the query's sum of squares is staged in K1's order below.
template <int METRIC, int G>
__global__ void __launch_bounds__(256) radius_rescore_kernel(RadiusRescoreParams p) {
    constexpr int RPG = 64 / G;
    constexpr bool NEED_XX = METRIC == MVF_METRIC_COSINE;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane % G, rsel = lane / G;
    const uint32_t q = blockIdx.x;
    const uint32_t VP = p.J * G;
    float* qs = reinterpret_cast<float*>(smem);
    float* red = reinterpret_cast<float*>(smem + ((VP * 16u + 15u) & ~15u));
    // the query in LDS and its sum of squares, in R1's (K1's) order
    float qq_part = 0.0f;
    for (uint32_t e = tid; e < VP * 4u; e += 256) {
        const float v = e < p.dim ? p.queries[(size_t)q * p.dim + e] : 0.0f;
        qs[e] = v;
        qq_part = fmaf(v, v, qq_part);
    }
    const float qsum = rgroup_sum<64>(qq_part);
    if (lane == 0) red[wave] = qsum;
    __syncthreads();
    const float qq = red[0] + red[1] + red[2] + red[3];
    const uint32_t bnd = p.bound[q];
    const uint32_t m = min(p.ccnt[q], p.ccap);
    const uint64_t* cand = p.cand + (size_t)q * p.ccap;
    uint64_t* list = p.lists ? p.lists + (size_t)q * p.cap : nullptr;
    for (uint32_t b = (uint32_t)wave * RPG; b < m; b += 4u * RPG) {  // wave-uniform bound: every lane reaches the ballot
        const uint32_t ci = b + rsel;
        const uint64_t c0 = ci < m ? cand[ci] : kPadComposite;
        const bool ok = c0 != kPadComposite;
        const uint32_t row = (uint32_t)c0;
        const unsigned char* rp = p.rows + (size_t)(ok ? row : 0u) * p.pitch;
        float acc = 0.0f, xx = 0.0f;
        for (uint32_t j = 0; j < p.J; j++) {
            const uint32_t v = j * G + sub;
            k1::u32x4 x = k1::u32x4{0, 0, 0, 0};
            if (ok && v < p.V) x = *reinterpret_cast<const k1::u32x4*>(rp + (size_t)v * 16);
            const float4 qv = *reinterpret_cast<const float4*>(qs + v * 4);
            acc = k1::acc4<METRIC>(acc, qv, x);
            if constexpr (NEED_XX) xx = k1::xx4(xx, x);
        }
        const float s = k1::group_sum<G>(acc);
        const float xxs = NEED_XX ? k1::group_sum<G>(xx) : 0.0f;
        const uint32_t key = k1::key<METRIC>(s, xxs, qq);
        const bool hit = sub == 0 && ok && key <= bnd;
        radius_append(hit, ((uint64_t)key << 32) | row, p.counts + q, list, p.cap, lane);
    }
}

template <int METRIC>
const void* pick_rescore(int G) {
    switch (G) {
        case 1: return reinterpret_cast<const void*>(&radius_rescore_kernel<METRIC, 1>);
        case 4: return reinterpret_cast<const void*>(&radius_rescore_kernel<METRIC, 4>);
        case 8: return reinterpret_cast<const void*>(&radius_rescore_kernel<METRIC, 8>);
        case 16: return reinterpret_cast<const void*>(&radius_rescore_kernel<METRIC, 16>);
        case 32: return reinterpret_cast<const void*>(&radius_rescore_kernel<METRIC, 32>);
        case 64: return reinterpret_cast<const void*>(&radius_rescore_kernel<METRIC, 64>);
        default: return nullptr;
    }
}

template <int DT, int METRIC, int NQ>
const void* pick_g(int G) {
    switch (G) {
        case 1: return reinterpret_cast<const void*>(&radius_scan_kernel<DT, METRIC, 1, NQ>);
        case 4: return reinterpret_cast<const void*>(&radius_scan_kernel<DT, METRIC, 4, NQ>);
        case 8: return reinterpret_cast<const void*>(&radius_scan_kernel<DT, METRIC, 8, NQ>);
        case 16: return reinterpret_cast<const void*>(&radius_scan_kernel<DT, METRIC, 16, NQ>);
        case 32: return reinterpret_cast<const void*>(&radius_scan_kernel<DT, METRIC, 32, NQ>);
        case 64: return reinterpret_cast<const void*>(&radius_scan_kernel<DT, METRIC, 64, NQ>);
        default: return nullptr;
    }
}

template <int DT, int METRIC>
const void* pick_nq(int G, int nqv) {
    return nqv == 4 ? pick_g<DT, METRIC, 4>(G) : nqv == 1 ? pick_g<DT, METRIC, 1>(G) : nullptr;
}

template <int DT>
const void* pick_metric(int metric, int G, int nqv) {
    switch (metric) {
        case MVF_METRIC_L2: return pick_nq<DT, MVF_METRIC_L2>(G, nqv);
        case MVF_METRIC_INNER_PRODUCT: return pick_nq<DT, MVF_METRIC_INNER_PRODUCT>(G, nqv);
        case MVF_METRIC_COSINE: return pick_nq<DT, MVF_METRIC_COSINE>(G, nqv);
        default: return nullptr;
    }
}

}  // namespace

const void* radius_scan_kernel_ptr(uint8_t dtype, int metric, int G, int nqv) {
    switch (dtype) {
        case MVF_DTYPE_FLOAT32: return pick_metric<MVF_DTYPE_FLOAT32>(metric, G, nqv);
        case MVF_DTYPE_FLOAT16: return pick_metric<MVF_DTYPE_FLOAT16>(metric, G, nqv);
        case MVF_DTYPE_INT8: return pick_metric<MVF_DTYPE_INT8>(metric, G, nqv);
        case MVF_DTYPE_UINT8: return pick_metric<MVF_DTYPE_UINT8>(metric, G, nqv);
        default: return nullptr;
    }
}

size_t radius_scan_lds_bytes(uint8_t dtype, int G, uint32_t J, int nqv) {
    const uint32_t qb = dtype == MVF_DTYPE_FLOAT16 ? 32u : 16u;
    return (((size_t)nqv * J * G * qb + 15u) & ~(size_t)15u) + (size_t)nqv * 16u;
}

hipError_t radius_scan_launch(uint8_t dtype, int metric, int G, int nqv, const RadiusParams& p, dim3 grid, size_t lds,
                              hipStream_t s) {
    const void* fn = radius_scan_kernel_ptr(dtype, metric, G, nqv);
    if (!fn) return hipErrorInvalidValue;
    RadiusParams arg = p;
    void* args[] = {&arg};
    return hipLaunchKernel(fn, grid, dim3(256), args, lds, s);
}

hipError_t radius_rescore_launch(int metric, int G, const RadiusRescoreParams& p, uint32_t nq, size_t lds, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    const void* fn = metric == MVF_METRIC_L2 ? pick_rescore<MVF_METRIC_L2>(G)
                     : metric == MVF_METRIC_INNER_PRODUCT ? pick_rescore<MVF_METRIC_INNER_PRODUCT>(G)
                     : metric == MVF_METRIC_COSINE ? pick_rescore<MVF_METRIC_COSINE>(G) : nullptr;
    if (!fn) return hipErrorInvalidValue;
    RadiusRescoreParams arg = p;
    void* args[] = {&arg};
    return hipLaunchKernel(fn, dim3(nq), dim3(256), args, lds, s);
}

hipError_t radius_pack_launch(const RadiusPackParams& p, uint32_t nq, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(radius_pack_kernel, dim3(nq), dim3(1024), (size_t)p.cap * 8u, s, p);
    return hipGetLastError();
}

}  // namespace mvf
