// scan_radius.hip — R1 (the streaming radius scan) and R2 (ordering + packing of the per-query match lists).
//
// R1 reads the rows exactly as K1 does (scan_stream.inc): G lanes per row, each lane owning the 16-B vectors
// v = j*G + sub, U = 4 row groups in flight per wave, non-temporal 16-B loads, the query staged in LDS (f32 / packed
// int8), Float16 widened exactly, sdot4 / udot4 for Int8 / UInt8 rows.  The per-lane accumulation, the G-lane sums and
// the score -> key arithmetic are K1's as k1_rowscore.h states them (the reduce-scatter below pairs the partial sums as
// its butterfly does), so for the same lane-group width the keys are bit-identical to those the top-k path ranks.  Two
// pieces stay written out here because the header's forms cost some one-query instantiations a wave per SIMD
// (profiles/r10_k1_rowscore_refactor.txt): the staging loop (k1::stage_queries' order, four queries interleaved) and the
// row's sum of squares of Float16 rows (k1::xx8_f16's line).  The epilogue differs: there is no running threshold, the bound is
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
    using Tr = k1::Traits<DT>;
    using Acc = typename Tr::Acc;
    constexpr int ES = Tr::ES;
    constexpr int EPV = 16 / ES;
    constexpr int RPG = 64 / G;
    constexpr int U = 4;
    constexpr int QB = Tr::INT ? 16 : EPV * 4;
    constexpr bool NEED_XX = k1::kNeedXX<DT, METRIC>;

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
        Acc s = k1::group_sum<64>(qq_part[q]);
        if (lane == 0) red[q * 4 + wave] = s;
    }
    __syncthreads();
    Acc qq[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) qq[q] = red[q * 4 + 0] + red[q * 4 + 1] + red[q * 4 + 2] + red[q * 4 + 3];

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
            k1::u32x4 x[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                x[u] = k1::u32x4{0, 0, 0, 0};
                if (vv && rv[u]) x[u] = __builtin_nontemporal_load(reinterpret_cast<const k1::u32x4*>(rp[u] + (size_t)v * 16));
            }
            if constexpr (DT == MVF_DTYPE_FLOAT32) {
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    const float4 qv = *reinterpret_cast<const float4*>(qs + q * qstride + v * 16);
#pragma unroll
                    for (int u = 0; u < U; u++) acc[u][q] = k1::acc4<METRIC>(acc[u][q], qv, x[u]);
                }
                if constexpr (NEED_XX) {
#pragma unroll
                    for (int u = 0; u < U; u++) xx[u] = k1::xx4(xx[u], x[u]);
                }
            } else if constexpr (DT == MVF_DTYPE_FLOAT16) {
                float xf[U][8];
#pragma unroll
                for (int u = 0; u < U; u++) k1::widen_f16(x[u], xf[u]);
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    const float4 qa = *reinterpret_cast<const float4*>(qs + q * qstride + v * 32);
                    const float4 qb = *reinterpret_cast<const float4*>(qs + q * qstride + v * 32 + 16);
#pragma unroll
                    for (int u = 0; u < U; u++) acc[u][q] = k1::acc8_f16<METRIC>(acc[u][q], qa, qb, xf[u]);
                }
                if constexpr (NEED_XX) {
#pragma unroll
                    for (int u = 0; u < U; u++)
#pragma unroll
                        for (int i = 0; i < 8; i++) xx[u] = fmaf(xf[u][i], xf[u][i], xx[u]);
                }
            } else {  // Int8 / UInt8: exact i32
                constexpr bool S = DT == MVF_DTYPE_INT8;
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    const uint4 qv = *reinterpret_cast<const uint4*>(qs + q * qstride + v * 16);
#pragma unroll
                    for (int u = 0; u < U; u++) acc[u][q] = k1::dot16_int<S>(acc[u][q], qv, x[u]);
                }
                if constexpr (NEED_XX) {
#pragma unroll
                    for (int u = 0; u < U; u++) xx[u] = k1::dot16_int<S>(xx[u], uint4{x[u].x, x[u].y, x[u].z, x[u].w}, x[u]);
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
            const uint32_t key = k1::make_key<DT, METRIC>(s1, xx1, qq[0]);
            const bool hit = (sub & (G / 4 - 1)) == 0 && rl < p.n && qvalid[0] && key <= bnd[0] && live(rl);
            radius_append(hit, ((uint64_t)key << 32) | rl, p.counts + q0, p.lists ? p.lists + (size_t)q0 * p.cap : nullptr, p.cap, lane);
        } else {
#pragma unroll
            for (int u = 0; u < U; u++) {
                Acc xxs = 0;
                if constexpr (NEED_XX) xxs = k1::group_sum<G>(xx[u]);
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    const Acc s = k1::group_sum<G>(acc[u][q]);
                    const uint32_t key = k1::make_key<DT, METRIC>(s, xxs, qq[q]);
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
// k1_rowscore.h, as R1's.
template <int METRIC, int G>
__global__ void __launch_bounds__(256) radius_rescore_kernel(RadiusRescoreParams p) {
    constexpr int RPG = 64 / G;
    constexpr bool NEED_XX = METRIC == MVF_METRIC_COSINE;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane % G, rsel = lane / G;
    const uint32_t q = blockIdx.x;
    const uint32_t VP = p.J * G;
    unsigned char* qs = smem;
    float* red = reinterpret_cast<float*>(smem + ((VP * 16u + 15u) & ~15u));
    // the query in LDS and its sum of squares, in R1's (K1's) order
    const float* const src[1] = {p.queries + (size_t)q * p.dim};
    float qq[1];
    k1::stage_queries<MVF_DTYPE_FLOAT32, 1, true>(src, p.dim, VP * 4u, qs, 0, red, qq);
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
        float acc[1][1] = {{0.0f}}, xx[1] = {0.0f};
        for (uint32_t j = 0; j < p.J; j++) {
            const uint32_t v = j * G + sub;
            k1::u32x4 x[1] = {k1::u32x4{0, 0, 0, 0}};
            if (ok && v < p.V) x[0] = *reinterpret_cast<const k1::u32x4*>(rp + (size_t)v * 16);
            k1::accumulate<MVF_DTYPE_FLOAT32, METRIC, 1, 1>(acc, xx, x, [&](int, int) __attribute__((always_inline)) {
                return *reinterpret_cast<const float4*>(qs + v * 16);
            });
        }
        const float s = k1::group_sum<G>(acc[0][0]);
        const float xxs = NEED_XX ? k1::group_sum<G>(xx[0]) : 0.0f;
        const uint32_t key = k1::key<METRIC>(s, xxs, qq[0]);
        const bool hit = sub == 0 && ok && key <= bnd;
        radius_append(hit, ((uint64_t)key << 32) | row, p.counts + q, list, p.cap, lane);
    }
}

template <int DT>
const void* pick_scan(int metric, int G, int nqv) {
    return k1::for_metric(metric, [&](auto m) {
        return k1::for_group(G, [&](auto g) -> const void* {
            constexpr int M = decltype(m)::value, GG = decltype(g)::value;
            return nqv == 4   ? reinterpret_cast<const void*>(&radius_scan_kernel<DT, M, GG, 4>)
                   : nqv == 1 ? reinterpret_cast<const void*>(&radius_scan_kernel<DT, M, GG, 1>)
                              : nullptr;
        });
    });
}

}  // namespace

const void* radius_scan_kernel_ptr(uint8_t dtype, int metric, int G, int nqv) {
    switch (dtype) {
        case MVF_DTYPE_FLOAT32: return pick_scan<MVF_DTYPE_FLOAT32>(metric, G, nqv);
        case MVF_DTYPE_FLOAT16: return pick_scan<MVF_DTYPE_FLOAT16>(metric, G, nqv);
        case MVF_DTYPE_INT8: return pick_scan<MVF_DTYPE_INT8>(metric, G, nqv);
        case MVF_DTYPE_UINT8: return pick_scan<MVF_DTYPE_UINT8>(metric, G, nqv);
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
    const void* fn = k1::for_metric(metric, [&](auto m) {
        return k1::for_group(G, [&](auto g) { return reinterpret_cast<const void*>(&radius_rescore_kernel<decltype(m)::value, decltype(g)::value>); });
    });
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
