// scan_gather.hip — K1's scores of rows read out of order: the one scoring kernel of the candidate search (its C1:
// per-query lists and counts from C0, scan_candidates.hip) and of the filtered search's list route (its F2: one list from
// F1, scan_filter.hip, for groups of queries), and the host tail both routes end in (DESIGN.md §5 "C0 / C1 — candidate
// search" and "F0 / F1 / F2 — filtered search").
//
// Each chunk of kGatherChunk list positions and each group of QG queries get one block: the queries are staged as K1 stages
// one (zero padded to J G vectors; sums of squares in K1's order), each G-lane group of K1's one-query shape loads a row
// once (non-temporal 16-byte loads, U = 4 rows in flight per wave) and accumulates it against every query of the group with
// K1's per-row arithmetic (k1_rowscore.h): K1's one-query bits for any number of queries.  Ties and NaN follow from the
// composites.  The kernels that keep the queries in LDS have the staging loop (k1::stage_queries' lines) and the step's
// order over rows and queries (k1::accumulate's operations) written out: that is the order the two former kernels had, and the
// header's forms cost five instantiations a wave per SIMD (profiles/r10_k1_rowscore_refactor.txt).  The kernels that read one
// float query through the cache take the header's step.
//
// Algorithmic HBM bytes: the listed rows' pitch once per group of queries (+ 4 bytes per listed row and block).

#include "scan_gather.h"
#include "aux_kernels.h"
#include "bitonic.h"
#include "k1_rowscore.h"
#include "mvf_common.h"

#include <algorithm>

namespace mvf {
namespace {

constexpr uint32_t kWindow = 1024;              // queries per window at most
constexpr size_t kScratchBytes = 512ull << 20;  // device scratch of a window (one query's or group's needs may exceed it)
constexpr uint32_t kSelectMaxLists = 2048;      // chunk lists select_final merges (its P = 4096 >= lists + k)

// grid (ceil(m / kGatherChunk), ceil(nq / QG)), block 256; dynamic LDS QG * kGatherChunk * 8 (composites) +
// kGatherChunk * 4 (rows) + QG * 16 (qq partials) (+ QG padded queries when QLDS).  The Float32 kernels that read the query
// through the cache are held to the 7 waves per SIMD the candidate search's former kernel had: left alone, the L2 and
// InnerProduct ones take 74-76 VGPRs, two to four past that step.
template <int DT, int METRIC, int G, int QG, bool QLDS>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(!QLDS && DT == MVF_DTYPE_FLOAT32 && METRIC != MVF_METRIC_COSINE ? 7 : 1, 8))) gather_score_kernel(GatherScoreParams p) {
    using Tr = k1::Traits<DT>;
    using Acc = typename Tr::Acc;
    using QT = typename Tr::Q;
    constexpr int EPV = 16 / Tr::ES;
    constexpr int RPG = 64 / G;
    constexpr int U = 4;
    constexpr bool NEED_XX = k1::kNeedXX<DT, METRIC>;
    static_assert(QLDS || (!Tr::INT && QG == 1), "only one float query is ever read through the cache");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* buf = reinterpret_cast<uint64_t*>(smem);                                       // [QG][kGatherChunk] composites
    uint32_t* rowbuf = reinterpret_cast<uint32_t*>(smem + QG * kGatherChunk * 8);            // [kGatherChunk] the chunk's rows
    Acc* red = reinterpret_cast<Acc*>(smem + QG * kGatherChunk * 8 + kGatherChunk * 4);      // [QG][4] qq partials
    unsigned char* qs = smem + QG * kGatherChunk * 8 + kGatherChunk * 4 + QG * 16;           // [QG][J G vectors] the queries (QLDS)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane % G, rsel = lane / G;
    const uint32_t q0 = blockIdx.y * QG, c0 = blockIdx.x * kGatherChunk;
    const uint32_t nqg = min((uint32_t)QG, p.nq - q0);     // queries of this group that exist
    const uint32_t span = min(kGatherChunk, p.m - c0);     // list positions of this chunk; >= 1: the grid covers m
    uint32_t nr = span;                                    // .. that hold a row
    if constexpr (QG == 1) {
        if (p.counts) {  // block-uniform
            const uint32_t cnt = p.counts[q0];
            nr = cnt > c0 ? min(kGatherChunk, cnt - c0) : 0u;
            if (p.dump)
                for (uint32_t i = nr + tid; i < span; i += 256) p.dump[(size_t)q0 * p.m + c0 + i] = rank_entry(0u, c0 + i, true);
            if (nr == 0) {
                if (p.lists)
                    for (uint32_t i = tid; i < p.kcap; i += 256) p.lists[((size_t)q0 * gridDim.x + blockIdx.x) * p.kcap + i] = kPadComposite;
                return;
            }
        }
    }

    // ---- the queries: K1's staging loop (zero padded to J G vectors) and sums of squares, one query after the other
    // (k1::stage_queries' lines); the chunk's rows
    const uint32_t VP = p.J * G;
    const size_t qstride = (size_t)VP * (EPV * sizeof(QT));  // bytes of a padded query in LDS
    const QT* src0 = reinterpret_cast<const QT*>(p.queries) + (size_t)q0 * p.dim;
#pragma unroll
    for (int qi = 0; qi < QG; qi++) {
        const QT* src = src0 + (size_t)qi * p.dim;
        const bool have = (uint32_t)qi < nqg;
        Acc qq_part = 0;
        for (uint32_t e = tid; e < VP * EPV; e += 256) {
            const QT v = (have && e < p.dim) ? src[e] : (QT)0;
            if constexpr (QLDS) reinterpret_cast<QT*>(qs + qi * qstride)[e] = v;
            if constexpr (Tr::INT) qq_part += (int32_t)v * (int32_t)v;
            else qq_part = fmaf(v, v, qq_part);
        }
        const Acc s = k1::group_sum<64>(qq_part);
        if (lane == 0) red[qi * 4 + wave] = s;
    }
    const uint32_t* list = p.list + (size_t)q0 * p.list_stride + c0;
    for (uint32_t i = tid; i < nr; i += 256) rowbuf[i] = list[i];
    __syncthreads();
    Acc qq[QG];
#pragma unroll
    for (int qi = 0; qi < QG; qi++) qq[qi] = red[qi * 4] + red[qi * 4 + 1] + red[qi * 4 + 2] + red[qi * 4 + 3];

    auto qload = [&](int qi, uint32_t v, int half) __attribute__((always_inline)) {  // float types: 4 query elements from LDS
        return *reinterpret_cast<const float4*>(qs + qi * qstride + (size_t)v * (EPV * 4) + half * 16);
    };

    const uint32_t ngroups = (nr + RPG - 1) / RPG;
    for (uint32_t g0 = (uint32_t)wave * U; g0 < ngroups; g0 += 4 * U) {  // wave-uniform: every lane reaches the shuffles
        uint32_t idx[U];
        bool rv[U];
        const unsigned char* rp[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            idx[u] = (g0 + u) * RPG + rsel;
            rv[u] = idx[u] < nr;
            rp[u] = p.rows + (size_t)(rv[u] ? rowbuf[idx[u]] : 0u) * p.pitch;
        }
        Acc acc[QG][U], xx[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            xx[u] = 0;
#pragma unroll
            for (int qi = 0; qi < QG; qi++) acc[qi][u] = 0;
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
            if constexpr (!QLDS) {
                k1::accumulate<DT, METRIC, U, 1>(acc, xx, x, [&](int, int half) __attribute__((always_inline)) {
                    return k1::query_global4(reinterpret_cast<const float*>(src0), p.dim, v * EPV + half * 4);
                });
            } else if constexpr (DT == MVF_DTYPE_FLOAT32) {
#pragma unroll
                for (int u = 0; u < U; u++)
                    if constexpr (NEED_XX) xx[u] = k1::xx4(xx[u], x[u]);
#pragma unroll
                for (int qi = 0; qi < QG; qi++) {
                    const float4 qv = qload(qi, v, 0);
#pragma unroll
                    for (int u = 0; u < U; u++) acc[qi][u] = k1::acc4<METRIC>(acc[qi][u], qv, x[u]);
                }
            } else if constexpr (DT == MVF_DTYPE_FLOAT16) {
#pragma unroll
                for (int u = 0; u < U; u++) {
                    float xf[8];
                    k1::widen_f16(x[u], xf);
                    if constexpr (NEED_XX) xx[u] = k1::xx8_f16(xx[u], xf);
#pragma unroll
                    for (int qi = 0; qi < QG; qi++) {
                        const float4 qa = qload(qi, v, 0), qb = qload(qi, v, 1);
                        acc[qi][u] = k1::acc8_f16<METRIC>(acc[qi][u], qa, qb, xf);
                    }
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; u++)
                    if constexpr (NEED_XX) xx[u] = k1::dot16_int<DT == MVF_DTYPE_INT8>(xx[u], uint4{x[u].x, x[u].y, x[u].z, x[u].w}, x[u]);
#pragma unroll
                for (int qi = 0; qi < QG; qi++) {
                    const uint4 qv = *reinterpret_cast<const uint4*>(qs + qi * qstride + (size_t)v * 16);
#pragma unroll
                    for (int u = 0; u < U; u++) acc[qi][u] = k1::dot16_int<DT == MVF_DTYPE_INT8>(acc[qi][u], qv, x[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            Acc xxs = 0;
            if constexpr (NEED_XX) xxs = k1::group_sum<G>(xx[u]);
#pragma unroll
            for (int qi = 0; qi < QG; qi++) {
                const uint32_t key = k1::make_key<DT, METRIC>(k1::group_sum<G>(acc[qi][u]), xxs, qq[qi]);
                if (sub == 0 && rv[u] && (uint32_t)qi < nqg) {
                    const uint32_t row = rowbuf[idx[u]];
                    if (p.dump) p.dump[(size_t)(q0 + qi) * p.m + c0 + idx[u]] = rank_entry(key, row, false);
                    else buf[qi * kGatherChunk + idx[u]] = ((uint64_t)key << 32) | row;
                }
            }
        }
    }
    if (!p.lists) return;
    // ---- per query, the chunk's best min(kcap, nr), sorted
    __syncthreads();
    const uint32_t P = next_pow2(nr < 2 ? 2u : nr);
    for (uint32_t qi = 0; qi < nqg; qi++) {  // block-uniform
        uint64_t* b = buf + qi * kGatherChunk;
        for (uint32_t i = nr + tid; i < P; i += 256) b[i] = kPadComposite;
        __syncthreads();
        bitonic_sort_u64_reg<256, kGatherChunk / 256>(b, P, tid);
        uint64_t* lout = p.lists + ((size_t)(q0 + qi) * gridDim.x + blockIdx.x) * p.kcap;
        for (uint32_t i = tid; i < p.kcap; i += 256) lout[i] = i < nr ? b[i] : kPadComposite;
    }
}

template <int DT>
const void* pick_kernel(int metric, int G, uint32_t qg, bool qlds) {
    return k1::for_metric(metric, [&](auto m) {
        return k1::for_group(G, [&](auto g) -> const void* {
            constexpr int M = decltype(m)::value, GG = decltype(g)::value;
            if (qg == 4) return reinterpret_cast<const void*>(&gather_score_kernel<DT, M, GG, 4, true>);
            if constexpr (!k1::Traits<DT>::INT) {
                if (!qlds) return reinterpret_cast<const void*>(&gather_score_kernel<DT, M, GG, 1, false>);
            }
            return reinterpret_cast<const void*>(&gather_score_kernel<DT, M, GG, 1, true>);
        });
    });
}

}  // namespace

hipError_t gather_score_launch(uint8_t dtype, int metric, int G, uint32_t qg, const GatherScoreParams& p, hipStream_t s) {
    if (p.nq == 0 || p.m == 0) return hipSuccess;
    if ((qg != 1 && qg != 4) || (qg != 1 && (p.counts || p.list_stride))) return hipErrorInvalidValue;
    const uint32_t qbytes = cand_query_bytes(dtype, G, p.J);
    const bool qlds = qg > 1 || is_int_dtype(dtype) || qbytes <= kCandQueryLdsMax;
    const void* fn = nullptr;
    switch (dtype) {
        case MVF_DTYPE_FLOAT32: fn = pick_kernel<MVF_DTYPE_FLOAT32>(metric, G, qg, qlds); break;
        case MVF_DTYPE_FLOAT16: fn = pick_kernel<MVF_DTYPE_FLOAT16>(metric, G, qg, qlds); break;
        case MVF_DTYPE_INT8: fn = pick_kernel<MVF_DTYPE_INT8>(metric, G, qg, qlds); break;
        case MVF_DTYPE_UINT8: fn = pick_kernel<MVF_DTYPE_UINT8>(metric, G, qg, qlds); break;
        default: break;
    }
    if (!fn) return hipErrorInvalidValue;
    const size_t lds = (size_t)qg * kGatherChunk * 8u + kGatherChunk * 4u + qg * 16u + (qlds ? (size_t)qg * qbytes : 0u);
    const dim3 grid((p.m + kGatherChunk - 1) / kGatherChunk, (p.nq + qg - 1) / qg);
    GatherScoreParams arg = p;
    void* args[] = {&arg};
    return hipLaunchKernel(fn, grid, dim3(256), args, lds, s);
}

int fill_padding(uint8_t metric, uint32_t nq, uint32_t k, float* d_scores, uint64_t* d_indices, int32_t* d_raw, hipStream_t s) {
    const size_t nres = (size_t)nq * k;
    MVF_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_scores), (int)f32_bits(pad_score(metric)), nres, s));
    MVF_HIP_TRY(hipMemsetAsync(d_indices, 0xFF, nres * 8, s));
    if (d_raw) MVF_HIP_TRY(hipMemsetAsync(d_raw, 0, nres * 4, s));
    return MVF_OK;
}

int gather_topk(const CorpusView& v, uint8_t metric, const void* d_queries, uint32_t nq, const GatherSource& src, uint32_t k,
                float* d_scores, uint64_t* d_indices, int32_t* d_raw, hipStream_t s) {
    const uint32_t m = src.m;
    int G = 64;
    uint32_t J = 1;
    k1_group(v.V, 1, v.k1_g, &G, &J);  // K1's one-query lane group: its bits
    const size_t qrow = query_row_bytes(v);
    const uint32_t nch = (m + kGatherChunk - 1) / kGatherChunk;
    const bool by_sort = k > MVFGPU_K_PER_PASS || nch > kSelectMaxLists;
    const bool sorts = by_sort || src.prep_sorts;
    const uint32_t kcap = by_sort ? 0u : next_pow2(k);
    const size_t per_q = (src.list ? 0 : (size_t)m * 4 + 4) + (sorts ? (size_t)m * 16 : 0) + (by_sort ? 0 : (size_t)nch * kcap * 8);
    uint32_t W = (uint32_t)std::max<size_t>(1, std::min<size_t>({(size_t)nq, (size_t)kWindow, kScratchBytes / per_q}));
    if (W > src.qg) W -= W % src.qg;  // whole groups, so that no row is read for a short group in the middle of a call
    GatherScratch sc{};
    if (sorts) MVF_HIP_TRY(sort_composites(nullptr, &sc.tmp_bytes, nullptr, nullptr, m, m, nullptr, s, W, m));

    AsyncBuf drows, dcnt, da, db, dtmp, dlists;
    if (!src.list) {
        MVF_HIP_TRY(drows.alloc((size_t)W * m * 4, s));
        MVF_HIP_TRY(dcnt.alloc((size_t)W * 4, s));
    }
    if (sorts) {
        MVF_HIP_TRY(da.alloc((size_t)W * m * 8, s));
        MVF_HIP_TRY(db.alloc((size_t)W * m * 8, s));
        MVF_HIP_TRY(dtmp.alloc(sc.tmp_bytes, s));
    }
    if (!by_sort) MVF_HIP_TRY(dlists.alloc((size_t)W * nch * kcap * 8, s));
    sc.a = static_cast<uint64_t*>(da.p);
    sc.b = static_cast<uint64_t*>(db.p);
    sc.tmp = dtmp.p;
    sc.rows = static_cast<uint32_t*>(drows.p);
    sc.counts = static_cast<uint32_t*>(dcnt.p);

    SelectParams fp{};
    fp.k = k;
    fp.metric = metric;
    fp.dtype = v.dtype;
    fp.index_base = v.index_base;
    fp.ids = v.ids;
    fp.out_scores = d_scores;
    fp.out_indices = d_indices;
    fp.out_raw = d_raw;
    for (uint32_t w0 = 0; w0 < nq; w0 += W) {
        const uint32_t wn = std::min(W, nq - w0);
        if (!src.list)
            if (const int rc = src.prep(w0, wn, sc)) return rc;
        GatherScoreParams sp{};
        sp.rows = v.rows;
        sp.queries = static_cast<const unsigned char*>(d_queries) + (size_t)w0 * qrow;
        sp.list = src.list ? src.list : sc.rows;
        sp.list_stride = src.list ? 0u : m;
        sp.counts = src.list ? nullptr : sc.counts;
        sp.m = m;
        sp.nq = wn;
        sp.dim = v.dim;
        sp.pitch = v.pitch;
        sp.V = v.V;
        sp.J = J;
        if (!by_sort) {
            sp.lists = static_cast<uint64_t*>(dlists.p);
            sp.kcap = kcap;
            MVF_HIP_TRY(gather_score_launch(v.dtype, metric, G, src.qg, sp, s));
            // K3: the chunks' lists merged, formatted (ids, index_base, raw, padding)
            fp.lists = sp.lists;
            fp.nlists = nch;
            fp.kcap = kcap;
            fp.heads = (k + nch - 1) / nch;
            fp.P = 4096;
            fp.out_scores = d_scores + (size_t)w0 * k;
            fp.out_indices = d_indices + (size_t)w0 * k;
            fp.out_raw = d_raw ? d_raw + (size_t)w0 * k : nullptr;
            MVF_HIP_TRY(launch_select_final(fp, wn, s));
        } else {
            sp.dump = sc.a;
            MVF_HIP_TRY(gather_score_launch(v.dtype, metric, G, src.qg, sp, s));
            size_t tb = sc.tmp_bytes;
            uint64_t* sorted = nullptr;
            MVF_HIP_TRY(sort_composites(sc.tmp, &tb, sc.a, sc.b, m, std::min<size_t>(k, m), &sorted, s, wn, m));
            for (uint32_t i = 0; i < wn; i++) MVF_HIP_TRY(launch_write_sorted(fp, sorted + (size_t)i * m, m, (size_t)(w0 + i) * k, s));
        }
    }
    return MVF_OK;
}

}  // namespace mvf
