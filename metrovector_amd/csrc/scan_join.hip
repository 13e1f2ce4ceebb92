// scan_join.hip — the two kernels of the k-NN join (join.hip; DESIGN.md §5 "J0 / J1 — k-NN join").
//
// J0 stages a window of stored rows as the queries of a search; J1 turns the search's k' ordered entries per query into the
// join's k: the query row's own position removed, the searched corpus' ids applied, deleted query rows padded.  Both move a
// few megabytes per window beside a search of milliseconds: plain coalesced loads and stores, no LDS.

#include "scan_join.h"

#include "mvf_common.h"

namespace mvf {

namespace {

constexpr int kStageThreads = 256;
constexpr int kFinishThreads = 256;  // four waves, one query row each

// J0.  One thread per 16-byte vector of a stored row (the access shape of every row reader: consecutive lanes read
// consecutive vectors).  ALIGNED: every query row of the output starts on a 16-byte boundary, so a vector that lies
// wholly inside the row leaves as 16-byte stores; otherwise, and for the row's last partial vector, element by element.
template <int DT, bool ALIGNED>
__global__ __launch_bounds__(kStageThreads) void join_stage_kernel(JoinStageParams p, uint32_t nq) {
    constexpr uint32_t EPV = DT == MVF_DTYPE_FLOAT32 ? 4u : DT == MVF_DTYPE_FLOAT16 ? 8u : 16u;  // elements per vector
    const uint64_t total = (uint64_t)nq * p.V;
    for (uint64_t t = (uint64_t)blockIdx.x * kStageThreads + threadIdx.x; t < total; t += (uint64_t)gridDim.x * kStageThreads) {
        const uint32_t q = (uint32_t)(t / p.V), v = (uint32_t)(t % p.V);
        const uint32_t e0 = v * EPV;
        if (e0 >= p.dim) continue;  // pitch padding
        const uint4 x = *reinterpret_cast<const uint4*>(p.rows + (p.first + q) * (uint64_t)p.pitch + (uint64_t)v * 16);
        const uint32_t ne = min(EPV, p.dim - e0);
        const uint64_t o = (uint64_t)q * p.dim + e0;
        if constexpr (DT == MVF_DTYPE_FLOAT32) {
            float* out = static_cast<float*>(p.queries) + o;
            if (ALIGNED && ne == EPV) {
                *reinterpret_cast<uint4*>(out) = x;
            } else {
                const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (uint32_t e = 0; e < 4; e++)
                    if (e < ne) out[e] = bits_f32(w[e]);
            }
        } else if constexpr (DT == MVF_DTYPE_FLOAT16) {
            float* out = static_cast<float*>(p.queries) + o;
            const uint32_t w[4] = {x.x, x.y, x.z, x.w};
            float f[8];
#pragma unroll
            for (uint32_t e = 0; e < 4; e++) {  // v_cvt_f32_f16: every half is a float, exactly
                f[2 * e] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[e] & 0xFFFFu));
                f[2 * e + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[e] >> 16));
            }
            if (ALIGNED && ne == EPV) {
                reinterpret_cast<float4*>(out)[0] = make_float4(f[0], f[1], f[2], f[3]);
                reinterpret_cast<float4*>(out)[1] = make_float4(f[4], f[5], f[6], f[7]);
            } else {
#pragma unroll
                for (uint32_t e = 0; e < 8; e++)
                    if (e < ne) out[e] = f[e];
            }
        } else {
            unsigned char* out = static_cast<unsigned char*>(p.queries) + o;
            if (ALIGNED && ne == EPV) {
                *reinterpret_cast<uint4*>(out) = x;
            } else {
                const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (uint32_t e = 0; e < 16; e++)
                    if (e < ne) out[e] = (unsigned char)(w[e >> 2] >> (8 * (e & 3)));
            }
        }
    }
}

// J1.  One wave per query row.  The list arrives ordered and its entries are distinct rows, so at most one of them is the
// query row itself: a ballot over 64 entries at a time finds it (wave-uniform), and entry j of the result is entry j, or
// j + 1 from that place on.  Nothing is sorted.
__global__ __launch_bounds__(kFinishThreads) void join_finish_kernel(JoinFinishParams p, uint32_t nq) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * (kFinishThreads / 64) + (threadIdx.x >> 6);
    if (q >= nq) return;
    const size_t ob = (size_t)q * p.k;
    const uint64_t qr = p.q_row0 + q;
    if (p.q_tomb && ((p.q_tomb[qr >> 5] >> (qr & 31)) & 1u)) {  // a deleted query row: all padding
        const float pad = pad_score(p.metric);
        for (uint32_t j = lane; j < p.k; j += 64) {
            p.out_scores[ob + j] = pad;
            p.out_indices[ob + j] = ~0ull;
            if (p.out_raw) p.out_raw[ob + j] = 0;
        }
        return;
    }
    const size_t ib = (size_t)q * p.kin;
    uint32_t cut = p.k;  // entries from here on move up by one
    if (p.exclude && p.kin > p.k) {
        const uint64_t self = p.q_pos0 + q;
        for (uint32_t j0 = 0; j0 < p.kin; j0 += 64) {
            const uint32_t j = j0 + lane;
            const unsigned long long m = __ballot(j < p.kin && p.in_indices[ib + j] == self);
            if (m) {
                cut = j0 + (uint32_t)__ffsll((long long)m) - 1u;
                break;
            }
        }
    }
    for (uint32_t j = lane; j < p.k; j += 64) {
        const size_t src = ib + j + (j >= cut ? 1u : 0u);
        const uint64_t pos = p.in_indices[src];
        p.out_indices[ob + j] = (pos != ~0ull && p.c_ids) ? p.c_ids[pos - p.c_index_base] : pos;
        p.out_scores[ob + j] = p.in_scores[src];
        if (p.out_raw) p.out_raw[ob + j] = p.in_raw[src];
    }
}

template <int DT>
hipError_t stage_launch_dt(const JoinStageParams& p, uint32_t nq, bool aligned, uint32_t blocks, hipStream_t s) {
    if (aligned) join_stage_kernel<DT, true><<<blocks, kStageThreads, 0, s>>>(p, nq);
    else join_stage_kernel<DT, false><<<blocks, kStageThreads, 0, s>>>(p, nq);
    return hipGetLastError();
}

}  // namespace

hipError_t join_stage_launch(const JoinStageParams& p, uint32_t nq, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    const uint64_t total = (uint64_t)nq * p.V;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + kStageThreads - 1) / kStageThreads, 8192);
    const uint32_t qrow = p.dim * (is_int_dtype(p.dtype) ? 1u : 4u);
    const bool aligned = qrow % 16 == 0 && (reinterpret_cast<uintptr_t>(p.queries) & 15u) == 0;
    switch (p.dtype) {
    case MVF_DTYPE_FLOAT32: return stage_launch_dt<MVF_DTYPE_FLOAT32>(p, nq, aligned, blocks, s);
    case MVF_DTYPE_FLOAT16: return stage_launch_dt<MVF_DTYPE_FLOAT16>(p, nq, aligned, blocks, s);
    default: return stage_launch_dt<MVF_DTYPE_INT8>(p, nq, aligned, blocks, s);  // Int8 / UInt8: bytes either way
    }
}

hipError_t join_finish_launch(const JoinFinishParams& p, uint32_t nq, hipStream_t s) {
    if (nq == 0 || p.k == 0) return hipSuccess;
    const uint32_t per = kFinishThreads / 64;
    join_finish_kernel<<<(nq + per - 1) / per, kFinishThreads, 0, s>>>(p, nq);
    return hipGetLastError();
}

}  // namespace mvf
