// scan_maxsim_score.inc — M0, the scoring kernel of the multi-vector search, as a template two translation units instantiate:
// scan_maxsim.hip (what is kept is the u32 order key) and scan_maxsim_align.hip (M0-arg: the key with the row that gave it).
// Included inside namespace mvf's anonymous namespace, behind scan_maxsim.h and k1_rowscore.h.

// k1::group_sum over N values per lane at once: the G lanes' partial sums of every value meet in group_sum's pairs, in its
// order (offsets G/2, G/4, .., 1) -- a + b is b + a, so every total has group_sum's bits -- but while a lane holds more than
// one value, each step leaves it HALF of them: the lane whose `sub` has the offset's bit clear keeps the lower half, its
// partner the upper half, and each sends the other half.  Behind it v[0 .. max(N / G, 1)) are the totals of the values
// first, first + 1, ..; the G / N lanes that differ only in the low bits of `sub` hold the same ones (N <= G).  log2(N) +
// N - 1 shuffles where N group_sums take N log2(G).
template <int OFF, int N, int NV, typename T>
__device__ __forceinline__ void scatter_sum(T (&v)[NV], int sub, int& first) {
    if constexpr (OFF > 0) {
        if constexpr (N > 1) {
            constexpr int H = N / 2;
            const bool upper = (sub & OFF) != 0;
#pragma unroll
            for (int i = 0; i < H; i++) {
                const T keep = upper ? v[i + H] : v[i], send = upper ? v[i] : v[i + H];
                v[i] = keep + __shfl_xor(send, OFF, 64);
            }
            first += upper ? H : 0;
            scatter_sum<OFF / 2, H, NV>(v, sub, first);
        } else {
            v[0] += __shfl_xor(v[0], OFF, 64);
            scatter_sum<OFF / 2, 1, NV>(v, sub, first);
        }
    }
}

// the bytes of M0's dynamic LDS in front of the tokens: minima [tc][kMaxsimRows], rows and local ordinals [kMaxsimRows] each,
// qq partials [tc][4] and sums [tc]; a minimum takes min_bytes: 4, or M0-arg's 8
__host__ __device__ constexpr uint32_t maxsim_lds_head(uint32_t tc, uint32_t min_bytes = 4u) {
    return tc * kMaxsimRows * min_bytes + kMaxsimRows * 8u + tc * 20u;
}

// grid (ceil(m / kMaxsimRows), sets), block 256; dynamic LDS maxsim_lds_head(tc) rounded up to 16 (+ tc padded tokens when QLDS)
// CAND, the candidate form: grid (m / kMaxsimRows, 1); the block's set and its number of positions come from p.blocks
// ARG (M0-arg, with CAND; the head is maxsim_lds_head(tc, 8)): what is kept per (token, key) is the u64 composite
// (order key << 32) | local row -- rowbuf[pos], the row behind the list position -- in lmin and in p.best64[set][t][n_keys],
// all-ones on entry.  A key's rows are listed in ascending position, kNanKey is the largest key and no local row is 0xFFFFFFFF:
// the smallest composite is the first row in mvfgpu_search's order, whatever the order of the atomics.  Every scoring line is
// shared, so the bits are M0's.
template <int DT, int METRIC, int G, bool REG, bool QLDS, bool CAND = false, bool ARG = false>
__global__ void __launch_bounds__(256) maxsim_score_kernel(MaxsimScoreParams p) {
    using Tr = k1::Traits<DT>;
    using Acc = typename Tr::Acc;
    using QT = typename Tr::Q;
    constexpr int EPV = 16 / Tr::ES;
    constexpr int RPG = 64 / G;
    constexpr int U = REG ? 2 : 4;
    constexpr int JR = REG ? (int)kMaxsimRegSteps : 1;
    constexpr int TG = (int)kMaxsimTokenGroup;
    constexpr bool NEED_XX = k1::kNeedXX<DT, METRIC>;
    constexpr int NV = TG * U;                     // sums per lane and step: (token of the group, row)
    constexpr int KEPT = NV > G ? NV / G : 1;      // .. that a lane holds behind scatter_sum
    constexpr int SAME = NV > G ? 1 : G / NV;      // .. and neighbouring lanes that hold the same ones
    static_assert(QLDS || !Tr::INT, "only float tokens are ever read through the cache");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tc = p.tc;
    using MinT = std::conditional_t<ARG, unsigned long long, uint32_t>;
    MinT* lmin = reinterpret_cast<MinT*>(smem);                                 // [tc][kMaxsimRows] the block's minima
    uint32_t* rowbuf = reinterpret_cast<uint32_t*>(lmin + tc * kMaxsimRows);    // [kMaxsimRows] the block's rows
    uint32_t* ordbuf = rowbuf + kMaxsimRows;                                    // [kMaxsimRows] .. and key ordinals - the first's
    Acc* red = reinterpret_cast<Acc*>(ordbuf + kMaxsimRows);                    // [tc][4] qq partials
    Acc* qqs = red + tc * 4;                                                    // [tc] the tokens' sums of squares
    unsigned char* qs = smem + ((maxsim_lds_head(tc, sizeof(MinT)) + 15u) & ~15u);  // [tc][J G vectors] the tokens (QLDS)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane % G, rsel = lane / G;
    const uint32_t c0 = blockIdx.x * kMaxsimRows;
    uint32_t set, nr;
    if constexpr (CAND) {
        const MaxsimCandBlock b = p.blocks[blockIdx.x];  // the same for every lane: kept in scalar registers
        set = __builtin_amdgcn_readfirstlane(b.set);
        nr = __builtin_amdgcn_readfirstlane(min(b.nr, kMaxsimRows));  // a host plan's: 1 .. kMaxsimRows
        if (nr == 0) return;  // P0's table (scan_maxsim_mfma.hip): the block holds no row of a candidate of its set
    } else {
        set = blockIdx.y, nr = min(kMaxsimRows, p.m - c0);  // >= 1: the grid covers m
    }

    // ---- the tokens: K1's staging loop and sums of squares, one token after the other (k1::stage_queries' lines)
    const uint32_t VP = p.J * G;
    const size_t qstride = (size_t)VP * (EPV * sizeof(QT));  // bytes of a padded token in LDS
    const QT* src0 = reinterpret_cast<const QT*>(p.queries) + ((size_t)set * p.n_tokens + p.t0) * p.dim;
    for (uint32_t t = 0; t < tc; t++) {
        const QT* src = src0 + (size_t)t * p.dim;
        Acc qq_part = 0;
        for (uint32_t e = tid; e < VP * EPV; e += 256) {
            const QT v = e < p.dim ? src[e] : (QT)0;
            if constexpr (QLDS) reinterpret_cast<QT*>(qs + t * qstride)[e] = v;
            if constexpr (Tr::INT) qq_part += (int32_t)v * (int32_t)v;
            else qq_part = fmaf(v, v, qq_part);
        }
        const Acc s = k1::group_sum<64>(qq_part);
        if (lane == 0) red[t * 4 + wave] = s;
    }
    const uint32_t ord0 = p.ord[c0];
    for (uint32_t i = tid; i < nr; i += 256) {
        rowbuf[i] = p.list[c0 + i];
        ordbuf[i] = min(p.ord[c0 + i] - ord0, kMaxsimRows - 1u);  // every key holds a row: at most i
    }
    for (uint32_t i = tid; i < tc * kMaxsimRows; i += 256) lmin[i] = ARG ? (MinT)~0ull : (MinT)kNanKey;
    __syncthreads();
    for (uint32_t t = tid; t < tc; t += 256) qqs[t] = red[t * 4] + red[t * 4 + 1] + red[t * 4 + 2] + red[t * 4 + 3];
    __syncthreads();

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
        k1::u32x4 xr[JR][U];
        if constexpr (REG) {  // the rows, once
#pragma unroll
            for (int j = 0; j < JR; j++) {
                const uint32_t v = (uint32_t)j * G + sub;
#pragma unroll
                for (int u = 0; u < U; u++) {
                    xr[j][u] = k1::u32x4{0, 0, 0, 0};
                    if ((uint32_t)j < p.J && v < p.V && rv[u])
                        xr[j][u] = __builtin_nontemporal_load(reinterpret_cast<const k1::u32x4*>(rp[u] + (size_t)v * 16));
                }
            }
        }
        for (uint32_t tg0 = 0; tg0 < tc; tg0 += TG) {
            Acc acc[TG][U], xx[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                xx[u] = 0;
#pragma unroll
                for (int q = 0; q < TG; q++) acc[q][u] = 0;
            }
            auto step = [&](uint32_t j, const k1::u32x4(&x)[U]) __attribute__((always_inline)) {
                const uint32_t v = j * G + sub;
                k1::accumulate<DT, METRIC, U, TG>(acc, xx, x, [&](int q, int half) __attribute__((always_inline)) {
                    const uint32_t t = min(tg0 + (uint32_t)q, tc - 1u);  // a short last group scores its last token again
                    if constexpr (Tr::INT) {
                        return *reinterpret_cast<const uint4*>(qs + t * qstride + (size_t)v * 16);
                    } else if constexpr (QLDS) {
                        return *reinterpret_cast<const float4*>(qs + t * qstride + (size_t)v * (EPV * 4) + half * 16);
                    } else {
                        return k1::query_global4(reinterpret_cast<const float*>(src0) + (size_t)t * p.dim, p.dim, v * EPV + half * 4);
                    }
                });
            };
            if constexpr (REG) {
#pragma unroll
                for (int j = 0; j < JR; j++)
                    if ((uint32_t)j < p.J) step((uint32_t)j, xr[j]);
            } else {
                for (uint32_t j = 0; j < p.J; j++) {
                    const uint32_t v = j * G + sub;
                    k1::u32x4 x[U];
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        x[u] = k1::u32x4{0, 0, 0, 0};
                        if (v < p.V && rv[u]) x[u] = *reinterpret_cast<const k1::u32x4*>(rp[u] + (size_t)v * 16);
                    }
                    step(j, x);
                }
            }
            // the group's sums, scattered over its lanes: each (token, row) of the step gets its key and its LDS minimum from one lane
            Acc flat[NV], xxs[U];
#pragma unroll
            for (int q = 0; q < TG; q++)
#pragma unroll
                for (int u = 0; u < U; u++) flat[q * U + u] = acc[q][u];
            int first = 0;
            scatter_sum<G / 2, NV>(flat, sub, first);
#pragma unroll
            for (int u = 0; u < U; u++) xxs[u] = NEED_XX ? k1::group_sum<G>(xx[u]) : (Acc)0;
#pragma unroll
            for (int i = 0; i < KEPT; i++) {
                const uint32_t q = (uint32_t)(first + i) / U, u = (uint32_t)(first + i) % U;
                Acc xsel = xxs[0];
#pragma unroll
                for (int uu = 1; uu < U; uu++) xsel = u == (uint32_t)uu ? xxs[uu] : xsel;
                const uint32_t t = min(tg0 + q, tc - 1u), pos = (g0 + u) * RPG + rsel;
                const uint32_t key = k1::make_key<DT, METRIC>(flat[i], xsel, qqs[t]);
                if ((sub & (SAME - 1)) == 0 && pos < nr && tg0 + q < tc) {
                    if constexpr (ARG) atomicMin(&lmin[t * kMaxsimRows + ordbuf[pos]], ((unsigned long long)key << 32) | rowbuf[pos]);
                    else atomicMin(&lmin[t * kMaxsimRows + ordbuf[pos]], key);
                }
            }
        }
    }
    __syncthreads();
    // ---- one atomicMin per (token, run of the block)
    const uint32_t nseg = ordbuf[nr - 1] + 1u;
    MinT* best;
    if constexpr (ARG) best = reinterpret_cast<MinT*>(p.best64) + (size_t)set * tc * p.n_keys;
    else best = p.best + (size_t)set * tc * p.n_keys;
    for (uint32_t i = tid; i < tc * nseg; i += 256) {
        const uint32_t t = i / nseg, sg = i % nseg;
        if (ord0 + sg < p.n_keys) atomicMin(&best[(size_t)t * p.n_keys + ord0 + sg], lmin[t * kMaxsimRows + sg]);
    }
}

// the score a result reports for an order key (write_result's lines)
__device__ __forceinline__ float maxsim_score_of(uint32_t key, uint8_t metric, bool raw_key) {
    if (raw_key) {
        const int32_t raw = raw_from_key(key, metric);
        return metric == MVF_METRIC_L2 ? sqrtf((float)raw) : (float)raw;
    }
    return score_from_key(key, metric);
}

template <int DT, bool CAND, bool ARG = false>
const void* pick_kernel(int metric, int G, bool reg, bool qlds) {
    return k1::for_metric(metric, [&](auto m) {
        return k1::for_group(G, [&](auto g) -> const void* {
            constexpr int M = decltype(m)::value, GG = decltype(g)::value;
            if constexpr (!k1::Traits<DT>::INT) {
                if (!qlds) return reinterpret_cast<const void*>(&maxsim_score_kernel<DT, M, GG, false, false, CAND, ARG>);
            }
            if (reg) return reinterpret_cast<const void*>(&maxsim_score_kernel<DT, M, GG, true, true, CAND, ARG>);
            return reinterpret_cast<const void*>(&maxsim_score_kernel<DT, M, GG, false, true, CAND, ARG>);
        });
    });
}

// the launch of M0 (CAND: over a concatenated list; ARG: M0-arg): the form, the instantiation and the dynamic LDS
template <bool CAND, bool ARG = false>
hipError_t score_launch(uint8_t dtype, int metric, int G, const MaxsimScoreParams& p, hipStream_t s) {
    if (p.sets == 0 || p.m == 0 || p.tc == 0) return hipSuccess;
    if (p.tc > kMaxsimChunkMax || p.t0 + p.tc > p.n_tokens || p.sets > 65535u) return hipErrorInvalidValue;
    if (CAND && (!p.blocks || p.m % kMaxsimRows)) return hipErrorInvalidValue;
    if (ARG && !p.best64) return hipErrorInvalidValue;
    const MaxsimForm form = maxsim_form(dtype, G, p.J);
    const uint32_t qbytes = form.token_bytes;
    const bool qlds = form.qlds, reg = form.reg;
    if (qlds && (size_t)p.tc * qbytes > kCandQueryLdsMax && p.tc > 1) return hipErrorInvalidValue;
    const void* fn = nullptr;
    switch (dtype) {
        case MVF_DTYPE_FLOAT32: fn = pick_kernel<MVF_DTYPE_FLOAT32, CAND, ARG>(metric, G, reg, qlds); break;
        case MVF_DTYPE_FLOAT16: fn = pick_kernel<MVF_DTYPE_FLOAT16, CAND, ARG>(metric, G, reg, qlds); break;
        case MVF_DTYPE_INT8: fn = pick_kernel<MVF_DTYPE_INT8, CAND, ARG>(metric, G, reg, qlds); break;
        case MVF_DTYPE_UINT8: fn = pick_kernel<MVF_DTYPE_UINT8, CAND, ARG>(metric, G, reg, qlds); break;
        default: break;
    }
    if (!fn) return hipErrorInvalidValue;
    const size_t lds = ((maxsim_lds_head(p.tc, ARG ? 8u : 4u) + 15u) & ~15u) + (qlds ? (size_t)p.tc * qbytes : 0u);
    if (ARG && lds > 48u * 1024u) {  // M0-arg's minima and 40 KiB of tokens pass the default bound of dynamic LDS
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((p.m + kMaxsimRows - 1) / kMaxsimRows, CAND ? 1u : p.sets);
    MaxsimScoreParams arg = p;
    void* args[] = {&arg};
    return hipLaunchKernel(fn, grid, dim3(256), args, lds, s);
}
