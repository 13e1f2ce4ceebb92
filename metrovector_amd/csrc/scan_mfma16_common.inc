// scan_mfma16_common.inc -- shared by the K2 kernels for the narrow types (LDS-DMA tiles: scan_mfma16_dma.hip, ping-pong:
// scan_mfma16_pp.hip, streaming: scan_mfma16_sb.hip): the per-query constants and the epilogue of one finished tile.
// Included inside namespace mvf { namespace { ... } }.

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// UInt8 rows ride the SIGNED int8 MFMA shifted by 128 (x_s = x_u - 128 = x_u ^ 0x80 as int8, same for q):
//   dot_u = dot_s + 128 (Sq_s + Sx_s) + 16384 d,   L2_u = qq_s + xx_s - 2 dot_s (shift invariant),
//   qq_u = qq_s + 256 Sq_s + 16384 d,  xx_u likewise -- all exact integers, so the results stay bit-identical to
//   K1's v_dot4_u32_u8 path.  Per row K4 stores xx_s and bx = 128 Sx_s; per query qq_s and cqq = 128 Sq_s + 16384 d.

// Per-query constants of one M-tile (BMQ queries) into LDS: qa_s (f16: 2^-e / i8: qq as int), qb_s (f16: |q| / u8: cqq),
// tau_s (threshold key) and thr_s, the pre-filter threshold in ACCUMULATOR units.
// FLT: scores are floats -- Float16 rows, or (QS) the INT8 SHADOW of a Float32 / Float16 corpus (shadow_i8.hip): int8 rows
// with a per-row scale p.xscale and int8 queries with a per-query scale qaux0; the i32 sums are converted and then
// treated exactly like the scaled-f16 shadow's (dot ~ acc * xscale[r] * qaux0[q]).
template <int DT, int METRIC, int BMQ, bool QS>
__device__ __forceinline__ void load_query_consts16(const Batch16Params& p, uint32_t q0, int tid, float* qa_s, float* qb_s,
                                                    uint32_t* tau_s, float* thr_s) {
    constexpr bool U8 = DT == MVF_DTYPE_UINT8;
    constexpr bool FLT = DT == MVF_DTYPE_FLOAT16 || QS;

        if (tid < BMQ) {
            const float qa = p.qaux0[q0 + tid], qb = p.qaux1[q0 + tid];
            const uint32_t tau = p.tau[q0 + tid];
            qa_s[tid] = qa;
            qb_s[tid] = qb;
            tau_s[tid] = tau;
            // Pre-filter threshold in ACCUMULATOR units (see scan_mfma.hip): a superset test, one or two ops per score.
            if constexpr (FLT) {
                const float ts = score_from_key(tau, METRIC);
                if (METRIC == MVF_METRIC_L2) {
                    // batched L2 selects on s2 = qq + xx - 2 dot, dot = acc * 2^-e (exact distances are re-scored
                    // afterwards); tau holds ord(thr).  s2 <= thr  <=>  acc * 2^(1-e) - xx >= qq - thr.
                    const float qq = qb * qb;
                    const float cq = qq - ts;
                    thr_s[tid] = cq - fabsf(cq) * 2e-6f - (qq + p.xxmax[0]) * 4e-7f;
                } else {
                    // score = acc * 2^-e [/ (|q||x|)] >= ts  <=>  acc [* 1/|x|] >= ts [* |q|] * 2^e
                    const float tq = (METRIC == MVF_METRIC_COSINE ? ts * qb : ts) / qa;
                    thr_s[tid] = tq - fabsf(tq) * 2e-6f;
                }
            } else {
                const int32_t qq = __float_as_int(qa);   // sum q^2 (UInt8: of the shifted query)
                const int32_t cqq = __float_as_int(qb);  // UInt8: 128 Sq_s + 16384 d (>= 0); Int8: 0
                if (METRIC == MVF_METRIC_INNER_PRODUCT) {
                    // dot_u = acc + bx + cqq >= traw  <=>  acc + bx >= traw - cqq   (exact; clamp the "no threshold" case)
                    const int32_t traw = raw_from_key(tau, METRIC);
                    thr_s[tid] = __int_as_float(traw < INT32_MIN + cqq ? INT32_MIN : traw - cqq);
                } else if (METRIC == MVF_METRIC_L2) {
                    thr_s[tid] = __int_as_float(qq - raw_from_key(tau, METRIC));       // 2 dot - xx >= qq - traw (exact)
                } else {
                    const float ts = score_from_key(tau, METRIC);
                    const int32_t qqu = U8 ? qq + 2 * cqq - 16384 * (int32_t)p.dim : qq;
                    const float tq = ts * sqrtf((float)qqu);                           // dot * 1/|x| >= ts * |q|
                    thr_s[tid] = tq - fabsf(tq) * 2e-6f;
                }
            }
            // Padding queries of the batch's last tile (zero vectors: every sum is 0) never pass and, unlike a real query
            // that has no threshold YET (tau = none: stage 1 of its wave is skipped, stage 2 decides), must not switch the
            // pre-filter off for the real queries beside them: tau = best possible key, pre-filter threshold out of reach.
            if (q0 + tid >= p.nq) {
                tau_s[tid] = 0u;
                thr_s[tid] = (FLT || METRIC == MVF_METRIC_COSINE) ? __builtin_inff() : __int_as_float(0x40000000);
            }
        }
    }

// ---- epilogue of one finished tile: a wave's WQ queries x WR corpus rows, as SH x SH MFMA sub-tiles ----------------
// (wave (wm, wn) of the block owns queries [wm WQ, wm WQ + WQ) and rows [wn WR, wn WR + WR) of the tile)
// C/D map of v_mfma_*_32x32x*: col = lane & 31 -> corpus row, row = (e&3) + 8 (e>>2) + 4 (lane>>5) -> query, 16 elements;
//            of v_mfma_*_16x16x*: col = lane & 15 -> corpus row, row = e + 4 (lane>>4) -> query, 4 elements.
// Two stages.  (1) ALWAYS: one or two ops + a compare per score against the per-query pre-filter, the compare results
// OR-ed on the scalar unit into ONE wave-wide mask for the whole wave tile; the thresholds are fetched once per query
// group (i outer, rows inner) and nothing branches.  (2) RARE (a few percent of the wave tiles once a threshold
// exists): the sub-tiles are walked again, the exact key is computed for the lanes that passed and the candidates are
// appended.  Per-row constants (norms, shadow scale, UInt8 bias) come from global memory, or -- RC_LDS, the ping-pong
// kernel -- from an LDS copy its loader DMA'd beside the tile (rc0 / rc1, indexed by the row's offset in the tile): an
// ordinary load there would make hipcc drain the whole LDS-DMA ring (s_waitcnt vmcnt(0)) once per tile.
template <int DT, int METRIC, bool DIRECT, bool XS, int BMQ, int SH, int WQ, int WR, int TR, bool RC_LDS, typename AccT>
__device__ __forceinline__ void epilogue16(const Batch16Params& p, AccT (&acc)[WQ / SH][WR / SH], uint32_t nt, uint32_t mt,
                                           int wm, int wn, int lane, const float* qa_s, const float* qb_s,
                                           const uint32_t* tau_s, const float* thr_s, const uint32_t* rc0 = nullptr,
                                           const uint32_t* rc1 = nullptr, uint32_t* bc_s = nullptr) {
    constexpr int NI = WQ / SH, NJ = WR / SH, NE = SH * SH / 64, NG = NE / 4;  // sub-tiles per wave, elements per lane
    constexpr bool U8 = DT == MVF_DTYPE_UINT8;
    // float scores: Float16 rows, or the int8 shadow of a float corpus (DT = Int8 with XS: i32 sums, converted)
    constexpr bool F16 = DT == MVF_DTYPE_FLOAT16 || (DT == MVF_DTYPE_INT8 && XS);

    const uint32_t q0 = mt * BMQ, r0 = p.row_begin + nt * TR;  // TR: corpus rows per block tile
    // keep this address arithmetic inside the epilogue (hoisted out of the k-tile loop it costs VGPRs there)
    int lane_q = wm * WQ + 4 * (lane / SH), lane_r = wn * WR + (lane & (SH - 1));
    asm volatile("" : "+v"(lane_q), "+v"(lane_r));

    // per-row constants of the lane's NJ rows
    bool rok[NJ];
    float xnf[NJ], rx[NJ], xxf[NJ], rs[NJ];
    int32_t xxi[NJ], bx[NJ], xxu[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const uint32_t rt = (uint32_t)lane_r + j * SH, r = r0 + rt;
        rok[j] = r < p.row_end;
        xnf[j] = 0.f, rx[j] = 1.f, xxf[j] = 0.f, rs[j] = 1.f;
        xxi[j] = 0, bx[j] = 0, xxu[j] = 0;
        if (RC_LDS || rok[j]) {
            if constexpr (F16) {
                if (METRIC == MVF_METRIC_COSINE) xnf[j] = RC_LDS ? __uint_as_float(rc0[rt]) : p.xnorm_f[r];
                if (METRIC == MVF_METRIC_L2) xxf[j] = RC_LDS ? __uint_as_float(rc0[rt]) : p.xx2[r];
                if constexpr (XS) rs[j] = RC_LDS ? __uint_as_float(rc1[rt]) : p.xscale[r];
            } else {
                if (METRIC != MVF_METRIC_INNER_PRODUCT) xxi[j] = RC_LDS ? (int32_t)rc0[rt] : p.xnorm_i[r];
                if (U8 && METRIC != MVF_METRIC_L2) bx[j] = RC_LDS ? (int32_t)rc1[rt] : p.xbias_i[r];
            }
        }
        if (U8) xxu[j] = xxi[j] + 2 * bx[j] + 16384 * (int32_t)p.dim;
        if (METRIC == MVF_METRIC_COSINE) {
            if constexpr (F16) rx[j] = xnf[j] > 0.0f ? rs[j] * __builtin_amdgcn_rcpf(xnf[j]) : 0.0f;
            else if (U8) rx[j] = xxu[j] > 0 ? __builtin_amdgcn_rcpf(sqrtf((float)xxu[j])) : 0.0f;
            else rx[j] = xxi[j] > 0 ? __builtin_amdgcn_rcpf(sqrtf((float)xxi[j])) : 0.0f;
        }
    }
    // pre-filter test of accumulator element (i, j, 4g+t) against its query's threshold
    auto passes = [&](int i, int j, int g, int t, const u32x4& th4, const u32x4& sc4) __attribute__((always_inline)) -> bool {
        if constexpr (F16) {
            const float a = XS && METRIC != MVF_METRIC_COSINE ? (float)acc[i][j][4 * g + t] * rs[j] : (float)acc[i][j][4 * g + t];
            const float y = METRIC == MVF_METRIC_COSINE ? a * rx[j]
                            : METRIC == MVF_METRIC_L2   ? fmaf(a, 2.0f * __uint_as_float(sc4[t]), -xxf[j])
                                                        : a;
            return !(y < __uint_as_float(th4[t]));
        } else if (METRIC == MVF_METRIC_INNER_PRODUCT) {
            return acc[i][j][4 * g + t] + bx[j] >= (int32_t)th4[t];
        } else if (METRIC == MVF_METRIC_L2) {
            return (acc[i][j][4 * g + t] << 1) - xxi[j] >= (int32_t)th4[t];
        } else {
            return !((float)(acc[i][j][4 * g + t] + bx[j] + (int32_t)sc4[t]) * rx[j] < __uint_as_float(th4[t]));
        }
    };
    auto load_thr = [&](int i, int g, u32x4& th4, u32x4& sc4) __attribute__((always_inline)) {
        th4 = *reinterpret_cast<const u32x4*>(thr_s + lane_q + i * SH + 8 * g);
        sc4 = u32x4{0, 0, 0, 0};
        if (F16 && METRIC == MVF_METRIC_L2)
            sc4 = *reinterpret_cast<const u32x4*>(qa_s + lane_q + i * SH + 8 * g);  // 2^-e per query
        if (U8 && METRIC == MVF_METRIC_COSINE)
            sc4 = *reinterpret_cast<const u32x4*>(qb_s + lane_q + i * SH + 8 * g);  // cqq per query
    };

    // ---- stage 1: does ANY score of the wave tile pass its pre-filter? ---------------------------------------------
    // Per element ONE op (score minus its query's threshold, both in accumulator units) and half a v_max3 into a
    // per-row running maximum; one compare per row at the end -- no per-score compare, no scalar OR chain.  A maximum
    // drops NaN operands: with a threshold in force a NaN score cannot enter the top-k anyway (k better candidates
    // exist), and while some query of the wave has NO threshold yet (tau = none) the stage is skipped and stage 2
    // decides everything with the exact test.  Integer sums: partial sums stay inside int32 for dim <= 8192
    // (dim 255^2 + |threshold| < 2^31); wider rows skip the stage as well.
    bool hitj[NJ];  // stage 1's verdict per row of the lane (all true when the stage is skipped)
#pragma unroll
    for (int j = 0; j < NJ; j++) hitj[j] = true;
    if (!DIRECT) {
        bool nothr = false;
#pragma unroll
        for (int h = 0; h < (WQ + 63) / 64; h++)
            if (WQ % 64 == 0 || h * 64 + lane < WQ) nothr |= tau_s[wm * WQ + h * 64 + lane] == kNanKey;
        const bool skip = __builtin_amdgcn_ballot_w64(nothr) != 0 || (!F16 && p.dim > 8192u);
        if (!skip) {
            using MT = typename std::conditional<F16 || METRIC == MVF_METRIC_COSINE, float, int32_t>::type;
            MT mx[NJ];
#pragma unroll
            for (int j = 0; j < NJ; j++) mx[j] = std::is_same<MT, float>::value ? (MT)-__builtin_inff() : (MT)INT32_MIN;
#pragma unroll
            for (int i = 0; i < NI; i++) {
#pragma unroll
                for (int g = 0; g < NG; g++) {
                    u32x4 th4, sc4;
                    load_thr(i, g, th4, sc4);
#pragma unroll
                    for (int j = 0; j < NJ; j++) {
                        MT d[4];
#pragma unroll
                        for (int t = 0; t < 4; t++) {
                            if constexpr (F16) {
                                const float a = (float)acc[i][j][4 * g + t], th = __uint_as_float(th4[t]);
                                if (METRIC == MVF_METRIC_COSINE) d[t] = fmaf(a, rx[j], -th);                 // rx carries rs
                                else if (METRIC == MVF_METRIC_L2)
                                    d[t] = fmaf(XS ? a * rs[j] : a, 2.0f * __uint_as_float(sc4[t]), -th);    // vs xx of the row
                                else d[t] = XS ? fmaf(a, rs[j], -th) : a - th;
                            } else if constexpr (METRIC == MVF_METRIC_COSINE) {
                                d[t] = fmaf((float)(acc[i][j][4 * g + t] + bx[j] + (int32_t)sc4[t]), rx[j], -__uint_as_float(th4[t]));
                            } else if constexpr (METRIC == MVF_METRIC_L2) {
                                d[t] = (acc[i][j][4 * g + t] << 1) - (int32_t)th4[t];                        // vs xx of the row
                            } else {
                                d[t] = acc[i][j][4 * g + t] - (int32_t)th4[t];                               // vs -bias of the row
                            }
                        }
                        if constexpr (std::is_same<MT, float>::value) {
                            mx[j] = __builtin_fmaxf(__builtin_fmaxf(mx[j], d[0]), d[1]);
                            mx[j] = __builtin_fmaxf(__builtin_fmaxf(mx[j], d[2]), d[3]);
                        } else {
                            mx[j] = max(max(mx[j], d[0]), d[1]);
                            mx[j] = max(max(mx[j], d[2]), d[3]);
                        }
                    }
                }
            }
            bool hit = false;
#pragma unroll
            for (int j = 0; j < NJ; j++) {
                if constexpr (F16) hitj[j] = METRIC == MVF_METRIC_L2 ? mx[j] >= xxf[j] : mx[j] >= 0.0f;
                else if constexpr (METRIC == MVF_METRIC_COSINE) hitj[j] = mx[j] >= 0.0f;
                else if constexpr (METRIC == MVF_METRIC_L2) hitj[j] = mx[j] >= xxi[j];
                else hitj[j] = mx[j] + bx[j] >= 0;
                hit |= hitj[j];
            }
            if (__builtin_amdgcn_ballot_w64(hit) == 0) return;  // wave-uniform; the common case
        }
    }

    // ---- stage 2: exact keys of the passing lanes, candidate append ---------------------------------------------------
    // Runs for the rows (j) some lane flagged in stage 1 -- with 1024 queries that is most 256 x 256 tiles of a late
    // phase (a handful of candidates per tile), so it is kept short: the pass masks of the row's NI sub-tiles are
    // computed in ONE branch-free sweep (the threshold reads pipeline like stage 1's; a branch per sub-tile would wait
    // for each read in turn), then only the actual hits are walked, one per iteration, the element picked by a select
    // over the row's accumulators.
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const uint32_t r = r0 + lane_r + j * SH;
        // deleted rows (tombstone bitmap): never appended; the direct phase stores padding in their slots
        const bool dead = p.tomb && rok[j] && ((p.tomb[r >> 5] >> (r & 31)) & 1u);
        if (!DIRECT && dead) rok[j] = false;
        const unsigned long long rokmask = __builtin_amdgcn_ballot_w64(rok[j]);
        if (!DIRECT && (__builtin_amdgcn_ballot_w64(hitj[j]) & rokmask) == 0) continue;  // no lane's row j passed stage 1
        static_assert(NI * NE <= 64, "one mask word pair per row");
        unsigned long long mall = 0;  // bit i * NE + e: element e of sub-tile (i, j) passes its pre-filter
        if (DIRECT) {
            mall = NI * NE == 64 ? ~0ull : ((1ull << (NI * NE)) - 1ull);
        } else {
#pragma unroll
            for (int i = 0; i < NI; i++) {
#pragma unroll
                for (int g = 0; g < NG; g++) {
                    u32x4 th4, sc4;
                    load_thr(i, g, th4, sc4);
#pragma unroll
                    for (int t = 0; t < 4; t++) mall |= (unsigned long long)(passes(i, j, g, t, th4, sc4) ? 1u : 0u) << (i * NE + 4 * g + t);
                }
            }
        }
        if (!rok[j]) mall = 0;
        for (; __builtin_amdgcn_ballot_w64(mall != 0) != 0; mall &= mall - 1) {
            if (mall == 0) continue;
            const int bit = __builtin_ctzll(mall);
            const int ii = bit / NE, e = bit % NE;
            auto av = acc[0][j][0];
#pragma unroll
            for (int i = 0; i < NI; i++)
#pragma unroll
                for (int x = 0; x < NE; x++) av = bit == i * NE + x ? acc[i][j][x] : av;
            const int ql = lane_q + ii * SH + (e & 3) + 8 * (e >> 2);
            uint32_t key;
            if constexpr (F16) {
                float sc_ = (float)av * qa_s[ql];       // undo the query scale (f16: a power of two, exact)
                if constexpr (XS) sc_ *= rs[j];          // ... and the shadow row's
                if (METRIC == MVF_METRIC_COSINE) {
                    const float den = qb_s[ql] * xnf[j];
                    sc_ = den > 0.0f ? sc_ / den : 0.0f;
                }
                if (METRIC == MVF_METRIC_L2) sc_ = qb_s[ql] * qb_s[ql] + xxf[j] - 2.0f * sc_;  // GEMM-form s2
                key = key_from_score(sc_, METRIC);
            } else {
                const int32_t qq = __float_as_int(qa_s[ql]);
                const int32_t cqq = __float_as_int(qb_s[ql]);
                const int32_t dot = U8 ? av + bx[j] + cqq : av;  // dot in the space's own domain
                if (METRIC == MVF_METRIC_L2) {
                    key = key_from_raw(qq + xxi[j] - 2 * av, METRIC);  // shift invariant
                } else if (METRIC == MVF_METRIC_INNER_PRODUCT) {
                    key = key_from_raw(dot, METRIC);
                } else {
                    const int32_t qqn = U8 ? qq + 2 * cqq - 16384 * (int32_t)p.dim : qq;
                    const int32_t xxn = U8 ? xxu[j] : xxi[j];
                    const float den = sqrtf((float)qqn) * sqrtf((float)xxn);
                    key = key_from_score(den > 0.0f ? (float)dot / den : 0.0f, METRIC);
                }
            }
            const uint32_t q = q0 + ql;
            if (q < p.nq && (DIRECT || key <= tau_s[ql])) {
                uint32_t bslot = p.blk_cap;
                if (!DIRECT && bc_s) bslot = atomicAdd(bc_s, 1u);  // LDS counter of the block's own region
                if (bslot < p.blk_cap) {
                    p.blk_cand[(size_t)blockIdx.x * p.blk_cap + bslot] = make_uint4(key, r, q, 0u);
                } else {  // phase 0 (slot = the row's offset), no region, or region full: the per-query list itself
                    const uint32_t slot_i = DIRECT ? r - p.row_begin : atomicAdd(&p.cnt[q], 1u);
                    if (slot_i < p.cap) p.cand[(size_t)q * p.cap + slot_i] = dead ? kPadComposite : ((uint64_t)key << 32) | r;
                }
            }
        }
    }
}
