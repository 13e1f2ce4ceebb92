// scan_stream.inc — K1: the HBM-bound streaming scan with a fused per-block
// running top-k.  Included once per data type (scan_stream_<dt>.hip defines
// MVF_SCAN_DT) so the four dtypes compile in parallel.
//
// Replaces the per-row loop of reference examples/similarity_search.rs:147-169
// (get_vector + as_f32 + distance + heap push/pop) for 1..NQ queries at once.
//
// Mapping (gfx950, wave64):
//   * a row is pitch = V*16 bytes; G lanes (1/4/8/16/32/64) cooperate on one row,
//     each lane owning the 16-B vectors v = j*G + sub (j = 0..J-1), so one
//     wave-load instruction fetches 64/G rows x G*16 contiguous bytes
//     (1 KiB per instruction, fully coalesced, non-temporal: read once);
//   * U = 4 row groups are in flight per wave (4 x 16 B per lane per step);
//   * the query lives in LDS as f32 (or packed int8), zero-padded to J*G
//     vectors, read with one ds_read_b128 per step (broadcast across groups);
//   * per-row sums are finished with a G-lane xor butterfly;
//   * the score becomes an order key; a row survives only if its composite
//     (key<<32 | row) beats the block's current k-th best (tau) — survivors
//     are appended to an LDS buffer and merged by a bitonic sort at the end
//     of each chunk.  Scores never go to HBM; each block emits one sorted
//     list of k composites.
//
// Algorithmic HBM bytes: rows * dim * elem_size (+ nothing else of note).

#include "mvf_common.h"
#include "scan_stream.h"
#include "bitonic.h"
#include "query_i8s.h"
#include "query_16s.h"
#include "shadow_6b.h"
#include "shadow_5p1.h"
#include "margin_key.h"

#include <hip/hip_fp16.h>

#include <type_traits>

namespace mvf {
namespace {

template <int DT> struct DtTraits;
template <> struct DtTraits<MVF_DTYPE_FLOAT32> { static constexpr int ES = 4; static constexpr bool INT = false; using Q = float; using Acc = float; };
template <> struct DtTraits<MVF_DTYPE_FLOAT16> { static constexpr int ES = 2; static constexpr bool INT = false; using Q = float; using Acc = float; };
template <> struct DtTraits<MVF_DTYPE_INT8> { static constexpr int ES = 1; static constexpr bool INT = true; using Q = int8_t; using Acc = int32_t; };
template <> struct DtTraits<MVF_DTYPE_UINT8> { static constexpr int ES = 1; static constexpr bool INT = true; using Q = uint8_t; using Acc = int32_t; };

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int G, typename T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ int32_t dot4_i8(uint32_t a, uint32_t b, int32_t c) {
    return __builtin_amdgcn_sdot4((int)a, (int)b, c, false);
}
__device__ __forceinline__ int32_t dot4_u8(uint32_t a, uint32_t b, int32_t c) {
    return (int32_t)__builtin_amdgcn_udot4(a, b, (uint32_t)c, false);
}

#ifndef MVF_SCAN_XS
#define MVF_SCAN_XS 0
#endif
// XS: this translation unit scans the scaled-f16 SHADOW of a Float32 corpus (api.hip, scan path 4): every widened
// element is multiplied by the row's xscale[r] = 2^-s_r, so all three metrics see x~ = x (1 + e), |e| <= 2^-11.
constexpr bool XS = MVF_SCAN_XS != 0;
// QSK: the XS unit over INT8 rows = the int8 shadow of a Float32 / Float16 corpus (shadow_i8.hip): the f32 queries are
// quantised to int8 in the prologue (query_i8s.h), exact i32 dot products, FLOAT keys dot * xscale[r] * qaux0[q] (cosine: / (|q| |x_r|); L2: the
// GEMM-form squared distance qq + xx - 2 dot) for the margin compaction + exact re-scoring that follow.
constexpr bool QSK = XS && MVF_SCAN_DT == MVF_DTYPE_INT8;
// S6: the QSK unit over the 6-BIT shadow of a Float32 corpus (MVF_SCAN_XS == 2; shadow_6b.h has the layout, shadow_6b.hip the
// bound).  One lane per row (G = 1) and one query: a "step" j is a 64-element UNIT -- three wave-loads of one aligned KiB each,
// plane p of unit j of the tile's 64 rows -- ScanParams::pitch is the TILE's size and V = J the units per row.  The query is
// quantised to sixteen bits in the prologue (query_16s.h) and sits in LDS as two int8 planes in natural element order, 64
// bytes per unit each: per row two exact i32 sums, combined exactly with the per-query constant 32 sum Q, then QSK's keys.
constexpr bool S6 = QSK && (MVF_SCAN_XS == 2 || MVF_SCAN_XS == 3);
// S51: the S6 unit over the same codes in the 5+1 LAYOUT (MVF_SCAN_XS == 3; shadow_5p1.h): a step is a 128-element unit, five
// wave-loads of hi planes.  Two phases per wave iteration:
//   1. the hi planes of every row: 2 Q.hi exactly, and with P = sum max(Q, 0) (query_16s.h) the integer
//      D_best = 2 Q.hi + P - 32 sum Q >= Q.x6 -- the most the row's dot product can be whatever its low bits are.  key_best is
//      make_key of D_best: every float operation behind the integer is monotone in it (one int64 -> f32 rounding, products
//      with the non-negative s_r and s_q, Cosine: a division by a positive number or the constant 0, L2: a subtraction from a
//      value that does not depend on it), so key_best is never worse than the row's 6-bit key.
//   2. only for the rows whose key_best reaches the SKIP KEY: the lo plane (lane-masked 16-byte loads of the 8-lane groups holding such a row: only touched 128-byte lines
//      are requested), Q.lo exactly, and from there S6's integer, rounding and key.  The other rows are no candidates.
//      (The block's own running threshold does not enter the decision: it is the 128-th best of ~13 000 rows, 2.2 sigma on
//      the benchmark's corpus, where every 128-byte line holds a row that beats it -- it only filters the candidates, as on S6.)
// The skip key is margin_key (2 delta behind) of a bound of the search's k-th best 6-bit key: the k-th best of the bests the
// blocks PUBLISH (ScanParams::pub) -- k distinct live rows scored with all six bits.  Select_final's margin threshold is the
// same expression of the true k-th best, so no row it keeps is ever skipped, and the k-th best itself is unchanged.
constexpr bool S51 = QSK && MVF_SCAN_XS == 3;

// The skip key of the 5+1 unit, by ONE wave (the same value in every lane): the rank-th best of the keys published under `seq`
// among the first min(nb, 1024) blocks, rounded to the worse end of its 4096-key bucket, moved by the margin.  0xFFFFFFFF
// (every row needs its low bit) while fewer than `rank` blocks have published.  Stale words only weaken the bound.
__device__ __forceinline__ uint32_t skip_key_51(const uint64_t* pub, uint32_t nb, uint32_t seq, uint32_t rank, float delta, uint8_t metric, uint32_t lane) {
    uint32_t keys[16];
    uint32_t valid = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t b = (uint32_t)i * 64u + lane;
        uint64_t w = 0;
        if (b < nb) w = __hip_atomic_load(pub + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        keys[i] = (b < nb && (uint32_t)(w >> 32) == seq) ? (uint32_t)w : 0xFFFFFFFFu;
        valid += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(keys[i] != 0xFFFFFFFFu));
    }
    if (valid < rank || !(delta < 3.0e38f)) return 0xFFFFFFFFu;  // (a non-finite query: every row is kept, as on the 6-bit unit)
    uint32_t lo = 0, hi = 0xFFFFFu;  // the smallest 20-bit prefix with at least `rank` keys at or in front of it
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        uint32_t c = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) c += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64((keys[i] >> 12) <= mid));
        if (c >= rank) hi = mid;
        else lo = mid + 1;
    }
    return margin_key((lo << 12) | 0xFFFu, delta, metric);
}

// Short rows (G <= 8: one step per row) are latency-bound -- a wave has 4 KiB in flight and its iteration is load -> wait ->
// sums -> keys in sequence -- so those instantiations of the narrow types ask for more waves per SIMD than the 3-4 the
// compiler would settle on.  Rounds 1-3 asked for 8 (64 registers: 1-31 of them spilled, outside the row loop --
// profiles/r04_kernel_spill_sites.csv); since round 3's long guarded pieces and reduce-scatter the iteration is shorter and
// FIVE waves on 96 registers, nothing spilled, are as fast or faster on every short shape (profiles/r04_k1_spill_ab.txt:
// 64-B Int8 rows 5.9-6.2 -> 6.4-6.6 TB/s, 16-B Float16 rows 4.3-4.6 -> 5.4-5.6, 128-B rows equal).  Not the Float32 ones:
// they lost 8 % at 64 registers and run at the compiler's choice.
// FLOOR: a pass of a k > MVFGPU_K_PER_PASS search (ScanParams::floor1) -- its own instantiation, so that the ordinary
// kernels carry neither the two registers nor the subtraction (the 64-register variants of short rows spill as it is).
#ifndef MVF_K1_SHORT_ROW_WAVES
#define MVF_K1_SHORT_ROW_WAVES 5  // A/B builds: -DMVF_K1_SHORT_ROW_WAVES=8|7|6|1
#endif
template <int DT, int METRIC, int G, int NQ, bool REDO = false, bool FLOOR = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(S51 ? 3 : (G <= 8 && NQ == 1 && DT != MVF_DTYPE_FLOAT32 && !S6) ? MVF_K1_SHORT_ROW_WAVES : 1, 8)))
scan_stream_kernel(ScanParams p) {
    using Tr = DtTraits<DT>;
    using Acc = typename Tr::Acc;
    constexpr int ES = Tr::ES;
    static_assert(!S6 || (G == 1 && NQ == 1 && !REDO && !FLOOR), "the 6-bit unit: one lane per row, one query");
    constexpr int EPV = S51 ? 128 : S6 ? 64 : 16 / ES;  // corpus elements per 16-B vector (S6: per unit)
    constexpr int RPG = 64 / G;   // rows per wave-load
    // row groups in flight per wave (8 for one-step rows measured SLOWER: 128-B rows 4.4 vs 5.3 TB/s).  S51: TWO tiles -- five
    // planes of a unit each, 10 KiB in flight per wave -- beside the 64 registers of a unit's query planes
    constexpr int U = S51 ? 2 : 4;
    constexpr int QB = S51 ? 256 : S6 ? 128 : Tr::INT ? 16 : EPV * 4;  // query bytes per corpus vector in LDS (S6: per unit, both planes)
    constexpr bool NEED_XX = !QSK && ((METRIC == MVF_METRIC_COSINE) || (Tr::INT && METRIC == MVF_METRIC_L2));
    constexpr bool NEED_QQ = NEED_XX;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane % G, rsel = lane / G;

    const uint32_t VP = p.J * G;  // padded vectors per row held in LDS
    unsigned char* qs = smem;     // [NQ][VP*QB]
    const uint32_t qstride = VP * QB;
    // (QSK: the first 24 floats of bufs are the scratch of the prologue's reductions -- bufs is first written in the row loop,
    // behind the barrier that ends the staging, and pmax >= 512 entries)
    uint64_t* bufs = reinterpret_cast<uint64_t*>(smem + ((NQ * qstride + 15u) & ~15u));  // [NQ][p.pmax]
    uint32_t* cnt = reinterpret_cast<uint32_t*>(bufs + (size_t)NQ * p.pmax);              // [NQ]
    uint32_t* kprev = cnt + NQ;                                                            // [NQ]
    float* red = reinterpret_cast<float*>(kprev + NQ);                                     // [NQ][4] qq partials
    uint64_t* tau = reinterpret_cast<uint64_t*>(red + NQ * 4);                             // [NQ] (8-B aligned by layout)
    [[maybe_unused]] uint32_t* s51w = reinterpret_cast<uint32_t*>(tau + NQ);  // S51: lo lines fetched, lo lines scanned, the skip key, delta's bits

    // Repair launches walk their flagged queries in groups of NQ, one pass over the rows per group; an ordinary launch
    // is the single group of its NQ queries.
    // (small corpora: several passes in ONE launch, pass blockIdx.y scanning for queries q0 .. q0 + NQ - 1 -- api.hip)
    const uint32_t pass = REDO ? 0u : blockIdx.y, q0 = p.q0 + pass * NQ;
    uint32_t avail = NQ, ngroups = 1;
    if constexpr (REDO) {
        const uint32_t nredo = *p.redo_cnt;
        avail = nredo > p.redo_base ? min(nredo - p.redo_base, p.redo_max) : 0u;
        if (avail == 0) return;  // the common case: nothing overflowed
        ngroups = (avail + NQ - 1) / NQ;
    }
    // (profiled searches: block 0 is dispatched first -- a plain store.  Every block folding a minimum into one word at the
    // same moment held its first row loads back behind the atomic: profiles/r07_stream_fixed_cost.txt)
    if (p.ts && tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) p.ts[0] = (uint64_t)wall_clock64();
    for (uint32_t grp = 0; grp < ngroups; grp++) {
    if (REDO && grp) __syncthreads();  // the previous group's lists have left LDS
    // ---- stage the queries in LDS (f32 / packed int8, zero padded) -----------
    Acc qq_part[NQ];
    float qsf[NQ], qnf[NQ];  // QSK: query scale and |q|
    [[maybe_unused]] int64_t qbias6 = 0;  // S6: 32 sum Q
    [[maybe_unused]] int64_t qpos51 = 0;  // S51: P = sum max(Q, 0)
    [[maybe_unused]] uint32_t pub_last = 0xFFFFFFFFu;  // S51, thread 0: the key this block published last
    // composites at or in front of the query's floor are not candidates (passes of a k > 1024 search); as ONE unsigned
    // compare: (comp - fl1) < (tau - fl1) with fl1 = floor + 1, which is comp < tau without a floor (fl1 = 0) and rejects
    // comp <= floor by wrapping (tau > floor always: the k-th best of the rows behind the floor, or the padding value)
    [[maybe_unused]] uint64_t fl1[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) qq_part[q] = 0, qsf[q] = 1.f, qnf[q] = 0.f, fl1[q] = 0;
    if constexpr (QSK) {
        // the caller's f32 queries are quantised here, by every block for itself (3 KiB of L2 hits per query against the
        // launch the stand-alone preparation cost in front of every search of one to four queries); block 0 leaves what
        // the margin select behind this launch reads.  The reductions' scratch is the head of the (still empty) candidate
        // buffers: a static array would count against the 160 KiB the dynamic LDS of the short-row shapes is raised to.
        float* prep_red = reinterpret_cast<float*>(bufs);
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const uint32_t qi = min(q0 + q, p.nq_total - 1u);  // padding lanes repeat the last query
            const bool owner = blockIdx.x == 0 && blockIdx.y == 0 && q0 + q < p.nq_total;
            float d = 0.f;
            if constexpr (S6) {  // both planes: lo at qs, hi behind it (VP * 64 bytes each)
                int32_t qsum = 0;
                if constexpr (S51) {  // every block moves its skip key by the query's bound: thread 0 of each computes it
                    int32_t qpos = 0;
                    prep_query_16s(reinterpret_cast<const float*>(p.queries) + (size_t)qi * p.dim, p.dim, VP * EPV, METRIC, p.qstats, p.xxmax,
                                   reinterpret_cast<int8_t*>(qs), reinterpret_cast<int8_t*>(qs) + VP * EPV, prep_red, true, &qsf[q], &qnf[q], &qsum, &d, &qpos);
                    qpos51 = qpos;
                    if (tid == 0) s51w[0] = 0, s51w[1] = 0, s51w[2] = 0xFFFFFFFFu, s51w[3] = __float_as_uint(d);
                } else
                prep_query_16s(reinterpret_cast<const float*>(p.queries) + (size_t)qi * p.dim, p.dim, VP * EPV, METRIC, p.qstats, p.xxmax,
                               reinterpret_cast<int8_t*>(qs), reinterpret_cast<int8_t*>(qs) + VP * EPV, prep_red, owner, &qsf[q], &qnf[q], &qsum, &d);
                qbias6 = (int64_t)kS6Bias * qsum;
            } else
            prep_query_i8s(reinterpret_cast<const float*>(p.queries) + (size_t)qi * p.dim, p.dim, VP * EPV, METRIC, p.qstats, p.xxmax,
                           reinterpret_cast<int8_t*>(qs + q * qstride), prep_red + (q & 1) * 12, owner, &qsf[q], &qnf[q], &d);
            if (owner && tid == 0) {
                p.qaux0[qi] = qsf[q];
                p.qaux1[qi] = qnf[q];
                p.qdelta[qi] = d;
            }
        }
    } else {
        const uint32_t nelem = VP * EPV;
        using QT = typename std::conditional<Tr::INT, typename Tr::Q, float>::type;
        const QT* src[NQ];
        QT* dst[NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            uint32_t qi = q0 + q;
            if (qi >= p.nq_total) qi = p.nq_total - 1;  // padding lanes repeat the last query
            if constexpr (REDO) qi = p.redo_list[p.redo_base + min(grp * NQ + q, avail - 1u)];
            if constexpr (FLOOR) fl1[q] = p.floor1 ? p.floor1[qi] : 0;
            src[q] = reinterpret_cast<const QT*>(p.queries) + (size_t)qi * p.dim;
            dst[q] = reinterpret_cast<QT*>(qs + q * qstride);
        }
        // the NQ queries' elements are fetched together (NQ loads in flight per step, not one query after the other: on a
        // small corpus the staging is a visible share of the launch); each query's sum of squares keeps its own order
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
    Acc qq[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        Acc s = group_sum<64>(qq_part[q]);
        if (lane == 0) reinterpret_cast<Acc*>(red)[q * 4 + wave] = s;
    }
    if (tid < NQ) {
        cnt[tid] = 0;
        kprev[tid] = 0;
        tau[tid] = kPadComposite;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        const Acc* r = reinterpret_cast<const Acc*>(red) + q * 4;
        qq[q] = r[0] + r[1] + r[2] + r[3];
    }
    (void)qq;

    const unsigned char* rows = p.rows;

    // A chunk (chunk_rows rows; the unit blocks take turns on) is scanned in PIECES, each ended by a barrier and the merge
    // of its survivors.  The candidate buffer holds pmax - kprev survivors; a piece of p.chunk_safe rows (k + chunk_safe <=
    // pmax) can never overflow it.  Short rows want long pieces -- a wave covers 4 * 64/G rows per iteration and every
    // barrier starts from an empty memory pipeline -- so once every threshold is set the block takes the REST of the chunk
    // as one piece and pushes guardedly: if more rows beat the threshold than the buffer holds (rows arriving best-last),
    // the piece's survivors (of every query of the pass) are dropped and the same rows are scanned again in safe pieces.
    // Hosts that pass chunk_rows == chunk_safe (rows of more than 16 steps per 512-row chunk) get exactly one piece per
    // chunk.
    // While a threshold is unset every row survives: a 512-row first piece meant a bitonic sort of 512 entries per query (13 us
    // a query -- on a corpus of one chunk per block a quarter of a one-query search and half of a four-query pass), so the
    // pieces stay at p.first_piece rows (>= k, counting-merge sized) until every query has its threshold.
    for (uint32_t chunk = blockIdx.x; chunk < p.nchunks; chunk += gridDim.x) {
      const uint32_t cend = (chunk + 1) * p.chunk_rows;
      bool safe_only = false;
      [[maybe_unused]] bool skip_fresh = false;  // S51: the skip key was read for this chunk
      for (uint32_t c0 = chunk * p.chunk_rows; c0 < cend && c0 < p.n;) {
        [[maybe_unused]] uint32_t kskip = 0xFFFFFFFFu;
        [[maybe_unused]] uint32_t lo_fetched = 0, lo_total = 0;  // S51, wave-uniform: this piece's low-plane lines
        if constexpr (S51) {
            // the published bests are read at the start of a chunk, and in front of every piece while there is no skip key yet
            // (block-uniform: s51w[2] was last written in front of a barrier)
            if (!skip_fresh || s51w[2] == 0xFFFFFFFFu) {
                __syncthreads();  // (every wave has read the old key)
                if (wave == 0) {
                    const uint32_t kk = skip_key_51(p.pub, gridDim.x, p.pub_seq, p.skip_rank, __uint_as_float(s51w[3]), (uint8_t)METRIC, (uint32_t)lane);
                    if (lane == 0) s51w[2] = kk;
                }
                __syncthreads();
                skip_fresh = true;
            }
            kskip = s51w[2];
        }
        uint64_t tau_r[NQ];
        uint32_t kprev_r[NQ];
        bool all_set = true;
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            tau_r[q] = tau[q];
            kprev_r[q] = kprev[q];
            all_set = all_set && tau_r[q] != kPadComposite;
            if constexpr (FLOOR) tau_r[q] -= fl1[q];  // from here on the threshold is relative to the floor, as the composites tested against it
        }
        if constexpr (S51) all_set = all_set || kskip != 0xFFFFFFFFu;  // with a skip key few rows survive whatever the block's own threshold: long guarded pieces
        const uint32_t piece_rows = (all_set && !safe_only) ? cend - c0 : min((all_set || p.first_piece == 0) ? p.chunk_safe : p.first_piece, cend - c0);
        const uint32_t groups_per_chunk = piece_rows / RPG;

        for (uint32_t g0 = wave * U; g0 < groups_per_chunk; g0 += 4 * U) {
            uint32_t r[U];
            const unsigned char* rp[U];
            bool rv[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                r[u] = c0 + (g0 + u) * RPG + rsel;
                rv[u] = r[u] < p.n;
                rp[u] = rows + (size_t)(rv[u] ? r[u] : 0u) * p.pitch;
                if constexpr (S6) rp[u] = rows + (size_t)((rv[u] ? r[u] : 0u) / kS6TileRows) * p.pitch + (size_t)lane * 16;  // the row's 16 bytes in plane 0 of unit 0 of its tile
            }
            Acc acc[U][NQ];
            [[maybe_unused]] int32_t acch[U];  // S6: the high plane's sums
            Acc xx[U];
            float rs[U], rn[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                rs[u] = 1.0f;
                rn[u] = 0.0f;
                if constexpr (XS) rs[u] = rv[u] ? p.xscale[r[u]] : 0.0f;
                if constexpr (QSK && METRIC != MVF_METRIC_INNER_PRODUCT) rn[u] = rv[u] ? p.xrow[r[u]] : 0.0f;
                xx[u] = 0;
                acch[u] = 0;
#pragma unroll
                for (int q = 0; q < NQ; q++) acc[u][q] = 0;
            }

            if constexpr (S51) {
                for (uint32_t j = 0; j < p.J; j++) {
                    u32x4 x[U][5];
#pragma unroll
                    for (int u = 0; u < U; u++)
#pragma unroll
                        for (int pl = 0; pl < 5; pl++) {
                            x[u][pl] = u32x4{0, 0, 0, 0};
                            if (rv[u]) x[u][pl] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(rp[u] + ((size_t)j * 5 + pl) * 1024));
                        }
                    // the unit's 128 query elements in two halves of 64 (32 registers of query at a time): [g] = elements 16 g .. 16 g + 15
#pragma unroll
                    for (int gh = 0; gh < 2; gh++) {
                        u32x4 ql[4], qh[4];
#pragma unroll
                        for (int g = 0; g < 4; g++) {
                            ql[g] = *reinterpret_cast<const u32x4*>(qs + j * 128 + (gh * 4 + g) * 16);
                            qh[g] = *reinterpret_cast<const u32x4*>(qs + VP * 128 + j * 128 + (gh * 4 + g) * 16);
                        }
#pragma unroll
                        for (int u = 0; u < U; u++)
#pragma unroll
                            for (int i = 0; i < 4; i++) {
                                const uint32_t p0 = x[u][0][i], p1 = x[u][1][i], p2 = x[u][2][i], p3 = x[u][3][i], p4 = x[u][4][i];
                                uint32_t y[4];  // hi of the elements 16 (4 gh + g) + 4 i .. + 3 (shadow_5p1.h)
                                if (gh == 0) {
                                    y[0] = p0 & 0x1F1F1F1Fu, y[1] = p1 & 0x1F1F1F1Fu, y[2] = p2 & 0x1F1F1F1Fu, y[3] = p3 & 0x1F1F1F1Fu;
                                } else {
                                    y[0] = p4 & 0x1F1F1F1Fu;
                                    y[1] = ((p0 >> 5) & 0x07070707u) | ((p1 >> 2) & 0x18181818u);
                                    y[2] = ((p1 >> 7) & 0x01010101u) | ((p2 >> 4) & 0x0E0E0E0Eu) | ((p3 >> 1) & 0x10101010u);
                                    y[3] = ((p3 >> 6) & 0x03030303u) | ((p4 >> 3) & 0x1C1C1C1Cu);
                                }
#pragma unroll
                                for (int g = 0; g < 4; g++) {
                                    acc[u][0] = dot4_i8(ql[g][i], y[g], acc[u][0]);
                                    acch[u] = dot4_i8(qh[g][i], y[g], acch[u]);
                                }
                            }
                    }
                }
            } else if constexpr (S6) {
                for (uint32_t j = 0; j < p.J; j++) {
                    u32x4 x[U][3];
#pragma unroll
                    for (int u = 0; u < U; u++)
#pragma unroll
                        for (int pl = 0; pl < 3; pl++) {
                            x[u][pl] = u32x4{0, 0, 0, 0};
                            if (rv[u]) x[u][pl] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(rp[u] + ((size_t)j * 3 + pl) * 1024));
                        }
                    u32x4 ql[4], qh[4];  // the unit's 64 query elements, low and high plane: [i] = elements 16 i .. 16 i + 15
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        ql[i] = *reinterpret_cast<const u32x4*>(qs + j * 64 + i * 16);
                        qh[i] = *reinterpret_cast<const u32x4*>(qs + VP * 64 + j * 64 + i * 16);
                    }
#pragma unroll
                    for (int u = 0; u < U; u++)
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const uint32_t p0 = x[u][0][i], p1 = x[u][1][i], p2 = x[u][2][i];
                            const uint32_t ya = p0 & 0x3F3F3F3Fu, yb = p1 & 0x3F3F3F3Fu, yc = p2 & 0x3F3F3F3Fu;
                            const uint32_t yd = ((p0 >> 6) & 0x03030303u) | ((p1 >> 4) & 0x0C0C0C0Cu) | ((p2 >> 2) & 0x30303030u);
                            acc[u][0] = dot4_i8(ql[0][i], ya, acc[u][0]);
                            acc[u][0] = dot4_i8(ql[1][i], yb, acc[u][0]);
                            acc[u][0] = dot4_i8(ql[2][i], yc, acc[u][0]);
                            acc[u][0] = dot4_i8(ql[3][i], yd, acc[u][0]);
                            acch[u] = dot4_i8(qh[0][i], ya, acch[u]);
                            acch[u] = dot4_i8(qh[1][i], yb, acch[u]);
                            acch[u] = dot4_i8(qh[2][i], yc, acch[u]);
                            acch[u] = dot4_i8(qh[3][i], yd, acch[u]);
                        }
                }
            } else
            for (uint32_t j = 0; j < p.J; j++) {
                const uint32_t v = j * G + sub;
                const bool vv = v < p.V;
                u32x4 x[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    x[u] = u32x4{0, 0, 0, 0};
                    if (vv && rv[u])
                        x[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(rp[u] + (size_t)v * 16));
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
                            // exact widening, as half::f16::to_f32 (reference src/vectors/vector.rs:85-86)
                            xf[u][2 * i] = __half2float(__ushort_as_half((unsigned short)(w[i] & 0xFFFFu)));
                            xf[u][2 * i + 1] = __half2float(__ushort_as_half((unsigned short)(w[i] >> 16)));
                            if constexpr (XS) {
                                xf[u][2 * i] *= rs[u];
                                xf[u][2 * i + 1] *= rs[u];
                            }
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
                } else {  // Int8 / UInt8: exact i32 via packed dot4
#pragma unroll
                    for (int q = 0; q < NQ; q++) {
                        const uint4 qv = *reinterpret_cast<const uint4*>(qs + q * qstride + v * 16);
#pragma unroll
                        for (int u = 0; u < U; u++) {
                            if constexpr (DT == MVF_DTYPE_INT8) {
                                acc[u][q] = dot4_i8(qv.x, x[u].x, acc[u][q]);
                                acc[u][q] = dot4_i8(qv.y, x[u].y, acc[u][q]);
                                acc[u][q] = dot4_i8(qv.z, x[u].z, acc[u][q]);
                                acc[u][q] = dot4_i8(qv.w, x[u].w, acc[u][q]);
                            } else {
                                acc[u][q] = dot4_u8(qv.x, x[u].x, acc[u][q]);
                                acc[u][q] = dot4_u8(qv.y, x[u].y, acc[u][q]);
                                acc[u][q] = dot4_u8(qv.z, x[u].z, acc[u][q]);
                                acc[u][q] = dot4_u8(qv.w, x[u].w, acc[u][q]);
                            }
                        }
                    }
                    if constexpr (NEED_XX) {
#pragma unroll
                        for (int u = 0; u < U; u++) {
                            if constexpr (DT == MVF_DTYPE_INT8) {
                                xx[u] = dot4_i8(x[u].x, x[u].x, xx[u]);
                                xx[u] = dot4_i8(x[u].y, x[u].y, xx[u]);
                                xx[u] = dot4_i8(x[u].z, x[u].z, xx[u]);
                                xx[u] = dot4_i8(x[u].w, x[u].w, xx[u]);
                            } else {
                                xx[u] = dot4_u8(x[u].x, x[u].x, xx[u]);
                                xx[u] = dot4_u8(x[u].y, x[u].y, xx[u]);
                                xx[u] = dot4_u8(x[u].z, x[u].z, xx[u]);
                                xx[u] = dot4_u8(x[u].w, x[u].w, xx[u]);
                            }
                        }
                    }
                }
            }

            // ---- finish the rows: G-lane sums, score -> key, threshold filter
            auto make_key = [&](Acc s, Acc xxs, Acc qqv, float rsv, float rnv, float sqv, float qnv) __attribute__((always_inline)) -> uint32_t {
                if constexpr (QSK) {
                    // (S6: `s` carries the bits of the f32 the exact combine of the two planes was rounded to)
                    const float dotf = (S6 ? __int_as_float((int)s) : (float)s) * rsv * sqv;
                    float sc;
                    if constexpr (METRIC == MVF_METRIC_INNER_PRODUCT) sc = dotf;
                    else if constexpr (METRIC == MVF_METRIC_COSINE) {
                        const float den = qnv * rnv;
                        sc = den > 0.0f ? dotf / den : 0.0f;
                    } else sc = qnv * qnv + rnv - 2.0f * dotf;  // GEMM-form squared distance (the re-scoring takes the root)
                    return key_from_score(sc, METRIC);
                } else if constexpr (Tr::INT) {
                    if constexpr (METRIC == MVF_METRIC_L2) {
                        return key_from_raw(qqv + xxs - 2 * s, METRIC);
                    } else if constexpr (METRIC == MVF_METRIC_INNER_PRODUCT) {
                        return key_from_raw(s, METRIC);
                    } else {
                        const float den = sqrtf((float)qqv) * sqrtf((float)xxs);
                        return key_from_score(den > 0.0f ? (float)s / den : 0.0f, METRIC);
                    }
                } else {
                    float sc;
                    if constexpr (METRIC == MVF_METRIC_L2) {
                        sc = sqrtf(s);
                    } else if constexpr (METRIC == MVF_METRIC_INNER_PRODUCT) {
                        sc = s;
                    } else {
                        const float den = sqrtf(qqv) * sqrtf(xxs);
                        sc = den > 0.0f ? s / den : 0.0f;
                    }
                    return key_from_score(sc, METRIC);
                }
            };
            // DUMP launches of the floor instantiation (ScanParams::dump): the row's key leaves for HBM as a rank entry
            // (mvf_common.h: position << 32 | key, a deleted row marked dead -- it sorts behind every row, NaN scores included)
            [[maybe_unused]] auto dump_row = [&](int ql, uint32_t rl, uint64_t comp) __attribute__((always_inline)) {
                const bool dead = p.tomb && ((p.tomb[rl >> 5] >> (rl & 31)) & 1u);
                p.dump[(size_t)ql * p.n + rl] = rank_entry((uint32_t)(comp >> 32), rl, dead);
            };
            if constexpr (S51) {
                // phase 1's verdict: which rows can still matter (the comment at S51)
                bool need[U];
                unsigned long long bal[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int64_t dbest = 2ll * (128ll * (int64_t)acch[u] + (int64_t)acc[u][0]) + qpos51 - qbias6;
                    const uint32_t kbest = make_key((Acc)__float_as_int((float)dbest), 0, qq[0], rs[u], rn[u], qsf[0], qnf[0]);
                    need[u] = rv[u] && kbest <= kskip;
                    bal[u] = __builtin_amdgcn_ballot_w64(need[u]);
                    const unsigned long long live = __builtin_amdgcn_ballot_w64(rv[u]);  // (the last tile: only the lines that hold rows)
#pragma unroll
                    for (int g = 0; g < 8; g++) lo_total += ((live >> (8 * g)) & 0xFFull) != 0 ? p.J : 0u;
                }
                // phase 2, per tile that holds such a row
#pragma unroll
                for (int u = 0; u < U; u++) {
                    if (bal[u] == 0) continue;  // wave-uniform
                    const bool grp = ((bal[u] >> (lane & 56)) & 0xFFull) != 0;  // a row of this lane's 128-byte line needs its bit
                    uint32_t lines = 0;
#pragma unroll
                    for (int g = 0; g < 8; g++) lines += ((bal[u] >> (8 * g)) & 0xFFull) != 0 ? 1u : 0u;
                    lo_fetched += lines * p.J;
                    int32_t bl = 0, bh = 0;
                    const unsigned char* lop = rp[u] + (size_t)p.J * 5u * 1024u;  // the tile's lo planes, this row's 16 bytes
                    constexpr int LB = 6;  // lo planes per round trip (768 dimensions: all of them)
                    for (uint32_t j0 = 0; j0 < p.J; j0 += LB) {
                        u32x4 lo[LB];
#pragma unroll
                        for (int jj = 0; jj < LB; jj++) {
                            lo[jj] = u32x4{0, 0, 0, 0};
                            if (grp && j0 + jj < p.J) lo[jj] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(lop + (size_t)(j0 + jj) * 1024));
                        }
#pragma unroll
                        for (int jj = 0; jj < LB; jj++) {
                            if (j0 + jj >= p.J) break;  // wave-uniform
                            if (!need[u]) continue;
                            const uint32_t j = j0 + jj;
#pragma unroll
                            for (int g = 0; g < 8; g++) {
                                const u32x4 qlg = *reinterpret_cast<const u32x4*>(qs + j * 128 + g * 16);
                                const u32x4 qhg = *reinterpret_cast<const u32x4*>(qs + VP * 128 + j * 128 + g * 16);
#pragma unroll
                                for (int i = 0; i < 4; i++) {  // elements 16 g + 4 i .. + 3: bits m, m + 8, m + 16, m + 24 of dword g / 2, m = 4 (g & 1) + i
                                    const uint32_t yl = (lo[jj][g >> 1] >> (4 * (g & 1) + i)) & 0x01010101u;
                                    bl = dot4_i8(qlg[i], yl, bl);
                                    bh = dot4_i8(qhg[i], yl, bh);
                                }
                            }
                        }
                    }
                    // Q.y = 2 Q.hi + Q.lo, exact: from here S6's integer, its one rounding and its key
                    const Acc s = (Acc)__float_as_int((float)(128ll * (2ll * (int64_t)acch[u] + (int64_t)bh) + 2ll * (int64_t)acc[u][0] + (int64_t)bl - qbias6));
                    const uint64_t comp = ((uint64_t)make_key(s, 0, qq[0], rs[u], rn[u], qsf[0], qnf[0]) << 32) | r[u];
                    if (need[u] && comp < tau_r[0] && !(p.tomb && ((p.tomb[r[u] >> 5] >> (r[u] & 31)) & 1u))) {
                        const uint32_t slot = atomicAdd(&cnt[0], 1u);
                        if (kprev_r[0] + slot < p.pmax) bufs[kprev_r[0] + slot] = comp;
                    }
                }
            } else if constexpr (NQ == 4 && U == 4 && G >= 16) {
                // Sixteen (row u, query q) sums per group.  A butterfly would leave all of them in every lane and the
                // key arithmetic (two sqrt and a divide for cosine) would run 16 times per lane -- that made this
                // variant VALU-bound at half the HBM rate.  REDUCE-SCATTER instead: each of the first four steps
                // halves the values a lane carries, so lane `sub` ends with the total of ONE pair p = u 4 + q
                // (p = sub >> 2 for G = 64, sub for G = 16) and the key is computed once for all pairs.  The pairing of
                // partial sums (xor G/2, G/4, ...) is the butterfly's, so the totals are bit-identical to NQ = 1.
                const bool h0 = (sub & (G / 2)) != 0, h1 = (sub & (G / 4)) != 0, h2 = (sub & (G / 8)) != 0,
                           h3 = (sub & (G / 16)) != 0;
                Acc v8[8], v4[4], v2[2], s1;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const Acc lo = acc[i >> 2][i & 3], hi = acc[(i + 8) >> 2][(i + 8) & 3];
                    v8[i] = (h0 ? hi : lo) + __shfl_xor(h0 ? lo : hi, G / 2, 64);
                }
#pragma unroll
                for (int i = 0; i < 4; i++) v4[i] = (h1 ? v8[i + 4] : v8[i]) + __shfl_xor(h1 ? v8[i] : v8[i + 4], G / 4, 64);
#pragma unroll
                for (int i = 0; i < 2; i++) v2[i] = (h2 ? v4[i + 2] : v4[i]) + __shfl_xor(h2 ? v4[i] : v4[i + 2], G / 8, 64);
                s1 = (h3 ? v2[1] : v2[0]) + __shfl_xor(h3 ? v2[0] : v2[1], G / 16, 64);
#pragma unroll
                for (int off = G / 32; off > 0; off >>= 1) s1 += __shfl_xor(s1, off, 64);
                Acc xx1 = 0;
                if constexpr (NEED_XX) {  // four row sums: the lane ends with its pair's row u = (h0, h1)
                    Acc x2[2];
#pragma unroll
                    for (int i = 0; i < 2; i++) x2[i] = (h0 ? xx[i + 2] : xx[i]) + __shfl_xor(h0 ? xx[i] : xx[i + 2], G / 2, 64);
                    xx1 = (h1 ? x2[1] : x2[0]) + __shfl_xor(h1 ? x2[0] : x2[1], G / 4, 64);
#pragma unroll
                    for (int off = G / 8; off > 0; off >>= 1) xx1 += __shfl_xor(xx1, off, 64);
                }
                const int ul = (h0 ? 2 : 0) + (h1 ? 1 : 0), ql = (h2 ? 2 : 0) + (h3 ? 1 : 0);
                const Acc qqv = ql == 0 ? qq[0] : ql == 1 ? qq[1] : ql == 2 ? qq[2] : qq[3];
                const float sqv = ql == 0 ? qsf[0] : ql == 1 ? qsf[1] : ql == 2 ? qsf[2] : qsf[3];
                const float qnv = ql == 0 ? qnf[0] : ql == 1 ? qnf[1] : ql == 2 ? qnf[2] : qnf[3];
                const float rsv = ul == 0 ? rs[0] : ul == 1 ? rs[1] : ul == 2 ? rs[2] : rs[3];
                const float rnv = ul == 0 ? rn[0] : ul == 1 ? rn[1] : ul == 2 ? rn[2] : rn[3];
                const uint64_t tauv = ql == 0 ? tau_r[0] : ql == 1 ? tau_r[1] : ql == 2 ? tau_r[2] : tau_r[3];
                [[maybe_unused]] const uint64_t flv = !FLOOR ? 0 : ql == 0 ? fl1[0] : ql == 1 ? fl1[1] : ql == 2 ? fl1[2] : fl1[3];
                const uint32_t kpv = ql == 0 ? kprev_r[0] : ql == 1 ? kprev_r[1] : ql == 2 ? kprev_r[2] : kprev_r[3];
                const uint32_t rl = c0 + (g0 + ul) * RPG + rsel;
                const uint64_t comp = ((uint64_t)make_key(s1, xx1, qqv, rsv, rnv, sqv, qnv) << 32) | rl;
                if constexpr (FLOOR) {
                    if (p.dump) {  // launch-uniform: rank every row (search_sorted_k)
                        if ((sub & (G / 16 - 1)) == 0 && rl < p.n && q0 + ql < p.nq_total) dump_row(ql, rl, comp);
                        continue;
                    }
                }
                // a deleted row (TombstoneInfo, schema/core.fbs:35-39) never becomes a candidate; the bitmap is read
                // only for the rare rows that beat the running threshold
                if ((sub & (G / 16 - 1)) == 0 && rl < p.n && (FLOOR ? comp - flv : comp) < tauv && !(p.tomb && ((p.tomb[rl >> 5] >> (rl & 31)) & 1u))) {
                    const uint32_t slot = atomicAdd(&cnt[ql], 1u);
                    if (kpv + slot < p.pmax) bufs[(size_t)ql * p.pmax + kpv + slot] = comp;
                }
            } else if constexpr (NQ == 4 && U == 4 && (G == 8 || G == 4)) {
                // The same reduce-scatter on the narrow groups of short rows: 8 lanes end with one row and TWO of the four
                // queries each (three halving steps: 8 + 4 + 2 exchanges instead of 16 sums x 3, two keys per lane instead
                // of sixteen), 4 lanes with one row and all four queries (8 + 4 exchanges, four keys).  Same pairing of the
                // partial sums as the butterfly (xor G/2, ..., 1): bit-identical totals.  (The generic branch below held
                // the four-query pass at 2 TB/s on rows of <= 128 B.)
                constexpr int NK = G == 8 ? 2 : 4;  // keys per lane
                const bool h0 = (sub & (G / 2)) != 0, h1 = (sub & (G / 4)) != 0;
                [[maybe_unused]] const bool h2 = G == 8 && (sub & 1) != 0;
                Acc v8[8], v4[4], vk[NK];
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const Acc lo = acc[i >> 2][i & 3], hi = acc[(i + 8) >> 2][(i + 8) & 3];
                    v8[i] = (h0 ? hi : lo) + __shfl_xor(h0 ? lo : hi, G / 2, 64);
                }
#pragma unroll
                for (int i = 0; i < 4; i++) v4[i] = (h1 ? v8[i + 4] : v8[i]) + __shfl_xor(h1 ? v8[i] : v8[i + 4], G / 4, 64);
                if constexpr (G == 8) {
#pragma unroll
                    for (int i = 0; i < 2; i++) vk[i] = (h2 ? v4[i + 2] : v4[i]) + __shfl_xor(h2 ? v4[i] : v4[i + 2], 1, 64);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++) vk[i] = v4[i];
                }
                Acc xx1 = 0;
                if constexpr (NEED_XX) {  // four row sums: the lane ends with its row u = (h0, h1)
                    Acc x2[2];
#pragma unroll
                    for (int i = 0; i < 2; i++) x2[i] = (h0 ? xx[i + 2] : xx[i]) + __shfl_xor(h0 ? xx[i] : xx[i + 2], G / 2, 64);
                    xx1 = (h1 ? x2[1] : x2[0]) + __shfl_xor(h1 ? x2[0] : x2[1], G / 4, 64);
                    if constexpr (G == 8) xx1 += __shfl_xor(xx1, 1, 64);
                }
                const int ul = (h0 ? 2 : 0) + (h1 ? 1 : 0);
                const float rsv = ul == 0 ? rs[0] : ul == 1 ? rs[1] : ul == 2 ? rs[2] : rs[3];
                const float rnv = ul == 0 ? rn[0] : ul == 1 ? rn[1] : ul == 2 ? rn[2] : rn[3];
                const uint32_t rl = c0 + (g0 + ul) * RPG + rsel;
#pragma unroll
                for (int i = 0; i < NK; i++) {
                    // query of key i: 2 h2 + i on 8 lanes (a two-way choice per lane), i on 4 lanes
                    const Acc qqv = G == 8 ? (h2 ? qq[2 + (i & 1)] : qq[i & 1]) : qq[i & 3];
                    const float sqv = G == 8 ? (h2 ? qsf[2 + (i & 1)] : qsf[i & 1]) : qsf[i & 3];
                    const float qnv = G == 8 ? (h2 ? qnf[2 + (i & 1)] : qnf[i & 1]) : qnf[i & 3];
                    const uint64_t tauv = G == 8 ? (h2 ? tau_r[2 + (i & 1)] : tau_r[i & 1]) : tau_r[i & 3];
                    [[maybe_unused]] const uint64_t flv = !FLOOR ? 0 : G == 8 ? (h2 ? fl1[2 + (i & 1)] : fl1[i & 1]) : fl1[i & 3];
                    const uint32_t kpv = G == 8 ? (h2 ? kprev_r[2 + (i & 1)] : kprev_r[i & 1]) : kprev_r[i & 3];
                    const int ql = G == 8 ? (h2 ? 2 : 0) + i : i;
                    const uint64_t comp = ((uint64_t)make_key(vk[i], xx1, qqv, rsv, rnv, sqv, qnv) << 32) | rl;
                    if constexpr (FLOOR) {
                        if (p.dump) {
                            if (rl < p.n && q0 + ql < p.nq_total) dump_row(ql, rl, comp);
                            continue;
                        }
                    }
                    if (rl < p.n && (FLOOR ? comp - flv : comp) < tauv && !(p.tomb && ((p.tomb[rl >> 5] >> (rl & 31)) & 1u))) {  // the bitmap only for the rare rows that beat the threshold
                        const uint32_t slot = atomicAdd(&cnt[ql], 1u);
                        if (kpv + slot < p.pmax) bufs[(size_t)ql * p.pmax + kpv + slot] = comp;
                    }
                }
            } else if constexpr (NQ == 1 && G >= 4) {
                // One query, four rows per lane group and pass.  The butterfly left all four totals in every lane and the
                // key arithmetic (two square roots and a division for cosine) ran four times per lane with G - 1 of G
                // lanes redundant: on short rows (<= 256 B: one or two loads per row) that, not HBM, set the pace
                // (3-4.8 TB/s, profiles/r02_k1_shape_sweep.csv).  REDUCE-SCATTER over the rows instead: two steps
                // halve the values a lane carries, lane `sub` ends with the total of row u = (h0, h1) and computes ONE
                // key.  Same pairing of partial sums as the butterfly (xor G/2, G/4, ...): the totals are bit-identical.
                const bool h0 = (sub & (G / 2)) != 0, h1 = (sub & (G / 4)) != 0;
                const int ul = (h0 ? 2 : 0) + (h1 ? 1 : 0);
#pragma unroll
                for (int ub = 0; ub < U; ub += 4) {
                    Acc v2[2], s1;
#pragma unroll
                    for (int i = 0; i < 2; i++)
                        v2[i] = (h0 ? acc[ub + i + 2][0] : acc[ub + i][0]) + __shfl_xor(h0 ? acc[ub + i][0] : acc[ub + i + 2][0], G / 2, 64);
                    s1 = (h1 ? v2[1] : v2[0]) + __shfl_xor(h1 ? v2[0] : v2[1], G / 4, 64);
#pragma unroll
                    for (int off = G / 8; off > 0; off >>= 1) s1 += __shfl_xor(s1, off, 64);
                    Acc xx1 = 0;
                    if constexpr (NEED_XX) {
                        Acc x2[2];
#pragma unroll
                        for (int i = 0; i < 2; i++) x2[i] = (h0 ? xx[ub + i + 2] : xx[ub + i]) + __shfl_xor(h0 ? xx[ub + i] : xx[ub + i + 2], G / 2, 64);
                        xx1 = (h1 ? x2[1] : x2[0]) + __shfl_xor(h1 ? x2[0] : x2[1], G / 4, 64);
#pragma unroll
                        for (int off = G / 8; off > 0; off >>= 1) xx1 += __shfl_xor(xx1, off, 64);
                    }
                    const float rsv = ul == 0 ? rs[ub] : ul == 1 ? rs[ub + 1] : ul == 2 ? rs[ub + 2] : rs[ub + 3];
                    const float rnv = ul == 0 ? rn[ub] : ul == 1 ? rn[ub + 1] : ul == 2 ? rn[ub + 2] : rn[ub + 3];
                    const uint32_t rl = c0 + (g0 + ub + ul) * RPG + rsel;
                    const uint64_t comp = ((uint64_t)make_key(s1, xx1, qq[0], rsv, rnv, qsf[0], qnf[0]) << 32) | rl;
                    if constexpr (FLOOR) {
                        if (p.dump) {
                            if ((sub & (G / 4 - 1)) == 0 && rl < p.n) dump_row(0, rl, comp);
                            continue;
                        }
                    }
                    if ((sub & (G / 4 - 1)) == 0 && rl < p.n && (FLOOR ? comp - fl1[0] : comp) < tau_r[0] && !(p.tomb && ((p.tomb[rl >> 5] >> (rl & 31)) & 1u))) {
                        const uint32_t slot = atomicAdd(&cnt[0], 1u);
                        if (kprev_r[0] + slot < p.pmax) bufs[kprev_r[0] + slot] = comp;
                    }
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; u++) {
                    Acc xxs = 0;
                    if constexpr (NEED_XX) xxs = group_sum<G>(xx[u]);
#pragma unroll
                    for (int q = 0; q < NQ; q++) {
                        Acc s = group_sum<G>(acc[u][q]);
                        if constexpr (S6) s = (Acc)__float_as_int((float)(128ll * (int64_t)acch[u] + (int64_t)s - qbias6));  // Q.x6, exact; one rounding
                        const uint64_t comp = ((uint64_t)make_key(s, xxs, qq[q], rs[u], rn[u], qsf[q], qnf[q]) << 32) | r[u];
                        if constexpr (FLOOR) {
                            if (p.dump) {
                                if (sub == 0 && rv[u] && q0 + q < p.nq_total) dump_row(q, r[u], comp);
                                continue;
                            }
                        }
                        if (sub == 0 && rv[u] && (FLOOR ? comp - fl1[q] : comp) < tau_r[q] && !(p.tomb && ((p.tomb[r[u] >> 5] >> (r[u] & 31)) & 1u))) {
                            const uint32_t slot = atomicAdd(&cnt[q], 1u);
                            if (kprev_r[q] + slot < p.pmax) bufs[(size_t)q * p.pmax + kprev_r[q] + slot] = comp;
                        }
                    }
                }
            }
        }
        if constexpr (S51) {
            if (lane == 0 && lo_total != 0) atomicAdd(&s51w[0], lo_fetched), atomicAdd(&s51w[1], lo_total);
        }
        __syncthreads();

        if (piece_rows > p.chunk_safe) {  // block-uniform
            bool over = false;
#pragma unroll
            for (int q = 0; q < NQ; q++) over = over || kprev_r[q] + cnt[q] > p.pmax;
            if (over) {  // drop the piece's survivors (the merged lists below kprev are untouched) and go over it in safe pieces
                __syncthreads();
                if (tid < NQ) cnt[tid] = 0;
                __syncthreads();
                safe_only = true;
                continue;
            }
        }

        // ---- merge this piece's survivors into the running top-k (bitonic in LDS)
        bool merged = false;
        if constexpr (NQ == 4) {
            // the four-query pass: when every query's merge is counting-sized (the usual piece), wave w merges query w's
            // survivors -- the four lists in parallel, one barrier instead of two per query in a row
            bool small = p.rank_merge_max != 0;
#pragma unroll
            for (int q = 0; q < NQ; q++) small = small && cnt[q] <= p.rank_merge_max && kprev_r[q] <= 256u;  // block-uniform
            if (small) {
                const uint32_t c = cnt[wave], kp0 = kprev[wave];
                if (c != 0) {  // wave-uniform
                    uint64_t* b = bufs + (size_t)wave * p.pmax;
                    merge_ranked_u64_wave(b, kp0, c, p.k, (uint32_t)lane);
                    if (lane == 0) {
                        const uint32_t total = kp0 + c, kp = total < p.k ? total : p.k;
                        kprev[wave] = kp;
                        cnt[wave] = 0;
                        if (kp == p.k) tau[wave] = b[p.k - 1];
                    }
                }
                merged = true;
            }
        }
        if (!merged) {
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const uint32_t c = cnt[q];
            if (c != 0) {  // block-uniform
                uint64_t* b = bufs + (size_t)q * p.pmax;
                const uint32_t total = kprev_r[q] + c;
                if (c <= p.rank_merge_max && kprev_r[q] <= 256u) {  // the usual piece: a few survivors join a short list by counting (bitonic.h)
                    merge_ranked_u64<256>(b, kprev_r[q], c, p.k, tid);
                } else {
                    const uint32_t P = next_pow2(total < 2 ? 2 : total);
                    for (uint32_t i = total + tid; i < P; i += 256) b[i] = kPadComposite;
                    __syncthreads();
                    bitonic_sort_u64<256>(b, P, tid);
                }
                if (tid == 0) {
                    const uint32_t kp = total < p.k ? total : p.k;
                    kprev[q] = kp;
                    cnt[q] = 0;
                    if (kp == p.k) tau[q] = b[p.k - 1];
                    if constexpr (S51) {  // a new head of the list: publish it (a plain vector store, device scope)
                        const uint32_t head = (uint32_t)(b[0] >> 32);
                        if (head != pub_last) {
                            __hip_atomic_store(p.pub + blockIdx.x, ((uint64_t)p.pub_seq << 32) | head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            pub_last = head;
                        }
                    }
                }
            }
        }
        }
        __syncthreads();
        c0 += piece_rows;
      }  // pieces
    }  // chunks

    // ---- emit the block's sorted list: cand[query][block][kcap], ~0-padded -------
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        if (REDO ? grp * NQ + q >= avail : q0 + q >= p.nq_total) break;
        const uint32_t kp = kprev[q];
        uint64_t* out = p.cand + ((size_t)(REDO ? grp * NQ + q : pass * NQ + q) * gridDim.x + blockIdx.x) * p.kcap;
        const uint64_t* b = bufs + (size_t)q * p.pmax;
        for (uint32_t i = tid; i < p.kcap; i += 256) out[i] = i < kp ? b[i] : kPadComposite;
    }

    }  // groups
    if constexpr (S51) {  // (behind the last piece's barriers)
        if (tid == 0) {
            uint32_t* st = p.lo_stats + (size_t)blockIdx.x * 4;
            st[1] = s51w[0], st[2] = s51w[1], st[3] = 0;
            st[0] = p.pub_seq;
        }
    }
    if (p.ts) {  // launch-uniform
        __syncthreads();
        if (tid == 0) atomicMax(reinterpret_cast<unsigned long long*>(p.ts) + 1, (unsigned long long)wall_clock64());
    }
}

template <int DT, int METRIC, int G>
hipError_t launch_nq(const ScanParams& p, int nq_variant, dim3 grid, size_t lds, hipStream_t stream) {
    if constexpr (!XS) {  // the repair variant reads the STORED rows: the shadow unit does not carry it
        if (p.redo_list) {
            if (nq_variant == 1) hipLaunchKernelGGL((scan_stream_kernel<DT, METRIC, G, 1, true>), grid, dim3(256), lds, stream, p);
            else hipLaunchKernelGGL((scan_stream_kernel<DT, METRIC, G, 4, true>), grid, dim3(256), lds, stream, p);
            return hipGetLastError();
        }
    }
    if constexpr (!XS) {  // passes of a k > 1024 search read the STORED rows too
        if (p.floor1 || p.dump) {
            if (nq_variant == 1) hipLaunchKernelGGL((scan_stream_kernel<DT, METRIC, G, 1, false, true>), grid, dim3(256), lds, stream, p);
            else hipLaunchKernelGGL((scan_stream_kernel<DT, METRIC, G, 4, false, true>), grid, dim3(256), lds, stream, p);
            return hipGetLastError();
        }
    }
    if ((XS && !QSK) || S6 || nq_variant == 1)  // the f16-shadow and 6-bit-shadow units only carry the one-query variant
        hipLaunchKernelGGL((scan_stream_kernel<DT, METRIC, G, 1>), grid, dim3(256), lds, stream, p);
    else
        hipLaunchKernelGGL((scan_stream_kernel<DT, METRIC, G, ((XS && !QSK) || S6) ? 1 : 4>), grid, dim3(256), lds, stream, p);
    return hipGetLastError();
}

template <int DT, int METRIC, int G>
const void* kernel_ptr(int nq_variant, bool redo, bool floor) {
    if constexpr (!XS) {
        if (floor)
            return nq_variant == 1 ? reinterpret_cast<const void*>(&scan_stream_kernel<DT, METRIC, G, 1, false, true>)
                                   : reinterpret_cast<const void*>(&scan_stream_kernel<DT, METRIC, G, 4, false, true>);
        if (redo)
            return nq_variant == 1 ? reinterpret_cast<const void*>(&scan_stream_kernel<DT, METRIC, G, 1, true>)
                                   : reinterpret_cast<const void*>(&scan_stream_kernel<DT, METRIC, G, 4, true>);
    }
    return ((XS && !QSK) || S6 || nq_variant == 1) ? reinterpret_cast<const void*>(&scan_stream_kernel<DT, METRIC, G, 1>)
                                                   : reinterpret_cast<const void*>(&scan_stream_kernel<DT, METRIC, G, ((XS && !QSK) || S6) ? 1 : 4>);
}

template <int DT, int METRIC>
hipError_t launch_g(const ScanParams& p, int G, int nqv, dim3 grid, size_t lds, hipStream_t s) {
    if constexpr (S6) return G == 1 ? launch_nq<DT, METRIC, 1>(p, nqv, grid, lds, s) : hipErrorInvalidValue;  // one lane per row only
    else
    switch (G) {
    case 1: return launch_nq<DT, METRIC, 1>(p, nqv, grid, lds, s);
    case 4: return launch_nq<DT, METRIC, 4>(p, nqv, grid, lds, s);
    case 8: return launch_nq<DT, METRIC, 8>(p, nqv, grid, lds, s);
    case 16: return launch_nq<DT, METRIC, 16>(p, nqv, grid, lds, s);
    case 32: return launch_nq<DT, METRIC, 32>(p, nqv, grid, lds, s);
    default: return launch_nq<DT, METRIC, 64>(p, nqv, grid, lds, s);
    }
}

template <int DT, int METRIC>
const void* kernel_g(int G, int nqv, bool redo, bool floor) {
    if constexpr (S6) return kernel_ptr<DT, METRIC, 1>(nqv, redo, floor);
    else
    switch (G) {
    case 1: return kernel_ptr<DT, METRIC, 1>(nqv, redo, floor);
    case 4: return kernel_ptr<DT, METRIC, 4>(nqv, redo, floor);
    case 8: return kernel_ptr<DT, METRIC, 8>(nqv, redo, floor);
    case 16: return kernel_ptr<DT, METRIC, 16>(nqv, redo, floor);
    case 32: return kernel_ptr<DT, METRIC, 32>(nqv, redo, floor);
    default: return kernel_ptr<DT, METRIC, 64>(nqv, redo, floor);
    }
}

}  // namespace

#if MVF_SCAN_XS == 3
#define MVF_SCAN_FN2(name, dt) name##dt##z
#elif MVF_SCAN_XS == 2
#define MVF_SCAN_FN2(name, dt) name##dt##y
#elif MVF_SCAN_XS
#define MVF_SCAN_FN2(name, dt) name##dt##x
#else
#define MVF_SCAN_FN2(name, dt) name##dt
#endif
#define MVF_SCAN_FN(name, dt) MVF_SCAN_FN2(name, dt)

hipError_t MVF_SCAN_FN(scan_stream_launch_dt, MVF_SCAN_DT)(const ScanParams& p, int metric, int G, int nqv,
                                                       dim3 grid, size_t lds, hipStream_t s) {
    switch (metric) {
    case MVF_METRIC_L2: return launch_g<MVF_SCAN_DT, MVF_METRIC_L2>(p, G, nqv, grid, lds, s);
    case MVF_METRIC_INNER_PRODUCT: return launch_g<MVF_SCAN_DT, MVF_METRIC_INNER_PRODUCT>(p, G, nqv, grid, lds, s);
    default: return launch_g<MVF_SCAN_DT, MVF_METRIC_COSINE>(p, G, nqv, grid, lds, s);
    }
}

const void* MVF_SCAN_FN(scan_stream_kernel_ptr_dt, MVF_SCAN_DT)(int metric, int G, int nqv, bool redo, bool floor) {
    switch (metric) {
    case MVF_METRIC_L2: return kernel_g<MVF_SCAN_DT, MVF_METRIC_L2>(G, nqv, redo, floor);
    case MVF_METRIC_INNER_PRODUCT: return kernel_g<MVF_SCAN_DT, MVF_METRIC_INNER_PRODUCT>(G, nqv, redo, floor);
    default: return kernel_g<MVF_SCAN_DT, MVF_METRIC_COSINE>(G, nqv, redo, floor);
    }
}

}  // namespace mvf
