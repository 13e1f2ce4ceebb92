// scan_hamming.h — the form and the launch interface of H0 / H1, the Hamming search over bit-packed UInt8 rows
// (scan_hamming.hip; hamming.hip; DESIGN.md §5 "H0 / H1 — Hamming search").
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mvf_common.h"

namespace mvf {

constexpr uint32_t kHamThreads = 256;          // threads of an H0 block
constexpr uint32_t kHamRegisterPitch = 256;    // rows up to this pitch stay in registers, one 16-byte step per lane
constexpr uint32_t kHamStepRows = 256;         // rows of one H0 iteration at most: what a query's buffer takes between two checks
constexpr uint32_t kHamBufMin = 512;           // entries of a query's LDS buffer at least: next_pow2(k) + kHamStepRows fit
constexpr uint32_t kHamMaxTile = 16;           // queries of a tile at most (register form); the streaming form holds 8
constexpr uint32_t kHamBufBudget = 64u << 10;  // bytes of a tile's buffers: two blocks share a CU's LDS in the register form
constexpr uint32_t kHamLdsBudget = 150u << 10; // bytes of a block's LDS in the streaming form (the part has 160 KiB)
constexpr uint32_t kHamSliceRows = 1024;       // rows of a slice at least
constexpr uint32_t kHamMergeMax = 65536;       // slices x next_pow2(k): the list entries H1 merges per query at most
constexpr uint32_t kHamMergeLds = 16384;       // of which it holds this many in LDS per round (128 KiB)

// The shape of one Hamming search, a pure function of its sizes: hamming_launch takes every figure from it and
// mvfgpu_selftest_hamming_form reports it.
struct HammingForm {
    uint32_t form;           // 0 = register form, 1 = streaming form
    uint32_t lanes;          // G: lanes of a row's group; lane j holds (register) or starts at (streaming) 16-byte step j
    uint32_t query_tile;     // QT: queries a block holds in LDS
    uint32_t batch;          // QB: queries reduced by one butterfly (min(G, QT); the streaming form's QT)
    uint32_t kcap, buf;      // next_pow2(k), entries of a query's LDS buffer (>= kcap + kHamStepRows, a power of two)
    uint32_t row_slices;     // S
    uint64_t slice_rows;     // rows of a slice (the last one may be shorter)
    uint32_t lds_bytes;      // dynamic LDS of an H0 block
};

static_assert(kHamBufMin >= 2 * kHamStepRows, "max(2 kcap, kHamBufMin) >= kcap + kHamStepRows for every kcap");

inline uint32_t ham_pow2_floor(uint32_t v) {
    uint32_t p = 1;
    while (p * 2 <= v) p *= 2;
    return p;
}

// dimension = packed bytes of a row (1 .. 33025), nq >= 1, k = 1 .. 1024
inline HammingForm hamming_form(uint32_t dimension, uint32_t nq, uint32_t k, uint64_t rows, uint32_t num_cus) {
    HammingForm f{};
    const uint32_t pitch = (dimension + 15u) & ~15u, V = pitch / 16u;
    f.form = pitch <= kHamRegisterPitch ? 0u : 1u;
    f.kcap = next_pow2(k);
    f.buf = f.kcap * 2u > kHamBufMin ? f.kcap * 2u : kHamBufMin;
    const uint32_t nq2 = next_pow2(nq < 1024u ? nq : 1024u);
    if (f.form == 0) {
        f.lanes = next_pow2(V);
        f.query_tile = ham_pow2_floor(kHamBufBudget / (f.buf * 8u));
        if (f.query_tile > kHamMaxTile) f.query_tile = kHamMaxTile;
    } else {
        f.lanes = V <= 32u ? 32u : 64u;
        f.query_tile = ham_pow2_floor(kHamLdsBudget / (f.buf * 8u + pitch));
        if (f.query_tile > 8u) f.query_tile = 8u;
    }
    if (f.query_tile > nq2) f.query_tile = nq2;
    f.batch = f.form == 0 && f.lanes < f.query_tile ? f.lanes : f.query_tile;
    // bufs, thresholds (two at least: the queries behind them stay 16-byte aligned), queries (the register form pads a query to
    // its group's lanes x 16 bytes), counts, flag
    f.lds_bytes = f.query_tile * f.buf * 8u + (f.query_tile > 2u ? f.query_tile : 2u) * 8u + f.query_tile * (f.form == 0 ? f.lanes * 16u : pitch) +
                  f.query_tile * 4u + 16u;
    // slices: two blocks per CU over all query tiles, a slice of kHamSliceRows rows at least, what H1 merges at most
    const uint32_t tiles = (nq + f.query_tile - 1u) / f.query_tile;
    uint64_t want = (2ull * (num_cus ? num_cus : 256u) + tiles - 1u) / tiles;
    const uint64_t by_rows = (rows + kHamSliceRows - 1u) / kHamSliceRows;
    if (want > by_rows) want = by_rows;
    if (want > kHamMergeMax / f.kcap) want = kHamMergeMax / f.kcap;
    if (want < 1) want = 1;
    f.slice_rows = rows ? (rows + want - 1u) / want : 0;
    f.row_slices = rows ? (uint32_t)((rows + f.slice_rows - 1u) / f.slice_rows) : 0u;
    return f;
}

struct HammingParams {
    const unsigned char* rows;     // [n][pitch]; the bytes behind `dim` of a row are never relied on
    const unsigned char* queries;  // [nq][dim], contiguous
    const uint32_t* tomb;          // NULL = no deletions
    uint64_t n, slice_rows;
    uint32_t dim, pitch, V, nq, k, kcap, buf, query_tile, row_slices;
    uint64_t* lists;               // [nq][row_slices][kcap] composites (distance << 32 | local row), ascending, kPadComposite behind
    uint64_t index_base;
    const uint64_t* ids;           // vector ids per local row, or NULL
    float* out_scores;             // [nq][k]
    uint64_t* out_indices;
    int32_t* out_raw;              // nullable
    int32_t score_bias;            // 0: a key is a distance, written as it is (+inf padding).  Otherwise (scan_signbits.hip) a key is
                                   // score_bias - s for a score s where larger is better: H1 writes s (-inf padding)
    uint32_t float_key;            // set (scan_tanimoto.hip): a key is score_bias - the bits of a non-negative f32 score: H1 writes
                                   // uint_as_float(score_bias - key) to out_scores (-inf padding); there is no out_raw
};

// H0 over the grid (row slices x query tiles), then H1 with one block per query: two launches on `s`, no host wait.
// marks (the stage timer only): three events, recorded in front of H0, between the two and behind H1.
hipError_t hamming_launch(const HammingForm& f, const HammingParams& p, hipStream_t s, hipEvent_t* marks = nullptr);
// H1 alone, over the lists[nq][p.row_slices][p.kcap] a scan left (hamming_launch's second launch; scan_hamming_mfma.hip's third)
hipError_t hamming_merge_launch(const HammingParams& p, hipStream_t s);

}  // namespace mvf
