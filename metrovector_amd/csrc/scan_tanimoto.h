// scan_tanimoto.h — the form and the launch interface of TQ / T2, the Tanimoto search: the exact top-k by Jaccard similarity of
// UInt8 queries over bit-packed UInt8 rows on the FP4 matrix unit (scan_tanimoto.hip; tanimoto.hip; include/mvf_gpu_tanimoto.h;
// DESIGN.md §5 "TQ / T2").
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mvf_common.h"
#include "scan_hamming.h"
#include "scan_hamming_mfma.h"

namespace mvf {

constexpr uint32_t kTaniMaxDim = kHamMfmaPitch;      // packed bytes of a row at most: a tile of 64 prepared queries fits LDS
constexpr uint32_t kTaniThreads = kHamMfmaThreads;   // threads of a T2 block: four waves
constexpr uint32_t kTaniWaveRows = kHamMfmaWaveRows; // rows of a wave: four 16-row A fragments against every query of the tile
constexpr uint32_t kTaniLds = 160u << 10;            // the part's LDS
// The order key of a score T = c / u in [0, 1] (include/mvf_gpu_tanimoto.h, "The score and the order key"): the bits of a
// non-negative float are monotone as u32, so kTaniBias - bits(T) is 0 for T = 1 and kTaniBias for T = 0: smaller is better.
constexpr int32_t kTaniBias = 0x3F800000;            // the bits of 1.0f

static_assert(kTaniThreads / 64u * kTaniWaveRows == kHamStepRows, "a block iteration is kHamStepRows rows: buf >= kcap + kHamStepRows");

// The shape of one window of a Tanimoto search, a pure function of its sizes: tanimoto_launch takes every figure from it and
// mvfgpu_selftest_tanimoto_form reports it.
struct TanimotoForm {
    uint32_t query_tile;     // QT: queries whose prepared bits a block holds in LDS (16, 32, 64 or 128)
    uint32_t chunks;         // T: 64-byte chunks of a row's pitch; a chunk is four MFMA steps of 128 bits
    uint32_t kcap, buf;      // next_pow2(k), entries of a query's candidate buffer (H0's)
    uint32_t tiles;          // query tiles of the window
    uint32_t row_slices;     // S
    uint64_t slice_rows;     // rows of a slice (the last one may be shorter)
    uint32_t lds_bytes;      // dynamic LDS of a T2 block
    uint64_t prepared_bytes; // TQ's scratch: the tiles' FP4 queries and their popcounts
    uint64_t scratch_bytes;  // the candidate buffers: S x tiles x QT x buf x 8
};

// bytes of one query's prepared bits: four FP4 bits per byte over the chunks (HQ's)
inline uint32_t tani_query_bytes(uint32_t chunks) { return ham_mfma_query_bytes(chunks); }

// bytes a query takes of a block's LDS beside its prepared bits: threshold, the composite its pair belongs to, the pair
// (c_t, u_t), popcount, count
constexpr uint32_t kTaniQueryLds = 8u + 8u + 8u + 4u + 4u;

// dimension = packed bytes of a row (1 .. 512), nq = 1 .. 1024, k = 1 .. 1024
inline TanimotoForm tanimoto_form(uint32_t dimension, uint32_t nq, uint32_t k, uint64_t rows, uint32_t num_cus) {
    TanimotoForm f{};
    const uint32_t pitch = (dimension + 15u) & ~15u;
    f.chunks = (pitch + 63u) / 64u;
    // the smallest tile of 16 x {1, 2, 4, 8} queries that holds the window's, capped by what the prepared tile takes of LDS
    // (128 KiB: H2's): 128 queries up to 256 bytes a row, 64 beyond -- one query pays for a tile of 16
    const uint32_t cap = pitch <= kHamMfmaWidePitch ? 128u : 64u;
    f.query_tile = 16u;
    while (f.query_tile < nq && f.query_tile < cap) f.query_tile *= 2u;
    f.kcap = next_pow2(k);
    f.buf = f.kcap * 2u > kHamBufMin ? f.kcap * 2u : kHamBufMin;
    f.tiles = (nq + f.query_tile - 1u) / f.query_tile;
    // the staged queries, the sort area, the queries' selection state, flag
    f.lds_bytes = f.query_tile * tani_query_bytes(f.chunks) + f.buf * 8u + f.query_tile * kTaniQueryLds + 16u;
    f.prepared_bytes = (uint64_t)f.tiles * f.query_tile * (tani_query_bytes(f.chunks) + 4u);
    // slices: two blocks per CU over all query tiles where two blocks' LDS fit a CU, else one (signbits_form's rule); a slice of
    // kHamSliceRows rows at least, what H1 merges and what the candidate scratch holds at most
    const uint64_t per_block = (uint64_t)f.query_tile * f.buf * 8u;
    const uint64_t per_cu = 2u * f.lds_bytes <= kTaniLds ? 2u : 1u;
    uint64_t want = (per_cu * (num_cus ? num_cus : 256u) + f.tiles - 1u) / f.tiles;
    const uint64_t by_rows = (rows + kHamSliceRows - 1u) / kHamSliceRows;
    if (want > by_rows) want = by_rows;
    if (want > kHamMergeMax / f.kcap) want = kHamMergeMax / f.kcap;
    if (want > kHamMfmaScratch / (per_block * f.tiles)) want = kHamMfmaScratch / (per_block * f.tiles);
    if (want < 1) want = 1;
    f.slice_rows = rows ? (rows + want - 1u) / want : 0;
    f.row_slices = rows ? (uint32_t)((rows + f.slice_rows - 1u) / f.slice_rows) : 0u;
    f.scratch_bytes = (uint64_t)f.row_slices * f.tiles * per_block;
    return f;
}

// what TQ and T2 take beside the search's own parameters (p.queries: UInt8 [nq][dim]; p.query_tile, p.buf, p.kcap, p.row_slices,
// p.slice_rows from the form; p.score_bias = kTaniBias, p.float_key = 1; p.out_raw = NULL)
struct TanimotoParams {
    HammingParams p;
    uint32_t chunks, tiles;
    unsigned char* prepared;  // [tiles][chunks][4][QT / 16][64] x 16 bytes: the B fragments in the order T2's lanes read them
    float* pops;              // [tiles][QT]: a = popcount(q)
    uint64_t* cand;           // [slice][tile][QT][buf] composites ((kTaniBias - bits(T)) << 32 | local row)
};

// TQ, T2 over the grid (row slices x query tiles), then H1: three launches on `s`, no host wait.
// marks (the stage timer only): four events, recorded in front of TQ, between the launches and behind H1.
hipError_t tanimoto_launch(const TanimotoForm& f, const TanimotoParams& a, hipStream_t s, hipEvent_t* marks = nullptr);

}  // namespace mvf
