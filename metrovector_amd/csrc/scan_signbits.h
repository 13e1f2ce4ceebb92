// scan_signbits.h — the form and the launch interface of SQ / S2, the sign-bit search: Int8 queries against bit-packed UInt8
// rows on the int8 matrix unit (scan_signbits.hip; signbits.hip; include/mvf_gpu_signbits.h; DESIGN.md §5 "SQ / S2").
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mvf_common.h"
#include "scan_hamming.h"
#include "scan_hamming_mfma.h"

namespace mvf {

constexpr uint32_t kSignMaxDim = 512;                // packed bytes of a row at most: a tile of 32 prepared queries fits LDS
constexpr uint32_t kSignThreads = kHamMfmaThreads;   // threads of an S2 block: four waves
constexpr uint32_t kSignWaveRows = kHamMfmaWaveRows; // rows of a wave: four 16-row A fragments against every query of the tile
constexpr uint32_t kSignTileBytes = 128u << 10;      // bytes of a tile's prepared queries in LDS at most
constexpr uint32_t kSignLds = 160u << 10;            // the part's LDS
constexpr int32_t kSignBias = 128 * 4096;            // |s| <= 524288: key = kSignBias - s is 0 .. 2^20, smaller is better

static_assert(kSignThreads / 64u * kSignWaveRows == kHamStepRows, "a block iteration is kHamStepRows rows: buf >= kcap + kHamStepRows");

// The shape of one window of a sign-bit search, a pure function of its sizes: signbits_launch takes every figure from it and
// mvfgpu_selftest_signbits_form reports it.
struct SignbitsForm {
    uint32_t query_tile;     // QT: queries whose prepared elements a block holds in LDS (16, 32, 64 or 128)
    uint32_t chunks;         // T: 64-byte chunks of a row's pitch; a chunk is eight MFMAs of 64 elements per column tile
    uint32_t kcap, buf;      // next_pow2(k), entries of a query's candidate buffer (H0's)
    uint32_t tiles;          // query tiles of the window
    uint32_t row_slices;     // S
    uint64_t slice_rows;     // rows of a slice (the last one may be shorter)
    uint32_t lds_bytes;      // dynamic LDS of an S2 block
    uint64_t prepared_bytes; // SQ's scratch: the tiles' prepared queries and their sums
    uint64_t scratch_bytes;  // the candidate buffers: S x tiles x QT x buf x 8
};

// bytes of one query's prepared elements: int8, over the chunks (8 x the pitch rounded up to 64)
inline uint32_t sign_query_bytes(uint32_t chunks) { return chunks * 512u; }

// dimension = packed bytes of a row (1 .. 512), nq = 1 .. 1024, k = 1 .. 1024
inline SignbitsForm signbits_form(uint32_t dimension, uint32_t nq, uint32_t k, uint64_t rows, uint32_t num_cus) {
    SignbitsForm f{};
    const uint32_t pitch = (dimension + 15u) & ~15u;
    f.chunks = (pitch + 63u) / 64u;
    // the smallest tile of 16 x {1, 2, 4, 8} queries that holds the window's, capped by what the prepared tile takes of LDS:
    // 128 queries up to 128 bytes a row, 64 up to 256, 32 up to 512 -- one query pays for a tile of 16
    const uint32_t cap = pitch <= 128u ? 128u : pitch <= 256u ? 64u : 32u;
    f.query_tile = 16u;
    while (f.query_tile < nq && f.query_tile < cap) f.query_tile *= 2u;
    f.kcap = next_pow2(k);
    f.buf = f.kcap * 2u > kHamBufMin ? f.kcap * 2u : kHamBufMin;
    f.tiles = (nq + f.query_tile - 1u) / f.query_tile;
    // the staged queries, the sort area, thresholds, sums, counts, flag
    f.lds_bytes = f.query_tile * sign_query_bytes(f.chunks) + f.buf * 8u + f.query_tile * (8u + 4u + 4u) + 16u;
    f.prepared_bytes = (uint64_t)f.tiles * f.query_tile * (sign_query_bytes(f.chunks) + 4u);
    // slices: two blocks per CU over all query tiles where two blocks' LDS fit a CU, else one; a slice of kHamSliceRows rows at
    // least, what H1 merges and what the candidate scratch holds at most
    const uint64_t per_block = (uint64_t)f.query_tile * f.buf * 8u;
    const uint64_t per_cu = 2u * f.lds_bytes <= kSignLds ? 2u : 1u;
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

// what SQ and S2 take beside the search's own parameters (p.queries: Int8 [nq][8 x dim]; p.query_tile, p.buf, p.kcap,
// p.row_slices, p.slice_rows from the form; p.score_bias = kSignBias)
struct SignbitsParams {
    HammingParams p;
    uint32_t chunks, tiles;
    unsigned char* prepared;  // [tiles][chunks][4][2][QT / 16][64] x 16 bytes: the B fragments in the order S2's lanes read them
    int32_t* sums;            // [tiles][QT]: the sum of a query's elements
    uint64_t* cand;           // [slice][tile][QT][buf] composites ((kSignBias - s) << 32 | local row)
};

// SQ, S2 over the grid (row slices x query tiles), then H1: three launches on `s`, no host wait.
// marks (the stage timer only): four events, recorded in front of SQ, between the launches and behind H1.
hipError_t signbits_launch(const SignbitsForm& f, const SignbitsParams& a, hipStream_t s, hipEvent_t* marks = nullptr);

}  // namespace mvf
