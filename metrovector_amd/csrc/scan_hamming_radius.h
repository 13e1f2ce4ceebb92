// scan_hamming_radius.h — the form and the launch interface of HR2 / HRP, the Hamming radius search: every row within r bits of
// each query, on the FP4 matrix unit (scan_hamming_radius.hip; hamming_radius.hip; include/mvf_gpu_hamming_radius.h; DESIGN.md §5
// "HR2 / HRP").
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mvf_common.h"
#include "scan_hamming.h"
#include "scan_hamming_mfma.h"

namespace mvf {

constexpr uint32_t kHamRadiusMaxDim = kHamMfmaPitch;        // packed bytes of a row at most: a tile of 64 prepared queries fits LDS
constexpr uint32_t kHamRadiusThreads = kHamMfmaThreads;     // threads of an HR2 block: four waves
constexpr uint32_t kHamRadiusWaveRows = kHamMfmaWaveRows;   // rows of a wave per iteration: four 16-row A fragments
constexpr uint32_t kHamRadiusBlocksPerCu = 8;               // blocks a CU is given at most (two waves per SIMD from each pair)
constexpr uint32_t kHamRadiusLds = 160u << 10;              // the part's LDS
constexpr uint32_t kHamRadiusListCap = 8192;                // entries of a query's device list: MVFGPU_RADIUS_LIST_CAP
constexpr uint32_t kHamRadiusMaxOut = 1024;                 // max_per_query at most: below the cap, so an overflowed query's
                                                            // entries are its Hamming top-max_per_query

static_assert(kHamRadiusMaxOut <= kHamRadiusListCap, "a query whose list ran over is completed by a top-k search");

// The shape of one window of a Hamming radius search, a pure function of its sizes: hamming_radius_launch takes every figure
// from it and mvfgpu_selftest_hamming_radius_form reports it.
struct HammingRadiusForm {
    uint32_t query_tile;     // QT: queries whose prepared bits a block holds in LDS (16, 32, 64 or 128)
    uint32_t chunks;         // T: 64-byte chunks of a row's pitch; a chunk is four MFMA steps of 128 bits
    uint32_t tiles;          // query tiles of the window
    uint32_t blocks_per_cu;  // blocks the slice rule gives a CU: what the tile's LDS admits, kHamRadiusBlocksPerCu at most
    uint32_t row_slices;     // S
    uint64_t slice_rows;     // rows of a slice (the last one may be shorter)
    uint32_t lds_bytes;      // dynamic LDS of an HR2 block: the staged tile and one u32 count per query
    uint64_t prepared_bytes; // HQ's scratch: the tiles' FP4 queries and their starts
    uint64_t scratch_bytes;  // all of a window's scratch where entries are asked for: prepared queries, two counters per query, lists
};

// dimension = packed bytes of a row (1 .. 512), nq = 1 .. 1024
inline HammingRadiusForm hamming_radius_form(uint32_t dimension, uint32_t nq, uint64_t rows, uint32_t num_cus) {
    HammingRadiusForm f{};
    const uint32_t pitch = (dimension + 15u) & ~15u;
    f.chunks = (pitch + 63u) / 64u;
    // the smallest tile of 16 x {1, 2, 4, 8} queries that holds the window's, capped by what the prepared tile takes of LDS as in
    // H2: 128 queries up to a pitch of 256 bytes, 64 up to 512 -- one query pays for a tile of 16
    const uint32_t cap = pitch <= kHamMfmaWidePitch ? 128u : 64u;
    f.query_tile = 16u;
    while (f.query_tile < nq && f.query_tile < cap) f.query_tile *= 2u;
    f.tiles = (nq + f.query_tile - 1u) / f.query_tile;
    f.lds_bytes = f.query_tile * ham_mfma_query_bytes(f.chunks) + f.query_tile * 4u;
    f.prepared_bytes = (uint64_t)f.tiles * f.query_tile * (ham_mfma_query_bytes(f.chunks) + 4u);
    // slices: as many blocks per CU as the tile's LDS admits, kHamRadiusBlocksPerCu at most, over all query tiles; a slice of
    // kHamSliceRows rows at least.  Nothing merges the slices, so nothing else caps them.
    f.blocks_per_cu = kHamRadiusLds / f.lds_bytes;
    if (f.blocks_per_cu > kHamRadiusBlocksPerCu) f.blocks_per_cu = kHamRadiusBlocksPerCu;
    uint64_t want = ((uint64_t)f.blocks_per_cu * (num_cus ? num_cus : 256u) + f.tiles - 1u) / f.tiles;
    const uint64_t by_rows = (rows + kHamSliceRows - 1u) / kHamSliceRows;
    if (want > by_rows) want = by_rows;
    if (want < 1) want = 1;
    f.slice_rows = rows ? (rows + want - 1u) / want : 0;
    f.row_slices = rows ? (uint32_t)((rows + f.slice_rows - 1u) / f.slice_rows) : 0u;
    f.scratch_bytes = f.prepared_bytes + (uint64_t)nq * (8u + (uint64_t)kHamRadiusListCap * 8u);
    return f;
}

// What HQ, HR2 and HRP take.  a.p: rows, queries, tomb, n, slice_rows, dim, pitch, V, nq, query_tile, row_slices, index_base,
// ids and the three entry outputs [nq][kout] (out_raw nullable; all unused where kout = 0); a.chunks, a.tiles, a.prepared and
// a.starts as HQ leaves them; a.cand is not used.
struct HammingRadiusParams {
    HammingMfmaParams a;
    const uint32_t* radii;  // [nq]; HR2 clamps a radius to 8 x dim
    uint32_t* counts;       // [nq], zero on entry: the exact number of matches
    uint32_t* fill;         // [nq], zero on entry: slots drawn from a query's list (at most the cap plus one per lane)
    uint64_t* lists;        // [nq][cap] composites (distance << 32 | local row) in arrival order; NULL where kout = 0
    uint32_t cap, kout;     // kHamRadiusListCap; max_per_query
    uint64_t* out_counts;   // [nq]
};

// HQ, HR2 over the grid (row slices x query tiles), then HRP with one block per query: three launches on `s`, no host wait.
// marks (the stage timer only): four events, recorded in front of HQ, between the launches and behind HRP.
hipError_t hamming_radius_launch(const HammingRadiusForm& f, const HammingRadiusParams& r, hipStream_t s, hipEvent_t* marks = nullptr);

}  // namespace mvf
