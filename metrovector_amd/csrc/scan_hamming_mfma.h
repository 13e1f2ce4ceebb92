// scan_hamming_mfma.h — the route, the form and the launch interface of HQ / H2, the Hamming search's batch route on the matrix
// unit (scan_hamming_mfma.hip; hamming.hip; include/mvf_gpu_hamming_route.h; DESIGN.md §5 "HQ / H2").
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mvf_common.h"
#include "scan_hamming.h"

namespace mvf {

constexpr uint32_t kHamMfmaPitch = 512;             // rows up to this pitch (4096 bits) are eligible: a tile's prepared queries fit LDS
constexpr uint32_t kHamMfmaWidePitch = 256;         // up to this pitch a tile holds 128 queries, beyond it 64
constexpr uint32_t kHamMfmaThreads = kHamThreads;   // threads of an H2 block: four waves
constexpr uint32_t kHamMfmaWaveRows = 64;           // rows of a wave: four 16-row A fragments against every query of the tile
constexpr uint64_t kHamMfmaScratch = 512ull << 20;  // bytes of the candidate buffers of one launch at most
// The automatic rule: the shapes from which route 2 was measured to beat route 1 by more than 7 % (profiles/r25_hamming_mfma.txt):
constexpr uint32_t kHamMfmaMinQueries = 1024;       // a full window (256 queries: no gain; between the two: not measured),
constexpr uint64_t kHamMfmaMinRows = 10000000;      // 10M rows (200k rows: a loss; between the two: not measured),
constexpr uint32_t kHamMfmaMinPitch = 64;           // rows of 64 bytes (32 bytes: a loss),
constexpr uint32_t kHamMfmaMaxAutoK = 128;          // lists of up to 128 entries (k = 100: a gain, k = 1024: none)

static_assert(kHamMfmaThreads / 64u * kHamMfmaWaveRows == kHamStepRows, "a block iteration is kHamStepRows rows: buf >= kcap + kHamStepRows");

// The route of one window of a Hamming search, a pure function (mvfgpu_selftest_hamming_route; the launch calls it): 1 = H0,
// 2 = HQ / H2.  forced: mvfgpu_set_hamming_route / MVF_HAMMING_ROUTE (0 = automatic).  Eligible: a pitch of up to 512 bytes and
// k up to 1024; everything else is route 1 whatever is forced.  Automatic: route 2 from kHamMfmaMinQueries queries in the
// window, kHamMfmaMinRows rows and a pitch of kHamMfmaMinPitch on, for lists of up to kHamMfmaMaxAutoK entries.
inline uint32_t hamming_route(uint32_t dimension, uint32_t nq, uint32_t k, uint64_t rows, int forced) {
    const uint32_t pitch = (dimension + 15u) & ~15u;
    if (pitch > kHamMfmaPitch || k > 1024u || forced == 1) return 1u;
    if (forced == 2) return 2u;
    return nq >= kHamMfmaMinQueries && rows >= kHamMfmaMinRows && pitch >= kHamMfmaMinPitch && next_pow2(k) <= kHamMfmaMaxAutoK ? 2u : 1u;
}

// The shape of one window on route 2, a pure function of its sizes: hamming_mfma_launch takes every figure from it and
// mvfgpu_selftest_hamming_mfma_form reports it.
struct HammingMfmaForm {
    uint32_t query_tile;     // QT: queries whose prepared bits a block holds in LDS (128 or 64)
    uint32_t chunks;         // T: 64-byte chunks of a row's pitch; a chunk is four MFMA steps of 128 bits
    uint32_t wave_rows;      // rows of a wave
    uint32_t threads;        // threads of a block
    uint32_t kcap, buf;      // next_pow2(k), entries of a query's candidate buffer (H0's)
    uint32_t tiles;          // query tiles of the window
    uint32_t row_slices;     // S
    uint64_t slice_rows;     // rows of a slice (the last one may be shorter)
    uint32_t lds_bytes;      // dynamic LDS of an H2 block
    uint64_t prepared_bytes; // HQ's scratch: the tiles' FP4 queries and their starts
    uint64_t scratch_bytes;  // the candidate buffers: S x tiles x QT x buf x 8
};

// bytes of one query's prepared bits: four FP4 bits per byte over the chunks
inline uint32_t ham_mfma_query_bytes(uint32_t chunks) { return chunks * 256u; }

// dimension = packed bytes of a row (1 .. 512), nq = 1 .. 1024, k = 1 .. 1024
inline HammingMfmaForm hamming_mfma_form(uint32_t dimension, uint32_t nq, uint32_t k, uint64_t rows, uint32_t num_cus) {
    HammingMfmaForm f{};
    const uint32_t pitch = (dimension + 15u) & ~15u;
    f.query_tile = pitch <= kHamMfmaWidePitch ? 128u : 64u;
    f.chunks = (pitch + 63u) / 64u;
    f.wave_rows = kHamMfmaWaveRows;
    f.threads = kHamMfmaThreads;
    f.kcap = next_pow2(k);
    f.buf = f.kcap * 2u > kHamBufMin ? f.kcap * 2u : kHamBufMin;
    f.tiles = (nq + f.query_tile - 1u) / f.query_tile;
    // the staged queries, the sort area, thresholds, starts, counts, flag
    f.lds_bytes = f.query_tile * ham_mfma_query_bytes(f.chunks) + f.buf * 8u + f.query_tile * (8u + 4u + 4u) + 16u;
    f.prepared_bytes = (uint64_t)f.tiles * f.query_tile * (ham_mfma_query_bytes(f.chunks) + 4u);
    // slices: one block per CU over all query tiles (a block's LDS leaves no room for a second, and every slice pays for the
    // start of its queries' selection), a slice of kHamSliceRows rows at least, what H1 merges and what the
    // candidate scratch holds at most
    const uint64_t per_block = (uint64_t)f.query_tile * f.buf * 8u;
    uint64_t want = ((uint64_t)(num_cus ? num_cus : 256u) + f.tiles - 1u) / f.tiles;
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

// what HQ and H2 take beside the search's own parameters (p.query_tile, p.buf, p.kcap, p.row_slices, p.slice_rows from the form)
struct HammingMfmaParams {
    HammingParams p;
    uint32_t chunks, tiles;
    unsigned char* prepared;  // [tiles][chunks][4][QT / 16][64] x 16 bytes: the B fragments in the order H2's lanes read them
    float* starts;            // [tiles][QT]: popcount(q), the accumulators' start value
    uint64_t* cand;           // [slice][tile][QT][buf] composites
};

// HQ alone: a.p.queries [a.p.nq][a.p.dim] -> a.prepared and a.starts for a.tiles tiles of a.p.query_tile = 16 x {1, 2, 4, 8}
// queries (H2 takes 128 or 64; scan_hamming_radius.hip's HR2 every one of them).  One launch on `s`.
hipError_t hamming_prepare_launch(const HammingMfmaParams& a, hipStream_t s);

// HQ, H2 over the grid (row slices x query tiles), then H1: three launches on `s`, no host wait.
// marks (the stage timer only): three events, recorded in front of HQ, between H2 and H1 and behind H1.
hipError_t hamming_mfma_launch(const HammingMfmaForm& f, const HammingMfmaParams& a, hipStream_t s, hipEvent_t* marks = nullptr);

}  // namespace mvf
