// scan_hamming_pairs.h — the form, the triangular block mapping and the launch interface of HJ / HJP, the Hamming pair join: every
// two live rows of one corpus within r bits of each other, on the FP4 matrix unit (scan_hamming_pairs.hip; hamming_pairs.hip;
// include/mvf_gpu_hamming_pairs.h; DESIGN.md §5 "HJ / HJP").
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mvf_common.h"
#include "scan_hamming.h"
#include "scan_hamming_mfma.h"

namespace mvf {

constexpr uint32_t kHamPairsMaxDim = kHamMfmaPitch;       // packed bytes of a row at most: a column tile of 64 rows fits LDS
constexpr uint32_t kHamPairsThreads = kHamMfmaThreads;    // threads of an HJ block: four waves
constexpr uint32_t kHamPairsWaveRows = kHamMfmaWaveRows;  // rows of a wave per iteration: four 16-row A fragments
constexpr uint32_t kHamPairsStepRows = kHamPairsThreads / 64u * kHamPairsWaveRows;  // rows of a block iteration: 256
constexpr uint32_t kHamPairsSpanMax = 8192;               // rows of a span at most: 32 block iterations behind one staged tile
constexpr uint32_t kHamPairsLds = 160u << 10;             // the part's LDS
constexpr uint64_t kHamPairsMaxPairs = 1ull << 24;        // listed pairs at most: MVFGPU_HAMMING_PAIRS_MAX
constexpr uint64_t kHamPairsGrid = 1ull << 30;            // blocks of one launch at most (a 1-D grid; more blocks: more launches)

static_assert(kHamSliceRows % kHamPairsStepRows == 0 && kHamPairsSpanMax % kHamPairsStepRows == 0, "a span is whole block iterations");

// The shape of one Hamming pair join, a pure function of its sizes: hamming_pairs_scan_launch takes every figure from it and
// mvfgpu_selftest_hamming_pairs_form reports it.
//
// The corpus is cut twice.  Column tile I = the QT rows [I QT, (I + 1) QT), which a block expands into LDS as H2's "queries";
// span J = the rows [J span_rows, (J + 1) span_rows), which the block streams through the matrix unit.  A pair (i, j), i < j,
// belongs to the block (tile of i, span of j), so only spans that hold a row above the tile's first row are launched: with
// span_rows = m QT those are the spans J >= I / m, for every tile whose first row is not the corpus' last.
struct HammingPairsForm {
    uint32_t query_tile;     // QT: rows of a column tile (16, 32, 64 or 128)
    uint32_t chunks;         // T: 64-byte chunks of a row's pitch; a chunk is four MFMA steps of 128 bits
    uint32_t span_rows;      // rows of a span: a multiple of 256, kHamSliceRows .. kHamPairsSpanMax
    uint32_t tiles_per_span; // m = span_rows / QT
    uint64_t tiles;          // column tiles that hold a row
    uint64_t active_tiles;   // of which those with a row behind their first: the tiles that are launched
    uint64_t spans;          // S
    uint64_t blocks;         // launched (tile, span) pairs
    uint32_t lds_bytes;      // dynamic LDS of an HJ block: the expanded tile, a start value and a count per column, the block's total
};

// blocks in front of tile group g (the m tiles [g m, (g + 1) m), each of which meets the spans g .. S - 1)
__host__ __device__ __forceinline__ uint64_t ham_pairs_blocks_before_group(uint64_t g, uint64_t spans, uint32_t m) {
    return (uint64_t)m * (g * spans - (g ? g * (g - 1u) / 2u : 0u));
}

// The triangular grid: block index b (0 .. blocks - 1) -> its column tile and its span.  Tiles in ascending order, each with its
// spans in ascending order.  Integers only: a bisection over the tile groups.
__host__ __device__ __forceinline__ void ham_pairs_decode(uint64_t b, uint64_t spans, uint32_t m, uint64_t* tile, uint64_t* span) {
    uint64_t lo = 0, hi = spans;  // the group g with before(g) <= b < before(g + 1): lo <= g < hi
    while (hi - lo > 1u) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (ham_pairs_blocks_before_group(mid, spans, m) <= b) lo = mid;
        else hi = mid;
    }
    const uint64_t rem = b - ham_pairs_blocks_before_group(lo, spans, m), per = spans - lo;
    *tile = lo * m + rem / per;
    *span = lo + rem % per;
}

// dimension = packed bytes of a row (1 .. 512), rows up to 2^32 - 65536
inline HammingPairsForm hamming_pairs_form(uint32_t dimension, uint64_t rows, uint32_t num_cus) {
    HammingPairsForm f{};
    const uint32_t pitch = (dimension + 15u) & ~15u;
    f.chunks = (pitch + 63u) / 64u;
    // hamming_radius_form's tile rule with the rows as the queries: the smallest of 16 x {1, 2, 4, 8} that holds them, 128 at most
    // up to a pitch of 256 bytes, 64 up to 512
    const uint32_t cap = pitch <= kHamMfmaWidePitch ? 128u : 64u;
    f.query_tile = 16u;
    while (f.query_tile < rows && f.query_tile < cap) f.query_tile *= 2u;
    f.lds_bytes = f.query_tile * ham_mfma_query_bytes(f.chunks) + f.query_tile * 8u + 16u;
    f.tiles = (rows + f.query_tile - 1u) / f.query_tile;
    f.active_tiles = rows >= 2u ? (rows - 1u + f.query_tile - 1u) / f.query_tile : 0u;
    // The span: a block expands its tile once (QT x chunks x 16 items of 16 bytes, a popcount per row) and then runs
    // span_rows / 256 iterations of chunks x 16 x QT / 16 MFMAs per wave, so from kHamSliceRows rows on the staging is a few per
    // cent of the block.  Longer spans amortise it further, shorter ones fill the part: about tiles x spans / 2 blocks are
    // launched, and four rounds of what the CUs hold at once (as many blocks per CU as the tile's LDS admits, 8 at most) are
    // wanted before a span grows beyond the minimum.  A 1M-row corpus gets spans of kHamPairsSpanMax and still launches
    // hundreds of thousands of blocks.
    uint32_t per_cu = kHamPairsLds / f.lds_bytes;
    if (per_cu > 8u) per_cu = 8u;
    const uint64_t want_blocks = 4ull * per_cu * (num_cus ? num_cus : 256u);
    uint64_t want_spans = f.tiles ? (2u * want_blocks + f.tiles - 1u) / f.tiles : 1u;
    if (want_spans < 1u) want_spans = 1u;
    uint64_t span = (rows + want_spans - 1u) / want_spans;
    span = (span + kHamPairsStepRows - 1u) / kHamPairsStepRows * kHamPairsStepRows;
    if (span < kHamSliceRows) span = kHamSliceRows;
    if (span > kHamPairsSpanMax) span = kHamPairsSpanMax;
    f.span_rows = (uint32_t)span;
    f.tiles_per_span = f.span_rows / f.query_tile;
    f.spans = (rows + f.span_rows - 1u) / f.span_rows;
    // every active tile I meets the spans I / m .. S - 1
    if (f.active_tiles) {
        const uint64_t g = f.active_tiles / f.tiles_per_span, r = f.active_tiles % f.tiles_per_span;
        f.blocks = ham_pairs_blocks_before_group(g, f.spans, f.tiles_per_span) + r * (f.spans - g);
    }
    return f;
}

// entries the call's list holds: what the caller has room for, the number of row pairs at most
inline uint64_t ham_pairs_list_cap(uint64_t rows, uint64_t max_pairs) {
    const uint64_t all = rows >= 2u ? rows * (rows - 1u) / 2u : 0u;  // (rows < 2^32: below 2^63)
    return max_pairs < all ? max_pairs : all;
}
// tiles of a radix pass over m pairs (radix_pass.h: kRsTile words each)
inline uint32_t ham_pairs_sort_tiles(uint64_t m) { return (uint32_t)((m + 2047u) / 2048u); }
// all of a call's device scratch where max_pairs entries are asked for and all of them are found: two counters, a degree per row,
// the list and its sort partner (a u64 composite and a u32 distance per entry each), the passes' counts
inline uint64_t ham_pairs_scratch_bytes(uint64_t rows, uint64_t max_pairs) {
    const uint64_t cap = ham_pairs_list_cap(rows, max_pairs);
    return 16u + rows * 4u + 2u * cap * 12u + (cap ? (uint64_t)ham_pairs_sort_tiles(cap) * 1024u + 1024u : 0u);
}

// What HJ and HJP take.  p: rows, tomb, n, dim, pitch, V, index_base, ids (nothing else of it is read).
struct HammingPairsParams {
    HammingParams p;
    uint32_t chunks, span_rows, tiles_per_span;
    uint64_t spans, block_base;  // block_base: the index of this launch's first block
    uint32_t radius;             // HJ clamps it to 8 x dim
    uint64_t* counters;          // [2], zero on entry: the exact number of pairs; slots drawn from the list
    uint32_t* degrees;           // [n], zero on entry, or NULL: per row, the live rows within the radius beside itself
    uint64_t* list;              // [cap] composites (i << 32 | j, row positions, i < j) in arrival order, or NULL
    uint32_t* dist;              // [cap] their distances
    uint64_t cap;
};

// HJ over the triangular grid, in launches of kHamPairsGrid blocks at most, on `s`; no host wait.
hipError_t hamming_pairs_scan_launch(const HammingPairsForm& f, const HammingPairsParams& r, hipStream_t s);

// HJP: the m composites of list_a / dist_a (all of the join's pairs, any order) sorted ascending with list_b / dist_b [m] as the
// passes' partner -- two passes per byte the row count leaves non-zero, so the result is back in list_a / dist_a --, then written
// as the call reports them: out_first / out_second = the rows' names (index_base + position, or the vector id), out_raw
// (nullable) = d.  The outputs may be the list's own arrays (out_second = list_a, out_first = list_b, out_raw = dist_a).
// bh: 256 x ham_pairs_sort_tiles(m) u32, tot: 256 u32.  On `s`, no host wait.
hipError_t hamming_pairs_order_launch(const HammingParams& p, uint64_t* list_a, uint32_t* dist_a, uint64_t* list_b, uint32_t* dist_b, uint64_t m,
                                      uint32_t* bh, uint32_t* tot, uint64_t* out_first, uint64_t* out_second, int32_t* out_raw, hipStream_t s);

}  // namespace mvf
