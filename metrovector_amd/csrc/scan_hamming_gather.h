// scan_hamming_gather.h — the route, the form and the launch interface of HG, the filtered Hamming search's list route: H2's
// arithmetic over the ascending list of a filter's admitted rows (scan_hamming_gather.hip; hamming_filtered.hip;
// include/mvf_gpu_hamming_filtered.h; DESIGN.md §5 "HG").
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mvf_common.h"
#include "scan_hamming.h"
#include "scan_hamming_mfma.h"

namespace mvf {

constexpr uint32_t kHamGatherSliceEntries = 1024;  // list entries of a slice at least: every slice pays for its queries' selection
// The automatic rule: the shapes in which route 2 was measured to beat route 1 by more than 7 % (profiles/r30_hamming_filtered.txt:
// 10M rows of 64, 128 and 512 bytes, k = 100, 1 .. 1024 queries; 1.6x at the least up to a tenth of the rows admitted).  The rows
// each route reads never speak against the list -- its query tiles are never more than the mask route's, H0's or H2's, and it
// reads admitted <= rows per tile -- so the measured region is the whole rule:
constexpr uint32_t kHamGatherMaxShare = 10;       // up to rows / 10 admitted (half: one loss, 0.91x at 128 bytes x 128 queries; between: not measured),
constexpr uint64_t kHamGatherMinRows = 10000000;  // 10M rows (smaller corpora: not measured; HG's floor of 0.05 .. 2 ms does not fall with the rows),
constexpr uint32_t kHamGatherMinPitch = 64;       // rows of 64 bytes (shorter rows: not measured),
constexpr uint32_t kHamGatherMaxAutoK = 128;      // lists of up to 128 entries (k = 100; larger k: not measured)

// The shape of one window on the list route, a pure function of its sizes: hamming_gather_launch takes every figure from it
// and mvfgpu_selftest_hamming_filtered_form reports it.
struct HammingGatherForm {
    uint32_t query_tile;     // QT: queries whose prepared bits a block holds in LDS (16, 32, 64 or 128)
    uint32_t chunks;         // T: 64-byte chunks of a row's pitch; a chunk is four MFMA steps of 128 bits
    uint32_t kcap, buf;      // next_pow2(k), entries of a query's candidate buffer (H0's)
    uint32_t tiles;          // query tiles of the window
    uint32_t list_slices;    // S: ranges the list is split into (0 for an empty list)
    uint64_t slice_entries;  // list entries of a slice, a multiple of an iteration's 256 (the last slice may hold fewer)
    uint32_t lds_bytes;      // dynamic LDS of an HG block
    uint64_t prepared_bytes; // HQ's scratch: the tiles' FP4 queries and their starts
    uint64_t scratch_bytes;  // the candidate buffers: S x tiles x QT x buf x 8
};

// the smallest tile of 16 x {1, 2, 4, 8} queries that holds the window's, capped as HR2's is: 128 up to a pitch of 256 bytes, 64
// up to 512 -- a selective filter's batch is small, and one query in a 128-query tile wastes seven eighths of the MFMAs
inline uint32_t hamming_gather_tile(uint32_t pitch, uint32_t nq) {
    const uint32_t cap = pitch <= kHamMfmaWidePitch ? 128u : 64u;
    uint32_t qt = 16u;
    while (qt < nq && qt < cap) qt *= 2u;
    return qt;
}

// dimension = packed bytes of a row (1 .. 512), nq = 1 .. 1024, k = 1 .. 1024, admitted = entries of the list
inline HammingGatherForm hamming_gather_form(uint32_t dimension, uint32_t nq, uint32_t k, uint64_t admitted, uint32_t num_cus) {
    HammingGatherForm f{};
    const uint32_t pitch = (dimension + 15u) & ~15u;
    f.query_tile = hamming_gather_tile(pitch, nq);
    f.chunks = (pitch + 63u) / 64u;
    f.kcap = next_pow2(k);
    f.buf = f.kcap * 2u > kHamBufMin ? f.kcap * 2u : kHamBufMin;
    f.tiles = (nq + f.query_tile - 1u) / f.query_tile;
    // the staged queries, the sort area, thresholds, starts, counts, flag (H2's layout)
    f.lds_bytes = f.query_tile * ham_mfma_query_bytes(f.chunks) + f.buf * 8u + f.query_tile * (8u + 4u + 4u) + 16u;
    f.prepared_bytes = (uint64_t)f.tiles * f.query_tile * (ham_mfma_query_bytes(f.chunks) + 4u);
    // slices: one block per CU over all query tiles, a slice of kHamGatherSliceEntries entries at least, what H1 merges and what
    // the candidate scratch holds at most (hamming_mfma_form's bounds)
    const uint64_t per_block = (uint64_t)f.query_tile * f.buf * 8u;
    uint64_t want = ((uint64_t)(num_cus ? num_cus : 256u) + f.tiles - 1u) / f.tiles;
    const uint64_t by_entries = admitted / kHamGatherSliceEntries;
    if (want > by_entries) want = by_entries;
    if (want > kHamMergeMax / f.kcap) want = kHamMergeMax / f.kcap;
    if (want > kHamMfmaScratch / (per_block * f.tiles)) want = kHamMfmaScratch / (per_block * f.tiles);
    if (want < 1) want = 1;
    f.slice_entries = ((admitted + want - 1u) / want + kHamStepRows - 1u) / kHamStepRows * kHamStepRows;
    if (f.slice_entries < kHamGatherSliceEntries) f.slice_entries = kHamGatherSliceEntries;
    f.list_slices = (uint32_t)((admitted + f.slice_entries - 1u) / f.slice_entries);
    f.scratch_bytes = (uint64_t)f.list_slices * f.tiles * per_block;
    return f;
}

// The route of one window of a filtered Hamming search, a pure function (mvfgpu_selftest_hamming_filtered_form; the launch
// calls it): 1 = mask (the Hamming search with the filter's deny mask in the tombstones' place), 2 = list (HG).  forced: the
// filter's forced route (MVF_FILTER_ROUTE when its handle read its tuning; 0 = automatic).  Eligible for the list: a pitch of
// up to 512 bytes, a filter that holds its row list, at least one admitted row; everything else is route 1 whatever is forced.
// Automatic: route 2 from kHamGatherMinRows rows of a pitch of kHamGatherMinPitch on, for lists of up to kHamGatherMaxAutoK
// entries, where the filter admits at most rows / kHamGatherMaxShare; nq (1 .. 1024 were measured) does not enter.
inline uint32_t hamming_filter_route(uint32_t dimension, uint32_t nq, uint32_t k, uint64_t rows, uint64_t admitted, bool has_list,
                                     int forced) {
    const uint32_t pitch = (dimension + 15u) & ~15u;
    if (pitch > kHamMfmaPitch || !has_list || admitted == 0 || forced == 1) return 1u;
    if (forced == 2) return 2u;
    return rows >= kHamGatherMinRows && pitch >= kHamGatherMinPitch && next_pow2(k) <= kHamGatherMaxAutoK &&
                   admitted * kHamGatherMaxShare <= rows ? 2u : 1u;
}

// what HQ, HG and H1 take: a.p as the Hamming search's (tomb NULL: the list holds admitted live rows only; query_tile, buf, kcap
// from the form; row_slices = the form's list_slices), a.chunks, a.tiles, a.prepared, a.starts, a.cand as H2 takes them
struct HammingGatherParams {
    HammingMfmaParams a;
    const uint32_t* list;    // [m] ascending row positions, each below a.p.n
    uint32_t m;              // entries of the list
    uint32_t slice_entries;  // the form's
};

// HQ, HG over the grid (list slices x query tiles), then H1: three launches on `s`, no host wait.
// marks (the stage timer only): four events, recorded in front of HQ, between HQ and HG, between HG and H1 and behind H1.
hipError_t hamming_gather_launch(const HammingGatherForm& f, const HammingGatherParams& g, hipStream_t s, hipEvent_t* marks = nullptr);

}  // namespace mvf
