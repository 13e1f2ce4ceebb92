// scan_grouped.h — launch interface of the grouped search's kernels (scan_grouped.hip; grouped.hip is the host side) and the
// tier rule of G1, a pure function host and device share (DESIGN.md §5 "G0 / G1 — grouped search").
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mvf_common.h"

namespace mvf {

constexpr uint32_t kGroupTile = 1024;    // entries of the key-ordered list one block of G1 covers
constexpr uint32_t kGroupRankMax = 128;  // a run of up to this many entries that lies inside one tile is ranked by counting

inline uint32_t group_tiles(uint64_t live) { return (uint32_t)((live + kGroupTile - 1) / kGroupTile); }

// A RUN is what one tile holds of one key's segment.  Its tier, from its length, the cap and whether the segment goes on in
// another tile (`crossing`):
//   0  the whole segment lies in the tile and holds at most per_key entries: every entry survives;
//   1  the whole segment lies in the tile, up to kGroupRankMax entries: every entry counts the entries of its run in front
//      of it (LDS broadcast reads) and survives below per_key;
//   2  longer runs and every run of a crossing segment: one wave keeps the run's 64 best, one per lane, and merges 64 entries
//      at a time; a crossing segment's runs leave their lists to G1's second kernel.
MVF_HD uint32_t group_run_tier(uint32_t len, uint32_t per_key, bool crossing) {
    if (crossing) return 2u;
    if (len <= per_key) return 0u;
    return len <= kGroupRankMax ? 1u : 2u;
}

// bounds[i] = (first entry, end) of the segment that entry i of the key-ordered list lies in, from the key table's offsets
// [n_keys + 1] (offsets[n_keys] = live); once per call
hipError_t group_bounds_launch(const uint64_t* offsets, uint64_t n_keys, uint32_t live, uint2* bounds, hipStream_t s);

// out[q][r] = the dead rank entry of local row r, r < n, for nq lists of stride n
hipError_t group_dead_fill_launch(uint64_t* out, uint32_t n, uint32_t nq, hipStream_t s);

// G1.  scored[q][live]: query q's rank entries in the key-ordered list's order (G0's dump); out[q][n]: row-indexed rank
// entries, all dead on entry.  The per_key best entries -- smallest (key, local row) -- of every segment are written to
// out[q][their row]; every other row stays dead.  partial: [nq][tiles][2][64] composites of scratch (the lists of crossing
// segments' runs: [0] the run that began in an earlier tile, [1] the run that goes on in the next).
struct GroupParams {
    const uint64_t* scored;
    const uint2* bounds;
    uint64_t* partial;
    uint64_t* out;
    uint32_t live, n, nq, per_key;
};
hipError_t group_best_launch(const GroupParams& p, hipStream_t s);

// out[i] = rows[i] == ~0 ? 0 : values[rows[i]] zero-extended (mvfgpu_column_gather)
hipError_t column_gather_launch(const void* values, bool is_u64, const uint64_t* rows, uint64_t count, uint64_t* out, hipStream_t s);

}  // namespace mvf
