// scan_hamming_maxsim.h — the form and the launch interface of B0 and the integer sums, the binary MaxSim's kernels
// (scan_hamming_maxsim.hip; hamming_maxsim.hip is the host side; include/mvf_gpu_hamming_maxsim.h; DESIGN.md §3 "Binary MaxSim",
// §5 "B0").
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mvf_common.h"
#include "scan_hamming_mfma.h"
#include "scan_maxsim.h"

namespace mvf {

constexpr uint32_t kBinMaxsimMaxDim = kHamMfmaPitch;  // packed bytes of a row at most
constexpr uint32_t kBinMaxsimTile = 16;               // query rows of one accumulator: HQ's smallest tile
constexpr uint32_t kBinMaxsimPassTiles = 4;           // MT: accumulator tiles a wave holds per fragment of its rows
constexpr uint32_t kBinMaxsimFrags = 2;               // 16-position fragments of a wave: 4 waves x 2 x 16 = kMaxsimRows
constexpr uint32_t kBinMaxsimRegPitch = 64;           // rows up to this pitch (one chunk) stay in registers over the launch

static_assert(4u * kBinMaxsimFrags * 16u == kMaxsimRows, "four waves cover a block's positions");

// The shape of a call, a pure function of its sizes: hamming_maxsim_core takes every figure from it and
// mvfgpu_selftest_hamming_maxsim_form reports it.
struct HammingMaxsimForm {
    uint32_t query_tile;     // query rows of one pass of B0 over a block's rows: kBinMaxsimTile x MT
    uint32_t chunks;         // 64-byte chunks of a row's pitch; a chunk is four MFMA steps of 128 bits
    bool reg;                // a lane's words of its rows stay in registers across every pass of the launch
    uint32_t chunk, window;  // tokens per chunk, query sets per window (maxsim_plan with token_bytes = 0)
    uint32_t lds_bytes;      // static LDS of a B0 block
    uint64_t prepared_row;   // HQ's bytes of one query row: its FP4 operands and its start
    uint64_t scratch_bytes;  // what the budget holds: per set of a window the minima, S, the sort buffers, the prepared tokens
};

// dimension = packed bytes of a row (1 .. 512).  HQ prepares every (set, token) of a window ONCE, so the prepared tokens are a
// per-set cost like S and the sort buffers: a set's share comes off the budget before maxsim_plan sizes the chunk, and the window
// is what the budget holds of whole sets.  One token group (all tokens where there are fewer) and one set whatever the budget.
inline HammingMaxsimForm hamming_maxsim_form(uint32_t dimension, uint32_t nq, uint32_t n_tokens, uint64_t n_keys, uint64_t budget_bytes) {
    HammingMaxsimForm f{};
    const uint32_t pitch = (dimension + 15u) & ~15u;
    f.query_tile = kBinMaxsimTile * kBinMaxsimPassTiles;
    f.chunks = (pitch + 63u) / 64u;
    f.reg = pitch <= kBinMaxsimRegPitch;
    f.lds_bytes = f.query_tile * (kMaxsimRows * 4u + 8u);  // the minima; the pass's rows' places and starts
    f.prepared_row = ham_mfma_query_bytes(f.chunks) + 4u;
    const uint64_t prep_set = (uint64_t)n_tokens * f.prepared_row;
    const MaxsimPlan pl = maxsim_plan(n_keys, n_tokens, nq, 0, budget_bytes > prep_set ? budget_bytes - prep_set : 0);
    const uint64_t per_set = (n_keys ? n_keys : 1) * ((uint64_t)pl.chunk * 4 + kMaxsimKeyBytes) + prep_set;
    f.chunk = pl.chunk;
    f.window = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(pl.window, budget_bytes / per_set));
    f.scratch_bytes = f.window * per_set;
    return f;
}

// query rows HQ prepares for `rows` (set, token) rows: whole tiles
inline uint64_t bin_maxsim_prepared_rows(uint64_t rows) { return (rows + kBinMaxsimTile - 1) / kBinMaxsimTile * kBinMaxsimTile; }

// every word of best[words] = 0xFFFFFFFF: once per call; the sums leave the words they read that way
hipError_t hamming_maxsim_clear_launch(uint32_t* best, size_t words, hipStream_t s);

// B0.  Grid (blocks of kMaxsimRows list positions), block 256.  best[set][t][n_keys], all 0xFFFFFFFF on entry, receives the
// smallest Hamming distance of tokens [t0, t0 + tc) of every query set over each key's rows.
struct HammingMaxsimParams {
    const unsigned char* rows;
    const unsigned char* prepared;  // HQ's operands of the window's sets x n_tokens query rows, tiles of kBinMaxsimTile
    const float* starts;            // [sets x n_tokens, whole tiles] popcount(q)
    const uint32_t* list;           // the key-ordered list [m]
    const uint32_t* ord;            // [m] key ordinals
    uint32_t* best;
    uint32_t m, n_keys, sets, n_tokens, t0, tc, dim, pitch, V, chunks;
};
hipError_t hamming_maxsim_score_launch(const HammingMaxsimParams& p, hipStream_t s);

// The integer sums.  sum[set][g] (f32 holding the exact integer S <= 2^22; not read when `first`) advances by the chunk's tc
// minima, and every word read of best goes back to 0xFFFFFFFF; `last`: rank[set][g] = rank_entry(S, g): S itself is the order
// key -- ascending, ties by ascending ordinal.
struct HammingMaxsimSumParams {
    uint32_t* best;
    float* sum;
    uint64_t* rank;
    uint32_t n_keys, sets, tc;
    bool first, last;
};
hipError_t hamming_maxsim_sum_launch(const HammingMaxsimSumParams& p, hipStream_t s);

}  // namespace mvf
