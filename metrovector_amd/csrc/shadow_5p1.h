// shadow_5p1.h — the "5+1" layout of the 6-bit shadow of a Float32 corpus: the same codes, row scales and bound maxima as
// shadow_6b.h (shadow_6b.hip quantises once for both), stored so that a scan can read five bits of every row and the sixth
// only of the rows that can still matter (scan_stream.inc, S51).  Stated once for the device, the host pack / unpack entry
// points and the tests.
//
// The code y = x6 + 32 (1..63; padding elements 32) is split as y = 2 hi + lo, hi in 0..31, lo in {0, 1}.  128 consecutive
// elements are one UNIT of 96 bytes per row: five 16-byte HI PLANES and one 16-byte LO PLANE.
//     hi plane p (0..4), byte b (0..15):  bits 0-4 = hi of element 16 p + b,  bits 5-7 = bits 3p .. 3p+2 of the 15-bit word
//         s = hi(80 + b) | hi(96 + b) << 5 | hi(112 + b) << 10
//     so one dword of each of the five planes unpacks into the eight dwords of hi values of the elements 16 g + 4 i .. (g = 0..7)
//     with five AND and seven shift-and-mask pieces (19 VALU operations per 32 elements against the 6-bit layout's 18): the
//     query sits in LDS in its NATURAL element order.
//     lo plane, dword d (0..3):  bit m + 8 t (m = 0..7, t = 0..3) = lo of element 32 d + 4 m + t
//     so (dword >> m) & 0x01010101 is the dword of lo values of the elements 32 d + 4 m .. + 3.
//
// 64 consecutive rows are one TILE.  First all hi planes in (unit, plane) order, one aligned KiB each with row r of the tile at
// byte 16 r; behind them the lo planes of all units, one KiB each, row r at byte 16 r -- eight rows share a 128-byte line,
// which is the unit the scan skips by.  The corpus is padded to whole tiles; the bytes of the rows behind the last one are zero.
//     10M x 768:  6 units, 36 KiB per tile (30 hi + 6 lo) = 5.76 GB, the 6-bit layout's size.
// The layout is no larger than the 6-bit one iff dim mod 128 is 0 or above 64 (s51_eligible).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "shadow_6b.h"

namespace mvf {

MVF_S6_HD inline uint32_t s51_units(uint32_t dim) { return (dim + 127u) / 128u; }
MVF_S6_HD inline size_t s51_hi_tile_bytes(uint32_t dim) { return (size_t)s51_units(dim) * 5u * 1024u; }
MVF_S6_HD inline size_t s51_tile_bytes(uint32_t dim) { return (size_t)s51_units(dim) * 6u * 1024u; }
MVF_S6_HD inline size_t s51_bytes(uint64_t rows, uint32_t dim) { return (size_t)((rows + kS6TileRows - 1) / kS6TileRows) * s51_tile_bytes(dim); }
MVF_S6_HD inline size_t s51_hi_bytes(uint64_t rows, uint32_t dim) { return (size_t)((rows + kS6TileRows - 1) / kS6TileRows) * s51_hi_tile_bytes(dim); }
MVF_S6_HD inline bool s51_eligible(uint32_t dim) { return dim != 0 && (dim % 128u == 0 || dim % 128u > 64u); }
// byte offset of hi plane `plane` (0..4) of unit `unit` of row `row` (its 16 bytes) ...
MVF_S6_HD inline size_t s51_hi_offset(uint64_t row, uint32_t dim, uint32_t unit, uint32_t plane) {
    return (size_t)(row / kS6TileRows) * s51_tile_bytes(dim) + ((size_t)unit * 5u + plane) * 1024u + (size_t)(row % kS6TileRows) * 16u;
}
// ... and of the lo plane of that unit
MVF_S6_HD inline size_t s51_lo_offset(uint64_t row, uint32_t dim, uint32_t unit) {
    return (size_t)(row / kS6TileRows) * s51_tile_bytes(dim) + s51_hi_tile_bytes(dim) + (size_t)unit * 1024u + (size_t)(row % kS6TileRows) * 16u;
}
// where the lo bit of element i (0..127) of a unit sits in its 16-byte lo plane: bit (i % 32 / 4) + 8 (i % 4) of dword i / 32
MVF_S6_HD inline uint32_t s51_lo_bit(uint32_t i) { return (i / 32u) * 32u + (i % 32u) / 4u + 8u * (i % 4u); }

// Host reference of the packing: codes[0..dim) in [-31, 31] of row `row` into / out of the shadow at `base`.
inline void s51_pack_row(const int8_t* codes, uint32_t dim, uint64_t row, unsigned char* base) {
    for (uint32_t u = 0; u < s51_units(dim); u++) {
        auto code = [&](uint32_t e) -> uint32_t { return (uint32_t)((e < dim ? codes[e] : 0) + kS6Bias) & 63u; };
        for (uint32_t b = 0; b < 16; b++) {
            const uint32_t s = (code(u * 128 + 80 + b) >> 1) | ((code(u * 128 + 96 + b) >> 1) << 5) | ((code(u * 128 + 112 + b) >> 1) << 10);
            for (uint32_t p = 0; p < 5; p++)
                base[s51_hi_offset(row, dim, u, p) + b] = (unsigned char)((code(u * 128 + p * 16 + b) >> 1) | (((s >> (3 * p)) & 7u) << 5));
        }
        unsigned char* lo = base + s51_lo_offset(row, dim, u);
        for (uint32_t b = 0; b < 16; b++) lo[b] = 0;
        for (uint32_t i = 0; i < 128; i++) {
            const uint32_t bit = s51_lo_bit(i);
            lo[bit / 8] = (unsigned char)(lo[bit / 8] | ((code(u * 128 + i) & 1u) << (bit % 8)));
        }
    }
}
inline void s51_unpack_row(const unsigned char* base, uint32_t dim, uint64_t row, int8_t* codes) {
    for (uint32_t e = 0; e < dim; e++) {
        const uint32_t u = e / 128, i = e % 128, b = i % 16;
        uint32_t hi;
        if (i < 80) hi = base[s51_hi_offset(row, dim, u, i / 16) + b] & 31u;
        else {
            uint32_t s = 0;
            for (uint32_t p = 0; p < 5; p++) s |= (uint32_t)(base[s51_hi_offset(row, dim, u, p) + b] >> 5) << (3 * p);
            hi = (s >> (5 * ((i - 80) / 16))) & 31u;
        }
        const uint32_t bit = s51_lo_bit(i);
        const uint32_t lo = (base[s51_lo_offset(row, dim, u) + bit / 8] >> (bit % 8)) & 1u;
        codes[e] = (int8_t)((int)(2 * hi + lo) - kS6Bias);
    }
}

}  // namespace mvf
