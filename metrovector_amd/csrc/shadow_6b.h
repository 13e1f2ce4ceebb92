// shadow_6b.h — the layout of the 6-BIT SHADOW of a Float32 corpus (shadow_6b.hip builds it, K1's dt2y unit streams it),
// stated once for the device, the host pack / unpack entry points and the tests.
//
// A row is quantised to x6 = rint(x / s_r) in [-31, 31], s_r = max|x| / 31, and stored as the CODE y = x6 + 32 (1..63, a
// non-negative byte value; padding elements carry 32 = the value 0).  64 consecutive elements are one UNIT of 48 bytes,
// three 16-byte PLANES:
//     plane p (0..2), byte b (0..15):  bits 0-5 = code of element 16 p + b,  bits 6-7 = bits 2p .. 2p+1 of the code of
//     element 48 + b
// so one dword of each plane unpacks into the four dwords of codes of the elements 4i.., 16 + 4i.., 32 + 4i.., 48 + 4i.. of the
// unit (i = 0..3) with three AND and three shift-and-mask-or: the query sits in LDS in its NATURAL element order.
//
// 64 consecutive rows are one TILE.  Inside a tile, the plane p of unit u of all 64 rows is one contiguous KiB, row r of the
// tile at byte 16 r of it; the KiBs follow each other in (u, p) order.  One lane of a wave owns one row: a wave-load of (u, p)
// reads exactly that aligned KiB, whatever the dimension -- no lane idles in a ragged last step and no row starts inside
// a 128-byte line (K1 over a plain 576-byte pitch would: DESIGN.md section 5).  The corpus is padded to whole tiles; the
// bytes of the rows behind the last one are zero.
//     10M x 768:  12 units, 36 KiB per tile, 156 250 tiles = 5.76 GB  (int8 shadow: 7.68 GB, stored rows: 30.72 GB)
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MVF_S6_HD __host__ __device__
#else
#define MVF_S6_HD
#endif

namespace mvf {

constexpr uint32_t kS6TileRows = 64;
constexpr int kS6Max = 31, kS6Bias = 32;

MVF_S6_HD inline uint32_t s6_units(uint32_t dim) { return (dim + 63u) / 64u; }
MVF_S6_HD inline size_t s6_tile_bytes(uint32_t dim) { return (size_t)s6_units(dim) * 3u * 1024u; }
MVF_S6_HD inline size_t s6_bytes(uint64_t rows, uint32_t dim) { return (size_t)((rows + kS6TileRows - 1) / kS6TileRows) * s6_tile_bytes(dim); }
// byte offset of plane `plane` of unit `unit` of row `row` (its 16 bytes)
MVF_S6_HD inline size_t s6_offset(uint64_t row, uint32_t dim, uint32_t unit, uint32_t plane) {
    return (size_t)(row / kS6TileRows) * s6_tile_bytes(dim) + ((size_t)unit * 3u + plane) * 1024u + (size_t)(row % kS6TileRows) * 16u;
}

// Host reference of the packing: codes[0..dim) in [-31, 31] of row `row` into / out of the shadow at `base`.
inline void s6_pack_row(const int8_t* codes, uint32_t dim, uint64_t row, unsigned char* base) {
    for (uint32_t u = 0; u < s6_units(dim); u++) {
        auto code = [&](uint32_t e) -> uint32_t { return (uint32_t)((e < dim ? codes[e] : 0) + kS6Bias) & 63u; };
        for (uint32_t p = 0; p < 3; p++) {
            unsigned char* dst = base + s6_offset(row, dim, u, p);
            for (uint32_t b = 0; b < 16; b++)
                dst[b] = (unsigned char)(code(u * 64 + p * 16 + b) | (((code(u * 64 + 48 + b) >> (2 * p)) & 3u) << 6));
        }
    }
}
inline void s6_unpack_row(const unsigned char* base, uint32_t dim, uint64_t row, int8_t* codes) {
    for (uint32_t e = 0; e < dim; e++) {
        const uint32_t u = e / 64, i = e % 64, b = i % 16;
        uint32_t y;
        if (i < 48) y = base[s6_offset(row, dim, u, i / 16) + b] & 63u;
        else y = (base[s6_offset(row, dim, u, 0) + b] >> 6) | ((base[s6_offset(row, dim, u, 1) + b] >> 6) << 2) | ((base[s6_offset(row, dim, u, 2) + b] >> 6) << 4);
        codes[e] = (int8_t)((int)y - kS6Bias);
    }
}

}  // namespace mvf
