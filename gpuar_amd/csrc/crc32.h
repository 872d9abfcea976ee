// crc32.h -- CRC-32/ISO-HDLC (the CRC of zlib.crc32 and gzip: reflected polynomial 0xEDB88320, initial value and final
// xor 0xFFFFFFFF, crc32("123456789") = 0xCBF43926) for the per-packet checksums of the .gip trailer (host/packet_index.hpp).
//
// The tables are built at compile time from the polynomial alone, and the same source serves the gfx950 kernels
// (gpuar_kernels.hip) and the host (`--host`, host/cpu_compressor.cpp).  tests/test_checksum_host.py checks every table
// here against zlib.
//
// The kernels cut a packet into 64 chunks of 128 bytes, one per lane.  Each lane computes the RAW CRC of its chunk (initial
// value 0, no final xor; lane 0 starts from 0xFFFFFFFF instead and so carries the initial value), multiplies it by
// x^(8 d) mod P, where d is the number of packet bytes behind its chunk, and the wavefront xors the 64 products: by
// linearity that is the packet's CRC before the final xor.  A raw CRC state is a polynomial of degree < 32 stored
// reflected: bit 31 is the coefficient of x^0, bit 0 that of x^31.
#ifndef GPUAR_CRC32_H
#define GPUAR_CRC32_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GPUAR_CRC_FN __host__ __device__ constexpr
#else
#define GPUAR_CRC_FN constexpr
#endif

namespace gpuar {

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcLanes = 64;                    // lanes per packet
constexpr uint32_t kCrcChunk = 8192u / kCrcLanes;      // bytes per lane: 128

// a * b mod P (both reflected)
GPUAR_CRC_FN uint32_t crc_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        if ((a >> i) & 1u) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? kCrcPoly : 0u);
    }
    return p;
}

// Slicing-by-4: t[0] is the byte table (state after one byte x: t[0][x] = x * x^32 mod P), t[k][x] the same byte followed by
// k zero bytes.  One step over a little-endian word w: c ^= w; c = t[3][c & 255] ^ t[2][c >> 8 & 255] ^ t[1][c >> 16 & 255] ^
// t[0][c >> 24].
struct CrcTables {
    uint32_t t[4][256];
    constexpr CrcTables() : t{} {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? kCrcPoly : 0u);
            t[0][i] = c;
        }
        for (uint32_t k = 1; k < 4; ++k)
            for (uint32_t i = 0; i < 256; ++i) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 255u];
    }
};

// x^(8 d) mod P for d = 0 .. 8192: what d zero bytes do to a raw CRC state (crc_mulmod(state, k[d]))
struct CrcShiftTable {
    uint32_t k[8193];
    constexpr CrcShiftTable() : k{} {
        const CrcTables tab = CrcTables();
        k[0] = 0x80000000u;                                     // x^0
        for (uint32_t d = 1; d <= 8192; ++d) k[d] = tab.t[0][k[d - 1] & 255u] ^ (k[d - 1] >> 8);
    }
};

// The multiply by x^(8 d) as a 32 x 32 matrix over GF(2), for the lanes of a FULL packet: lane l's chunk has
// d = 8192 - 128 (l + 1) bytes behind it, and c[i][l] = (1 << i) * x^(8 d) mod P, so that the product of a state s is the
// xor of c[i][l] over the bits i set in s (column-major: the 64 lanes read one row of a column at a time).
struct CrcLaneColumns {
    uint32_t c[32][kCrcLanes];
    constexpr CrcLaneColumns() : c{} {
        const CrcShiftTable sh = CrcShiftTable();
        for (uint32_t l = 0; l < kCrcLanes; ++l)
            for (uint32_t i = 0; i < 32; ++i) c[i][l] = crc_mulmod(1u << i, sh.k[8192u - kCrcChunk * (l + 1u)]);
    }
};

#if !defined(__HIP_DEVICE_COMPILE__)
// Host: zlib.crc32(data, crc) -- `crc` is a previous result (0 to start), as in zlib
inline uint32_t crc32_update(uint32_t crc, const uint8_t *p, size_t n) {
    static const CrcTables tab = CrcTables();
    uint32_t c = ~crc;
    for (; n >= 4; n -= 4, p += 4) {
        c ^= static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8 | static_cast<uint32_t>(p[2]) << 16 | static_cast<uint32_t>(p[3]) << 24;
        c = tab.t[3][c & 255u] ^ tab.t[2][(c >> 8) & 255u] ^ tab.t[1][(c >> 16) & 255u] ^ tab.t[0][c >> 24];
    }
    for (; n; --n, ++p) c = tab.t[0][(c ^ *p) & 255u] ^ (c >> 8);
    return ~c;
}
#endif

}  // namespace gpuar

#endif  // GPUAR_CRC32_H
