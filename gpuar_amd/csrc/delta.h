// delta.h -- an element-wise delta filter in front of the byte planes (planes.h).
//
// Byte planes only regroup bytes; they cannot remove the redundancy of neighbouring elements that are close in value
// (sorted indices, offsets, timestamps, samples): the low bytes of such data are noise to an order-0 model, the low bytes of
// its differences are not.  Integers only.  The groups are those of planes.h: G = w * 8192 bytes counted from the buffer's
// start, w = 1, 2, 4 or 8, and a tail of r = n mod G bytes holding e = r div w elements.  Inside one group, or inside the
// tail's e elements, with the elements read as little-endian unsigned w-byte integers v[0 .. m):
//     DELTA:    d[0] = v[0]     d[i] = v[i] - v[i - 1]   (mod 2^(8 w))
//     UNDELTA:  v[i] = d[0] + ... + d[i]                 (mod 2^(8 w)): the inclusive prefix sum
// and the tail's last r mod w bytes stay as they are.  The predictor resets at every group, which keeps groups -- and so
// CLI chunks, shards and batch buffers -- independent of each other.  By definition
//     split_delta(x, w) = split_planes(delta(x, w), w)          merge_delta = undelta after merge_planes
// and w = 1 is meaningful: a byte delta per packet with no regrouping (not a no-op, not even in place).
//
// The same source serves the host (`--host`, host/cpu_compressor.cpp; gpuar_hip_split_delta_host) and the gfx950 kernels
// (gpuar_kernels.hip), which take from here the register transform of one 16-element block, as they take planes_block from
// planes.h: delta_block() and undelta_block() work on the block's 4 w dwords in place, several elements per dword where
// w < 4 (a masked add or subtract: no carry or borrow crosses an element), a carry pair where w = 8.
// tests/test_delta_host.py runs them against the definition.
#ifndef GPUAR_DELTA_H
#define GPUAR_DELTA_H

#include "planes.h"

namespace gpuar {

// the top bit of every W-byte element of a dword (W = 1, 2)
template <int W>
GPUAR_PLANES_FN constexpr uint32_t delta_tops() { return W == 1 ? 0x80808080u : W == 2 ? 0x80008000u : 0x80000000u; }

// x + y and x - y in every W-byte element of a dword (W = 1, 2, 4), each mod 2^(8 W)
template <int W>
GPUAR_PLANES_FN uint32_t delta_add(uint32_t x, uint32_t y) {
    if constexpr (W == 4) return x + y;
    constexpr uint32_t H = delta_tops<W>();
    return ((x & ~H) + (y & ~H)) ^ ((x ^ y) & H);
}
template <int W>
GPUAR_PLANES_FN uint32_t delta_sub(uint32_t x, uint32_t y) {
    if constexpr (W == 4) return x - y;
    constexpr uint32_t H = delta_tops<W>();
    return ((x | H) - (y & ~H)) ^ ((x ^ ~y) & H);
}

// the low W bytes of `v` in every element of a dword (W = 1, 2, 4)
template <int W>
GPUAR_PLANES_FN uint32_t delta_spread(uint32_t v) {
    if constexpr (W == 1) return (v & 0xFFu) * 0x01010101u;
    else if constexpr (W == 2) return (v & 0xFFFFu) * 0x00010001u;
    else return v;
}

// One block of 16 elements, `mixed` as in planes_block: the elements back to back, little-endian.  `pred` is the element in
// front of the block (its low W bytes; 0 for a group's first block).  In place: mixed becomes the 16 differences.
template <int W>
GPUAR_PLANES_FN void delta_block(uint32_t (&mixed)[4 * W], uint64_t pred) {
    static_assert(W == 1 || W == 2 || W == 4 || W == 8, "element widths of 1, 2, 4 and 8 bytes");
    if constexpr (W == 8) {
#pragma unroll
        for (int i = 15; i >= 0; --i) {
            const uint64_t v = static_cast<uint64_t>(mixed[2 * i + 1]) << 32 | mixed[2 * i];
            const uint64_t p = i ? static_cast<uint64_t>(mixed[2 * i - 1]) << 32 | mixed[2 * i - 2] : pred;
            const uint64_t d = v - p;
            mixed[2 * i] = static_cast<uint32_t>(d), mixed[2 * i + 1] = static_cast<uint32_t>(d >> 32);
        }
    } else {
        // a dword's predecessors: the dword itself moved up by one element, with the top element of the dword in front
#pragma unroll
        for (int d = 4 * W - 1; d >= 0; --d) {
            const uint32_t front = d ? mixed[d - 1] : static_cast<uint32_t>(pred) << (32 - 8 * W);
            uint32_t prev = front;
            if constexpr (W < 4) prev = mixed[d] << (8 * W) | front >> (32 - 8 * W);
            mixed[d] = delta_sub<W>(mixed[d], prev);
        }
    }
}

// The inverse without an offset: mixed (16 differences) becomes their inclusive prefix sums; returns the block's total, the
// last of them (its low W bytes count).
template <int W>
GPUAR_PLANES_FN uint64_t delta_scan_block(uint32_t (&mixed)[4 * W]) {
    static_assert(W == 1 || W == 2 || W == 4 || W == 8, "element widths of 1, 2, 4 and 8 bytes");
    if constexpr (W == 8) {
        uint64_t sum = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            sum += static_cast<uint64_t>(mixed[2 * i + 1]) << 32 | mixed[2 * i];
            mixed[2 * i] = static_cast<uint32_t>(sum), mixed[2 * i + 1] = static_cast<uint32_t>(sum >> 32);
        }
        return sum;
    } else {
        uint32_t carry = 0;                                      // the sum so far
#pragma unroll
        for (int d = 0; d < 4 * W; ++d) {
            uint32_t x = mixed[d];
            if constexpr (W <= 2) x = delta_add<W>(x, x << (8 * W));
            if constexpr (W == 1) x = delta_add<W>(x, x << 16);
            x = delta_add<W>(x, delta_spread<W>(carry));
            mixed[d] = x;
            carry = x >> (32 - 8 * W);
        }
        return carry;
    }
}

// `offset` (its low W bytes) added to each of the block's 16 elements
template <int W>
GPUAR_PLANES_FN void delta_offset_block(uint32_t (&mixed)[4 * W], uint64_t offset) {
    if constexpr (W == 8) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint64_t v = (static_cast<uint64_t>(mixed[2 * i + 1]) << 32 | mixed[2 * i]) + offset;
            mixed[2 * i] = static_cast<uint32_t>(v), mixed[2 * i + 1] = static_cast<uint32_t>(v >> 32);
        }
    } else {
        const uint32_t each = delta_spread<W>(static_cast<uint32_t>(offset));
#pragma unroll
        for (int d = 0; d < 4 * W; ++d) mixed[d] = delta_add<W>(mixed[d], each);
    }
}

// The inverse of delta_block: mixed becomes the inclusive local prefix sums plus `offset`, the sum of everything in front of
// the block in its group (= pred); returns the block's total without the offset.  Modular addition is associative: a caller may
// scan with an offset of 0, combine the totals of many blocks in any order and add each block's offset afterwards.
template <int W>
GPUAR_PLANES_FN uint64_t undelta_block(uint32_t (&mixed)[4 * W], uint64_t offset) {
    const uint64_t total = delta_scan_block<W>(mixed);
    delta_offset_block<W>(mixed, offset);
    return total;
}

inline uint64_t delta_load(const uint8_t *p, uint32_t w) {
    uint64_t v = 0;
    for (uint32_t k = 0; k < w; ++k) v |= static_cast<uint64_t>(p[k]) << (8 * k);
    return v;
}
inline void delta_store(uint8_t *p, uint32_t w, uint64_t v) {
    for (uint32_t k = 0; k < w; ++k) p[k] = static_cast<uint8_t>(v >> (8 * k));
}

// Host: the definition of DELTA (Undo = false) and UNDELTA (true), group by group.  `out` may be `in` (an element is read
// before it is written); any other overlap is the caller's to avoid.
template <bool Undo>
inline void delta_host(const uint8_t *in, size_t n, uint32_t w, uint8_t *out) {
    const size_t G = static_cast<size_t>(w) * kPlanePacket;
    for (size_t B = 0; B < n; B += G) {
        const size_t r = n - B < G ? n - B : G, e = r / w;          // e = 8192 for a full group
        uint64_t carried = 0;                                       // delta: v[i - 1]; undelta: the sum so far
        for (size_t i = 0; i < e; ++i) {
            const uint64_t x = delta_load(in + B + i * w, w);
            delta_store(out + B + i * w, w, Undo ? carried + x : x - carried);
            carried = Undo ? carried + x : x;
        }
        if (out != in)
            for (size_t i = e * w; i < r; ++i) out[B + i] = in[B + i];
    }
}

// split_delta = split_planes of delta; merge_delta its inverse.  `out` may be `in`.
inline void split_delta_host(const uint8_t *in, size_t n, uint32_t w, uint8_t *out) {
    delta_host<false>(in, n, w, out);
    planes_host<false>(out, n, w, out);
}
inline void merge_delta_host(const uint8_t *in, size_t n, uint32_t w, uint8_t *out) {
    planes_host<true>(in, n, w, out);
    delta_host<true>(out, n, w, out);
}

}  // namespace gpuar

#endif  // GPUAR_DELTA_H
