// xorbase.h -- XOR against a base buffer in front of the byte planes (planes.h).
//
// Every filter so far looks inside one buffer.  The next checkpoint of a model is almost the previous one: XOR with the
// previous tensor turns the unchanged sign, exponent and high mantissa bits into zero bytes, which the order-0 model codes to
// almost nothing.  Integers only.  For a buffer x and a base b of the same n bytes:
//     XOR:          y[i] = x[i] ^ b[i]        0 <= i < n            (its own inverse)
//     split_xor(x, b, w) = split_planes(y, w)                       merge_xor(s, b, w) = merge_planes(s, w) ^ b
// with w = 1, 2, 4 or 8.  XOR works on single bytes, so it needs no element rule, covers every byte of a tail (the last
// r mod w included) and commutes with the regrouping; groups, tails and chunk independence are those of planes.h.  w = 1 is
// meaningful: a plain XOR with no regrouping (not a no-op, not even in place).  The base is only read and never overlaps
// the output.
//
// The same source serves the host (`--host`, host/cpu_compressor.cpp; gpuar_hip_split_xor_host) and the gfx950 kernels
// (gpuar_kernels.hip), which take from here the register form of one 16-element block, as they take planes_block from
// planes.h.
#ifndef GPUAR_XORBASE_H
#define GPUAR_XORBASE_H

#include "planes.h"

namespace gpuar {

// One block of 16 elements, `mixed` as in planes_block: the elements back to back; `base`: the same bytes of the base.
// In place: mixed becomes mixed ^ base.
template <int W>
GPUAR_PLANES_FN void xor_block(uint32_t (&mixed)[4 * W], const uint32_t (&base)[4 * W]) {
    static_assert(W == 1 || W == 2 || W == 4 || W == 8, "element widths of 1, 2, 4 and 8 bytes");
#pragma unroll
    for (int d = 0; d < 4 * W; ++d) mixed[d] ^= base[d];
}

// Host: the definition.  `out` may be `in`; `base` lies apart from `out`.
inline void xor_host(const uint8_t *in, const uint8_t *base, size_t n, uint8_t *out) {
    for (size_t i = 0; i < n; ++i) out[i] = static_cast<uint8_t>(in[i] ^ base[i]);
}

// split_xor = split_planes of the XOR; merge_xor its inverse.  `out` may be `in`.
inline void split_xor_host(const uint8_t *in, const uint8_t *base, size_t n, uint32_t w, uint8_t *out) {
    xor_host(in, base, n, out);
    planes_host<false>(out, n, w, out);
}
inline void merge_xor_host(const uint8_t *in, const uint8_t *base, size_t n, uint32_t w, uint8_t *out) {
    planes_host<true>(in, n, w, out);
    xor_host(out, base, n, out);
}

}  // namespace gpuar

#endif  // GPUAR_XORBASE_H
