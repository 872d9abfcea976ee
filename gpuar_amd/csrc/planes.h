// planes.h -- byte-plane splitting of typed data in front of the packet codec.
//
// A buffer of elements `w` bytes wide (w = 2, 4 or 8; w = 1 is the identity) is regrouped so that every 8192-byte packet
// holds ONE byte position of 8192 elements: a packet's adaptive order-0 model then learns one distribution (the exponent
// bytes of bf16 weights, say) instead of a mixture of w of them.  A GROUP is G = w * 8192 bytes = w whole packets, counted
// from the buffer's start.  For a buffer of n bytes:
//     every full group at base B = g * G:     out[B + k * 8192 + i] = in[B + i * w + k]      0 <= i < 8192, 0 <= k < w
//     the tail of r = n mod G bytes at base B = n - r, with e = r div w:
//                                             out[B + k * e + i]    = in[B + i * w + k]      0 <= i < e,    0 <= k < w
//                                             the last r mod w bytes are copied as they are
// That map is SPLIT; MERGE is its inverse.  The output has n bytes; groups are independent of each other.
//
// The same source serves the host (`--host`, host/cpu_compressor.cpp; gpuar_hip_split_planes_host) and the gfx950 kernels
// (gpuar_kernels.hip), which take from here the register transform of one 16-element block: planes_block() regroups
// 16 elements = 4 w dwords with byte permutes alone -- `perm` is v_perm_b32 on the device and perm_bytes() below on the host,
// where tests/test_planes_host.py runs it against the definition.
#ifndef GPUAR_PLANES_H
#define GPUAR_PLANES_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#if defined(__HIPCC__)
#define GPUAR_PLANES_FN __host__ __device__ __forceinline__
#else
#define GPUAR_PLANES_FN inline
#endif

// The most workgroups a launch of the filter, move and sparse pack / unpack kernels gets (gpuar_kernels.hip: kPlaneGridCap, read by
// the launch code alone -- the kernels stride over their items by gridDim.x, whatever it is).
#ifndef GPUAR_PLANE_GRID_CAP                 /* only tests/grid_cap_build.py ever overrides it (to 3: every workgroup strides on, many times) */
#define GPUAR_PLANE_GRID_CAP (1u << 22)
#endif

namespace gpuar {

constexpr uint32_t kPlanePacket = 8192;      // bytes per packet: one plane of a full group
constexpr uint32_t kPlaneBlock = 16;         // elements per register block: one 16-byte piece of every plane

inline bool planes_width_ok(uint64_t w) { return w == 1 || w == 2 || w == 4 || w == 8; }

// v_perm_b32 D, a, b, sel restricted to selector bytes 0 .. 7: byte j of the result is byte sel[j] of the 8 bytes {b (0-3), a (4-7)}
inline uint32_t perm_bytes(uint32_t a, uint32_t b, uint32_t sel) {
    const uint64_t both = static_cast<uint64_t>(a) << 32 | b;
    uint32_t r = 0;
    for (int j = 0; j < 4; ++j) r |= static_cast<uint32_t>((both >> (8 * ((sel >> (8 * j)) & 7u))) & 255u) << (8 * j);
    return r;
}

// the 4 x 4 byte transpose: o[c] = { d[0].byte c, d[1].byte c, d[2].byte c, d[3].byte c }; eight permutes, its own inverse
template <typename Perm>
GPUAR_PLANES_FN void planes_transpose4(uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3, uint32_t (&o)[4], Perm perm) {
    const uint32_t t0 = perm(d1, d0, 0x05010400u), t1 = perm(d1, d0, 0x07030602u);      // {d0.0 d1.0 d0.1 d1.1}, {d0.2 d1.2 d0.3 d1.3}
    const uint32_t t2 = perm(d3, d2, 0x05010400u), t3 = perm(d3, d2, 0x07030602u);
    o[0] = perm(t2, t0, 0x05040100u);
    o[1] = perm(t2, t0, 0x07060302u);
    o[2] = perm(t3, t1, 0x05040100u);
    o[3] = perm(t3, t1, 0x07060302u);
}

// One block of 16 elements.  `mixed`: the elements back to back, dword d = bytes 4 d .. 4 d + 3 of the block; `planes`:
// planes[4 k + m] = dword m of plane k (elements 4 m .. 4 m + 3).  Merge = false: mixed -> planes; true: planes -> mixed.
template <int W, bool Merge, typename Perm>
GPUAR_PLANES_FN void planes_block(const uint32_t (&from)[4 * W], uint32_t (&to)[4 * W], Perm perm) {
    static_assert(W == 1 || W == 2 || W == 4 || W == 8, "element widths of 1, 2, 4 and 8 bytes");
    if constexpr (W == 1) {
#pragma unroll
        for (int d = 0; d < 4 * W; ++d) to[d] = from[d];
    } else if constexpr (W == 2) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if (!Merge) {
                to[m] = perm(from[2 * m + 1], from[2 * m], 0x06040200u);
                to[4 + m] = perm(from[2 * m + 1], from[2 * m], 0x07050301u);
            } else {
                to[2 * m] = perm(from[4 + m], from[m], 0x05010400u);
                to[2 * m + 1] = perm(from[4 + m], from[m], 0x07030602u);
            }
        }
    } else {
        // an element's bytes 4 h .. 4 h + 3 are dword h of its W / 4 dwords: a 4 x 4 transpose of four elements' dwords h
        constexpr int H = W / 4 ? W / 4 : 1;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int h = 0; h < H; ++h) {
                uint32_t o[4];
                if (!Merge) {
                    planes_transpose4(from[H * (4 * m) + h], from[H * (4 * m + 1) + h], from[H * (4 * m + 2) + h], from[H * (4 * m + 3) + h], o, perm);
                    for (int c = 0; c < 4; ++c) to[4 * (4 * h + c) + m] = o[c];
                } else {
                    planes_transpose4(from[4 * (4 * h) + m], from[4 * (4 * h + 1) + m], from[4 * (4 * h + 2) + m], from[4 * (4 * h + 3) + m], o, perm);
                    for (int j = 0; j < 4; ++j) to[H * (4 * m + j) + h] = o[j];
                }
            }
    }
}

// Host: the definition, group by group.  `out` may be `in` (every group is copied before it is written); any other
// overlap is the caller's to avoid.
template <bool Merge>
inline void planes_host(const uint8_t *in, size_t n, uint32_t w, uint8_t *out) {
    if (w == 1) {
        if (out != in && n) memmove(out, in, n);
        return;
    }
    const size_t G = static_cast<size_t>(w) * kPlanePacket;
    std::vector<uint8_t> group(G);
    for (size_t B = 0; B < n; B += G) {
        const size_t r = n - B < G ? n - B : G, e = r / w;          // e = 8192 for a full group
        memcpy(group.data(), in + B, r);
        uint8_t *o = out + B;
        for (size_t k = 0; k < w; ++k)
            for (size_t i = 0; i < e; ++i) {
                if (!Merge) o[k * e + i] = group[i * w + k];
                else o[i * w + k] = group[k * e + i];
            }
        for (size_t i = e * w; i < r; ++i) o[i] = group[i];
    }
}

}  // namespace gpuar

#endif  // GPUAR_PLANES_H
