// xor_survey.h -- what a buffer would compress to XORed against a base at every byte-plane width, and which of its packets would
// be sparse, from one read of the buffer and one of the base.
//
// For a buffer x and a base b of the same n bytes with P packets, and j = 0 .. 3 for the widths w = 1, 2, 4, 8, BY DEFINITION
//     xest[j][p]  = estimate(split_xor(x, b, w))[p]
//     xscan[j][p] = sparse_scan(split_xor(x, b, w))[p]
// -- estimate.h's est_clen and sparse.h's scan word of packet p of xorbase.h's filtered, split layout; packet p of a split layout
// has the length of packet p of the original.  Nothing of those headers is restated here.  XOR works on single bytes and commutes
// with the regrouping (xorbase.h), so split_xor(x, b, w) = split_planes(x ^ b, w) and xest is survey.h's survey of x ^ b: one set
// of 64 residue histograms of a supergroup serves all four widths, as it does there.
//
// Both values of a packet come from its histogram.  The estimate is est_clen_from_sum over it.  The scan word needs the bin with
// the highest count: a majority byte is that bin, and it is unique, so which of several equal bins a maximum names does not
// matter.  xor_scan_key packs (count, bin) into one word ordered by count, so that a maximum over keys -- the kernel's second
// reduction -- finds the bin, and xor_scan_word turns the highest key into sparse.h's scan word.
//
// The same source serves the host (gpuar_hip_survey_xor_host, `gpuar c --base-auto`) and the gfx950 kernel (survey_xor_kernel in
// gpuar_kernels.hip).  The host twin is the definition, composed supergroup by supergroup from the other headers' host functions:
// a supergroup (8 packets = 65536 bytes) is a multiple of every width's group, so it is filtered and split independently of the
// others, and a buffer's last, short supergroup as a buffer of its own would be (survey_packet's rule).
#ifndef GPUAR_XOR_SURVEY_H
#define GPUAR_XOR_SURVEY_H

#include "sparse.h"
#include "survey.h"
#include "xorbase.h"

namespace gpuar {

static_assert(kSparsePacket == kPlanePacket, "the scan's packets are the planes' packets");

// (count, bin) of one histogram bin as a word that orders by count first; a count is at most 8192
GPUAR_SPARSE_FN uint32_t xor_scan_key(uint32_t count, uint32_t bin) { return count << 8 | bin; }

// sparse.h's scan word of a packet of n bytes from the highest key of its histogram
GPUAR_SPARSE_FN uint32_t xor_scan_word(uint32_t key, uint32_t n) { return sparse_scan_word(key & 255u, key >> 8, n); }

// Host: est[j * stride + p] and scan[j * stride + p] for every width j and packet p of the n bytes at `in` XORed with the n bytes
// at `base`, supergroup by supergroup.  Either output may be null and is then left alone.
inline void xor_survey_host(const uint8_t *in, const uint8_t *base, size_t n, uint32_t *est, uint32_t *scan, size_t stride) {
    std::vector<uint8_t> y(kSurveyBytes), split(kSurveyBytes);
    for (size_t at = 0, first = 0; at < n; at += kSurveyBytes, first += kSurveyPackets) {
        const uint32_t len = n - at < kSurveyBytes ? static_cast<uint32_t>(n - at) : kSurveyBytes;
        xor_host(in + at, base + at, len, y.data());
        if (est) survey_host(y.data(), len, est + first, stride);
        if (!scan) continue;
        for (uint32_t j = 0; j < kSurveyWidths; ++j) {
            planes_host<false>(y.data(), len, 1u << j, split.data());
            for (uint32_t p = 0; p * kPlanePacket < len; ++p) {
                const uint32_t count = len - p * kPlanePacket < kPlanePacket ? len - p * kPlanePacket : kPlanePacket;
                uint32_t h[256] = {}, key = 0;
                for (uint32_t i = 0; i < count; ++i) ++h[split[p * kPlanePacket + i]];
                for (uint32_t s = 0; s < 256u; ++s) key = xor_scan_key(h[s], s) > key ? xor_scan_key(h[s], s) : key;
                scan[j * stride + first + p] = xor_scan_word(key, count);
            }
        }
    }
}

}  // namespace gpuar

#endif  // GPUAR_XOR_SURVEY_H
