// survey.h -- what a buffer would compress to at every byte-plane width, from one read of its bytes.
//
// For a buffer of n bytes with P packets, survey[j][p] (j = 0 .. 3 for the widths w = 1, 2, 4, 8) is BY DEFINITION
//     estimate(split_planes(buffer, w))[p]
// -- estimate.h's est_clen of packet p of planes.h's split layout.  Nothing of either is restated here: the estimate is
// est_clen_from_sum over estimate.h's LF table, and the layout is planes.h's map, of which this header keeps only
// "which packet does input byte o land in" (survey_packet).
//
// The split is never made.  A SUPERGROUP is 8 packets = 65536 bytes, a multiple of every width's group (w * 8192), so a
// buffer's supergroups are split independently of each other at every width.  Cut a full supergroup into 8 EIGHTHS e
// (8192 bytes each) and 8 RESIDUES r = byte offset mod 8: 64 base histograms h[e][r] of 1024 bytes each.  The byte at offset
// o goes, at width w, to plane o mod w of group (o div 8192) div w, so the histogram of every packet of every layout is a sum
// of base histograms:
//     w = 1   packet e                              sum over r of h[e][r]
//     w = 2   packet 2 g + k   (k = 0, 1)           sum over e in {2 g, 2 g + 1}, r = k mod 2 of h[e][r]
//     w = 4   packet 4 g + k   (k = 0 .. 3)         sum over e in {4 g .. 4 g + 3}, r = k mod 4 of h[e][r]
//     w = 8   packet k         (k = 0 .. 7)         sum over e of h[e][k]
// A buffer's last supergroup may be short (1 .. 65535 bytes): it splits exactly as a buffer of its own would, by the tail
// rule of planes.h, and its bytes are counted one by one into the packet they land in (survey_packet).
//
// choose_width picks from the four totals.  The same source serves the host (gpuar_hip_survey_planes_host, `gpuar c
// --planes=auto`) and the gfx950 kernel (survey_planes_kernel in gpuar_kernels.hip), which has survey_host's structure.
#ifndef GPUAR_SURVEY_H
#define GPUAR_SURVEY_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "estimate.h"
#include "planes.h"

#if defined(__HIPCC__)
#define GPUAR_SURVEY_FN __host__ __device__ __forceinline__
#else
#define GPUAR_SURVEY_FN inline
#endif

namespace gpuar {

constexpr uint32_t kSurveyWidths = 4;                                   // w = 1 << j
constexpr uint32_t kSurveyPackets = 8;                                  // packets per supergroup
constexpr uint32_t kSurveyBytes = kSurveyPackets * kPlanePacket;        // 65536
static_assert(kEstPacket == kPlanePacket, "the estimate's packets are the planes' packets");

// The packet, counted from the buffer's start, that byte o of a buffer of n bytes lands in when the buffer is split into planes
// of width w = 1 << log_w (planes.h: full groups, then the tail of n mod G bytes with e = that div w whole elements, the last
// bytes in place).  The kernel calls it with a short supergroup as the buffer (n < 65536).
GPUAR_SURVEY_FN uint32_t survey_packet(uint32_t o, uint32_t n, uint32_t log_w) {
    const uint32_t w = 1u << log_w, G = w * kPlanePacket;
    const uint32_t B = o & ~(G - 1u), k = o & (w - 1u);
    if (n - B >= G) return (B + k * kPlanePacket + ((o - B) >> log_w)) / kPlanePacket;      // a full group: plane k of it
    const uint32_t e = (n - B) >> log_w, t = o - B;
    if (t >= e << log_w) return o / kPlanePacket;                                           // the last (n mod G) mod w bytes
    return (B + k * e + (t >> log_w)) / kPlanePacket;
}

// The smallest width whose predicted total is within one byte per packet of the best one: the estimate's own resolution is
// +-1 byte a packet, and on data of element width w every multiple of w ties within it.
GPUAR_EST_FN uint32_t choose_width(const uint64_t total[4], uint64_t n_packets) {
    uint64_t best = total[0];
    for (uint32_t j = 1; j < kSurveyWidths; ++j) best = total[j] < best ? total[j] : best;
    for (uint32_t j = 0; j < kSurveyWidths - 1u; ++j)
        if (total[j] <= best + n_packets) return 1u << j;
    return 1u << (kSurveyWidths - 1u);
}

// Host: est[j * stride + p] for every width j and packet p of the n bytes at `in`, supergroup by supergroup
inline void survey_host(const uint8_t *in, size_t n, uint32_t *est, size_t stride) {
    static const EstimateTable tab = EstimateTable();
    std::vector<uint32_t> base(64u * 256u), hist(kSurveyWidths * kSurveyPackets * 256u);
    for (size_t at = 0, first = 0; at < n; at += kSurveyBytes, first += kSurveyPackets) {
        const uint32_t len = n - at < kSurveyBytes ? static_cast<uint32_t>(n - at) : kSurveyBytes;
        const uint8_t *sg = in + at;
        hist.assign(hist.size(), 0u);
        auto packet_hist = [&](uint32_t j, uint32_t p) { return hist.data() + (j * kSurveyPackets + p) * 256u; };
        if (len == kSurveyBytes) {
            base.assign(base.size(), 0u);
            for (uint32_t o = 0; o < kSurveyBytes; ++o) ++base[((o / kPlanePacket) * 8u + (o & 7u)) * 256u + sg[o]];
            for (uint32_t j = 0; j < kSurveyWidths; ++j) {
                const uint32_t w = 1u << j;
                for (uint32_t e = 0; e < 8u; ++e)
                    for (uint32_t r = 0; r < 8u; ++r) {
                        uint32_t *to = packet_hist(j, (e & ~(w - 1u)) + (r & (w - 1u)));      // group e div w, plane r mod w
                        const uint32_t *from = base.data() + (e * 8u + r) * 256u;
                        for (uint32_t s = 0; s < 256u; ++s) to[s] += from[s];
                    }
            }
        } else {
            for (uint32_t o = 0; o < len; ++o)
                for (uint32_t j = 0; j < kSurveyWidths; ++j) ++packet_hist(j, survey_packet(o, len, j))[sg[o]];
        }
        for (uint32_t p = 0; p * kPlanePacket < len; ++p) {
            const uint32_t count = len - p * kPlanePacket < kPlanePacket ? len - p * kPlanePacket : kPlanePacket;
            for (uint32_t j = 0; j < kSurveyWidths; ++j) {
                const uint32_t *h = packet_hist(j, p);
                uint64_t sum = 0;
                for (uint32_t s = 0; s < 256u; ++s) sum += tab.lf[h[s]];
                est[j * stride + first + p] = est_clen_from_sum(tab.lf[count + 255u], tab.lf[255], sum);
            }
        }
    }
}

}  // namespace gpuar

#endif  // GPUAR_SURVEY_H
