// delta_survey.h -- what a buffer would compress to WITH the delta filter at every byte-plane width, from one read of its bytes
// (DESIGN.md 4.11), and the choice between (width, filter) pairs.
//
// For a buffer of n bytes with P packets, dsurvey[j][p] (j = 0 .. 3 for the widths w = 1, 2, 4, 8) is BY DEFINITION
//     estimate(split_delta(buffer, w))[p]
// -- estimate.h's est_clen of packet p of delta.h's filtered, split layout.  Nothing of either is restated here: the estimate is
// est_clen_from_sum over estimate.h's LF table, a byte lands where survey.h's survey_packet says, and which element precedes
// which -- the reset at every group, the tail's whole elements only, its last bytes as they are -- is delta_host's.
//
// Neither the filter's output nor the split is kept.  As in survey.h a SUPERGROUP (8 packets = 65536 bytes) is filtered and
// split independently of the others at every width, and a buffer's last, short supergroup as a buffer of its own would be.  The
// filtered byte at a position differs per width, so every width counts its own filtered bytes; within one width survey.h's
// residue sums hold: in a full supergroup, filtered byte k of an element in eighth e lands in packet (e & ~(w - 1)) + (k mod w).
//
// The same source serves the host (gpuar_hip_survey_delta_host, `gpuar c --delta=auto`) and the gfx950 kernel
// (survey_delta_kernel in gpuar_kernels.hip), which filters in registers with delta.h's delta_block.
#ifndef GPUAR_DELTA_SURVEY_H
#define GPUAR_DELTA_SURVEY_H

#include "delta.h"
#include "survey.h"

namespace gpuar {

constexpr uint32_t kSurveyAllWidths = (1u << kSurveyWidths) - 1u;      // widths_mask: bit j asks for the row of width 1 << j

// (width, filter) from the totals of both surveys: the filter at its best width iff it is predicted to win by more than the
// estimate's resolution of one byte per packet against the best width without it (the rule of batch.compress(delta="auto");
// a tie goes to no filter, and so does a buffer without packets).
struct FilterChoice {
    uint32_t width;
    bool filter;
};
GPUAR_EST_FN uint32_t survey_row(uint32_t width) { return width == 1u ? 0u : width == 2u ? 1u : width == 4u ? 2u : 3u; }
GPUAR_EST_FN FilterChoice choose_filter(const uint64_t plain[4], const uint64_t filtered[4], uint64_t n_packets) {
    const uint32_t wp = choose_width(plain, n_packets), wd = choose_width(filtered, n_packets);
    if (n_packets != 0u && filtered[survey_row(wd)] + n_packets <= plain[survey_row(wp)]) return FilterChoice{wd, true};
    return FilterChoice{wp, false};
}

// Host: est[j * stride + p] for every width j whose bit is set in widths_mask and every packet p of the n bytes at `in`,
// supergroup by supergroup; the other rows are not touched
inline void delta_survey_host(const uint8_t *in, size_t n, uint32_t widths_mask, uint32_t *est, size_t stride) {
    static const EstimateTable tab = EstimateTable();
    std::vector<uint8_t> filtered(kSurveyBytes);
    std::vector<uint32_t> hist(kSurveyPackets * 256u);
    for (size_t at = 0, first = 0; at < n; at += kSurveyBytes, first += kSurveyPackets) {
        const uint32_t len = n - at < kSurveyBytes ? static_cast<uint32_t>(n - at) : kSurveyBytes;
        for (uint32_t j = 0; j < kSurveyWidths; ++j) {
            if (!(widths_mask >> j & 1u)) continue;
            const uint32_t w = 1u << j;
            delta_host<false>(in + at, len, w, filtered.data());
            hist.assign(hist.size(), 0u);
            if (len == kSurveyBytes) {
                for (uint32_t o = 0; o < kSurveyBytes; ++o) {
                    const uint32_t e = o / kPlanePacket;
                    ++hist[((e & ~(w - 1u)) + (o & (w - 1u))) * 256u + filtered[o]];          // group e div w, plane o mod w
                }
            } else {
                for (uint32_t o = 0; o < len; ++o) ++hist[survey_packet(o, len, j) * 256u + filtered[o]];
            }
            for (uint32_t p = 0; p * kPlanePacket < len; ++p) {
                const uint32_t count = len - p * kPlanePacket < kPlanePacket ? len - p * kPlanePacket : kPlanePacket;
                uint64_t sum = 0;
                for (uint32_t s = 0; s < 256u; ++s) sum += tab.lf[hist[p * 256u + s]];
                est[j * stride + first + p] = est_clen_from_sum(tab.lf[count + 255u], tab.lf[255], sum);
            }
        }
    }
}

}  // namespace gpuar

#endif  // GPUAR_DELTA_SURVEY_H
