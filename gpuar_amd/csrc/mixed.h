// mixed.h -- width, delta and base chosen per supergroup of a buffer instead of once per buffer.
//
// A SUPERGROUP is survey.h's: 8 packets = 65536 bytes counted from the buffer's start, a multiple of every width's group, so it is
// filtered and split independently of the others at every width, and a buffer's last, short supergroup as a buffer of its own would
// be.  Supergroup s of a buffer of n bytes therefore carries a MODE byte m of its own:
//     bits 0-1   log2(w), w = 1, 2, 4, 8              bit 2   delta (delta.h)              bit 3   base (xorbase.h)
// Delta and base exclude each other: the modes are 0 .. 11, and 12 .. 15 and everything from 16 on are invalid.  A buffer has
// mode_count(n) = ceil(n / 65536) of them.  With span(s) = [65536 s, min(n, 65536 (s + 1))), BY DEFINITION
//     split_mixed(x, b, modes)[span(s)] = split_planes(x[span(s)], w)                     m = log2(w)
//                                         split_delta(x[span(s)], w)                      m = 4 + log2(w)
//                                         split_xor(x[span(s)], b[span(s)], w)            m = 8 + log2(w)
// and merge_mixed is its inverse.  Nothing of those headers is restated here.  Only a buffer's last supergroup can have a tail:
// its n mod (w * 8192) bytes at the width of its mode.
//
// choose_mode picks a supergroup's mode from the totals of the three surveys (survey.h, delta_survey.h, xor_survey.h) over the
// supergroup's 1 .. 8 packets, by the rules the whole-buffer choices follow: choose_filter between planes and delta, then the base
// at its own best width iff that is predicted to win by more than the estimate's resolution of one byte per packet (a tie goes to
// no base).  Every candidate's whole-buffer total is the sum of its supergroups' totals, and a supergroup's chosen total is at
// most its lowest candidate's plus two such margins, so
//     sum of the chosen totals  <=  the smallest whole-buffer total over all candidates offered  +  2 * n_packets.
//
// The same source serves the host (gpuar_hip_split_mixed_host, gpuar_hip_choose_modes_host) and the gfx950 kernels
// (split_mixed_kernel, merge_mixed_kernel, mixed_tail_kernel, choose_modes_kernel in gpuar_kernels.hip).
#ifndef GPUAR_MIXED_H
#define GPUAR_MIXED_H

#include "delta_survey.h"
#include "xor_survey.h"

namespace gpuar {

constexpr uint32_t kMixedModes = 12;                                    // the valid modes are 0 .. 11
constexpr uint32_t kMixedPlanes = 0, kMixedDelta = 1, kMixedBase = 2;   // a mode's kind: m >> 2

GPUAR_EST_FN bool mixed_mode_ok(uint32_t m) { return m < kMixedModes; }
GPUAR_EST_FN uint32_t mixed_width(uint32_t m) { return 1u << (m & 3u); }
GPUAR_EST_FN uint32_t mixed_kind(uint32_t m) { return m >> 2; }
GPUAR_EST_FN uint32_t mixed_mode(uint32_t width, uint32_t kind) { return survey_row(width) | kind << 2; }

GPUAR_EST_FN uint64_t mode_count(uint64_t n_bytes) { return n_bytes / kSurveyBytes + (n_bytes % kSurveyBytes ? 1u : 0u); }

// a supergroup's mode and its predicted total
struct ModeChoice {
    uint32_t mode;
    uint64_t total;
};
// The four totals of one survey, by value: the kernel keeps them in registers, and the total of the row of `width` is a chain of
// selects over them.
struct SurveyTotals {
    uint64_t w1, w2, w4, w8;
};
GPUAR_EST_FN uint64_t mixed_total(SurveyTotals t, uint32_t width) { return width == 1u ? t.w1 : width == 2u ? t.w2 : width == 4u ? t.w4 : t.w8; }

// A supergroup's choice from the four totals of each survey over its `packets` packets; with_delta and with_base: that filter is
// offered.  The totals are read by selects (mixed_total), never through a pointer that is chosen at run time: the kernel has no
// scratch memory.
GPUAR_EST_FN ModeChoice choose_mode_of(SurveyTotals plain, bool with_delta, SurveyTotals delta, bool with_base, SurveyTotals xored,
                                       uint64_t packets) {
    const uint64_t p4[4] = {plain.w1, plain.w2, plain.w4, plain.w8}, d4[4] = {delta.w1, delta.w2, delta.w4, delta.w8};
    const uint64_t x4[4] = {xored.w1, xored.w2, xored.w4, xored.w8};
    const FilterChoice c = with_delta ? choose_filter(p4, d4, packets) : FilterChoice{choose_width(p4, packets), false};
    ModeChoice r = {mixed_mode(c.width, c.filter ? kMixedDelta : kMixedPlanes), 0u};
    const uint64_t with = mixed_total(delta, c.width), without = mixed_total(plain, c.width);
    r.total = c.filter ? with : without;
    if (with_base && packets != 0u) {
        const uint32_t wx = choose_width(x4, packets);
        if (mixed_total(xored, wx) + packets <= r.total) r = ModeChoice{mixed_mode(wx, kMixedBase), mixed_total(xored, wx)};
    }
    return r;
}
// the same from arrays; `delta` and `xored` may be null: that filter is not offered
GPUAR_EST_FN ModeChoice choose_mode(const uint64_t plain[4], const uint64_t *delta, const uint64_t *xored, uint64_t packets) {
    const SurveyTotals none = {0u, 0u, 0u, 0u}, p = {plain[0], plain[1], plain[2], plain[3]};
    const SurveyTotals d = delta ? SurveyTotals{delta[0], delta[1], delta[2], delta[3]} : none;
    const SurveyTotals x = xored ? SurveyTotals{xored[0], xored[1], xored[2], xored[3]} : none;
    return choose_mode_of(p, delta != nullptr, d, xored != nullptr, x, packets);
}

// the four totals of a survey's rows (null: zeros) over the packets first .. first + count - 1
GPUAR_EST_FN SurveyTotals survey_sums(const uint32_t *rows, uint64_t stride, uint64_t first, uint64_t count) {
    SurveyTotals t = {0u, 0u, 0u, 0u};
    for (uint64_t p = 0; rows && p < count; ++p) {
        t.w1 += rows[first + p], t.w2 += rows[stride + first + p];
        t.w4 += rows[2u * stride + first + p], t.w8 += rows[3u * stride + first + p];
    }
    return t;
}

// choose_mode for supergroup s of a buffer whose survey rows stand at plain / delta / xored (row j at + j * stride, entry p of a
// row the buffer's packet p; delta and xored may be null), the buffer having n_packets packets: the rows summed over the
// supergroup's packets.  The kernel's lane and the host's loop are this function.
GPUAR_EST_FN ModeChoice choose_supergroup_mode(const uint32_t *plain, const uint32_t *delta, const uint32_t *xored, uint64_t stride, uint64_t s,
                                               uint64_t n_packets) {
    const uint64_t first = s * kSurveyPackets, count = n_packets - first < kSurveyPackets ? n_packets - first : kSurveyPackets;
    return choose_mode_of(survey_sums(plain, stride, first, count), delta != nullptr, survey_sums(delta, stride, first, count), xored != nullptr,
                          survey_sums(xored, stride, first, count), count);
}

// Host: the mode (and, where `totals` is not null, the predicted total) of every supergroup of a buffer of n_bytes bytes
inline void choose_modes_host(const uint32_t *plain, const uint32_t *delta, const uint32_t *xored, size_t stride, size_t n_bytes, uint8_t *modes,
                              uint32_t *totals) {
    const uint64_t n_packets = (n_bytes + kPlanePacket - 1u) / kPlanePacket;
    for (uint64_t s = 0; s < mode_count(n_bytes); ++s) {
        const ModeChoice c = choose_supergroup_mode(plain, delta, xored, stride, s, n_packets);
        modes[s] = static_cast<uint8_t>(c.mode);
        if (totals) totals[s] = static_cast<uint32_t>(c.total);
    }
}

// every mode of a buffer of n_bytes bytes is valid, and none asks for a base where there is none
inline bool mixed_modes_ok(const uint8_t *modes, size_t n_bytes, bool based) {
    for (uint64_t s = 0; s < mode_count(n_bytes); ++s)
        if (!mixed_mode_ok(modes[s]) || (mixed_kind(modes[s]) == kMixedBase && !based)) return false;
    return true;
}

// Host: the definition, supergroup by supergroup, composed from the other headers' host functions.  `out` may be `in`; `base`
// lies apart from `out` and may be null where no mode asks for it.  The modes are valid (mixed_modes_ok).
template <bool Merge>
inline void mixed_host(const uint8_t *in, const uint8_t *base, size_t n, const uint8_t *modes, uint8_t *out) {
    for (size_t at = 0, s = 0; at < n; at += kSurveyBytes, ++s) {
        const size_t len = n - at < kSurveyBytes ? n - at : kSurveyBytes;
        const uint32_t w = mixed_width(modes[s]), kind = mixed_kind(modes[s]);
        if (kind == kMixedBase) {
            if (Merge) merge_xor_host(in + at, base + at, len, w, out + at);
            else split_xor_host(in + at, base + at, len, w, out + at);
        } else if (kind == kMixedDelta) {
            if (Merge) merge_delta_host(in + at, len, w, out + at);
            else split_delta_host(in + at, len, w, out + at);
        } else {
            planes_host<Merge>(in + at, len, w, out + at);
        }
    }
}
inline void split_mixed_host(const uint8_t *in, const uint8_t *base, size_t n, const uint8_t *modes, uint8_t *out) {
    mixed_host<false>(in, base, n, modes, out);
}
inline void merge_mixed_host(const uint8_t *in, const uint8_t *base, size_t n, const uint8_t *modes, uint8_t *out) {
    mixed_host<true>(in, base, n, modes, out);
}

}  // namespace gpuar

#endif  // GPUAR_MIXED_H
