// estimate.h -- the coded length of a packet from its byte histogram alone.
//
// The codec's model starts every symbol at count 1, adds 1 per occurrence and never rescales inside a packet (the total is
// 256 + i <= 8447 in front of symbol i), so the ideal code length of a packet of n bytes with histogram h is
//     bits = log2((n + 255)! / 255!) - sum over s of log2(h[s]!)
// whatever the order of its bytes.  In integers, one definition for the host and the gfx950 kernels:
//     lg16(k)        = floor(2^16 log2 k)                              1 <= k <= 8447
//     LF[c]          = sum of lg16(k) for k = 2 .. c                   0 <= c <= 8447   (LF[0] = LF[1] = 0)
//     cost16(h, n)   = LF[n + 255] - LF[255] - sum over s of LF[h[s]]
//     est_clen(h, n) = 4 + ((cost16 + 2^19 - 1) >> 19)                 1 <= n <= 8192   (the 4-byte header included)
// A packet is STORED (kept raw, n bytes) iff est_clen >= 4 + n.  Against the reference codec's real clen the estimate is within
// +-1 byte on every packet it was measured on (tests/test_estimate_host.py), so a stored packet is at least
// 3 bytes smaller than its coded form.  tests/test_estimate_host.py pins LF[255], LF[8447] and the sum of the table.
#ifndef GPUAR_ESTIMATE_H
#define GPUAR_ESTIMATE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GPUAR_EST_FN __host__ __device__ constexpr
#else
#define GPUAR_EST_FN constexpr
#endif

namespace gpuar {

constexpr uint32_t kEstPacket = 8192;                  // bytes per packet
constexpr uint32_t kEstCounts = kEstPacket + 256;      // LF's entries: counts 0 .. 8447

// floor(2^16 log2 k): the integer part is k's top bit; the 16 fraction bits come from squaring the mantissa m (Q62, in [1, 2))
// 16 times -- each square doubles the logarithm, and a result in [2, 4) is the next fraction bit (then halved)
GPUAR_EST_FN uint32_t lg16(uint32_t k) {
    uint32_t e = 0;
    while ((k >> e) > 1u) ++e;
    uint64_t m = static_cast<uint64_t>(k) << (62u - e);
    uint32_t r = e;
    for (int i = 0; i < 16; ++i) {
        m = static_cast<uint64_t>((static_cast<unsigned __int128>(m) * m) >> 62);
        r <<= 1;
        if (m >> 63) m >>= 1, r |= 1u;
    }
    return r;
}

struct EstimateTable {
    uint64_t lf[kEstCounts];
    constexpr EstimateTable() : lf{} {
        for (uint32_t c = 2; c < kEstCounts; ++c) lf[c] = lf[c - 1] + lg16(c);
    }
};

// est_clen from the sum of LF[h[s]] over the 256 symbols
GPUAR_EST_FN uint32_t est_clen_from_sum(uint64_t lf_n255, uint64_t lf_255, uint64_t sum_lf_h) {
    return 4u + static_cast<uint32_t>((lf_n255 - lf_255 - sum_lf_h + ((1ull << 19) - 1u)) >> 19);
}

GPUAR_EST_FN bool est_stored(uint32_t est, uint32_t n) { return est >= 4u + n; }

// Host: est[p] for every packet of the n bytes at `in`
inline void estimate_host(const uint8_t *in, size_t n, uint32_t *est) {
    static const EstimateTable tab = EstimateTable();
    for (size_t at = 0, p = 0; at < n; at += kEstPacket, ++p) {
        const uint32_t len = n - at < kEstPacket ? static_cast<uint32_t>(n - at) : kEstPacket;
        uint32_t h[256] = {};
        for (uint32_t i = 0; i < len; ++i) ++h[in[at + i]];
        uint64_t sum = 0;
        for (uint32_t s = 0; s < 256; ++s) sum += tab.lf[h[s]];
        est[p] = est_clen_from_sum(tab.lf[len + 255u], tab.lf[255], sum);
    }
}

}  // namespace gpuar

#endif  // GPUAR_ESTIMATE_H
