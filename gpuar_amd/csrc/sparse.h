// sparse.h -- a packet that is one byte value almost everywhere, kept as that byte and a list of exceptions.
//
// The codec's model starts every symbol at count 1, so a packet of 8192 equal bytes cannot code below log2 C(8447, 255) bits:
// 210 bytes by estimate.h.  Such packets are what the XOR-base filter makes of everything that did not change.  In integers,
// one definition for the host and the gfx950 kernels:
//     scan(packet of n bytes, 1 <= n <= 8192)  =  (k << 8) | f     if some byte value f has 2 count(f) > n  (f is then unique),
//                                                                  with k = n - count(f), the number of exceptions
//                                              =  kSparseNone      otherwise
//     record, little-endian, at a 4-byte-aligned address:
//         u8 fill | u8 0 | u16 k | u16 pos[k] | u8 val[k] | zero bytes up to a multiple of 4
//         pos strictly ascending and < n, val[i] the byte at pos[i] and != fill;  sparse_len(k) = (4 + 3 k + 3) & ~3 bytes,
//         the pad bytes written: a packet's record is one defined byte string
//     a record of rec_bytes for a packet of n bytes is VALID iff  rec_bytes >= 4, byte 1 is 0, 2 k < n, sparse_len(k) <= rec_bytes,
//         the positions are strictly ascending and < n, and no val[i] == fill
//     kind(scan, est, n, stored_on)  =  2 (sparse)  iff  s + 1 < est and (!raw_ok or s < n)
//                                       1 (raw)     else iff raw_ok
//                                       0 (coded)   else
//         with s = sparse_len(scan >> 8) (infinite for kSparseNone), est the packet's estimate (estimate.h) and
//         raw_ok = stored_on and est_stored(est, n).  The + 1 is the estimate's resolution: a sparse packet is smaller than its
//         real coded form, not only than the estimate.  A tie with raw goes to raw.
#ifndef GPUAR_SPARSE_H
#define GPUAR_SPARSE_H

#include <stddef.h>
#include <stdint.h>

#include "estimate.h"

#if defined(__HIPCC__)
#define GPUAR_SPARSE_FN __host__ __device__ constexpr
#else
#define GPUAR_SPARSE_FN constexpr
#endif

namespace gpuar {

constexpr uint32_t kSparsePacket = 8192;               // bytes per packet
constexpr uint32_t kSparseNone = 0xFFFFFFFFu;          // scan: no majority byte

constexpr uint32_t kSparseCoded = 0, kSparseRaw = 1, kSparseSparse = 2;      // kind

GPUAR_SPARSE_FN uint32_t sparse_len(uint32_t k) { return (4u + 3u * k + 3u) & ~3u; }

// scan from the candidate byte and the number of the packet's n bytes that equal it
GPUAR_SPARSE_FN uint32_t sparse_scan_word(uint32_t fill, uint32_t count, uint32_t n) {
    return 2u * count > n ? ((n - count) << 8) | fill : kSparseNone;
}

// the record's first dword: fill | 0 << 8 | k << 16
GPUAR_SPARSE_FN uint32_t sparse_head(uint32_t fill, uint32_t k) { return fill | (k << 16); }

// what of a record's validity its first dword says (the positions and values are the caller's to walk)
GPUAR_SPARSE_FN bool sparse_head_ok(uint32_t head, uint64_t rec_bytes, uint32_t n) {
    const uint32_t k = head >> 16;
    return ((head >> 8) & 255u) == 0u && 2u * k < n && sparse_len(k) <= rec_bytes;
}

GPUAR_SPARSE_FN uint32_t sparse_kind(uint32_t scan, uint32_t est, uint32_t n, bool stored_on) {
    const bool raw_ok = stored_on && est_stored(est, n);
    if (scan != kSparseNone) {
        const uint64_t s = (4u + 3ull * (scan >> 8) + 3u) & ~3ull;      // (sparse_len in 64 bits: any scan word is taken)
        if (s + 1u < est && (!raw_ok || s < n)) return kSparseSparse;
    }
    return raw_ok ? kSparseRaw : kSparseCoded;
}

// Host: scan of the n bytes (1 .. 8192) of one packet
inline uint32_t sparse_scan_packet(const uint8_t *in, uint32_t n) {
    uint32_t h[256] = {};
    for (uint32_t i = 0; i < n; ++i) ++h[in[i]];
    for (uint32_t f = 0; f < 256; ++f)
        if (2u * h[f] > n) return sparse_scan_word(f, h[f], n);
    return kSparseNone;
}

// Host: scan[p] for every packet of the n bytes at `in`
inline void sparse_scan_host(const uint8_t *in, size_t n, uint32_t *scan) {
    for (size_t at = 0, p = 0; at < n; at += kSparsePacket, ++p)
        scan[p] = sparse_scan_packet(in + at, n - at < kSparsePacket ? static_cast<uint32_t>(n - at) : kSparsePacket);
}

// Host: the record of a packet of n bytes (1 .. 8192) into rec[0 .. rec_room); false (nothing written) when the packet has no
// majority byte or the record does not fit.  *rec_len = sparse_len(k).
inline bool sparse_pack_host(const uint8_t *in, uint32_t n, uint8_t *rec, size_t rec_room, size_t *rec_len) {
    if (n == 0u || n > kSparsePacket) return false;
    const uint32_t scan = sparse_scan_packet(in, n);
    if (scan == kSparseNone) return false;
    const uint32_t fill = scan & 255u, k = scan >> 8, len = sparse_len(k);
    if (len > rec_room) return false;
    rec[0] = static_cast<uint8_t>(fill), rec[1] = 0, rec[2] = static_cast<uint8_t>(k), rec[3] = static_cast<uint8_t>(k >> 8);
    uint8_t *pos = rec + 4, *val = rec + 4 + 2u * k;
    for (uint32_t i = 0, slot = 0; i < n; ++i) {
        if (in[i] == fill) continue;
        pos[2u * slot] = static_cast<uint8_t>(i), pos[2u * slot + 1u] = static_cast<uint8_t>(i >> 8);
        val[slot++] = in[i];
    }
    for (uint32_t at = 4u + 3u * k; at < len; ++at) rec[at] = 0;
    *rec_len = len;
    return true;
}

// Host: the packet of n bytes (1 .. 8192) from the record in rec[0 .. rec_bytes); false for a record that is not valid (out[0 .. n)
// is then unspecified; nothing else is written, and nothing is read beyond rec_bytes)
inline bool sparse_unpack_host(const uint8_t *rec, size_t rec_bytes, uint8_t *out, uint32_t n) {
    if (n == 0u || n > kSparsePacket || rec_bytes < 4u) return false;
    const uint32_t head = rec[0] | static_cast<uint32_t>(rec[1]) << 8 | static_cast<uint32_t>(rec[2]) << 16 | static_cast<uint32_t>(rec[3]) << 24;
    if (!sparse_head_ok(head, rec_bytes, n)) return false;
    const uint32_t fill = head & 255u, k = head >> 16;
    const uint8_t *pos = rec + 4, *val = rec + 4 + 2u * k;
    for (uint32_t i = 0; i < n; ++i) out[i] = static_cast<uint8_t>(fill);
    for (uint32_t i = 0, behind = 0; i < k; ++i) {          // behind: the lowest position entry i may have
        const uint32_t at = pos[2u * i] | static_cast<uint32_t>(pos[2u * i + 1u]) << 8;
        if (at < behind || at >= n || val[i] == fill) return false;
        out[at] = val[i];
        behind = at + 1u;
    }
    return true;
}

}  // namespace gpuar

#endif  // GPUAR_SPARSE_H
