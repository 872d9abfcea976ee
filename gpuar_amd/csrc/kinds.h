// kinds.h -- raw and sparse packets in a packet STREAM: every packet keeps its 4-byte header.
//
// batch.compress keeps a packet in the cheapest of three forms (estimate.h, sparse.h) and names the form beside the stream.
// For a .gip file the form goes INTO the stream, so that `off += clen` still walks it, and the trailer (version 6,
// host/packet_index.hpp) says which packet is which.  In integers, one definition for the host and the gfx950 kernels:
//     every packet starts with  u16 clen (these 4 bytes included) | u16 ulen (1 .. 8192, the bytes it holds), little-endian
//     kind 0 (coded)   the bitstream, as ever                                              clen as ever
//     kind 1 (raw)     the packet's ulen bytes                                             clen = 4 + ulen              (<= 8196)
//     kind 2 (sparse)  the record of sparse.h, pads included                               clen = 4 + sparse_len(k)
//     kind(packet)  =  sparse_kind(scan, est, ulen, stored_on) of sparse.h, scan = kSparseNone where sparse is off: exactly
//         what batch.compress applies.  The rule is NOT re-tuned for the 4 header bytes of this form: at the tie a sparse
//         packet in a file may be up to 3 bytes longer than its coded form, and in exchange batch, the GPU pipeline and
//         --host take the same decision -- a file does not depend on which of them wrote it.
//     A packet of any kind fits its 8704-byte slot: raw is 8196 bytes; a packet is sparse only if sparse_len(k) + 1 < est,
//         and est <= kKindsMaxEst = 8281 (8192 bytes that hold each value 32 times; tests/test_kinds_host.py pins it), so
//         a sparse packet is at most 4 + 8276 bytes.
//     a packet of pkt_bytes for n plain bytes is VALID as kind 1 iff  pkt_bytes >= 4, clen == pkt_bytes, ulen == n and
//         clen == 4 + ulen;  as kind 2 iff  pkt_bytes >= 8, clen == pkt_bytes, ulen == n and the record in bytes
//         [4, clen) is valid for n (sparse.h).  Any other kind has no form here (kind 0 is the decoder's).
// In a slot the record sits at slot + 4, 4-byte aligned; in a compacted stream nothing is aligned: whoever takes a packet
// out reads at any byte alignment.
//
// Left out on purpose: counting kinds in the two surveys and in --planes=auto / --delta=auto (they predict coded sizes);
// one read for scan and estimate together; skipping the encode of packets that end up non-coded in the CLI (it is bound by
// the file system).  (Reading version-6 files back into a batch.Compressed is batch.from_gip)
#ifndef GPUAR_KINDS_H
#define GPUAR_KINDS_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "estimate.h"
#include "sparse.h"

#if defined(__HIPCC__)
#define GPUAR_KINDS_FN __host__ __device__ constexpr
#else
#define GPUAR_KINDS_FN constexpr
#endif

namespace gpuar {

constexpr uint32_t kKindsPacket = 8192;                // bytes per packet
constexpr uint32_t kKindsSlot = 8704;                  // bytes per slot
constexpr uint32_t kKindsHeader = 4;                   // u16 clen | u16 ulen
constexpr uint32_t kKindsMaxEst = 8281;                // the largest estimate of any packet (pinned by the host test)

// the header's dword
GPUAR_KINDS_FN uint32_t kinds_header(uint32_t clen, uint32_t ulen) { return clen | (ulen << 16); }

// a non-coded packet's length: k is the sparse packet's exception count
GPUAR_KINDS_FN uint32_t kinds_raw_clen(uint32_t ulen) { return kKindsHeader + ulen; }
GPUAR_KINDS_FN uint32_t kinds_sparse_clen(uint32_t k) { return kKindsHeader + sparse_len(k); }

// what the header of a non-coded packet must say: pkt_bytes is what the stream gives the packet (offsets[p + 1] - offsets[p]),
// n the bytes the packet has in the output
GPUAR_KINDS_FN bool kinds_header_ok(uint32_t header, uint64_t pkt_bytes, uint32_t n) {
    return pkt_bytes >= kKindsHeader && (header & 0xFFFFu) == pkt_bytes && (header >> 16) == n && n >= 1u && n <= kKindsPacket;
}
GPUAR_KINDS_FN bool kinds_raw_ok(uint32_t header, uint64_t pkt_bytes, uint32_t n) {
    return kinds_header_ok(header, pkt_bytes, n) && (header & 0xFFFFu) == kinds_raw_clen(n);
}

// Host: packet `in[0 .. n)` (1 .. 8192 bytes) in its stream form.  Returns the kind; for kSparseCoded nothing is written and
// *clen = 0 (the encoder's packet stands), else pkt[0 .. *clen) is the packet.  `room` too small for it: returns ~0u, nothing written.
inline uint32_t kinds_store_packet(const uint8_t *in, uint32_t n, bool stored_on, bool sparse_on, uint8_t *pkt, size_t room, uint32_t *clen) {
    uint32_t est = 0;
    estimate_host(in, n, &est);
    const uint32_t scan = sparse_on ? sparse_scan_packet(in, n) : kSparseNone;
    const uint32_t kind = sparse_kind(scan, est, n, stored_on);
    *clen = 0;
    if (kind == kSparseCoded) return kind;
    const uint32_t len = kind == kSparseRaw ? kinds_raw_clen(n) : kinds_sparse_clen(scan >> 8);
    if (len > room) return ~0u;
    pkt[0] = static_cast<uint8_t>(len), pkt[1] = static_cast<uint8_t>(len >> 8), pkt[2] = static_cast<uint8_t>(n), pkt[3] = static_cast<uint8_t>(n >> 8);
    if (kind == kSparseRaw) {
        memcpy(pkt + kKindsHeader, in, n);
    } else {
        size_t rec_len = 0;
        if (!sparse_pack_host(in, n, pkt + kKindsHeader, len - kKindsHeader, &rec_len) || rec_len != len - kKindsHeader) return ~0u;
    }
    *clen = len;
    return kind;
}

// Host: the n bytes (1 .. 8192) of the raw or sparse packet pkt[0 .. pkt_bytes) into out; false for a packet that is not valid
// (a raw packet's out is then left as it was, a sparse packet's out[0 .. n) is unspecified; nothing else is written and nothing
// is read beyond pkt_bytes) and for any kind but kSparseRaw and kSparseSparse
inline bool kinds_expand_packet(const uint8_t *pkt, size_t pkt_bytes, uint32_t kind, uint8_t *out, uint32_t n) {
    if ((kind != kSparseRaw && kind != kSparseSparse) || pkt_bytes < kKindsHeader) return false;
    const uint32_t header = pkt[0] | static_cast<uint32_t>(pkt[1]) << 8 | static_cast<uint32_t>(pkt[2]) << 16 | static_cast<uint32_t>(pkt[3]) << 24;
    if (kind == kSparseRaw) {
        if (!kinds_raw_ok(header, pkt_bytes, n)) return false;
        memcpy(out, pkt + kKindsHeader, n);
        return true;
    }
    if (!kinds_header_ok(header, pkt_bytes, n)) return false;
    return sparse_unpack_host(pkt + kKindsHeader, pkt_bytes - kKindsHeader, out, n);
}

}  // namespace gpuar

#endif  // GPUAR_KINDS_H
