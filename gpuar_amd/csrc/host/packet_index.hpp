// packet_index.hpp -- optional packet-offset index behind the packet stream of a .gip file
// (SURVEY.md section 8(f) row 2).
//
// The reference finds packet boundaries by walking `off += clen` through the file, one packet
// header at a time (/root/reference/src/gpu_compressor.cpp:299-312, src/cpu_compressor.cpp:47-56).
// With the index a reader cuts the stream into per-device ranges, reads each range with one bulk
// read and gets the packet offsets from a prefix sum.
//
// The index is a TRAILER: it follows the last packet and is not counted in the header's
// compressed-size field, which keeps meaning "20 + bytes of packets" (src/cpu_compressor.cpp:136,162).
// The reference stops at that size, so a file with an index still decodes there, and bytes 0..size of
// the file are exactly what is written without `--index`.  Layout, little-endian:
//     "GIPX"  u32 version = 1  u64 n_packets  |  u16 clen[n_packets]  |  zero pad to 8  |
//     u64 trailer_bytes (everything from "GIPX" to the end)  "XPIG"
// Version 2 (`--checksum`) adds the CRC-32 (crc32.h: zlib.crc32) of every packet's uncompressed bytes:
//     "GIPX"  u32 version = 2  u64 n_packets  |  u16 clen[n_packets]  |  zero pad to 4  |  u32 crc32[n_packets]  |
//     zero pad to 8  |  u64 trailer_bytes  "XPIG"
// (pads counted from "GIPX").  A reader that knows only version 1 sees version 2 and walks the packet headers.
// Version 3 (`--planes=W`, W = 2, 4 or 8: the input was split into byte planes before it was coded, ../planes.h) tells the reader
// the element width, without which it would hand back the split bytes; the CRCs -- of the ORIGINAL bytes -- are optional in it:
//     "GIPX"  u32 version = 3  u64 n_packets  |  u32 elem_bytes  |  u32 flags (bit 0: crc32[] present, others 0)  |
//     u16 clen[n_packets]  |  zero pad to 4  |  u32 crc32[n_packets] if flagged  |  zero pad to 8  |  u64 trailer_bytes  "XPIG"
// A trailer that says it is version 3 and cannot be used is an ERROR for the reader, not a trailer to ignore.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

namespace gip {

class PacketIndex {
  public:
    static constexpr uint32_t kVersion = 1;
    static constexpr uint32_t kVersionChecksums = 2;

    // appends the trailer at the current position of `f`: version 1, or version 2 when `crcs` (one per packet) is given
    static void write(FILE *f, const std::vector<uint16_t> &clens, const std::vector<uint32_t> *crcs = nullptr) {
        const uint64_t n = clens.size();
        const uint64_t body = bodyBytes(n, crcs != nullptr), total = 16 + body + 12;
        uint8_t head[16] = {'G', 'I', 'P', 'X'};
        put32(head + 4, crcs ? kVersionChecksums : kVersion);
        put64(head + 8, n);
        uint8_t tail[12];
        put64(tail, total);
        std::memcpy(tail + 8, "XPIG", 4);
        std::vector<uint8_t> le(body, 0);             // the zero pads included
        for (uint64_t i = 0; i < n; ++i) le[2 * i] = static_cast<uint8_t>(clens[i]), le[2 * i + 1] = static_cast<uint8_t>(clens[i] >> 8);
        if (crcs) {
            if (crcs->size() != n) throw std::runtime_error("Write packet index failed");
            const uint64_t at = crcAt(n);
            for (uint64_t i = 0; i < n; ++i) put32(le.data() + at + 4 * i, (*crcs)[i]);
        }
        if (std::fwrite(head, sizeof head, 1, f) != 1 || (body && std::fwrite(le.data(), body, 1, f) != 1) ||
            std::fwrite(tail, sizeof tail, 1, f) != 1)
            throw std::runtime_error("Write packet index failed");
    }

    static constexpr uint32_t kVersionPlanes = 3;

    // appends the version-3 trailer: the packets hold byte planes of elements `elem_bytes` wide; `crcs`: as for write()
    static void writePlanes(FILE *f, const std::vector<uint16_t> &clens, uint32_t elem_bytes, const std::vector<uint32_t> *crcs = nullptr) {
        const uint64_t n = clens.size();
        if (crcs && crcs->size() != n) throw std::runtime_error("Write packet index failed");
        std::vector<uint8_t> t(planesBytes(n, crcs != nullptr), 0);      // the zero pads included
        std::memcpy(t.data(), "GIPX", 4);
        put32(t.data() + 4, kVersionPlanes);
        put64(t.data() + 8, n);
        put32(t.data() + 16, elem_bytes);
        put32(t.data() + 20, crcs ? 1u : 0u);
        for (uint64_t i = 0; i < n; ++i) t[24 + 2 * i] = static_cast<uint8_t>(clens[i]), t[24 + 2 * i + 1] = static_cast<uint8_t>(clens[i] >> 8);
        if (crcs)
            for (uint64_t i = 0; i < n; ++i) put32(t.data() + planesCrcAt(n) + 4 * i, (*crcs)[i]);
        put64(t.data() + t.size() - 12, t.size());
        std::memcpy(t.data() + t.size() - 4, "XPIG", 4);
        if (std::fwrite(t.data(), t.size(), 1, f) != 1) throw std::runtime_error("Write packet index failed");
    }

    enum class Planes { none, ok, unusable };
    // Looks for a version-3 trailer at stream_end.  none: what is there does not say "GIPX", 3 (the caller goes on to find());
    // ok: `clens`, `elem_bytes` (2, 4 or 8) and, when has_crcs, `crcs` are filled; unusable: it says version 3 but its lengths do
    // not add up, its width is not 2, 4 or 8 or it carries flags this reader does not know -- the caller must refuse the file.
    static Planes findPlanes(FILE *f, uint64_t stream_begin, uint64_t stream_end, uint64_t file_size, std::vector<uint16_t> &clens,
                             std::vector<uint32_t> &crcs, uint32_t &elem_bytes, bool &has_crcs) {
        clens.clear();
        crcs.clear();
        elem_bytes = 1;
        has_crcs = false;
        const long here = std::ftell(f);
        Planes found = Planes::none;
        uint8_t magic[8];
        if (file_size >= stream_end + sizeof magic && std::fseek(f, static_cast<long>(stream_end), SEEK_SET) == 0 &&
            std::fread(magic, sizeof magic, 1, f) == 1 && std::memcmp(magic, "GIPX", 4) == 0 && get32(magic + 4) == kVersionPlanes) {
            found = Planes::unusable;
            const uint64_t room = file_size - stream_end;
            std::vector<uint8_t> t(room);
            if (room >= 24 + 12 && std::fseek(f, static_cast<long>(stream_end), SEEK_SET) == 0 && std::fread(t.data(), room, 1, f) == 1) {
                const uint64_t n = get64(t.data() + 8);
                const uint32_t w = get32(t.data() + 16), flags = get32(t.data() + 20);
                if ((w == 2 || w == 4 || w == 8) && (flags & ~1u) == 0 && n <= room / 2 && planesBytes(n, flags & 1u) == room &&
                    std::memcmp(t.data() + room - 4, "XPIG", 4) == 0 && get64(t.data() + room - 12) == room) {
                    clens.resize(n);
                    uint64_t sum = 0;
                    for (uint64_t i = 0; i < n; ++i) sum += clens[i] = static_cast<uint16_t>(t[24 + 2 * i] | (t[24 + 2 * i + 1] << 8));
                    if (flags & 1u) {
                        crcs.resize(n);
                        for (uint64_t i = 0; i < n; ++i) crcs[i] = get32(t.data() + planesCrcAt(n) + 4 * i);
                    }
                    if (sum == stream_end - stream_begin) {
                        found = Planes::ok;
                        elem_bytes = w;
                        has_crcs = (flags & 1u) != 0;
                    }
                }
            }
        }
        if (found != Planes::ok) clens.clear(), crcs.clear();
        std::fseek(f, here, SEEK_SET);
        return found;
    }

    enum class Found { none, v1, v2, malformed };
    // Like read(), for a reader that also takes version 2: fills `clens` and, for version 2, `crcs`.  `malformed`: a trailer
    // that says it is version 2 ("GIPX", 2 behind the packets) but whose lengths do not add up -- ignored like any bad
    // trailer, but the caller can tell the user that nothing was verified.
    static Found find(FILE *f, uint64_t stream_begin, uint64_t stream_end, uint64_t file_size, std::vector<uint16_t> &clens,
                      std::vector<uint32_t> &crcs) {
        clens.clear();
        crcs.clear();
        if (read(f, stream_begin, stream_end, file_size, clens)) return Found::v1;
        const long here = std::ftell(f);
        Found found = Found::none;
        uint8_t head[16], tail[12];
        if (file_size >= stream_end + sizeof head && std::fseek(f, static_cast<long>(stream_end), SEEK_SET) == 0 &&
            std::fread(head, sizeof head, 1, f) == 1 && std::memcmp(head, "GIPX", 4) == 0 && get32(head + 4) == kVersionChecksums) {
            found = Found::malformed;
            const uint64_t n = get64(head + 8);
            const uint64_t room = file_size - stream_end;
            if (n <= room / 6 && 16 + bodyBytes(n, true) + 12 == room && std::fseek(f, static_cast<long>(file_size - 12), SEEK_SET) == 0 &&
                std::fread(tail, sizeof tail, 1, f) == 1 && std::memcmp(tail + 8, "XPIG", 4) == 0 && get64(tail) == room) {
                std::vector<uint8_t> le(bodyBytes(n, true));
                if (std::fseek(f, static_cast<long>(stream_end + 16), SEEK_SET) == 0 && (le.empty() || std::fread(le.data(), le.size(), 1, f) == 1)) {
                    clens.resize(n);
                    crcs.resize(n);
                    uint64_t sum = 0;
                    for (uint64_t i = 0; i < n; ++i) sum += clens[i] = static_cast<uint16_t>(le[2 * i] | (le[2 * i + 1] << 8));
                    for (uint64_t i = 0; i < n; ++i) crcs[i] = get32(le.data() + crcAt(n) + 4 * i);
                    if (sum == stream_end - stream_begin) found = Found::v2;
                }
            }
        }
        if (found != Found::v2) clens.clear(), crcs.clear();
        std::fseek(f, here, SEEK_SET);
        return found;
    }

    // Looks for a trailer in [stream_end, file_size); on success fills `clens`, restores the file
    // position and returns true.  A trailer whose lengths do not add up to the stream is rejected.
    static bool read(FILE *f, uint64_t stream_begin, uint64_t stream_end, uint64_t file_size, std::vector<uint16_t> &clens) {
        clens.clear();
        if (file_size < stream_end + 28) return false;
        const long here = std::ftell(f);
        bool ok = false;
        uint8_t tail[12], head[16];
        if (std::fseek(f, static_cast<long>(file_size - 12), SEEK_SET) == 0 && std::fread(tail, sizeof tail, 1, f) == 1 &&
            std::memcmp(tail + 8, "XPIG", 4) == 0 && get64(tail) == file_size - stream_end &&
            std::fseek(f, static_cast<long>(stream_end), SEEK_SET) == 0 && std::fread(head, sizeof head, 1, f) == 1 &&
            std::memcmp(head, "GIPX", 4) == 0 && get32(head + 4) == kVersion) {
            const uint64_t n = get64(head + 8), body = 2 * n, pad = (8 - body % 8) % 8;
            if (16 + body + pad + 12 == file_size - stream_end) {
                std::vector<uint8_t> le(body);
                if (!body || std::fread(le.data(), body, 1, f) == 1) {
                    clens.resize(n);
                    uint64_t sum = 0;
                    for (uint64_t i = 0; i < n; ++i) sum += clens[i] = static_cast<uint16_t>(le[2 * i] | (le[2 * i + 1] << 8));
                    ok = sum == stream_end - stream_begin;
                }
            }
        }
        if (!ok) clens.clear();
        std::fseek(f, here, SEEK_SET);
        return ok;
    }

  private:
    // where the CRCs start inside the body (behind "GIPX" u32 u64), and the body's length: everything between head and tail
    static uint64_t crcAt(uint64_t n) { return 2 * n + (4 - (2 * n) % 4) % 4; }
    static uint64_t bodyBytes(uint64_t n, bool checksums) {
        const uint64_t body = checksums ? crcAt(n) + 4 * n : 2 * n;
        return body + (8 - body % 8) % 8;
    }
    // version 3, offsets from "GIPX": 24 bytes of fixed fields, the lengths, pad to 4, the CRCs when there are any, pad to 8, 12 bytes
    static uint64_t planesCrcAt(uint64_t n) { return (24 + 2 * n + 3) / 4 * 4; }
    static uint64_t planesBytes(uint64_t n, bool checksums) { return (planesCrcAt(n) + (checksums ? 4 * n : 0) + 7) / 8 * 8 + 12; }
    static void put32(uint8_t *p, uint32_t v) { for (int b = 0; b < 4; ++b) p[b] = static_cast<uint8_t>(v >> (8 * b)); }
    static void put64(uint8_t *p, uint64_t v) { for (int b = 0; b < 8; ++b) p[b] = static_cast<uint8_t>(v >> (8 * b)); }
    static uint32_t get32(const uint8_t *p) { uint32_t v = 0; for (int b = 0; b < 4; ++b) v |= static_cast<uint32_t>(p[b]) << (8 * b); return v; }
    static uint64_t get64(const uint8_t *p) { uint64_t v = 0; for (int b = 0; b < 8; ++b) v |= static_cast<uint64_t>(p[b]) << (8 * b); return v; }
};

}  // namespace gip
