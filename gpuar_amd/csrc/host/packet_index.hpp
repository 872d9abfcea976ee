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
// Version 4 (`--delta`, alone or with `--planes=W`: the elements of every group were replaced by their differences before the
// split, ../delta.h) has version 3's layout; W may be 1 in it, and bit 1 of the flags (delta) must be set:
//     "GIPX"  u32 version = 4  u64 n_packets  |  u32 elem_bytes (1, 2, 4 or 8)  |  u32 flags (bit 0: crc32[] present, bit 1: delta,
//     others 0)  |  u16 clen[n_packets]  |  zero pad to 4  |  u32 crc32[n_packets] if flagged  |  zero pad to 8  |  u64 trailer_bytes  "XPIG"
// It is written only when the filter is on, and one that cannot be used is an error too.
// Version 5 (`--base=FILE`, alone or with `--planes=W`: the input was XORed with a base file of the same length before the split,
// ../xorbase.h) has version 3's layout; W may be 1 in it, bit 2 of the flags (XOR base) must be set and so must bit 0: the CRCs
// -- of the ORIGINAL bytes -- are what tells a reader that it was given the wrong base, so they are mandatory:
//     "GIPX"  u32 version = 5  u64 n_packets  |  u32 elem_bytes (1, 2, 4 or 8)  |  u32 flags = 5 (bit 0: crc32[] present, bit 2: base,
//     others 0)  |  u16 clen[n_packets]  |  zero pad to 4  |  u32 crc32[n_packets]  |  zero pad to 8  |  u64 trailer_bytes  "XPIG"
// It is written only with a base, and one that cannot be used is an error too.
// Version 6 (`--stored=auto` and / or `--sparse=auto`: a packet may be kept raw or sparse instead of coded, ../kinds.h) has version
// 3's layout with one array more, the kind of every packet (0 coded, 1 raw, 2 sparse), and carries what versions 3-5 say in its flags:
//     "GIPX"  u32 version = 6  u64 n_packets  |  u32 elem_bytes (1, 2, 4 or 8)  |  u32 flags (bit 0: crc32[] present, bit 1: delta,
//     bit 2: base -- needs bit 0, excludes bit 1 --, bit 3: kinds, must be set, others 0)  |  u16 clen[n_packets]  |  zero pad to 4  |
//     u32 crc32[n_packets] if flagged  |  u8 kind[n_packets]  |  zero pad to 8  |  u64 trailer_bytes  "XPIG"
// It is written exactly when one of the two options was given, whatever the packets turned out to be, and one that cannot be
// used (a kind above 2 included) is an error too.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

namespace gip {

// what stands behind the packet stream of a .gip file; `version` 0: nothing a reader may use
struct Trailer {
    uint32_t version = 0;
    std::vector<uint16_t> clens;      // of every packet
    std::vector<uint32_t> crcs;       // of every packet's original bytes, when has_crcs
    bool has_crcs = false;
    uint32_t elem_bytes = 1;          // 2, 4 or 8 in version 3, 1 too in versions 4 to 6: the packets hold byte planes of elements this wide
    std::vector<uint8_t> kinds;       // version 6: of every packet, 0 coded, 1 raw, 2 sparse (../kinds.h)
    uint32_t flags = 0;               // versions 3 to 6: as stored

    bool indexed() const { return version != 0; }        // the packet offsets are the prefix sums of `clens`
    bool verify() const { return has_crcs; }             // every decoded packet is checked against `crcs`
    // the decoded bytes are merged back from planes of `elem_bytes` (version 6: only where there is something to merge)
    bool merging() const { return version == 3 || version == 4 || version == 5 || (version == 6 && (elem_bytes > 1 || (flags & 6u) != 0)); }
    bool filtering() const { return version == 4 || (version == 6 && (flags & 2u) != 0); }      // ... and are differences of elements that wide, summed up by the merge
    bool based() const { return version == 5 || (version == 6 && (flags & 4u) != 0); }          // ... and are XORed with the base the reader must be given
    bool mixed() const { return version == 6; }          // `kinds` says which packets are raw or sparse

    // offsets from "GIPX": the fixed fields end and the lengths begin at `fixed`, the CRCs (when there are any) begin at `crcs`,
    // and the trailer is `total` bytes long
    // (version 6: the kinds begin at `kinds`, behind the CRCs)
    struct Layout {
        uint64_t fixed, crcs, kinds, total;
    };
    static Layout layout(uint32_t version, uint64_t n, bool has_crcs) {
        Layout at;
        at.fixed = version >= 3 && version <= 6 ? 24 : 16;
        at.crcs = has_crcs || version == 6 ? (at.fixed + 2 * n + 3) / 4 * 4 : at.fixed + 2 * n;
        at.kinds = at.crcs + (has_crcs ? 4 * n : 0);
        at.total = (at.kinds + (version == 6 ? n : 0) + 7) / 8 * 8 + 12;
        return at;
    }

    // appends the trailer at the current position of `f`: version 5 when the packets were XORed with a base (`crcs` is required), else version 4 when the packets went through the delta filter, else version 3
    // when they hold byte planes of elements `elem_bytes` > 1 wide, else version 2 when `crcs` (one per packet) is given, else version 1
    // `kinds` (one per packet): version 6, which carries all of that in its flags
    static void save(FILE *f, const std::vector<uint16_t> &clens, uint32_t elem_bytes = 1, const std::vector<uint32_t> *crcs = nullptr,
                     bool delta = false, bool base = false, const std::vector<uint8_t> *kinds = nullptr) {
        const uint64_t n = clens.size();
        if ((crcs && crcs->size() != n) || (base && (!crcs || delta)) || (kinds && kinds->size() != n)) throw std::runtime_error("Write packet index failed");
        const uint32_t version = kinds ? 6 : base ? 5 : delta ? 4 : elem_bytes > 1 ? 3 : crcs ? 2 : 1;
        const Layout at = layout(version, n, crcs != nullptr);
        std::vector<uint8_t> t(at.total, 0);      // the zero pads included
        std::memcpy(t.data(), "GIPX", 4);
        put32(t.data() + 4, version);
        put64(t.data() + 8, n);
        if (version >= 3) put32(t.data() + 16, elem_bytes), put32(t.data() + 20, (crcs ? 1u : 0u) | (delta ? 2u : 0u) | (base ? 4u : 0u) | (kinds ? 8u : 0u));
        for (uint64_t i = 0; i < n; ++i) t[at.fixed + 2 * i] = static_cast<uint8_t>(clens[i]), t[at.fixed + 2 * i + 1] = static_cast<uint8_t>(clens[i] >> 8);
        if (crcs)
            for (uint64_t i = 0; i < n; ++i) put32(t.data() + at.crcs + 4 * i, (*crcs)[i]);
        if (kinds && n) std::memcpy(t.data() + at.kinds, kinds->data(), n);
        put64(t.data() + at.total - 12, at.total);
        std::memcpy(t.data() + at.total - 4, "XPIG", 4);
        if (std::fwrite(t.data(), t.size(), 1, f) != 1) throw std::runtime_error("Write packet index failed");
    }

    enum class Status { none, ok, malformed, unusable, unusable_delta, unusable_base, unusable_kinds };
    // Looks for a trailer in [stream_end, file_size) and restores the file position.  ok: `t` is filled.  Otherwise `t` is empty:
    //   unusable   what is there says "GIPX", 3 but its width is not 2, 4 or 8, it carries flags this reader does not know, or its
    //              lengths, its tail or the sum of its clens do not fit: the caller must refuse the file
    //   unusable_delta  the same for "GIPX", 4: a width that is not 1, 2, 4 or 8, the delta flag missing, a flag it does not know
    //   unusable_base   the same for "GIPX", 5: a width that is not 1, 2, 4 or 8, flags other than base + CRCs
    //   unusable_kinds  the same for "GIPX", 6: a width that is not 1, 2, 4 or 8, the kinds flag missing, base without CRCs or with
    //              delta, a flag it does not know, a kind above 2
    //   malformed  it says "GIPX", 2 (in 16 bytes) and does not fit in the same way: ignored like any bad trailer, but the caller
    //              can tell the user that nothing was verified
    //   none       anything else, a version 1 that does not fit and versions this reader does not know included
    static Status load(FILE *f, uint64_t stream_begin, uint64_t stream_end, uint64_t file_size, Trailer &t) {
        t = Trailer();
        const long here = std::ftell(f);
        const uint64_t room = file_size > stream_end ? file_size - stream_end : 0;
        const Status status = [&] {
            uint8_t head[24] = {}, tail[12];
            const size_t have = static_cast<size_t>(room < sizeof head ? room : sizeof head);
            if (have < 8 || std::fseek(f, static_cast<long>(stream_end), SEEK_SET) != 0 || std::fread(head, have, 1, f) != 1 ||
                std::memcmp(head, "GIPX", 4) != 0)
                return Status::none;
            const uint32_t version = get32(head + 4);
            Status bad;                               // what a trailer of this version is when it does not fit
            if (version == 3) bad = Status::unusable;
            else if (version == 4) bad = Status::unusable_delta;
            else if (version == 5) bad = Status::unusable_base;
            else if (version == 6) bad = Status::unusable_kinds;
            else if (version == 2 && have >= 16) bad = Status::malformed;
            else if (version == 1) bad = Status::none;
            else return Status::none;
            if (room < layout(version, 0, false).total) return bad;
            const uint64_t n = get64(head + 8);
            const bool wide = version >= 3 && version <= 6;
            const uint32_t width = wide ? get32(head + 16) : 1u, flags = wide ? get32(head + 20) : version == 2 ? 1u : 0u;
            if (version == 4 && ((width != 1 && width != 2 && width != 4 && width != 8) || (flags & ~1u) != 2u)) return bad;
            if (version == 5 && ((width != 1 && width != 2 && width != 4 && width != 8) || flags != 5u)) return bad;
            if (version == 6 && ((width != 1 && width != 2 && width != 4 && width != 8) || (flags & ~7u) != 8u || ((flags & 4u) && (flags & 3u) != 1u))) return bad;
            if ((version == 3 && width != 2 && width != 4 && width != 8) || (version != 4 && version != 5 && version != 6 && (flags & ~1u) != 0) || n > room / 2) return bad;
            const Layout at = layout(version, n, flags & 1u);
            if (at.total != room || std::fseek(f, static_cast<long>(file_size - sizeof tail), SEEK_SET) != 0 || std::fread(tail, sizeof tail, 1, f) != 1 ||
                std::memcmp(tail + 8, "XPIG", 4) != 0 || get64(tail) != room)
                return bad;
            std::vector<uint8_t> body(room - at.fixed - sizeof tail);      // lengths, CRCs and pads
            if (std::fseek(f, static_cast<long>(stream_end + at.fixed), SEEK_SET) != 0 || (!body.empty() && std::fread(body.data(), body.size(), 1, f) != 1))
                return bad;
            t.clens.resize(n);
            uint64_t sum = 0;
            for (uint64_t i = 0; i < n; ++i) sum += t.clens[i] = static_cast<uint16_t>(body[2 * i] | (body[2 * i + 1] << 8));
            if (sum != stream_end - stream_begin) return bad;
            if (flags & 1u) {
                t.crcs.resize(n);
                for (uint64_t i = 0; i < n; ++i) t.crcs[i] = get32(body.data() + at.crcs - at.fixed + 4 * i);
            }
            if (version == 6) {
                t.kinds.assign(body.begin() + (at.kinds - at.fixed), body.begin() + (at.kinds - at.fixed + n));
                for (uint64_t i = 0; i < n; ++i)
                    if (t.kinds[i] > 2) return bad;
            }
            t.flags = flags;
            t.version = version;
            t.has_crcs = (flags & 1u) != 0;
            t.elem_bytes = width;
            return Status::ok;
        }();
        if (status != Status::ok) t = Trailer();
        std::fseek(f, here, SEEK_SET);
        return status;
    }

  private:
    static void put32(uint8_t *p, uint32_t v) { for (int b = 0; b < 4; ++b) p[b] = static_cast<uint8_t>(v >> (8 * b)); }
    static void put64(uint8_t *p, uint64_t v) { for (int b = 0; b < 8; ++b) p[b] = static_cast<uint8_t>(v >> (8 * b)); }
    static uint32_t get32(const uint8_t *p) { uint32_t v = 0; for (int b = 0; b < 4; ++b) v |= static_cast<uint32_t>(p[b]) << (8 * b); return v; }
    static uint64_t get64(const uint8_t *p) { uint64_t v = 0; for (int b = 0; b < 8; ++b) v |= static_cast<uint64_t>(p[b]) << (8 * b); return v; }
};

}  // namespace gip
