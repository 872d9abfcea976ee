// gip_read.cpp -- a whole .gip file in memory, read by the CLI's own reader and checked packet by packet: gpuar_hip_gip_read_host
// and gpuar_hip_gip_tables_host of include/gpuar_hip.h.  Plain C++, no HIP: linked into libgpuar_hip.so, and
// built on its own -- with sanitizers -- by tests/gip_read_client.cpp.
//
// Nothing of the container is restated here: the sizes are FileHeader::getInfo's, the trailer is Trailer::load's (fed the
// memory through fmemopen), the packet forms are kinds.h's and sparse.h's.  What this file adds is the walk that holds every
// packet header against the tables BEFORE anything goes to a device: batch.from_gip hands the lengths to a kernel as they are.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gpuar_hip.h"

#include "../kinds.h"
#include "file_header.hpp"
#include "packet_index.hpp"

namespace {

struct GipFile {
    uint64_t info[GPUAR_GIP_INFO_WORDS] = {};
    std::vector<uint16_t> clens;
    gip::Trailer trailer;
};

int defect(GipFile &g, int code, uint64_t packet, uint64_t at) {
    g.info[8] = packet;
    g.info[9] = at;
    return code;
}

// the number of `status`, and the version a trailer of that status claims where it cannot be used (else 0)
uint64_t status_number(gip::Trailer::Status s) {
    using S = gip::Trailer::Status;
    return s == S::none ? 0u : s == S::ok ? 1u : s == S::malformed ? 2u : s == S::unusable ? 3u : s == S::unusable_delta ? 4u : s == S::unusable_base ? 5u : 6u;
}

int read_file(const uint8_t *file, size_t file_bytes, GipFile &g) {
    constexpr uint64_t kHeader = gip::FileHeader::HEADER_LENGTH;
    if (file_bytes < kHeader) return defect(g, GPUAR_GIP_SHORT, 0, file_bytes);
    gip::FileHeader header;
    header.setData(file);
    if (!header.checkHeaderVersion()) return defect(g, GPUAR_GIP_VERSION, 0, 0);
    const gip::CompressionInfo sizes = header.getInfo(file_bytes);
    const uint64_t unc = sizes.uncompressedFileSize, end = sizes.compressedFileSize;
    g.info[0] = unc;
    g.info[1] = kHeader;
    g.info[2] = end;
    g.info[5] = 1;
    if (end < kHeader || end > file_bytes) return defect(g, GPUAR_GIP_SIZE, 0, gip::FileHeader::COMPRESSED_FILE_SIZE_POSITION);

    FILE *f = fmemopen(const_cast<uint8_t *>(file), file_bytes, "rb");
    if (!f) return GPUAR_ERR_ARGUMENT;
    const gip::Trailer::Status status = gip::Trailer::load(f, kHeader, end, file_bytes, g.trailer);
    std::fclose(f);
    g.info[7] = status_number(status);
    if (g.info[7] >= 3u) {
        g.info[3] = g.info[7];                                 // (the statuses of versions 3 .. 6 are numbered by their version)
        return defect(g, GPUAR_GIP_TRAILER, 0, end);
    }
    const bool indexed = g.trailer.indexed();
    g.info[3] = g.trailer.version;
    g.info[5] = g.trailer.elem_bytes;
    g.info[6] = g.trailer.flags;

    const uint64_t need = (unc + gpuar::kKindsPacket - 1) / gpuar::kKindsPacket;
    if (indexed && g.trailer.clens.size() != need) return defect(g, GPUAR_GIP_COUNT, g.trailer.clens.size(), end);
    g.info[4] = indexed ? need : 0;
    uint64_t at = kHeader, p = 0;
    for (; indexed ? p < need : at < end; ++p) {
        if (p >= need) return defect(g, GPUAR_GIP_COUNT, p, at);              // (a walk only: more packets than the size needs)
        if (end - at < gpuar::kKindsHeader) return defect(g, GPUAR_GIP_CUT, p, at);
        const uint32_t clen = file[at] | static_cast<uint32_t>(file[at + 1]) << 8, ulen = file[at + 2] | static_cast<uint32_t>(file[at + 3]) << 8;
        const uint32_t listed = indexed ? g.trailer.clens[p] : clen;
        if (listed < gpuar::kKindsHeader || listed > gpuar::kKindsSlot) return defect(g, GPUAR_GIP_CLEN, p, at);
        if (clen != listed) return defect(g, GPUAR_GIP_TABLE, p, at);
        if (clen > end - at) return defect(g, GPUAR_GIP_CUT, p, at);
        const uint64_t left = unc - p * gpuar::kKindsPacket;
        if (ulen != (left < gpuar::kKindsPacket ? left : gpuar::kKindsPacket)) return defect(g, GPUAR_GIP_ULEN, p, at);
        const uint32_t kind = g.trailer.mixed() ? g.trailer.kinds[p] : gpuar::kSparseCoded;
        if (kind > gpuar::kSparseSparse) return defect(g, GPUAR_GIP_KIND, p, at);
        if (kind == gpuar::kSparseRaw && clen != gpuar::kinds_raw_clen(ulen)) return defect(g, GPUAR_GIP_RAW, p, at);
        if (kind == gpuar::kSparseSparse) {
            if (clen < gpuar::kKindsHeader + 4u) return defect(g, GPUAR_GIP_SPARSE, p, at);
            const uint8_t *rec = file + at + gpuar::kKindsHeader;
            const uint32_t head = rec[0] | static_cast<uint32_t>(rec[1]) << 8 | static_cast<uint32_t>(rec[2]) << 16 | static_cast<uint32_t>(rec[3]) << 24;
            if (!gpuar::sparse_head_ok(head, clen - gpuar::kKindsHeader, ulen) || clen != gpuar::kinds_sparse_clen(head >> 16))
                return defect(g, GPUAR_GIP_SPARSE, p, at);
        }
        g.clens.push_back(static_cast<uint16_t>(clen));
        at += clen;
    }
    g.info[4] = p;
    if (p != need) return defect(g, GPUAR_GIP_COUNT, p, at);
    if (at != end) return defect(g, GPUAR_GIP_SUM, p, at);
    return GPUAR_OK;
}

}  // namespace

extern "C" {

int gpuar_hip_gip_read_host(const uint8_t *file, size_t file_bytes, uint64_t info[GPUAR_GIP_INFO_WORDS]) {
    if (!file || !info) return GPUAR_ERR_ARGUMENT;
    GipFile g;
    int code;
    try {
        code = read_file(file, file_bytes, g);
    } catch (...) {                                            // (an allocation the reader could not make)
        code = GPUAR_ERR_ARGUMENT;
    }
    for (int i = 0; i < GPUAR_GIP_INFO_WORDS; ++i) info[i] = g.info[i];
    return code;
}

int gpuar_hip_gip_tables_host(const uint8_t *file, size_t file_bytes, uint16_t *clen, uint32_t *crc, uint8_t *kind, size_t n_packets) {
    if (!file || (!clen && n_packets)) return GPUAR_ERR_ARGUMENT;
    GipFile g;
    try {
        const int code = read_file(file, file_bytes, g);
        if (code != GPUAR_OK) return code;
    } catch (...) {
        return GPUAR_ERR_ARGUMENT;
    }
    if (g.clens.size() != n_packets || (crc && !g.trailer.has_crcs)) return GPUAR_ERR_ARGUMENT;
    for (size_t p = 0; p < n_packets; ++p) {
        clen[p] = g.clens[p];
        if (crc) crc[p] = g.trailer.crcs[p];
        if (kind) kind[p] = g.trailer.mixed() ? g.trailer.kinds[p] : static_cast<uint8_t>(gpuar::kSparseCoded);
    }
    return GPUAR_OK;
}

}  // extern "C"
