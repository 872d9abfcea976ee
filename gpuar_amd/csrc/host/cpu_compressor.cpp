// cpu_compressor.cpp -- host packet loop of `gpuar --host`
// (what src/cpu_compressor.cpp:10-206 does), running the same per-lane codec
// source the GPU kernels run (../lane_codec.h compiled for the host).  This is
// an explicit user-selected mode, as in the reference; it is never a fallback
// of the GPU path.
#include "cpu_compressor.hpp"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <thread>
#include <vector>

#include <unistd.h>

#include "../crc32.h"
#include "../lane_codec.h"
#include "../planes.h"
#include "../delta.h"
#include "../xorbase.h"
#include "../kinds.h"
#include "file_header.hpp"
#include "packet_index.hpp"

namespace gip {

namespace {

const gpuar::RecipTable kRecip = gpuar::RecipTable();
const gpuar::DecodeConstTable kDecode = gpuar::DecodeConstTable();
constexpr size_t kBatchPackets = 4096;   // 32 MiB of input per batch

// one packet through the same three lane programs the GPU's encoder wavefronts run
size_t encode_one(const uint8_t *in, uint32_t len, uint8_t *slot) {
    uint16_t table[gpuar::kTreeRows];
    uint8_t *col = reinterpret_cast<uint8_t *>(table);
    gpuar::TopModeler<1> top;
    gpuar::LowModeler<1> low;
    top.open(col, 0, in[0]);
    low.open(col, 0, in[0]);
    gpuar::CarryCoderLane coder;     // (the carry form: the same bytes in fewer operations, lane_codec.h)
    coder.open(slot, 0);
    for (uint32_t i = 0; i < len; ++i) {
        const uint32_t x = in[i], next = i + 1 < len ? in[i + 1] : 0u;
        coder.step(top.step(x, 256u + i, next) + low.step(x, 256u + i, next), kRecip.r[i]);
    }
    bool overflowed = false;
    const uint32_t clen = coder.finish(len, overflowed);
    if (overflowed) throw std::runtime_error("a packet outgrew its 8704-byte slot");
    return clen;
}

// ... and the decoder lane program
size_t decode_one(const uint8_t *pkt, const uint8_t *limit, uint8_t *out) {
    alignas(16) uint8_t records[gpuar::kDecodeRecords * 16];
    gpuar::DecoderLane<3> dec;
    const size_t readable = static_cast<size_t>(limit - pkt);
    dec.open(records, pkt, 0, readable < 0x7FFFFFFFu ? static_cast<uint32_t>(readable) : 0x7FFFFFFFu, true);
    for (uint32_t i = 0; i < dec.ulen; ++i) dec.step(i, kDecode.c[i], out);
    dec.finish(out);
    if (dec.bad) throw std::runtime_error("Incorrect file format");
    return dec.ulen;
}

// f(p) for p in [0, n) on `threads` host threads.  The first exception wins and stops the others
// at their next packet.
template <typename F>
void for_each_packet(size_t n, unsigned threads, F &&f) {
    if (threads <= 1 || n < 2) {
        for (size_t p = 0; p < n; ++p) f(p);
        return;
    }
    std::vector<std::thread> pool;
    std::exception_ptr failure;
    std::mutex failure_lock;
    std::atomic<bool> stop{false};
    for (unsigned t = 0; t < threads; ++t)
        pool.emplace_back([&, t] {
            try {
                for (size_t p = t; p < n && !stop.load(std::memory_order_relaxed); p += threads) f(p);
            } catch (...) {
                std::lock_guard<std::mutex> hold(failure_lock);
                if (!failure) failure = std::current_exception();
                stop.store(true, std::memory_order_relaxed);
            }
        });
    for (auto &th : pool) th.join();
    if (failure) std::rethrow_exception(failure);
}

// What a plan does to `n` bytes in front of the coder: XOR with `base`, else delta, else planes, else nothing.  Returns where the
// bytes to code are: `out` when the plan transforms, else `in`.
const uint8_t *split_host(const PacketPlan &plan, const uint8_t *in, const uint8_t *base, size_t n, uint8_t *out) {
    if (plan.based) gpuar::split_xor_host(in, base, n, plan.elem, out);
    else if (plan.delta) gpuar::split_delta_host(in, n, plan.elem, out);
    else if (plan.elem > 1) gpuar::planes_host<false>(in, n, plan.elem, out);
    return plan.transforms() ? out : in;
}

// ... and undoes behind the decoder: decoded[0..n) -> out[0..n); only for a plan that transforms
void merge_host(const PacketPlan &plan, const uint8_t *decoded, const uint8_t *base, size_t n, uint8_t *out) {
    if (plan.based) gpuar::merge_xor_host(decoded, base, n, plan.elem, out);
    else if (plan.delta) gpuar::merge_delta_host(decoded, n, plan.elem, out);
    else gpuar::planes_host<true>(decoded, n, plan.elem, out);
}

}  // namespace

CPUCompressor::CPUCompressor() {}
CPUCompressor::~CPUCompressor() {}

CompressionInfo CPUCompressor::compress(ProgressMonitor *monitor) {
    CompressionInfo info;
    monitor->reset();
    process_timer.reset();
    io_timer.reset();
    io_timer.start();
    openFiles();
    info.uncompressedFileSize = getFileSize(openFile);
    if (std::fseek(saveFile, FileHeader::HEADER_LENGTH, SEEK_SET) != 0) throw std::runtime_error("Seek file failed");
    io_timer.stop();
    info.compressedFileSize = FileHeader::HEADER_LENGTH;

    const unsigned nthreads = threads ? threads : std::max(1u, std::thread::hardware_concurrency());
    std::vector<uint8_t> in(kBatchPackets * gpuar::kPacket + 16), slots(kBatchPackets * gpuar::kSlot);
    // --planes: what is coded is the batch split into byte planes (a batch is a whole number of groups: 4096 packets; only the
    // file's last one can be shorter, and its tail is the file's tail); the CRCs stay those of the bytes as read
    static_assert(kBatchPackets % 8 == 0, "a batch starts on a group boundary for every element width");
    // --delta: the same with the elements' differences inside every group in front of the split (at a width of 1 too)
    // --base: the same with the XOR against the base's bytes at the same file offsets in front of the split (at a width of 1 too)
    const PacketPlan plan = this->plan();
    std::vector<uint8_t> split(plan.transforms() ? in.size() : 0), base(plan.based ? in.size() : 0);
    uint64_t file_at = 0;
    std::vector<uint32_t> clen(kBatchPackets), crc(kBatchPackets);
    std::vector<uint16_t> all_clens;                   // for the optional index trailer
    std::vector<uint32_t> all_crcs;                    // for the optional checksum trailer
    std::vector<uint8_t> kind(kBatchPackets), all_kinds;      // --stored / --sparse: what every packet is kept as (version-6 trailer)
    const bool trailer = wantsTrailer();
    try {
        if (plan.based) openBase(info.uncompressedFileSize, "the input");
        for (;;) {
            io_timer.start();
            const size_t got = std::fread(in.data(), 1, kBatchPackets * gpuar::kPacket, openFile);
            if (got && plan.based) readBase(base.data(), got, file_at);
            file_at += got;
            io_timer.stop();
            if (got == 0) break;
            const size_t np = (got + gpuar::kPacket - 1) / gpuar::kPacket;
            process_timer.start();     // model init + codec only, as src/cpu_compressor.cpp:157-161
            const uint8_t *coded = split_host(plan, in.data(), base.data(), got, split.data());
            for_each_packet(np, nthreads, [&](size_t p) {
                const size_t off = p * gpuar::kPacket;
                const uint32_t len = static_cast<uint32_t>(std::min<size_t>(gpuar::kPacket, got - off));
                // --stored=auto / --sparse=auto: the rule of ../kinds.h over the bytes that are coded; a raw or sparse packet is
                // its own stream form in the slot (what the GPU pipeline overwrites the encoder's packet with), a coded one as ever
                uint32_t kept = 0;
                if (plan.kinds) {
                    kind[p] = static_cast<uint8_t>(gpuar::kinds_store_packet(coded + off, len, plan.stored, plan.sparse, slots.data() + p * gpuar::kSlot, gpuar::kSlot, &kept));
                    if (kind[p] > gpuar::kSparseSparse) throw std::runtime_error("a packet outgrew its 8704-byte slot");
                }
                clen[p] = kept ? kept : static_cast<uint32_t>(encode_one(coded + off, len, slots.data() + p * gpuar::kSlot));
                if (plan.crcs) crc[p] = gpuar::crc32_update(0, in.data() + off, len);
            });
            process_timer.stop();
            io_timer.start();
            for (size_t p = 0; p < np; ++p) {
                if (std::fwrite(slots.data() + p * gpuar::kSlot, clen[p], 1, saveFile) != 1)
                    throw std::runtime_error("Write data to file failed");
                info.compressedFileSize += clen[p];
                if (trailer) all_clens.push_back(static_cast<uint16_t>(clen[p]));
                if (plan.crcs) all_crcs.push_back(crc[p]);
                if (plan.kinds) all_kinds.push_back(kind[p]);
            }
            io_timer.stop();
            info.processedUncompressedSize += got;
            monitor->updateProgress(&info);
        }
        io_timer.start();
        saveTrailer(plan, all_clens, all_crcs, all_kinds);
        FileHeader header;
        header.setCompressedFileSize(info.compressedFileSize);
        header.setUncompressedFileSize(info.uncompressedFileSize);
        if (std::fseek(saveFile, 0, SEEK_SET) != 0) throw std::runtime_error("Seek file failed");
        if (std::fwrite(header.getData(), FileHeader::HEADER_LENGTH, 1, saveFile) != 1)
            throw std::runtime_error("Write data to file failed");
        closeFiles();
        io_timer.stop();
    } catch (...) {
        closeFiles();
        throw;
    }
    info.processTime = process_timer.value();
    info.ioTime = io_timer.value();
    return info;
}

CompressionInfo CPUCompressor::decompress(ProgressMonitor *monitor) {
    CompressionInfo info;
    monitor->reset();
    process_timer.reset();
    io_timer.reset();
    io_timer.start();
    openFiles();
    FileHeader header;
    const size_t fileSize = getFileSize(openFile);
    bool mixed_file = false;                     // a version-6 file: a failed job leaves an empty output, as the GPU pipeline does
    try {
        if (std::fread(header.getData(), FileHeader::HEADER_LENGTH, 1, openFile) != 1 || !header.checkHeaderVersion())
            throw std::runtime_error("Incorrect file format");
        info = header.getInfo(fileSize);
        const size_t stream_end = streamEnd(info, fileSize);
        // packet lengths, per-packet CRCs (every decoded packet is checked against them) and the width of the byte planes the
        // packets hold (merged back below), as far as the file's trailer gives them
        const Trailer trailer = loadTrailer(stream_end, fileSize);
        const std::vector<uint16_t> &index = trailer.clens;
        const PacketPlan plan = PacketPlan::of(trailer);
        const bool indexed = trailer.indexed(), merging = plan.transforms();
        mixed_file = plan.kinds;
        size_t first_packet = 0;                 // of the window
        io_timer.stop();

        // The stream is taken in windows of at most kBatchPackets packets, as GPUCompressor does:
        // memory stays bounded whatever the file size (the 64-bit header exists for 8-64 GiB inputs).
        // With an index the window's extent comes from the stored lengths; without one the bytes are
        // read first and `off += clen` is walked in memory (src/cpu_compressor.cpp:47-56 walks it
        // through the file), then the file is wound back to the end of the last whole packet.
        const unsigned nthreads = threads ? threads : std::max(1u, std::thread::hardware_concurrency());
        std::vector<uint8_t> window(kBatchPackets * gpuar::kSlot + 65536 + 16), out(kBatchPackets * gpuar::kPacket);
        std::vector<uint8_t> decoded(merging ? out.size() : 0);      // byte planes: a window is decoded here and merged into `out`
        std::vector<uint8_t> base(plan.based ? out.size() : 0);      // ... and XORed with these bytes of the base
        if (plan.based) openBase(info.uncompressedFileSize, "the file");
        std::vector<size_t> offsets(kBatchPackets + 1);
        std::vector<uint32_t> ulen(kBatchPackets);
        size_t file_pos = FileHeader::HEADER_LENGTH, next_packet = 0;
        while (file_pos < stream_end) {
            size_t np = 0, bytes = 0;
            io_timer.start();
            if (indexed) {
                offsets[0] = 0;
                while (next_packet < index.size() && np < kBatchPackets && bytes + index[next_packet] + 16 <= window.size()) {
                    const size_t c = index[next_packet++];
                    // (byte planes: no packet longer than a slot, so that every window but the last holds kBatchPackets packets,
                    // a whole number of groups)
                    if (c < gpuar::kHdr || ((merging || plan.kinds) && c > gpuar::kSlot)) throw std::runtime_error("Incorrect file format");
                    bytes += c;
                    offsets[++np] = bytes;
                }
                if (!np) throw std::runtime_error("Incorrect file format");
                if (std::fread(window.data(), 1, bytes, openFile) != bytes) throw std::runtime_error("Invalid file length");
            } else {
                const size_t want = std::min(stream_end - file_pos, kBatchPackets * static_cast<size_t>(gpuar::kSlot) + 65536);
                if (std::fread(window.data(), 1, want, openFile) != want) throw std::runtime_error("Invalid file length");
                offsets[0] = 0;
                while (bytes < want && np < kBatchPackets) {
                    if (want - bytes < gpuar::kHdr) {
                        if (file_pos + want == stream_end) throw std::runtime_error("Incorrect file format");
                        break;                             // header cut by the window: next round
                    }
                    const size_t c = window[bytes] | (static_cast<size_t>(window[bytes + 1]) << 8);
                    if (c < gpuar::kHdr || file_pos + bytes + c > stream_end) throw std::runtime_error("Incorrect file format");
                    if (bytes + c > want) break;           // packet cut by the window: next round
                    bytes += c;
                    offsets[++np] = bytes;
                }
                if (!np) throw std::runtime_error("Incorrect file format");
                if (bytes != want && std::fseek(openFile, static_cast<long>(file_pos + bytes), SEEK_SET) != 0)
                    throw std::runtime_error("Seek file failed");
            }
            io_timer.stop();
            file_pos += bytes;
            process_timer.start();
            uint8_t *const plain = merging ? decoded.data() : out.data();
            for_each_packet(np, nthreads, [&](size_t p) {
                const uint8_t *pkt = window.data() + offsets[p];
                const uint32_t kind = plan.kinds ? trailer.kinds[first_packet + p] : gpuar::kSparseCoded;
                if (kind == gpuar::kSparseCoded) {
                    ulen[p] = static_cast<uint32_t>(decode_one(pkt, window.data() + bytes, plain + p * gpuar::kPacket));
                } else {                                   // raw or sparse (../kinds.h): the header is checked, the decoder never sees it
                    const uint32_t n = pkt[2] | static_cast<uint32_t>(pkt[3]) << 8;
                    if (!gpuar::kinds_expand_packet(pkt, offsets[p + 1] - offsets[p], kind, plain + p * gpuar::kPacket, n))
                        throw std::runtime_error("Incorrect file format (malformed " + std::string(kind == gpuar::kSparseRaw ? "raw" : "sparse") + " packet " +
                                                 std::to_string(first_packet + p) + ")");
                    ulen[p] = n;
                }
            });
            // (byte planes, and raw and sparse packets, as the GPU pipeline requires of such a file: every packet but the file's last
            // holds 8192 bytes)
            if (merging || plan.kinds)
                for (size_t p = 0; p < np; ++p) checkPlanesPacket(first_packet + p, index.size(), ulen[p]);
            if (merging) {
                size_t total = 0;
                for (size_t p = 0; p < np; ++p) total += ulen[p];
                // (every packet in front of this window holds 8192 bytes: checkPlanesPacket)
                if (plan.based) readBase(base.data(), total, static_cast<uint64_t>(first_packet) * gpuar::kPacket);
                merge_host(plan, decoded.data(), base.data(), total, out.data());
            }
            if (plan.crcs) {
                for (size_t p = 0; p < np; ++p) {
                    const size_t g = first_packet + p;
                    const uint64_t begin = static_cast<uint64_t>(g) * gpuar::kPacket;
                    checkChecksumPacket(g, trailer.crcs.size(), ulen[p]);
                    if (gpuar::crc32_update(0, out.data() + p * gpuar::kPacket, ulen[p]) != trailer.crcs[g]) throw checksumError(g, begin, begin + ulen[p]);
                }
            }
            first_packet += np;
            process_timer.stop();
            io_timer.start();
            for (size_t p = 0; p < np; ++p) {
                if (ulen[p] && std::fwrite(out.data() + p * gpuar::kPacket, ulen[p], 1, saveFile) != 1)
                    throw std::runtime_error("Write raw data to file failed");
                info.processedUncompressedSize += ulen[p];
            }
            io_timer.stop();
            monitor->updateProgress(&info);
        }
        info.uncompressedFileSize = info.processedUncompressedSize;     // what the packets held
        io_timer.start();
        closeFiles();
        io_timer.stop();
    } catch (...) {
        if (mixed_file && saveFile && (std::fflush(saveFile) != 0 || ::ftruncate(fileno(saveFile), 0) != 0)) {}
        closeFiles();
        throw;
    }
    info.processTime = process_timer.value();
    info.ioTime = io_timer.value();
    return info;
}

}  // namespace gip
