// executor_client.cpp -- calls initConstantRange / garCompressExecutor / garDecompressExecutor the way a program written
// against the reference's header calls them, from plain C++ (g++, <hip/hip_runtime_api.h>, gpuar_hip.h; no kernel here):
//
//   * two device buffers, 8192 * T and 8704 * T bytes, allocated once per process and NEVER cleared -- not between batches,
//     not between jobs: stale input lies behind the bytes of a short batch, stale packets in the slots behind the last
//     live one, stale bytes of earlier packets behind every packet's clen;
//   * input goes up one packet per hipMemcpyAsync, round-robin over a few ordinary (blocking) streams, out of a pinned
//     staging slot per stream; meanwhile the previous batch's results come down one packet per copy on an output stream;
//   * the executor runs on the NULL stream with numBlocks = ceil(packets / per-block) and is followed by
//     hipDeviceSynchronize(), whose result and gpuar_hip_last_error() are checked;
//   * compress: the u16 at the start of each 8704-byte slot says how many of its bytes go to the file;
//     decompress: 4 header bytes are read, then clen - 4 more, exactly clen bytes go to slot k, `size` is packets * 8704,
//     and min(8192, bytes left by the header's count) of each decoded packet are written;
//   * at the end of every job gpuar_hip_status() must read 0.
//
//   executor_client [--packets=T] [--per-block=32] [--factor=8] [--streams=4] [--poison=BYTE] [--tight-size] (c|d IN OUT)...
//
// T defaults to per-block * multiProcessorCount * factor.  --poison fills both device buffers ONCE, before the first job.
// --tight-size: the decoder's `size` ends with the last live packet, (packets - 1) * 8704 + its clen, instead of with its
// slot: include/gpuar_hip.h promises every packet whose slot STARTS in front of `size`, and a multiple of 8704 cannot tell
// a ceiling from a floor.
// One line per job on stderr: "ok c|d ..." or "error ...: what"; the first error ends the run with exit code 1 (nothing
// more is started on a device after an error).  Test-only (tests/test_executor_caller.py builds it into tests/_build/).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "file_header.hpp"
#include "gpuar_hip.h"

namespace {

constexpr size_t kPacket = GPUAR_PACKET_BYTES, kSlot = GPUAR_SLOT_BYTES, kHeader = GPUAR_PACKET_HEADER_BYTES;

void hip(hipError_t e, const char *what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

struct File {
    FILE *f = nullptr;
    File(const std::string &name, const char *mode) : f(std::fopen(name.c_str(), mode)) {
        if (!f) throw std::runtime_error("cannot open " + name);
    }
    ~File() {
        if (f) std::fclose(f);
    }
    void close() {
        FILE *g = f;
        f = nullptr;
        if (g && std::fclose(g) != 0) throw std::runtime_error("close failed");
    }
};

struct Caller {
    size_t packets = 0, per_block = 32, n_streams = 4;
    bool tight_size = false;
    uint8_t *d_plain = nullptr, *d_slots = nullptr;      // 8192 * packets, 8704 * packets: the only device memory there is
    uint8_t *h_in = nullptr, *h_out = nullptr;           // pinned: one slot per input stream, one for the output stream
    std::vector<hipStream_t> in_streams;
    hipStream_t out_stream = nullptr;

    void open(int poison) {
        hip(hipMalloc(reinterpret_cast<void **>(&d_plain), kPacket * packets), "hipMalloc");
        hip(hipMalloc(reinterpret_cast<void **>(&d_slots), kSlot * packets), "hipMalloc");
        hip(hipHostMalloc(reinterpret_cast<void **>(&h_in), kSlot * n_streams, hipHostMallocDefault), "hipHostMalloc");
        hip(hipHostMalloc(reinterpret_cast<void **>(&h_out), kSlot, hipHostMallocDefault), "hipHostMalloc");
        in_streams.resize(n_streams);
        for (auto &s : in_streams) hip(hipStreamCreate(&s), "hipStreamCreate");
        hip(hipStreamCreate(&out_stream), "hipStreamCreate");
        if (poison >= 0) {
            hip(hipMemset(d_plain, poison, kPacket * packets), "hipMemset");
            hip(hipMemset(d_slots, poison, kSlot * packets), "hipMemset");
            hip(hipDeviceSynchronize(), "hipDeviceSynchronize");
        }
        initConstantRange();
    }
    void close() {
        (void)hipDeviceSynchronize();
        for (auto &s : in_streams) (void)hipStreamDestroy(s);
        if (out_stream) (void)hipStreamDestroy(out_stream);
        (void)hipHostFree(h_in);
        (void)hipHostFree(h_out);
        (void)hipFree(d_plain);
        (void)hipFree(d_slots);
    }
    void syncInputs() {
        for (auto &s : in_streams) hip(hipStreamSynchronize(s), "hipStreamSynchronize");
    }
    // after an executor: the device-wide synchronise the reference's caller does, and the two places errors surface
    void afterLaunch(const char *who) {
        hip(hipDeviceSynchronize(), who);
        const int e = gpuar_hip_last_error();
        if (e != GPUAR_OK) throw std::runtime_error(std::string(who) + ": " + gpuar_hip_error_string(e));
    }
    void endOfJob() {
        uint32_t flags = 0;
        const int e = gpuar_hip_status(&flags);
        if (e != GPUAR_OK) throw std::runtime_error(std::string("gpuar_hip_status: ") + gpuar_hip_error_string(e));
        if (flags) throw std::runtime_error("gpuar_hip_status reads " + std::to_string(flags) + " at the end of the job");
    }

    // -> batches launched
    size_t compress(const std::string &in_name, const std::string &out_name) {
        File in(in_name, "rb"), out(out_name, "wb");
        gip::FileHeader header;
        if (std::fwrite(header.getData(), gip::FileHeader::HEADER_LENGTH, 1, out.f) != 1) throw std::runtime_error("write failed");
        uint64_t plain_total = 0, file_total = gip::FileHeader::HEADER_LENGTH;
        size_t batches = 0, coded = 0;       // coded: packets of the previous batch waiting in d_slots
        bool at_end = false;
        for (;;) {
            size_t read_bytes = 0, taken = 0, fetched = 0;
            // upload this batch packet by packet while the previous one comes down packet by packet
            while ((!at_end && taken < packets) || fetched < coded) {
                if (fetched < coded)
                    hip(hipMemcpyAsync(h_out, d_slots + fetched * kSlot, kSlot, hipMemcpyDeviceToHost, out_stream), "D2H");
                if (!at_end && taken < packets) {
                    const size_t s = taken % n_streams;
                    hip(hipStreamSynchronize(in_streams[s]), "hipStreamSynchronize");      // its staging slot is free again
                    const size_t got = std::fread(h_in + s * kSlot, 1, kPacket, in.f);
                    if (got) {
                        hip(hipMemcpyAsync(d_plain + read_bytes, h_in + s * kSlot, got, hipMemcpyHostToDevice, in_streams[s]), "H2D");
                        read_bytes += got;
                        ++taken;
                    }
                    if (got < kPacket) at_end = true;
                }
                if (fetched < coded) {
                    hip(hipStreamSynchronize(out_stream), "hipStreamSynchronize");
                    const size_t clen = h_out[0] | (static_cast<size_t>(h_out[1]) << 8);
                    if (clen < kHeader || clen > kSlot) throw std::runtime_error("a slot's length field reads " + std::to_string(clen));
                    if (std::fwrite(h_out, clen, 1, out.f) != 1) throw std::runtime_error("write failed");
                    file_total += clen;
                    ++fetched;
                }
            }
            syncInputs();
            coded = 0;
            if (!read_bytes) break;
            const size_t blocks = (read_bytes + kPacket * per_block - 1) / (kPacket * per_block);
            garCompressExecutor(d_plain, read_bytes, d_slots, static_cast<uint32_t>(blocks));
            afterLaunch("garCompressExecutor");
            ++batches;
            plain_total += read_bytes;
            coded = taken;
        }
        header.setUncompressedFileSize(plain_total);
        header.setCompressedFileSize(file_total);
        if (std::fseek(out.f, 0, SEEK_SET) != 0 || std::fwrite(header.getData(), gip::FileHeader::HEADER_LENGTH, 1, out.f) != 1)
            throw std::runtime_error("write failed");
        out.close();
        endOfJob();
        return batches;
    }

    size_t decompress(const std::string &in_name, const std::string &out_name) {
        File in(in_name, "rb"), out(out_name, "wb");
        std::fseek(in.f, 0, SEEK_END);
        const uint64_t file_size = static_cast<uint64_t>(std::ftell(in.f));
        std::fseek(in.f, 0, SEEK_SET);
        gip::FileHeader header;
        if (std::fread(header.getData(), gip::FileHeader::HEADER_LENGTH, 1, in.f) != 1 || !header.checkHeaderVersion())
            throw std::runtime_error("Incorrect file format");
        const gip::CompressionInfo info = header.getInfo(file_size);
        const uint64_t stream_end = info.compressedFileSize;
        if (stream_end < gip::FileHeader::HEADER_LENGTH || stream_end > file_size) throw std::runtime_error("Invalid file length");
        uint64_t at = gip::FileHeader::HEADER_LENGTH, left = info.uncompressedFileSize;
        size_t batches = 0, decoded = 0;     // decoded: packets of the previous batch waiting in d_plain
        for (;;) {
            size_t taken = 0, fetched = 0, last_clen = 0;
            while ((at < stream_end && taken < packets) || fetched < decoded) {
                if (fetched < decoded)
                    hip(hipMemcpyAsync(h_out, d_plain + fetched * kPacket, kPacket, hipMemcpyDeviceToHost, out_stream), "D2H");
                if (at < stream_end && taken < packets) {
                    const size_t s = taken % n_streams;
                    hip(hipStreamSynchronize(in_streams[s]), "hipStreamSynchronize");
                    uint8_t *stage = h_in + s * kSlot;
                    if (std::fread(stage, kHeader, 1, in.f) != 1) throw std::runtime_error("Incorrect file format");
                    const size_t clen = stage[0] | (static_cast<size_t>(stage[1]) << 8);
                    // (what keeps every copy inside slot `taken`: the reference's caller trusts the field)
                    if (clen < kHeader || clen > kSlot || at + clen > stream_end) throw std::runtime_error("Invalid file length");
                    if (clen > kHeader && std::fread(stage + kHeader, 1, clen - kHeader, in.f) != clen - kHeader)
                        throw std::runtime_error("Invalid file length");
                    hip(hipMemcpyAsync(d_slots + taken * kSlot, stage, clen, hipMemcpyHostToDevice, in_streams[s]), "H2D");
                    at += clen;
                    last_clen = clen;
                    ++taken;
                }
                if (fetched < decoded) {
                    hip(hipStreamSynchronize(out_stream), "hipStreamSynchronize");
                    const size_t n = static_cast<size_t>(std::min<uint64_t>(kPacket, left));
                    if (n && std::fwrite(h_out, n, 1, out.f) != 1) throw std::runtime_error("write failed");
                    left -= n;
                    ++fetched;
                }
            }
            syncInputs();
            decoded = 0;
            if (!taken) break;
            const size_t blocks = (taken + per_block - 1) / per_block;
            garDecompressExecutor(d_slots, tight_size ? (taken - 1) * kSlot + last_clen : taken * kSlot, d_plain, static_cast<uint32_t>(blocks));
            afterLaunch("garDecompressExecutor");
            ++batches;
            decoded = taken;
        }
        out.close();
        endOfJob();
        return batches;
    }
};

}  // namespace

int main(int argc, char **argv) {
    Caller caller;
    size_t factor = 8;
    int poison = -1;
    std::vector<std::string> words;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto value = [&](const char *name, size_t &dst) {
            const std::string key = std::string("--") + name + "=";
            if (a.rfind(key, 0) != 0) return false;
            dst = std::strtoul(a.c_str() + key.size(), nullptr, 0);
            return true;
        };
        size_t p = 0;
        if (value("packets", caller.packets) || value("per-block", caller.per_block) || value("factor", factor) || value("streams", caller.n_streams)) continue;
        if (value("poison", p)) {
            poison = static_cast<int>(p & 0xFF);
            continue;
        }
        if (a == "--tight-size") {
            caller.tight_size = true;
            continue;
        }
        words.push_back(a);
    }
    if (words.size() % 3 != 0 || caller.per_block == 0 || caller.n_streams == 0 || caller.n_streams > 64 || factor == 0) {
        std::fprintf(stderr, "usage: executor_client [--packets=T] [--per-block=32] [--factor=8] [--streams=4] [--poison=BYTE] [--tight-size] (c|d IN OUT)...\n");
        return 2;
    }
    for (size_t j = 0; j < words.size(); j += 3)
        if (words[j] != "c" && words[j] != "d") {
            std::fprintf(stderr, "executor_client: c or d, not %s\n", words[j].c_str());
            return 2;
        }
    int code = 0;
    bool opened = false;
    try {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw std::runtime_error("No HIP device found");
        hip(hipSetDevice(0), "hipSetDevice");
        if (!caller.packets) {
            hipDeviceProp_t prop;
            hip(hipGetDeviceProperties(&prop, 0), "hipGetDeviceProperties");
            caller.packets = caller.per_block * static_cast<size_t>(prop.multiProcessorCount) * factor;
        }
        if (caller.packets > (1u << 20)) throw std::runtime_error("more than 2^20 packets per batch");
        opened = true;
        caller.open(poison);
        for (size_t j = 0; j < words.size(); j += 3) {
            try {
                const size_t batches = words[j] == "c" ? caller.compress(words[j + 1], words[j + 2]) : caller.decompress(words[j + 1], words[j + 2]);
                std::fprintf(stderr, "ok %s packets=%zu batches=%zu\n", words[j].c_str(), caller.packets, batches);
            } catch (const std::exception &e) {
                std::fprintf(stderr, "error %s: %s\n", words[j].c_str(), e.what());
                code = 1;
                break;
            }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error start: %s\n", e.what());
        code = 1;
    }
    if (opened) caller.close();
    return code;
}
