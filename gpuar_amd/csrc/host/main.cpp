// main.cpp -- the `gpuar` command line (flags and output text of src/main.cpp:59-205).
//
//   gpuar c|d --in=F --out=G [--host] [--device=N] [--gpus=K] [--threads=T] [--batch=P] [--index] [--checksum] [--planes=W|auto] [--delta[=on|off|auto]] [--base=FILE [--base-auto]] [--stored[=auto|off]] [--sparse[=auto|off]] [--nointeractive] [--help]
//
// Differences from the reference, all on the error side: `--in F` and `--in=F`
// are both accepted on purpose (the reference's `--in F` works by accident of
// argv layout), device 0 can be chosen explicitly, a missing GPU is an error
// unless --host is given (no silent CPU fallback), and failures exit non-zero
// with a message instead of std::terminate.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>

#include "cpu_compressor.hpp"
#ifndef GPUAR_HOST_ONLY
#include "gpu_compressor.hpp"
#endif

using namespace gip;

namespace {

// flags are matched after stripping leading '-' and case-insensitively, as
// common/helper_string.h:104-130 does
bool flag_name_is(const char *arg, const char *name, const char **value) {
    while (*arg == '-') ++arg;
    const size_t n = std::strlen(name);
    for (size_t i = 0; i < n; ++i)
        if (std::tolower(static_cast<unsigned char>(arg[i])) != name[i]) return false;
    if (arg[n] == '\0') {
        *value = nullptr;
        return true;
    }
    if (arg[n] == '=') {
        *value = arg + n + 1;
        return true;
    }
    return false;
}

void usage() {
    std::cout << "Usage: gpuar [options] --in=inputfile --out=outputfile" << std::endl << std::endl;
    std::cout << "where options inclide:" << std::endl;
    std::cout << "c             compress input file" << std::endl;
    std::cout << "d             decompress input file" << std::endl;
    std::cout << "--in          input file" << std::endl;
    std::cout << "--out         outputt file" << std::endl;
    std::cout << "--help        print this help message" << std::endl;
    std::cout << "--host        execute kernel code on host (cpu mode), otherwise execute kernel code on the GPU" << std::endl;
    std::cout << "--device      specify GPU device, otherwise use device 0" << std::endl;
    std::cout << "--gpus        shard the packets over this many GPUs (devices 0..K-1)" << std::endl;
    std::cout << "--threads     host threads for --host (default 1, 0 = all cores)" << std::endl;
    std::cout << "--batch       largest chunk of packets a pipeline lane takes at a time (default 65536 = 512 MiB)" << std::endl;
    std::cout << "--index       (compress) append the packet-offset index trailer; decompress uses it when present" << std::endl;
    std::cout << "--checksum    (compress) append the trailer with a CRC-32 per packet (and the index); decompress verifies it when present" << std::endl;
    std::cout << "--planes      (compress) W = 2, 4 or 8: split the input into byte planes of W-byte elements first (typed data compresses better);" << std::endl;
    std::cout << "              the file then carries a trailer with W, which decompress needs; 1 = off (default);" << std::endl;
    std::cout << "              auto: W is chosen from the first 16 MiB of the input (a histogram pass on the host predicts its size at every W)" << std::endl;
    std::cout << "--delta       (compress) replace the W-byte integers of the input (W from --planes; alone: bytes) by their differences first:" << std::endl;
    std::cout << "              ordered integers (offsets, sorted indices, timestamps, samples) compress several times smaller, other data grows;" << std::endl;
    std::cout << "              the file then carries a trailer that says so, which decompress needs; --delta=on: the same; --delta=off: no filter" << std::endl;
    std::cout << "              (default); --delta=auto: the filter is chosen from the first 16 MiB of the input (a histogram pass on the host predicts" << std::endl;
    std::cout << "              the size with and without it) -- at the W of --planes, or together with W where --planes=auto" << std::endl;
    std::cout << "--base        (compress) XOR the input with FILE, of exactly the input's length, first (at the width of --planes; alone: bytes):" << std::endl;
    std::cout << "              a file that is close to its base (the next checkpoint of a model) compresses several times smaller, an unrelated" << std::endl;
    std::cout << "              base makes it grow; implies --checksum; not together with --delta; the file then carries a trailer that says so;" << std::endl;
    std::cout << "              (decompress) the same FILE: required for a file written with --base (a wrong one is a checksum mismatch)," << std::endl;
    std::cout << "              refused for any other file" << std::endl;
    std::cout << "--base-auto   (compress, with --base=FILE) keep the base only if it is predicted to pay: the first 16 MiB of the input and of FILE are" << std::endl;
    std::cout << "              surveyed on the host as they are and XORed -- at the W of --planes, or together with W where --planes=auto, and W is" << std::endl;
    std::cout << "              then that of the bytes that get coded; a dropped base leaves the file of no --base at all" << std::endl;
    std::cout << "--stored      (compress) --stored or --stored=auto: a packet that the coder cannot shrink (its estimate says so: mantissa planes," << std::endl;
    std::cout << "              data that is already compressed) is kept raw behind its 4-byte header; --stored=off: every packet is coded (default)" << std::endl;
    std::cout << "--sparse      (compress) --sparse or --sparse=auto: a packet that is one byte value almost everywhere (what --base makes of" << std::endl;
    std::cout << "              everything that did not change) is kept as that byte and its exceptions: 8 bytes instead of 210 for an unchanged" << std::endl;
    std::cout << "              packet; --sparse=off: no such packets (default).  Either option: the file carries a trailer that says which packet is" << std::endl;
    std::cout << "              which, and decompress needs no flag to read it" << std::endl;
    std::cout << "--nointeractive no interactive mode" << std::endl;
}

}  // namespace

int main(int argc, char **argv) {
    bool decompress = false, host = false, help = argc <= 1, index = false, checksum = false;
    std::string in, out = "output.gip", base;
    bool has_in = false, planes_auto = false, delta = false, delta_auto = false, stored = false, sparse = false, base_auto = false;
    int device = -1, gpus = 0, threads = 1, planes = 1;
    long batch = 0;
    for (int i = 1; i < argc; ++i) {
        const char *v = nullptr;
        auto take = [&](const char **dst) {            // value after '=' or in the next argument
            if (*dst) return true;
            if (i + 1 < argc) {
                *dst = argv[++i];
                return true;
            }
            return false;
        };
        if (!std::strcmp(argv[i], "c")) {
        } else if (!std::strcmp(argv[i], "d")) {
            decompress = true;
        } else if (flag_name_is(argv[i], "help", &v)) {
            help = true;
        } else if (flag_name_is(argv[i], "host", &v)) {
            host = true;
        } else if (flag_name_is(argv[i], "index", &v)) {
            index = true;
        } else if (flag_name_is(argv[i], "checksum", &v)) {
            checksum = true;
        } else if (flag_name_is(argv[i], "delta", &v)) {
            delta_auto = v && !std::strcmp(v, "auto");
            delta = !v || !std::strcmp(v, "on") || delta_auto;
            if (!delta && std::strcmp(v, "off")) {
                std::cerr << "--delta takes on, off or auto: " << v << std::endl;
                return 2;
            }
        } else if (flag_name_is(argv[i], "stored", &v) || flag_name_is(argv[i], "sparse", &v)) {
            const bool is_stored = flag_name_is(argv[i], "stored", &v);
            const bool on = !v || !std::strcmp(v, "auto");
            if (!on && std::strcmp(v, "off")) {
                std::cerr << (is_stored ? "--stored" : "--sparse") << " takes auto or off: " << v << std::endl;
                return 2;
            }
            (is_stored ? stored : sparse) = on;
        } else if (flag_name_is(argv[i], "nointeractive", &v)) {
        } else if (flag_name_is(argv[i], "in", &v)) {
            if (!take(&v)) break;
            in = v;
            has_in = true;
        } else if (flag_name_is(argv[i], "out", &v)) {
            if (!take(&v)) break;
            out = v;
        } else if (flag_name_is(argv[i], "device", &v)) {
            if (!take(&v)) break;
            device = std::atoi(v);
        } else if (flag_name_is(argv[i], "gpus", &v)) {
            if (!take(&v)) break;
            gpus = std::atoi(v);
        } else if (flag_name_is(argv[i], "threads", &v)) {
            if (!take(&v)) break;
            threads = std::atoi(v);
        } else if (flag_name_is(argv[i], "planes", &v)) {
            if (!take(&v)) break;
            planes_auto = !std::strcmp(v, "auto");
            planes = planes_auto || !std::strcmp(v, "1") ? 1 : !std::strcmp(v, "2") ? 2 : !std::strcmp(v, "4") ? 4 : !std::strcmp(v, "8") ? 8 : 0;
            if (!planes) {
                std::cerr << "--planes takes 1, 2, 4, 8 or auto: " << v << std::endl;
                return 2;
            }
        } else if (flag_name_is(argv[i], "base-auto", &v)) {
            base_auto = true;
        } else if (flag_name_is(argv[i], "base", &v)) {
            if (!take(&v) || !*v) {
                std::cerr << "--base takes a file name" << std::endl;
                return 2;
            }
            base = v;
        } else if (flag_name_is(argv[i], "batch", &v)) {
            if (!take(&v)) break;
            batch = std::atol(v);
        } else {
            std::cerr << "Unknown argument: " << argv[i] << std::endl;
            return 2;
        }
    }
    if (help) {
        usage();
        return 0;
    }
    if (!base.empty() && delta) {
        std::cerr << "--base and --delta cannot be combined" << std::endl;
        return 2;
    }
    if (base_auto && (base.empty() || decompress)) {
        std::cerr << "--base-auto goes with c and --base=FILE" << std::endl;
        return 2;
    }
    try {
        if (!has_in) throw std::runtime_error("Please specify the input file name by command: --in filename");
        ProgressMonitor monitor;
        std::unique_ptr<Compressor> compressor;
        if (host) {
            auto *cpu = new CPUCompressor();
            cpu->setThreads(static_cast<unsigned>(threads < 0 ? 1 : threads));
            compressor.reset(cpu);
            std::cout << "Attention: execute kernel code on host." << std::endl;
        } else {
#ifdef GPUAR_HOST_ONLY
            (void)device; (void)gpus; (void)batch;
            throw std::runtime_error("this build (gpuar-host) has no GPU path: pass --host, or use gpuar");
#else
            auto *gpu = new GPUCompressor();
            compressor.reset(gpu);
            if (batch > 0) gpu->setBatchPackets(static_cast<size_t>(batch));
            if (device >= 0) {
                std::cout << "Choose GPU device: " << device << "." << std::endl;
                gpu->chooseDevice(device);
            } else if (gpus > 0) {
                std::cout << "Shard packets over " << gpus << " GPUs." << std::endl;
                gpu->useDevices(gpus);
            }
#endif
        }
        compressor->setWriteIndex(index);
        compressor->setWriteChecksum(checksum);
        compressor->setPlanes(planes);
        compressor->setDelta(delta && !delta_auto);
        compressor->setStored(stored);
        compressor->setSparse(sparse);
        compressor->setBaseFileName(base);
        compressor->setOpenFileName(in);
        compressor->setSaveFileName(out);
        CompressionInfo info;
        if (!decompress) {
            if (delta_auto) {
                unsigned long long plain[4], filtered[4];
                const bool on = compressor->chooseFilter(planes_auto, plain, filtered);
                std::cout << "delta=auto: filter " << (on ? "on" : "off") << ", width " << compressor->getPlanes()
                          << " (predicted bytes at widths 1, 2, 4, 8 without the filter: " << plain[0] << ", " << plain[1] << ", " << plain[2] << ", "
                          << plain[3] << "; with it: " << filtered[0] << ", " << filtered[1] << ", " << filtered[2] << ", " << filtered[3] << ")"
                          << std::endl;
            } else if (base_auto) {
                unsigned long long plain[4], xored[4];
                const bool kept = compressor->chooseBase(planes_auto, plain, xored);
                std::cout << "base-auto: base " << (kept ? "kept" : "dropped") << ", width " << compressor->getPlanes()
                          << " (predicted bytes at widths 1, 2, 4, 8 without the base: " << plain[0] << ", " << plain[1] << ", " << plain[2] << ", "
                          << plain[3] << "; against it: " << xored[0] << ", " << xored[1] << ", " << xored[2] << ", " << xored[3] << ")" << std::endl;
            } else if (planes_auto) {
                unsigned long long total[4];
                const int w = compressor->choosePlanes(total);
                std::cout << "planes=auto: width " << w << " (predicted bytes at widths 1, 2, 4, 8: " << total[0] << ", " << total[1] << ", "
                          << total[2] << ", " << total[3] << ")" << std::endl;
            }
            std::cout << "Start to compress " << in << " to " << out << "." << std::endl;
            info = compressor->compress(&monitor);
        } else {
            std::cout << "Start to decompress " << in << " to " << out << "." << std::endl;
            info = compressor->decompress(&monitor);
        }
        const double ratio = static_cast<double>(info.compressedFileSize) / info.uncompressedFileSize;
        std::cout << "Complete" << std::endl << std::endl;
        std::cout << "Statistics: " << std::endl;
        std::cout << "Uncompressed file size " << info.uncompressedFileSize << " bytes" << std::endl;
        std::cout << "Compressed file size  " << info.compressedFileSize << " bytes" << std::endl;
        std::cout << "Compression ratio     " << ratio << std::endl;
        std::cout << "Compute time          " << info.processTime / 1000 << " s" << std::endl;
        std::cout << "I/O time              " << info.ioTime / 1000 << " s" << std::endl;
        std::cout << "Score                 " << (1000 / (std::pow(ratio, 0.6) * std::pow(info.processTime / 1000, 0.4)))
                  << std::endl;
        // The files are closed and the statistics printed: leave without tearing the GPU context down buffer by buffer
        // (unpinning and freeing a few GiB takes a tenth of a second the user would wait for; the process is ending anyway).
        // (GPUAR_NO_FAST_EXIT=1 keeps the ordinary exit path: a profiler writes its files from an exit handler)
        if (!std::getenv("GPUAR_NO_FAST_EXIT")) {
            std::cout.flush();
            std::cerr.flush();
            (void)compressor.release();
            std::_Exit(0);
        }
    } catch (const std::exception &e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
    return 0;
}
