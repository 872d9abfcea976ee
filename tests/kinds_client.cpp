// kinds_client.cpp -- one GPUCompressor object through jobs in both directions with --stored / --sparse on and off: its lanes'
// buffers outlive a job, and the next job may need what the last one never allocated (tests/test_gpu_kinds.py).
//
//   kinds_client IN DIR
//
// compresses IN with both options, decompresses that, compresses IN plainly, decompresses the version-6 file again, compresses
// with both options again -- all with the same object -- and prints "ok" when every output is what it should be.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

#include "gpu_compressor.hpp"

using namespace gip;

static std::vector<char> slurp(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const std::string in = argv[1], dir = argv[2];
    try {
        GPUCompressor gpu;
        ProgressMonitor monitor;
        gpu.setBatchPackets(64);
        auto job = [&](bool compress, bool kinds, const std::string &from, const std::string &to) {
            gpu.setStored(kinds);
            gpu.setSparse(kinds);
            gpu.setOpenFileName(from);
            gpu.setSaveFileName(to);
            if (compress) gpu.compress(&monitor);
            else gpu.decompress(&monitor);
        };
        job(true, true, in, dir + "/a.gip");
        job(false, false, dir + "/a.gip", dir + "/a.back");
        job(true, false, in, dir + "/b.gip");
        job(false, false, dir + "/a.gip", dir + "/a2.back");
        job(false, false, dir + "/b.gip", dir + "/b.back");
        job(true, true, in, dir + "/c.gip");
        const std::vector<char> x = slurp(in);
        const bool ok = slurp(dir + "/a.back") == x && slurp(dir + "/a2.back") == x && slurp(dir + "/b.back") == x &&
                        slurp(dir + "/a.gip") == slurp(dir + "/c.gip") && slurp(dir + "/a.gip") != slurp(dir + "/b.gip");
        std::cout << std::endl << (ok ? "ok" : "mismatch") << std::endl;
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
