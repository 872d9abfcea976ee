// packet_plan_test.cpp -- what PacketPlan::of (gpuar_amd/csrc/host/compressor.hpp) makes of every trailer Trailer::load accepts,
// beside what the Trailer says of itself.  tests/test_packet_plan.py writes the files and holds the lines to the format.
//
//   packet_plan_test CASES      CASES: .gip files back to back, each behind a u64 LE with its length; one line per file:
//       <status of Trailer::load, 1 = ok> <version> <merging()> | <elem> <delta> <based> <crcs> <stored> <sparse> <kinds> <transforms()>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "compressor.hpp"

int main(int argc, char **argv) {
    FILE *cases = argc == 2 ? std::fopen(argv[1], "rb") : nullptr;
    if (!cases) return 2;
    uint8_t word[8];
    while (std::fread(word, sizeof word, 1, cases) == 1) {
        uint64_t n = 0;
        for (int b = 0; b < 8; ++b) n |= static_cast<uint64_t>(word[b]) << (8 * b);
        std::vector<uint8_t> file(n);
        if (n < gip::FileHeader::HEADER_LENGTH || std::fread(file.data(), n, 1, cases) != 1) return 3;
        // where the packets end: the header's field when it is sane, else the end of the file (Compressor::streamEnd)
        uint64_t claimed = 0;
        for (int b = 0; b < 8; ++b) claimed |= static_cast<uint64_t>(file[12 + b]) << (8 * b);
        const uint64_t stream_end = claimed >= gip::FileHeader::HEADER_LENGTH && claimed <= n ? claimed : n;
        FILE *f = fmemopen(file.data(), n, "rb");
        if (!f) return 3;
        gip::Trailer t;
        const gip::Trailer::Status status = gip::Trailer::load(f, gip::FileHeader::HEADER_LENGTH, stream_end, n, t);
        std::fclose(f);
        const gip::PacketPlan plan = gip::PacketPlan::of(t);
        std::printf("%d %u %d | %u %d %d %d %d %d %d %d\n", static_cast<int>(status), t.version, t.merging(), plan.elem, plan.delta, plan.based, plan.crcs,
                    plan.stored, plan.sparse, plan.kinds, plan.transforms());
    }
    std::fclose(cases);
    return 0;
}
