// gip_read_client.cpp -- a stand-alone caller of the two host readers of include/gpuar_hip.h (gpuar_hip_gip_read_host,
// gpuar_hip_gip_tables_host), for a build with -fsanitize=address,undefined: tests/test_gip_read_host.py compiles this file together
// with gpuar_amd/csrc/host/gip_read.cpp into tests/_build/ and runs it over the same good and damaged files it gives the library.
//
//   gip_read_client FILE...      one line per file:  <code> | info[0] .. info[9] | clen ... | crc ... | kind ...
// (the tables only where the code is 0; "-" for a table the file does not have).  Every file is read into a heap block of exactly
// its size, so that a read past either end of it is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpuar_hip.h"

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        FILE *f = std::fopen(argv[i], "rb");
        if (!f) {
            std::fprintf(stderr, "cannot open %s\n", argv[i]);
            return 2;
        }
        std::fseek(f, 0, SEEK_END);
        const size_t n = static_cast<size_t>(std::ftell(f));
        std::fseek(f, 0, SEEK_SET);
        uint8_t *file = static_cast<uint8_t *>(std::malloc(n ? n : 1));
        if (n && std::fread(file, n, 1, f) != 1) {
            std::fprintf(stderr, "cannot read %s\n", argv[i]);
            return 2;
        }
        std::fclose(f);
        uint64_t info[GPUAR_GIP_INFO_WORDS];
        const int code = gpuar_hip_gip_read_host(file, n, info);
        std::printf("%d |", code);
        for (int k = 0; k < GPUAR_GIP_INFO_WORDS; ++k) std::printf(" %llu", static_cast<unsigned long long>(info[k]));
        if (code == GPUAR_OK) {
            const size_t packets = static_cast<size_t>(info[4]);
            const bool has_crcs = (info[6] & 1u) != 0, has_kinds = info[3] == 6;
            std::vector<uint16_t> clen(packets);
            std::vector<uint32_t> crc(packets);
            std::vector<uint8_t> kind(packets);
            const int again = gpuar_hip_gip_tables_host(file, n, clen.data(), has_crcs ? crc.data() : nullptr, has_kinds ? kind.data() : nullptr, packets);
            if (again != GPUAR_OK) {
                std::fprintf(stderr, "%s: the tables give %d, the read gave 0\n", argv[i], again);
                return 3;
            }
            std::printf(" |");
            for (size_t p = 0; p < packets; ++p) std::printf(" %u", clen[p]);
            std::printf(" |");
            if (!has_crcs) std::printf(" -");
            for (size_t p = 0; has_crcs && p < packets; ++p) std::printf(" %u", crc[p]);
            std::printf(" |");
            if (!has_kinds) std::printf(" -");
            for (size_t p = 0; has_kinds && p < packets; ++p) std::printf(" %u", kind[p]);
        }
        std::printf("\n");
        std::free(file);
    }
    return 0;
}
