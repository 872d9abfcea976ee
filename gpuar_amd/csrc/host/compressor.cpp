#include "compressor.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdlib>
#include <vector>

#include "../delta_survey.h"
#include "../xor_survey.h"
#include "gpuar_hip.h"

namespace gip {

// The reference checks its packet geometry at construction time
// (src/compressor.cpp:8-16); here the same facts are compile-time.
static_assert(GPUAR_PACKET_BYTES % 16 == 0, "packets are read 16 bytes at a time");
static_assert(GPUAR_PACKET_BYTES < (1u << 14) - 257u, "model total must stay below 2^14 (coder precision 16 bits)");

Compressor::Compressor() {}

Compressor::~Compressor() { closeFiles(); }

void Compressor::openFiles(bool truncate_output) {
    openFile = std::fopen(openFileName.c_str(), "rb");
    if (!openFile) throw std::runtime_error("Can not open input file: " + openFileName);
    if (truncate_output) {
        saveFile = std::fopen(saveFileName.c_str(), "wb");
    } else {
        const int fd = ::open(saveFileName.c_str(), O_CREAT | O_WRONLY, 0666);
        saveFile = fd < 0 ? nullptr : ::fdopen(fd, "wb");
        if (fd >= 0 && !saveFile) ::close(fd);
    }
    if (!saveFile) {
        closeFiles();
        throw std::runtime_error("Can not open output file: " + saveFileName);
    }
}

size_t Compressor::getFileSize(FILE *stream) {
    const long at = std::ftell(stream);
    std::fseek(stream, 0, SEEK_END);
    const long end = std::ftell(stream);
    std::fseek(stream, at, SEEK_SET);
    return end < 0 ? 0 : static_cast<size_t>(end);
}

std::vector<uint8_t> Compressor::readSurveyPrefix() const {
    const int fd = ::open(openFileName.c_str(), O_RDONLY);
    if (fd < 0) throw std::runtime_error("Can not open input file: " + openFileName);
    std::vector<uint8_t> head(kSurveyPrefix);
    size_t n = 0;
    while (n < head.size()) {
        const ssize_t got = ::pread(fd, head.data() + n, head.size() - n, static_cast<off_t>(n));
        if (got < 0) {
            ::close(fd);
            throw std::runtime_error("Can not read input file: " + openFileName);
        }
        if (got == 0) break;
        n += static_cast<size_t>(got);
    }
    ::close(fd);
    head.resize(n);
    return head;
}

// the four totals of a survey's rows
static void survey_totals(const std::vector<uint32_t> &est, size_t n_packets, uint64_t sums[4], unsigned long long total[4]) {
    for (uint32_t j = 0; j < gpuar::kSurveyWidths; ++j) {
        sums[j] = 0;
        for (size_t p = 0; p < n_packets; ++p) sums[j] += est[j * n_packets + p];
        total[j] = sums[j];
    }
}

int Compressor::choosePlanes(unsigned long long total[4]) {
    const std::vector<uint8_t> head = readSurveyPrefix();
    const size_t n_packets = (head.size() + GPUAR_PACKET_BYTES - 1) / GPUAR_PACKET_BYTES;
    std::vector<uint32_t> est(gpuar::kSurveyWidths * n_packets);
    gpuar::survey_host(head.data(), head.size(), est.data(), n_packets);
    uint64_t sums[gpuar::kSurveyWidths];
    survey_totals(est, n_packets, sums, total);
    planes = static_cast<int>(gpuar::choose_width(sums, n_packets));
    return planes;
}

bool Compressor::chooseFilter(bool choose_width_too, unsigned long long plain[4], unsigned long long filtered[4]) {
    if (based()) throw std::runtime_error("--base together with --delta is not supported");
    const std::vector<uint8_t> head = readSurveyPrefix();
    const size_t n_packets = (head.size() + GPUAR_PACKET_BYTES - 1) / GPUAR_PACKET_BYTES;
    std::vector<uint32_t> est(gpuar::kSurveyWidths * n_packets);
    uint64_t sums_plain[gpuar::kSurveyWidths], sums_filtered[gpuar::kSurveyWidths];
    gpuar::survey_host(head.data(), head.size(), est.data(), n_packets);
    survey_totals(est, n_packets, sums_plain, plain);
    gpuar::delta_survey_host(head.data(), head.size(), gpuar::kSurveyAllWidths, est.data(), n_packets);
    survey_totals(est, n_packets, sums_filtered, filtered);
    if (choose_width_too) {
        const gpuar::FilterChoice c = gpuar::choose_filter(sums_plain, sums_filtered, n_packets);
        planes = static_cast<int>(c.width);
        delta = c.filter;
    } else {
        const uint32_t j = gpuar::survey_row(static_cast<uint32_t>(planes));
        delta = n_packets != 0 && sums_filtered[j] + n_packets <= sums_plain[j];
    }
    return delta;
}

bool Compressor::chooseBase(bool choose_width_too, unsigned long long plain[4], unsigned long long xored[4]) {
    if (!based()) throw std::runtime_error("--base-auto needs --base=FILE");
    const std::vector<uint8_t> head = readSurveyPrefix();
    struct stat st;
    if (::stat(openFileName.c_str(), &st) != 0) throw std::runtime_error("Can not open input file: " + openFileName);
    openBase(static_cast<uint64_t>(st.st_size), "the input");
    std::vector<uint8_t> base(head.size());
    if (!base.empty()) readBase(base.data(), base.size(), 0);
    ::close(baseFd);
    baseFd = -1;
    const size_t n_packets = (head.size() + GPUAR_PACKET_BYTES - 1) / GPUAR_PACKET_BYTES;
    std::vector<uint32_t> est(gpuar::kSurveyWidths * n_packets);
    uint64_t sums_plain[gpuar::kSurveyWidths], sums_xored[gpuar::kSurveyWidths];
    gpuar::survey_host(head.data(), head.size(), est.data(), n_packets);
    survey_totals(est, n_packets, sums_plain, plain);
    gpuar::xor_survey_host(head.data(), base.data(), head.size(), est.data(), nullptr, n_packets);
    survey_totals(est, n_packets, sums_xored, xored);
    bool keep = false;
    if (choose_width_too) {
        const gpuar::FilterChoice c = gpuar::choose_filter(sums_plain, sums_xored, n_packets);
        planes = static_cast<int>(c.width);
        keep = c.filter;
    } else {
        const uint32_t j = gpuar::survey_row(static_cast<uint32_t>(planes));
        keep = n_packets != 0 && sums_xored[j] + n_packets <= sums_plain[j];
    }
    if (!keep) setBaseFileName("");
    return keep;
}

void Compressor::openBase(uint64_t expect, const char *what) {
    if (delta) throw std::runtime_error("--base together with --delta is not supported");
    if (baseFd >= 0) ::close(baseFd);
    baseFd = ::open(baseFileName.c_str(), O_RDONLY);
    struct stat st;
    if (baseFd < 0 || ::fstat(baseFd, &st) != 0) throw std::runtime_error("Can not open base file: " + baseFileName);
    if (static_cast<uint64_t>(st.st_size) != expect)
        throw std::runtime_error("The base file holds " + std::to_string(st.st_size) + " bytes, " + what + " " + std::to_string(expect) +
                                 ": --base takes a file of exactly that length");
}

void Compressor::readBase(uint8_t *dst, size_t n, uint64_t at) {
    for (size_t done = 0; done < n;) {
        const ssize_t got = ::pread(baseFd, dst + done, n - done, static_cast<off_t>(at + done));
        if (got <= 0) throw std::runtime_error("Read base file failed");
        done += static_cast<size_t>(got);
    }
}

void Compressor::closeFiles() {
    if (baseFd >= 0) ::close(baseFd);
    baseFd = -1;
    if (saveFile) std::fclose(saveFile);
    if (openFile) std::fclose(openFile);
    saveFile = openFile = nullptr;
}

// src/compressor.cpp:28-44: `size` bytes of rand() output, 4 at a time
void Compressor::generateRandomFile(const size_t size) {
    saveFile = std::fopen(saveFileName.c_str(), "wb");
    if (!saveFile) throw std::runtime_error("Can not open output file: " + saveFileName);
    for (size_t i = 0; i < size; i += 4) {
        const int d = std::rand();
        if (std::fwrite(&d, sizeof d, 1, saveFile) != 1) {
            closeFiles();
            throw std::runtime_error("Write raw data to file failed");
        }
    }
    closeFiles();
}

}  // namespace gip
