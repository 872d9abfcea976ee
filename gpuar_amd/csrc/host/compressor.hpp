// compressor.hpp -- abstract base of the two compressors, API as
// src/compressor.hpp:10-65 (setOpenFileName, setSaveFileName, compress,
// decompress, closeFiles, getFileSize, generateRandomFile).  Unlike the
// reference's base class (src/compressor.cpp:23-25, cudaMallocHost) it touches
// no GPU runtime, so `--host` works on a machine without one.
#pragma once
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "compress_info.hpp"
#include "file_header.hpp"
#include "packet_index.hpp"
#include "progress_monitor.hpp"

namespace gip {

// millisecond stopwatch with start/stop accumulation (the role of StopWatchInterface)
class StopWatch {
  public:
    void reset() { total_ms = 0; }
    void start() { t0 = clock::now(); }
    void stop() { total_ms += std::chrono::duration<double, std::milli>(clock::now() - t0).count(); }
    double value() const { return total_ms; }

  private:
    using clock = std::chrono::steady_clock;
    clock::time_point t0;
    double total_ms = 0;
};

// What the packets of one job go through between the file's bytes and the coder, whichever way the job runs and on whichever
// path: built from the compressor's options for a compress job (Compressor::plan) and from the file's trailer for a decompress job
// (PacketPlan::of), and nowhere else.
struct PacketPlan {
    uint32_t elem = 1;       // the element width, 1, 2, 4 or 8: the packets hold byte planes of elements this wide (../planes.h)
    bool delta = false;      // ... of the elements' differences (../delta.h)
    bool based = false;      // ... of the bytes XORed with a base (../xorbase.h)
    bool crcs = false;       // the CRC-32 of every packet's original bytes is written, or verified
    bool stored = false, sparse = false;      // compress: a packet may be kept raw, or sparse (../kinds.h)
    bool kinds = false;      // the file carries a kind per packet
    // whether what is coded differs from what is read or written: XOR, else delta, else planes, else nothing
    bool transforms() const { return elem > 1 || delta || based; }
    // (the fields in their order)
    static PacketPlan of(const Trailer &t) { return {t.elem_bytes, t.filtering(), t.based(), t.verify(), false, false, t.mixed()}; }
};

class Compressor {
  protected:
    std::string openFileName;
    std::string saveFileName;
    StopWatch process_timer;
    StopWatch io_timer;
    FILE *openFile = nullptr;
    FILE *saveFile = nullptr;
    bool writeIndex = false;          // append the packet-offset index trailer (packet_index.hpp)
    bool writeChecksum = false;       // append the trailer with per-packet CRC-32s (version 2), which decompress verifies
    int planes = 1;                   // compress: split the input into byte planes of elements this wide (../planes.h) and say so in a
                                      // version-3 trailer, from which decompress learns the width; 1: no transform, no such trailer
    bool delta = false;               // compress: replace the elements (`planes` bytes wide; 1 too) of every group by their differences
                                      // before the split (../delta.h) and say so in a version-4 trailer
    std::string baseFileName;         // compress: XOR the input with this file of the same length before the split (../xorbase.h) and say
                                      // so in a version-5 trailer, with CRCs; decompress: the base a version-5 file needs
    int baseFd = -1;                  // ... open while a job runs (openBase)
    bool checksumAsked = false;       // what setWriteChecksum was given: a base turns writeChecksum on by itself
    bool stored = false;              // compress (`--stored=auto`): a packet whose estimate says it does not shrink is kept raw, and
    bool sparse = false;              // (`--sparse=auto`) one that is a single byte value almost everywhere as that byte and its exceptions
                                      // (../kinds.h); either says so in a version-6 trailer, whatever the packets turn out to be

    // the first min(file size, kSurveyPrefix) bytes of the input, from one pread: what choosePlanes and chooseFilter survey
    std::vector<uint8_t> readSurveyPrefix() const;

    // the error a decompress raises for a packet whose decoded bytes do not match the CRC-32 of its trailer
    static std::runtime_error checksumError(size_t packet, uint64_t begin, uint64_t end) {
        return std::runtime_error("Checksum mismatch: packet " + std::to_string(packet) + " (uncompressed bytes " + std::to_string(begin) +
                                  " .. " + std::to_string(end) + ") does not decode to what was compressed");
    }
    // a trailer that says the file holds byte planes but cannot be used: going on would hand back the split bytes
    static std::runtime_error planesTrailerError() {
        return std::runtime_error("Incorrect file format: the trailer says the file holds byte planes (version 3) but it is damaged, "
                                  "carries a width other than 2, 4 or 8, or carries flags this gpuar does not know");
    }
    // the same for a trailer that says the file went through the delta filter: going on would hand back differences
    static std::runtime_error deltaTrailerError() {
        return std::runtime_error("Incorrect file format: the trailer says the file holds delta-filtered elements (version 4) but it is damaged, "
                                  "carries a width other than 1, 2, 4 or 8, lacks the delta flag, or carries flags this gpuar does not know");
    }
    // the same for a trailer that says the file was XORed with a base: going on would hand back the XOR
    static std::runtime_error baseTrailerError() {
        return std::runtime_error("Incorrect file format: the trailer says the file was XORed with a base (version 5) but it is damaged, "
                                  "carries a width other than 1, 2, 4 or 8, lacks the base flag or the checksums, or carries flags this gpuar does not know");
    }
    // the same for a trailer that says which packets are raw or sparse: going on would feed raw bytes to the decoder
    static std::runtime_error kindsTrailerError() {
        return std::runtime_error("Incorrect file format: the trailer says the file holds raw or sparse packets (version 6) but it is damaged, "
                                  "carries a width other than 1, 2, 4 or 8, a packet kind above 2, lacks the kinds flag, or carries flags this gpuar does not know");
    }
    static std::runtime_error planesPacketError(size_t packet) {
        return std::runtime_error("Incorrect file format: packet " + std::to_string(packet) + " of a file of byte planes is not the last one and "
                                  "does not hold 8192 bytes");
    }
    static void warnMalformedTrailer() {
        std::fprintf(stderr, "Warning: ignoring a malformed checksum trailer: nothing was verified\n");
    }

    // The trailer of the open .gip (packet_index.hpp), empty when there is none a reader may use: one that says version 3 and
    // cannot be used is an error, one that says version 2 and does not fit a warning.  A version-5 file needs the base it was
    // compressed against (setBaseFileName), any other file refuses one: both are errors before anything is written.
    Trailer loadTrailer(size_t stream_end, size_t fileSize) {
        Trailer trailer;
        const Trailer::Status status = Trailer::load(openFile, FileHeader::HEADER_LENGTH, stream_end, fileSize, trailer);
        if (status == Trailer::Status::unusable) throw planesTrailerError();
        if (status == Trailer::Status::unusable_delta) throw deltaTrailerError();
        if (status == Trailer::Status::unusable_base) throw baseTrailerError();
        if (status == Trailer::Status::unusable_kinds) throw kindsTrailerError();
        if (trailer.based() && !based())
            throw std::runtime_error("This file was compressed against a base (trailer version " + std::to_string(trailer.version) + "): pass the same file with --base=FILE");
        if (!trailer.based() && based())
            throw std::runtime_error("--base was given, but this file was not compressed against a base (no version-5 trailer)");
        if (status == Trailer::Status::malformed) warnMalformedTrailer();
        return trailer;
    }
    // compress: whether the options ask for a trailer, and that trailer appended at the current position of the output
    bool based() const { return !baseFileName.empty(); }
    PacketPlan plan() const { return {static_cast<uint32_t>(planes), delta, based(), writeChecksum, stored, sparse, stored || sparse}; }
    bool wantsTrailer() const { return writeIndex || plan().crcs || plan().transforms() || plan().kinds; }
    // `crcs`, `kinds`: of every packet, read only where the plan has them
    void saveTrailer(const PacketPlan &plan, const std::vector<uint16_t> &clens, const std::vector<uint32_t> &crcs, const std::vector<uint8_t> &kinds) {
        if (wantsTrailer()) Trailer::save(saveFile, clens, plan.elem, plan.crcs ? &crcs : nullptr, plan.delta, plan.based, plan.kinds ? &kinds : nullptr);
    }
    // Opens the base file and checks that it holds exactly `expect` bytes (those of `what`); with the delta filter on it throws:
    // that combination is not built.  closeFiles() closes it.
    void openBase(uint64_t expect, const char *what);
    // base[at .. at + n) -> dst, or throws
    void readBase(uint8_t *dst, size_t n, uint64_t at);
    static constexpr size_t kPacketBytes = 8192;
    // What a trailer of `n_packets` packets says of the bytes that packet `packet` of the file holds by its header (`ulen`).
    // Byte planes: every packet but the file's last holds 8192 bytes, or the groups are not where the merge takes them to be.
    static void checkPlanesPacket(size_t packet, size_t n_packets, size_t ulen) {
        if (packet + 1 < n_packets && ulen != kPacketBytes) throw planesPacketError(packet);
    }
    // CRCs: they cover the packets' original bytes, all 8192 long but the file's last, which holds 1 .. 8192: a packet that says
    // otherwise does not decode to them.
    static void checkChecksumPacket(size_t packet, size_t n_packets, size_t ulen) {
        const uint64_t begin = static_cast<uint64_t>(packet) * kPacketBytes;
        if (packet + 1 < n_packets ? ulen != kPacketBytes : ulen == 0) throw checksumError(packet, begin, begin + (ulen < kPacketBytes ? ulen : kPacketBytes));
    }

    // where the packets of an open .gip end: the header's size field when it is sane (the reference's
    // reading, src/cpu_compressor.cpp:47-56), else the end of the file
    static size_t streamEnd(const CompressionInfo &info, size_t fileSize) {
        const size_t claimed = info.compressedFileSize;
        return claimed >= 20 && claimed <= fileSize ? claimed : fileSize;
    }

    // throws std::runtime_error naming the file.  truncate_output = false: an existing output file keeps its pages
    // (dropping 8 GiB of page cache costs most of a second); the caller sets the final length itself
    void openFiles(bool truncate_output = true);

  public:
    Compressor();
    virtual ~Compressor();

    size_t getFileSize(FILE *stream);
    void setOpenFileName(const std::string &fileName) { openFileName = fileName; }
    void setSaveFileName(const std::string &fileName) { saveFileName = fileName; }
    void setWriteIndex(bool on) { writeIndex = on; }
    void setWriteChecksum(bool on) {
        checksumAsked = on;
        writeChecksum = on || based();
    }
    void setPlanes(int elem_bytes) {
        if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8) throw std::invalid_argument("planes: the element width is 1, 2, 4 or 8");
        planes = elem_bytes;
    }
    void setDelta(bool on) { delta = on; }
    void setStored(bool on) { stored = on; }
    void setSparse(bool on) { sparse = on; }
    int getPlanes() const { return planes; }
    // compress: XOR against this file (implies the checksums); decompress: the base of a version-5 file.  Empty: none.
    void setBaseFileName(const std::string &fileName) {
        baseFileName = fileName;
        writeChecksum = checksumAsked || based();
    }
    // `--planes=auto`: sets the width from the input's own bytes and returns it -- gpuar::choose_width of the totals that
    // gpuar::survey_host (../survey.h) predicts for the first min(file size, kSurveyPrefix) bytes taken as a buffer of their own,
    // written to total[4] (widths 1, 2, 4, 8).  On the host, from one pread, before either pipeline starts: the prefix is a
    // constant, so the file written does not depend on --batch, --gpus, --threads or --host.
    static constexpr size_t kSurveyPrefix = size_t(16) << 20;
    int choosePlanes(unsigned long long total[4]);
    // `--delta=auto`: sets the filter -- and with choose_width_too (`--planes=auto` as well) the width -- from the same prefix, and
    // returns the filter.  plain[4] are the totals of gpuar::survey_host, filtered[4] those of gpuar::delta_survey_host
    // (../delta_survey.h: the prefix filtered and split at widths 1, 2, 4, 8).  With the width fixed the filter is on iff
    // filtered[W] + packets <= plain[W], the rule of batch.compress(delta="auto"); with both open it is gpuar::choose_filter.
    // On the host, before either pipeline starts, as choosePlanes.
    bool chooseFilter(bool choose_width_too, unsigned long long plain[4], unsigned long long filtered[4]);
    // `--base-auto`: keeps or drops the base -- and with choose_width_too (`--planes=auto` as well) sets the width -- from the same
    // prefix of the input and the same byte range of the base, and returns whether the base is kept.  plain[4] are the totals of
    // gpuar::survey_host, xored[4] those of gpuar::xor_survey_host (../xor_survey.h: the prefix XORed with the base and split at
    // widths 1, 2, 4, 8).  With the width fixed the base is kept iff xored[W] + packets <= plain[W], the rule of
    // batch.compress(base_auto=...); with both open it is gpuar::choose_filter with the base in the filter's place.  A dropped base
    // is forgotten (setBaseFileName("")): the file is that of no --base at all, the implied checksums included.  The base must have
    // the input's length, kept or not.  On the host, before either pipeline starts, as choosePlanes.
    bool chooseBase(bool choose_width_too, unsigned long long plain[4], unsigned long long xored[4]);
    virtual CompressionInfo compress(ProgressMonitor *monitor) = 0;
    virtual CompressionInfo decompress(ProgressMonitor *monitor) = 0;
    void closeFiles();
    void generateRandomFile(const size_t size);
};

}  // namespace gip
