// gpu_compressor.cpp -- host pipeline of the GPU path.
//
// The reference moves one 8704-byte packet per memcpy and per fwrite, all on one thread
// (/root/reference/src/gpu_compressor.cpp:134-171, 280-340).  Here the file is cut into CHUNKS of
// whole packets (a multiple of 64; by default large enough to fill the chip: 65536 packets = 512 MiB
// of input = 1024 wavefronts) and every chunk goes down a lane:
//
//     input file, MAPPED and registered for DMA: H2D straight out of the page cache (no pread, no staging copy;
//         if the file cannot be mapped or registered: pread into the lane's pinned pieces instead)
//       -> kernels (+ device-side compaction when compressing)
//       -> D2H in PIECES of 64 MiB into the lane's two pinned buffers
//       -> the writer thread: one stream of pwrite()s, each cut into slices on a few helper threads
//
// Each GPU runs kLanesPerDevice lanes at once, each a host thread with its own non-blocking HIP stream,
// device buffers, pinned pieces and status word, so the copies and kernels of one chunk overlap the
// draining of another.  The file is cut into contiguous packet ranges (chunks) in file order, sized so that every lane of
// every device gets one (ensureBuffers: at most ceil(packets / (G * lanes)) packets each, whole wavefronts), and chunk c
// goes to device c mod G: the packet-range sharding of SURVEY.md section 8(e) at CHUNK grain -- every device codes the same
// number of chunks to within one, hence the same bytes to within one chunk -- dealt in file order because the one writer
// consumes in file order (one contiguous range per device would have devices 1..G-1 finish their first chunks and then hold
// them, pinned, until the writer is through all of device 0's range).  What bounds the wall time
// on a page-cached file is the ONE thing that cannot be spread: buffered writes to a single file are
// serialised by the file system (tools/io_probe.cpp: ~9-11 GB/s into a new file whatever the number of
// threads, against 57 GB/s per direction over PCIe and 76+ GB/s of pread), so the pipeline is built to keep
// exactly that writer busy from the first piece to the last.  The only serial quantity besides it is the
// running output offset of the compressor, which the ordered writer carries by itself.
// Decoding works the same way in the other direction; where the packets of a chunk start is known from the
// index trailer (packet_index.hpp) or from a scanner thread that walks the packet headers through the mapping
// (`off += clen`, 4 bytes per packet) ahead of the lanes.  The files produced are byte-identical to those
// of the reference's loop from byte 20 on.
//
// What never touches the HIP runtime -- the trace, sliced file I/O, the writer and its pieces, the chunk map, the chunks' turn at
// the output offset, the first failure -- lives in pipeline_parts.hpp and is tested on the CPU.  What a job's packets go through
// (element width, delta, base, CRCs, raw and sparse packets) is one PacketPlan (compressor.hpp), built from the options when
// compressing and from the trailer when decompressing; a lane's buffers are prepared for it and its chunks coded by it.
#include "gpu_compressor.hpp"

#include <fcntl.h>
#include <hip/hip_runtime_api.h>
#include <sys/mman.h>
#include <sys/stat.h>

#include <cstring>

#include "gpuar_hip.h"
#include "input_guard.hpp"
#include "pipeline_parts.hpp"

namespace gip {

using namespace pipeline;

namespace {

constexpr size_t kPacket = GPUAR_PACKET_BYTES;
constexpr size_t kSlot = GPUAR_SLOT_BYTES;
constexpr size_t kLanesPerDevice = 3;      // chunks in flight per GPU
constexpr size_t kPieceBytes = 64u << 20;  // what one D2H copy / one pwrite moves
constexpr size_t kPiecesPerLane = 2;       // pinned buffers per lane: one being filled while the other is written

void hip_check(hipError_t e, const char *what) {
    // same message shape as src/gpu_compressor.cpp:189-192
    if (e != hipSuccess) throw std::runtime_error(std::string("Fail to execute kernel code: ") + what + ": " + hipGetErrorString(e));
}
void gpuar_check(int code, const char *what) {
    if (code != GPUAR_OK) throw std::runtime_error(std::string("Fail to execute kernel code: ") + what + ": " + gpuar_hip_error_string(code));
}

// The input file mapped read-only and registered with the HIP runtime, so that hipMemcpyAsync reads the page
// cache directly (tools/io_probe.cpp: 57 GB/s, the same as from hipHostMalloc memory, with no copy on the CPU).
// Registration costs ~15 ms per GiB and is therefore done window by window (256 MiB), by the lane that is about
// to copy from the window, while the other lanes and the writer are already at work -- registering an 8 GiB file
// in one go would hold the whole pipeline up for 0.12 s.  The FIRST registration of a process costs ~35 ms whatever its
// size: the jobs start it on a thread of its own, next to the lanes' buffer allocation (warmFirstWindow).  `data() == nullptr` means the file could not be mapped,
// `require()` returning false that a window could not be registered: callers fall back to pread.
class MappedInput {
  public:
    ~MappedInput() { close(); }
    void open(int fd, size_t bytes) {
        close();
        if (bytes == 0 || std::getenv("GPUAR_NO_MMAP")) return;
        void *m = ::mmap(nullptr, bytes, PROT_READ, MAP_SHARED, fd, 0);
        if (m == MAP_FAILED) return;
        base = static_cast<const uint8_t *>(m);
        size = bytes;
        guard = InputGuard::watch(base, size);     // a file cut short under the mapping: zeros and a mark instead of SIGBUS (input_guard.hpp)
        (void)::madvise(m, bytes, MADV_SEQUENTIAL);
        state.assign((bytes + kWindow - 1) / kWindow, 0);
        users.assign(state.size(), 0);
        live = 0;
        frontier = 0;
        if (const char *cap = std::getenv("GPUAR_MAX_WINDOWS")) max_live = std::max<size_t>(1, std::strtoul(cap, nullptr, 10));
        // (tests only: time for somebody to cut the file short between the mapping and the first read of it;
        // and says on stderr that it is there, so the test need not guess how long start-up took)
        if (const char *hold = std::getenv("GPUAR_TEST_HOLD_AFTER_MAP_MS")) {
            std::fprintf(stderr, "[gpuar] input mapped\n");
            std::fflush(stderr);
            ::usleep(1000u * static_cast<useconds_t>(std::strtoul(hold, nullptr, 10)));
        }
    }
    // makes [at, at + n) DMA-able and counts the caller as a user of its windows until release(at, n);
    // false: this file cannot be registered (the caller reads it with pread instead, and owes no release)
    bool require(uint64_t at, size_t n) {
        if (!base || n == 0) return base != nullptr;
        std::unique_lock<std::mutex> hold(lock);
        if (refused) return false;
        const size_t first = at / kWindow, last = (at + n - 1) / kWindow;
        // The caller counts as a user of EVERY window of its range before anything below can wait: dropped.wait() lets go of
        // the lock, and a release() on another lane only ever marks windows with no users -- so a window of this range that is
        // already registered cannot be taken away while a later one is waited for (with the count taken after the
        // loop, a chunk straddling a window boundary could be handed a window that was being unregistered).
        for (size_t w = first; w <= last; ++w) ++users[w];
        for (size_t w = first; w <= last; ++w) {
            dropped.wait(hold, [&] { return state[w] != kDropping; });      // (a trim of this very window is on its way out: let it finish)
            if (state[w] == kRegistered) continue;
            const size_t begin = w * kWindow, len = std::min(kWindow, size - begin);
            if (refused || hipHostRegister(const_cast<uint8_t *>(base) + begin, len, hipHostRegisterPortable) != hipSuccess) {
                if (!refused) (void)hipGetLastError();
                refused = true;       // e.g. the memlock / userptr limit: from here on everybody reads with pread
                for (size_t u = first; u <= last; ++u) --users[u];            // (the caller owes no release)
                return false;         // (windows registered so far stay until their users are done)
            }
            state[w] = kRegistered;
            ++live;
        }
        frontier = std::max(frontier, last);
        return true;
    }
    // the copies out of [at, at + n) have completed (the caller synchronised its stream).  Windows nobody uses any more
    // are unregistered, oldest first, once more than `max_live` are registered: the registered (pinned, DMA-mapped)
    // footprint of a job stays at max_live * 256 MiB however large the file is, instead of growing to the whole input.
    // Never the window the furthest lane has reached (the next chunk starts in it: it would be registered again a moment
    // later), and never under the lock: hipHostUnregister may synchronise the device, and every other lane's
    // require() / release() would wait behind it -- the windows to drop are marked under the lock and let go
    // after it.
    void release(uint64_t at, size_t n) {
        if (!base || n == 0) return;
        std::vector<size_t> drop;
        {
            std::lock_guard<std::mutex> hold(lock);
            for (size_t w = at / kWindow; w <= (at + n - 1) / kWindow; ++w)
                if (users[w]) --users[w];
            for (size_t w = 0; w < state.size() && w < frontier && live > max_live; ++w)
                if (state[w] == kRegistered && !users[w]) {      // (no users AT MARKING TIME, and require() counts before it waits)
                    state[w] = kDropping;
                    --live;
                    drop.push_back(w);
                }
        }
        if (drop.empty()) return;
        const double t0 = trace_now();
        for (size_t w : drop) (void)hipHostUnregister(const_cast<uint8_t *>(base) + w * kWindow);
        {
            std::lock_guard<std::mutex> hold(lock);
            for (size_t w : drop) state[w] = kFree;
            trimmed += drop.size();
            trim_seconds += trace_now() - t0;
        }
        dropped.notify_all();
    }
    void close() {
        if (warmer.joinable()) warmer.join();
        if (!base) return;
        for (size_t w = 0; w < state.size(); ++w)
            if (state[w] == kRegistered) (void)hipHostUnregister(const_cast<uint8_t *>(base) + w * kWindow);
        InputGuard::unwatch(guard);
        guard = -1;
        ::munmap(const_cast<uint8_t *>(base), size);
        base = nullptr;
        state.clear();
        users.clear();
        live = 0;
        refused = false;
    }
    // registers the first window on a thread of its own (the first registration of a process costs ~35 ms, as long as a lane
    // takes to allocate its buffers: the two then run side by side); close() waits for it
    void warmFirstWindow(int device) {
        if (!base) return;
        warmer = std::thread([this, device] {
            const size_t n = std::min(kWindow, size);
            if (hipSetDevice(device) == hipSuccess && require(0, n)) release(0, n);
        });
    }
    const uint8_t *data() const { return base; }
    // Is the file still what was mapped?  false once an access to the mapping has faulted (somebody cut the file short:
    // what was read behind the new end are zeros, input_guard.hpp) or the file's length is no longer the mapped one.
    // The reference's fread() would have come back short (src/gpu_compressor.cpp:146-150); callers throw its message.
    bool intact(int fd) const {
        if (!base) return true;
        if (InputGuard::cut(guard)) return false;
        struct stat st;
        return ::fstat(fd, &st) == 0 && static_cast<uint64_t>(st.st_size) >= size;
    }
    // a copy must not straddle two registrations: the end of the window `at` lies in
    static size_t windowEnd(uint64_t at) { return (at / kWindow + 1) * kWindow; }
    size_t windowsTrimmed() {
        std::lock_guard<std::mutex> hold(lock);
        return trimmed;
    }
    double trimSeconds() {
        std::lock_guard<std::mutex> hold(lock);
        return trim_seconds;
    }
    bool wasRefused() {
        std::lock_guard<std::mutex> hold(lock);
        return refused;
    }

  private:
    static constexpr size_t kWindow = 256u << 20;
    static constexpr uint8_t kFree = 0, kRegistered = 1, kDropping = 2;
    std::thread warmer;
    const uint8_t *base = nullptr;
    size_t size = 0;
    int guard = -1;
    std::mutex lock;
    std::condition_variable dropped;
    std::vector<uint8_t> state;      // per window: kFree / kRegistered / kDropping (being unregistered by a release())
    std::vector<uint32_t> users;     // per window: chunks whose copies out of it may still be in flight
    size_t live = 0;                 // registered windows
    size_t frontier = 0;             // the highest window any lane has required so far: never trimmed
    size_t max_live = 16;            // ... of which at most this many are kept once nobody uses them (4 GiB; GPUAR_MAX_WINDOWS)
    size_t trimmed = 0;
    double trim_seconds = 0;         // spent inside hipHostUnregister by the trims (GPUAR_TRACE)
    bool refused = false;
};

// Device memory (kPinned: pinned host memory) that frees itself, and moves but is never copied.  ensure(count) makes room for
// `count` elements, on the current device, unless there is room already: all of a lane's buffers are sized by the lane's one chunk size.
template <typename T, bool kPinned>
class Memory {
  public:
    Memory() = default;
    Memory(Memory &&other) noexcept { std::swap(p, other.p); }
    ~Memory() {
        if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
    }
    void ensure(size_t count) {
        void **to = reinterpret_cast<void **>(&p);
        if (!p) hip_check(kPinned ? hipHostMalloc(to, count * sizeof(T), hipHostMallocDefault) : hipMalloc(to, count * sizeof(T)), kPinned ? "hipHostMalloc" : "hipMalloc");
    }
    operator T *() const { return p; }

  private:
    T *p = nullptr;
};
template <typename T>
using Device = Memory<T, false>;
template <typename T>
using Pinned = Memory<T, true>;

// what a chunk's kernels reported (GPUAR_STATUS_*), and how many bytes its packets came to
struct Encoded {
    size_t n_stream;
    uint32_t flags;
};
// ... and, under GPUAR_STATUS_CHECKSUM, the chunk's lowest packet that does not match its CRC
struct Decoded {
    uint32_t flags;
    uint64_t first_bad;
};

}  // namespace

// Everything one lane needs for one chunk of `cap` packets.
struct GPUCompressor::DeviceBuffers {
    int device = 0;
    size_t cap = 0;                 // packets
    size_t piece_bytes = 0;
    hipStream_t stream = nullptr;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    Device<uint8_t> d_plain;       // cap * 8192
    Device<uint8_t> d_slots;       // cap * 8704 (compress only)
    Device<uint8_t> d_stream;      // cap * 8704 (+16)
    Device<uint64_t> d_offsets;    // cap + 1, then this lane's status word
    Pinned<uint64_t> h_offsets;    // cap + 2: the word behind the offsets receives the status word
    Device<uint32_t> d_crc;        // cap packet CRC-32s (--checksum), then the verify's lowest bad packet (u64)
    Pinned<uint32_t> h_crc;        // the same
    Device<uint8_t> d_planes;      // cap * 8192 (--planes, --delta / a version-3 or -4 trailer): the chunk split into byte planes, or merged back
    Device<uint8_t> d_base;        // cap * 8192 (--base / a version-5 trailer): the base's bytes of the chunk's byte range
    Device<uint32_t> d_est;        // cap estimates and cap scan words (--stored / --sparse): what the kind of every packet is decided from
    Device<uint32_t> d_scan;
    Device<uint8_t> d_kind;        // cap packet kinds (--stored / --sparse, a version-6 trailer)
    Pinned<uint8_t> h_kind;        // the same
    Device<uint64_t> d_desc;       // 4 * (cap + 1): a version-6 chunk's coded packets as a batch of one-packet buffers (decodeChunk)
    Pinned<uint64_t> h_desc;       // the same
    Pinned<uint8_t> pieces[kPiecesPerLane];      // the lane's pinned pieces
    hipEvent_t epoch = nullptr;     // the device's common time base (owned by the GPUCompressor)
    std::vector<std::pair<float, float>> busy;   // [begin, end) of every chunk's kernels, ms since `epoch`
    // which of the lane's pinned pieces are free
    std::mutex piece_lock;
    std::condition_variable piece_free;
    bool piece_busy[kPiecesPerLane] = {};
    bool aborted = false;

    void allocate(size_t packets, bool compressing) {
        cap = packets;
        piece_bytes = std::min(kPieceBytes, cap * kSlot + 16);
        hip_check(hipSetDevice(device), "hipSetDevice");
        // non-blocking: a lane must never wait for another lane's copies or kernels through the NULL stream
        hip_check(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate");
        hip_check(hipEventCreate(&t0), "hipEventCreate");
        hip_check(hipEventCreate(&t1), "hipEventCreate");
        d_plain.ensure(cap * kPacket);
        if (compressing) d_slots.ensure(cap * kSlot);
        d_stream.ensure(cap * kSlot + 16);
        d_offsets.ensure(cap + 2);
        h_offsets.ensure(cap + 2);
        // (the pinned pieces are allocated when the first one is asked for: by then the lane's first copy and kernels are
        // on their way, and pinning 128 MiB takes as long as they do)
    }
    // this lane's own status word (device), behind the offsets: its launches report here, nobody else's do
    uint32_t *status() const { return reinterpret_cast<uint32_t *>(d_offsets + cap + 1); }
    // What a job of this plan needs beside that; the current device is the lane's.  An object's lanes outlive a job, and the next
    // one may go the other way: what is there stays.
    //   CRCs (compress --checksum, decompress of a file whose trailer has them): room for a chunk's CRC-32s
    //   a transform: one more buffer of chunk size for the chunk split into byte planes, or merged back
    //   a base: and one for the base's bytes
    //   kinds (compress --stored / --sparse, decompress of a version-6 file): room for a chunk's packet kinds, with the estimates and
    //   scan words they are decided from when compressing, with the descriptors of the chunk's coded packets when decompressing
    void prepare(const PacketPlan &plan, bool compressing) {
        if (plan.crcs) d_crc.ensure(crcSlots() + 2), h_crc.ensure(crcSlots() + 2);
        if (plan.transforms()) d_planes.ensure(cap * kPacket);
        if (plan.based) d_base.ensure(cap * kPacket);
        if (plan.kinds) d_kind.ensure(cap), h_kind.ensure(cap);
        if (plan.kinds && compressing) d_est.ensure(cap), d_scan.ensure(cap);
        if (plan.kinds && !compressing) d_desc.ensure(4 * (cap + 1)), h_desc.ensure(4 * (cap + 1));
    }
    // (a lane's buffers live as long as the object that holds them: the memory frees itself behind this)
    ~DeviceBuffers() {
        if (!cap) return;
        (void)hipSetDevice(device);
        (void)hipEventDestroy(t0);
        (void)hipEventDestroy(t1);
        (void)hipStreamDestroy(stream);
    }

    // a free pinned piece (blocks while the writer still holds both)
    size_t takePiece() {
        std::unique_lock<std::mutex> hold(piece_lock);
        for (;;) {
            if (aborted) throw std::runtime_error("pipeline stopped");
            for (size_t k = 0; k < kPiecesPerLane; ++k)
                if (!piece_busy[k]) {
                    piece_busy[k] = true;
                    hold.unlock();
                    try {
                        pieces[k].ensure(piece_bytes);
                    } catch (...) {
                        givePiece(k);
                        throw;
                    }
                    return k;
                }
            piece_free.wait(hold);
        }
    }
    void givePiece(size_t k) {
        std::lock_guard<std::mutex> hold(piece_lock);
        piece_busy[k] = false;
        piece_free.notify_all();
    }
    void abortWaits() {
        std::lock_guard<std::mutex> hold(piece_lock);
        aborted = true;
        piece_free.notify_all();
    }
    void resetPieces() {
        std::lock_guard<std::mutex> hold(piece_lock);
        aborted = false;
        for (auto &b : piece_busy) b = false;
    }

    // where this chunk's kernels ran on the device's clock
    void noteBusy() {
        float begin = 0, end = 0;
        hip_check(hipEventElapsedTime(&begin, epoch, t0), "event");
        hip_check(hipEventElapsedTime(&end, epoch, t1), "event");
        busy.emplace_back(begin, end);
    }

    // `n` bytes of the input file at `at` -> dst (device): straight from the mapping when there is one, else through
    // the lane's pinned pieces
    // Returns true when the copies were queued straight out of the mapping: the caller then owes in.release(at, n)
    // once it has synchronised this lane's stream.
    bool upload(uint8_t *dst, MappedInput &in, int fd, uint64_t at, size_t n, const char *error) {
        if (in.data() && in.require(at, n)) {
            for (size_t done = 0; done < n;) {           // one copy per registered window
                const size_t part = std::min<uint64_t>(n - done, MappedInput::windowEnd(at + done) - (at + done));
                hip_check(hipMemcpyAsync(dst + done, in.data() + at + done, part, hipMemcpyHostToDevice, stream), "H2D");
                done += part;
            }
            return true;
        }
        stage(dst, fd, at, n, error);
        return false;
    }
    // `n` bytes of file `fd` at `at` -> dst (device) by pread into the lane's pinned pieces, each copied on the lane's stream
    void stage(uint8_t *dst, int fd, uint64_t at, size_t n, const char *error) {
        for (size_t done = 0; done < n;) {
            const size_t k = takePiece();
            const size_t part = std::min(piece_bytes, n - done);
            try {
                sliced_io<false>(fd, pieces[k], part, at + done, error);
                hip_check(hipMemcpyAsync(dst + done, pieces[k], part, hipMemcpyHostToDevice, stream), "H2D");
                hip_check(hipStreamSynchronize(stream), "sync");
            } catch (...) {
                givePiece(k);
                throw;
            }
            givePiece(k);
            done += part;
        }
    }

    // `n` bytes of the base file at `at` -> d_base, staged (the CLI is bound by its one writer, so the base does without the
    // mapped-window machinery)
    void uploadBase(int fd, uint64_t at, size_t n) { stage(d_base, fd, at, n, "Read base file failed"); }

    // src[0..n) (device) -> the writer, piece by piece; `at`: file offset of the first byte (unordered writer).
    // `closes_chunk`: the last piece of these is the chunk's last (the ordered writer then moves on to chunk + 1).
    void drain(Writer &writer, size_t chunk, const uint8_t *src, size_t n, uint64_t at, size_t plain_bytes, bool closes_chunk = true) {
        size_t done = 0;
        do {
            const size_t k = takePiece();
            const size_t part = std::min(piece_bytes, n - done);
            try {
                if (part) {
                    hip_check(hipMemcpyAsync(pieces[k], src + done, part, hipMemcpyDeviceToHost, stream), "D2H");
                    hip_check(hipStreamSynchronize(stream), "sync");
                }
            } catch (...) {
                givePiece(k);
                throw;
            }
            Piece p;
            p.data = pieces[k];
            p.bytes = part;
            p.at = at + done;
            done += part;
            p.last_of_chunk = closes_chunk && done >= n;
            p.plain_bytes = done >= n ? plain_bytes : 0;
            p.give_back = [this, k] { givePiece(k); };
            writer.submit(chunk, std::move(p));
        } while (done < n);
    }

    // Which buffer holds the bytes that are coded (compress), or the bytes that are written (decompress): the far side of the
    // plan's transform when it has one.
    uint8_t *transformed(const PacketPlan &plan) const { return plan.transforms() ? d_planes : d_plain; }
    // d_plain[0..n) -> d_planes: XORed with d_base, else the elements' differences, else as they are, split into byte planes of
    // elements plan.elem wide (delta and base at a width of 1 too); else nothing
    void split(const PacketPlan &plan, size_t n) {
        if (plan.based) gpuar_check(gpuar_hip_split_xor(d_plain, d_base, n, plan.elem, d_planes, stream), "gpuar_hip_split_xor");
        else if (plan.delta) gpuar_check(gpuar_hip_split_delta(d_plain, n, plan.elem, d_planes, stream), "gpuar_hip_split_delta");
        else if (plan.elem > 1) gpuar_check(gpuar_hip_split_planes(d_plain, n, plan.elem, d_planes, stream), "gpuar_hip_split_planes");
    }
    // ... and back: the n decoded bytes in d_plain are such byte planes, merged into d_planes
    void merge(const PacketPlan &plan, size_t n) {
        if (plan.based) gpuar_check(gpuar_hip_merge_xor(d_plain, d_base, n, plan.elem, d_planes, stream), "gpuar_hip_merge_xor");
        else if (plan.delta) gpuar_check(gpuar_hip_merge_delta(d_plain, n, plan.elem, d_planes, stream), "gpuar_hip_merge_delta");
        else if (plan.elem > 1) gpuar_check(gpuar_hip_merge_planes(d_plain, n, plan.elem, d_planes, stream), "gpuar_hip_merge_planes");
    }

    // d_plain[0..n_plain) -> d_stream[0..n_stream), h_offsets[0..n_packets]; returns n_stream and
    // what THIS chunk's launches reported (GPUAR_STATUS_*): the status word travels back with the offsets, on the
    // lane's own stream -- no device-wide synchronisation, no flag shared with another lane
    // `mode`: GPUAR_MODE_* -- which encode kernel (the caller knows whether this launch has the chip to itself)
    // plan.crcs: also the CRC-32 of every packet of the input, into h_crc[0..n_packets)
    // a plan that transforms: what is coded is the chunk after split(); the CRCs stay the input's
    // plan.stored / plan.sparse: behind the encoder, the packets the rule of ../kinds.h keeps raw or sparse overwrite their slots (every packet
    // is coded first: the CLI is bound by the file system, not by the encoder); the kinds go to h_kind[0..n_packets)
    Encoded encodeChunk(size_t n_plain, const PacketPlan &plan, int mode) {
        const size_t n_packets = (n_plain + kPacket - 1) / kPacket;
        hip_check(hipMemsetAsync(status(), 0, sizeof(uint32_t), stream), "memset");
        hip_check(hipEventRecord(t0, stream), "event");
        split(plan, n_plain);
        const uint8_t *coded = transformed(plan);
        gpuar_check(gpuar_hip_encode_mode(coded, n_plain, d_slots, status(), stream, mode), "gpuar_hip_encode_mode");
        if (plan.kinds) {
            gpuar_check(gpuar_hip_estimate(coded, n_plain, d_est, stream), "gpuar_hip_estimate");
            if (plan.sparse) gpuar_check(gpuar_hip_sparse_scan(coded, n_plain, d_scan, stream), "gpuar_hip_sparse_scan");
            gpuar_check(gpuar_hip_kinds_store(coded, n_plain, d_est, plan.sparse ? &d_scan[0] : nullptr, plan.stored ? 1 : 0, d_slots, d_kind, status(), stream),
                        "gpuar_hip_kinds_store");
        }
        gpuar_check(gpuar_hip_compact(d_slots, n_packets, d_stream, d_offsets, stream), "gpuar_hip_compact");
        if (plan.crcs) gpuar_check(gpuar_hip_crc32(d_plain, n_plain, d_crc, stream), "gpuar_hip_crc32");
        hip_check(hipEventRecord(t1, stream), "event");
        hip_check(hipMemcpyAsync(h_offsets, d_offsets, (n_packets + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "D2H");
        hip_check(hipMemcpyAsync(h_offsets + n_packets + 1, status(), sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "D2H");
        if (plan.crcs) hip_check(hipMemcpyAsync(h_crc, d_crc, n_packets * sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "D2H");
        if (plan.kinds) hip_check(hipMemcpyAsync(h_kind, d_kind, n_packets, hipMemcpyDeviceToHost, stream), "D2H");
        hip_check(hipStreamSynchronize(stream), "sync");
        noteBusy();
        return {static_cast<size_t>(h_offsets[n_packets]), *reinterpret_cast<const uint32_t *>(h_offsets + n_packets + 1)};
    }

    // d_stream[0..n_stream) with h_offsets[0..n_packets] -> d_plain[0..n_packets*8192); returns this chunk's status flags.
    // crcs (n_packets values, or null): the decoded packets -- n_plain bytes back to back -- are verified against them;
    // GPUAR_STATUS_CHECKSUM in the flags then, and the chunk's lowest bad packet in `first_bad`
    // a plan that transforms: the n_plain decoded bytes go through merge() before they are verified; the result is in transformed(plan)
    // `kinds` (n_packets values, or null: every packet is coded): the chunk of a version-6 file, whose packets all hold 8192 bytes but
    // the last.  Its coded packets are decoded as a batch of one-packet buffers (raw bytes are never fed to the decoder; a chunk
    // without a coded packet launches no decoder), then one launch takes the raw and sparse ones out of the stream
    Decoded decodeChunk(size_t n_packets, size_t n_plain, const PacketPlan &plan, const uint32_t *crcs, const uint8_t *kinds) {
        hip_check(hipMemsetAsync(status(), 0, sizeof(uint32_t), stream), "memset");
        hip_check(hipMemcpyAsync(d_offsets, h_offsets, (n_packets + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream), "H2D");
        uint64_t *d_first_bad = crcs ? reinterpret_cast<uint64_t *>(d_crc + crcSlots()) : nullptr;
        if (crcs) {
            std::memcpy(h_crc, crcs, n_packets * sizeof(uint32_t));
            hip_check(hipMemcpyAsync(d_crc, h_crc, n_packets * sizeof(uint32_t), hipMemcpyHostToDevice, stream), "H2D");
            hip_check(hipMemsetAsync(d_first_bad, 0xFF, sizeof(uint64_t), stream), "memset");
        }
        hip_check(hipEventRecord(t0, stream), "event");
        if (kinds) {
            uint64_t *out_ptrs = h_desc, *out_bytes = h_desc + (cap + 1), *first = h_desc + 2 * (cap + 1), *coded_at = h_desc + 3 * (cap + 1);
            size_t n_coded = 0;
            for (size_t p = 0; p < n_packets; ++p) {
                if (kinds[p] != 0) continue;
                out_ptrs[n_coded] = reinterpret_cast<uint64_t>(d_plain + p * kPacket);
                out_bytes[n_coded] = std::min<uint64_t>(kPacket, n_plain - p * kPacket);
                first[n_coded] = n_coded;
                coded_at[n_coded++] = h_offsets[p];
            }
            first[n_coded] = n_coded;
            coded_at[n_coded] = h_offsets[n_packets];
            std::memcpy(h_kind, kinds, n_packets);
            hip_check(hipMemcpyAsync(d_kind, h_kind, n_packets, hipMemcpyHostToDevice, stream), "H2D");
            if (n_coded) {
                hip_check(hipMemcpyAsync(d_desc, h_desc, 4 * (cap + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream), "H2D");
                gpuar_check(gpuar_hip_decode_stream_batch(d_stream, d_desc + 3 * (cap + 1), d_desc + 2 * (cap + 1), n_coded, n_coded,
                                                          reinterpret_cast<uint8_t *const *>(&d_desc[0]), d_desc + (cap + 1), status(), stream),
                            "gpuar_hip_decode_stream_batch");
            }
            gpuar_check(gpuar_hip_kinds_expand(d_stream, d_offsets, d_kind, n_packets, d_plain, n_plain, status(), stream), "gpuar_hip_kinds_expand");
        } else {
            gpuar_check(gpuar_hip_decode_stream(d_stream, d_offsets, n_packets, d_plain, status(), stream), "gpuar_hip_decode_stream");
        }
        merge(plan, n_plain);
        if (crcs) gpuar_check(gpuar_hip_verify_crc32(transformed(plan), n_plain, d_crc, d_first_bad, status(), stream), "gpuar_hip_verify_crc32");
        hip_check(hipEventRecord(t1, stream), "event");
        hip_check(hipMemcpyAsync(h_offsets + n_packets + 1, status(), sizeof(uint32_t), hipMemcpyDeviceToHost, stream), "D2H");
        if (crcs) hip_check(hipMemcpyAsync(h_crc + crcSlots(), d_first_bad, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), "D2H");
        hip_check(hipStreamSynchronize(stream), "sync");
        noteBusy();
        Decoded done{*reinterpret_cast<const uint32_t *>(h_offsets + n_packets + 1), 0};
        if (crcs) std::memcpy(&done.first_bad, h_crc + crcSlots(), sizeof(uint64_t));
        return done;
    }
    size_t crcSlots() const { return (cap + 1) / 2 * 2; }      // u32 slots in front of the u64 (8-byte aligned), itself two more
};

GPUCompressor::GPUCompressor() {
    trace("GPUCompressor: constructing (the HIP runtime starts here)");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        throw std::runtime_error("No HIP device found (use --host to run the codec on the CPU)");
    devices.push_back(0);
    trace("GPUCompressor: devices counted");
    initConstantRange();     // kept for parity with src/gpu_compressor.cpp:19; a no-op for these kernels
}

GPUCompressor::~GPUCompressor() { releaseBuffers(); }

void GPUCompressor::releaseBuffers() {
    for (DeviceBuffers *b : buffers) delete b;
    buffers.clear();
    for (size_t g = 0; g < epochs.size(); ++g)
        if (epochs[g]) {
            (void)hipSetDevice(devices[g]);
            (void)hipEventDestroy(static_cast<hipEvent_t>(epochs[g]));
        }
    epochs.clear();
}

// kLanesPerDevice buffer sets per device, sized for the job at hand: a file of `total_packets` is cut
// into chunks of at most batchPackets packets, small enough that every lane of every device gets one
// (whole wavefronts: multiples of 64 packets -- hence whole groups of byte planes, 2, 4 or 8 packets, whatever --batch says:
// with chunks that start on group boundaries counted from the file's start, a file of planes does not depend on how it
// was cut).  A lane's buffers are allocated when it first gets a
// chunk -- pinned allocations are what a short run of the CLI spends most of its time on.
void GPUCompressor::ensureBuffers(size_t total_packets, bool compressing) {
    const size_t G = devices.size();
    const size_t lanes = G * kLanesPerDevice;
    const size_t share = ((total_packets + lanes - 1) / lanes + 63) / 64 * 64;
    const size_t cap = std::max<size_t>(64, std::min(batchPackets, share));
    bool have = buffers.size() == lanes && !buffers.empty() && chunkPackets == cap;
    if (have && compressing)
        for (DeviceBuffers *b : buffers) have = have && (!b->cap || b->d_slots);
    if (have) {
        for (DeviceBuffers *b : buffers) b->resetPieces();
        return;
    }
    releaseBuffers();
    chunkPackets = cap;
    for (size_t l = 0; l < lanes; ++l) {
        buffers.push_back(new DeviceBuffers());
        buffers.back()->device = devices[l / kLanesPerDevice];
    }
}

void GPUCompressor::chooseDevice(const int id) {
    int count = 0;
    hip_check(hipGetDeviceCount(&count), "hipGetDeviceCount");
    if (id < 0 || id >= count) throw std::runtime_error("No such HIP device: " + std::to_string(id));
    releaseBuffers();
    devices.assign(1, id);
}

void GPUCompressor::useDevices(const int n) {
    int count = 0;
    hip_check(hipGetDeviceCount(&count), "hipGetDeviceCount");
    // GPUAR_OVERSUBSCRIBE_DEVICES=1 lets logical device d run on physical device d % count, so the
    // sharding / ordered-concatenation path can be exercised on a box with fewer GPUs (tests only)
    const char *over = std::getenv("GPUAR_OVERSUBSCRIBE_DEVICES");
    const bool oversubscribe = over && over[0] == '1';
    if (n < 1 || (n > count && !oversubscribe))
        throw std::runtime_error("Asked for " + std::to_string(n) + " GPUs, " + std::to_string(count) + " visible");
    releaseBuffers();
    devices.clear();
    for (int d = 0; d < n; ++d) devices.push_back(d % count);
}

// Runs `work(lane, buffers, failure)` on every lane (lanes g*kLanesPerDevice .. belong to device g) and
// rethrows the first failure.  `work` pulls chunk numbers until there are none left; `on_failure` runs on the
// failing lane's thread, so that whoever the other lanes are waiting for lets them go.
template <typename Work, typename OnFailure>
void GPUCompressor::runLanes(Work &&work, OnFailure &&on_failure) {
    Failure failure;
    std::vector<std::thread> threads;
    for (size_t l = 0; l < buffers.size(); ++l)
        threads.emplace_back([&, l] {
            try {
                work(l, *buffers[l], failure);
            } catch (...) {
                failure.set(std::current_exception());      // (what a lane woken by an abort throws comes second: never the cause)
                for (DeviceBuffers *b : buffers) b->abortWaits();
                on_failure();
            }
        });
    for (auto &t : threads) t.join();
    if (failure.first) {
        // A lane that failed may have left copies out of the mapped input queued on its stream; the caller's unwinding
        // unregisters and unmaps that file next.  Nothing may still be reading it: drain every lane's stream first
        // (results ignored -- the failure that is about to be reported is the first one).
        for (DeviceBuffers *b : buffers)
            if (b->cap && b->stream) {
                (void)hipSetDevice(b->device);
                (void)hipStreamSynchronize(b->stream);
            }
        std::rethrow_exception(failure.first);
    }
}

namespace {

// Deals a job's chunks to the devices -- contiguous packet ranges in file order, dealt round-robin: chunk c belongs to device
// c mod G -- and counts what each device did (GPUAR_TRACE).
struct Dealer {
    explicit Dealer(size_t G) : next_of_device(G), device_bytes(G), device_chunks(G) {}      // (all zero)
    // the next chunk of device g
    size_t take(size_t g) { return g + next_of_device.size() * next_of_device[g].fetch_add(1); }
    void count(size_t g, uint64_t bytes) {
        device_bytes[g] += bytes;
        device_chunks[g] += 1;
    }
    // "<job>: device g <did> N bytes in M chunks<of>"
    void report(const char *job, const char *did, const std::string &of = "") {
        for (size_t g = 0; g < next_of_device.size(); ++g)
            trace((std::string(job) + ": device " + std::to_string(g) + " " + did + " " + std::to_string(device_bytes[g].load()) + " bytes in " + std::to_string(device_chunks[g].load()) + " chunks" + of).c_str());
    }
    std::vector<std::atomic<size_t>> next_of_device;
    std::vector<std::atomic<uint64_t>> device_bytes, device_chunks;
};

// the writer's progress callback (the writer is one thread): what the pieces written so far complete, to the monitor
std::function<void(size_t)> progressTo(CompressionInfo &info, ProgressMonitor *monitor) {
    return [&info, monitor](size_t plain) {
        if (!plain) return;
        info.processedUncompressedSize += plain;
        monitor->updateProgress(&info);
    };
}

// After the lanes: if one of them failed, its failure goes on up -- unless the writer has a failure of its own (disk full), which
// is the cause then: the lanes only saw "pipeline stopped".
void rethrowLaneFailure(Writer &writer, std::exception_ptr lane_failure) {
    if (!lane_failure) return;
    writer.abort();
    (void)writer.finish(0);      // rethrows the writer's own failure when it has one: that is the cause then
    std::rethrow_exception(lane_failure);
}

// the chunks' tables, one behind the other
template <typename T>
std::vector<T> joined(const std::vector<std::vector<T>> &chunks) {
    std::vector<T> all;
    for (const auto &v : chunks) all.insert(all.end(), v.begin(), v.end());
    return all;
}

// How many packets chunk c holds.  The first chunks of a job are small and double from one to the next (64 MiB of input,
// 128, 256 ...) until they reach the full chunk size: the writer gets its first piece a few milliseconds after the
// start instead of after the first 512 MiB have crossed PCIe three lanes abreast, and it is the writer that bounds the
// wall time.  (Chunks stay multiples of 64 packets: whole wavefronts.)
size_t rampPackets(size_t c, size_t full) {
    constexpr size_t kFirst = 8192;
    if (c >= 8 || full <= kFirst) return full;
    return std::min(full, kFirst << c);
}

}  // namespace

// Runs `job()` between the opening of the files and the times: a failed job leaves an empty file, not a half-written one.
template <typename Job>
CompressionInfo GPUCompressor::runJob(ProgressMonitor *monitor, Job &&job) {
    CompressionInfo info;
    monitor->reset();
    process_timer.reset();
    io_timer.reset();
    io_timer.start();
    openFiles(false);
    const int out_fd = fileno(saveFile);
    try {
        job(info, out_fd);
    } catch (...) {
        if (::ftruncate(out_fd, 0) != 0) {}      // a failed job leaves an empty file, not a half-written one
        closeFiles();
        dropTimes();
        throw;
    }
    io_timer.stop();
    finishTimes(info);
    return info;
}

// One compress job: what its steps share.
struct GPUCompressor::CompressJob {
    GPUCompressor &self;
    CompressionInfo &info;
    ProgressMonitor *monitor;
    const int out_fd;
    const PacketPlan plan = self.plan();
    const bool trailer = self.wantsTrailer();
    const int in_fd = fileno(self.openFile);
    MappedInput mapped;
    std::vector<uint64_t> chunk_at;      // where chunk c starts in the input; one entry more: the input's end
    size_t n_chunks = 0;
    std::vector<std::vector<uint16_t>> chunk_clens;      // for the optional index trailer
    std::vector<std::vector<uint32_t>> chunk_crcs;       // and the checksums in it
    std::vector<std::vector<uint8_t>> chunk_kinds;       // and the packet kinds (--stored / --sparse)
    Dealer deal{self.devices.size()};

    // contiguous packet ranges in file order: where chunk c starts and how long it is
    void cutChunks() {
        for (uint64_t at = 0; at < info.uncompressedFileSize; at += rampPackets(chunk_at.size() - 1, self.chunkPackets) * kPacket) chunk_at.push_back(at);
        n_chunks = chunk_at.size();
        chunk_at.push_back(info.uncompressedFileSize);
        for (size_t c = 0; c < n_chunks && c < 8; ++c)      // (GPUAR_TRACE: the ramp, and where the chunks behind it start)
            trace(("compress: packets in chunk " + std::to_string(c) + ":").c_str(), static_cast<double>((chunk_at[c + 1] - chunk_at[c] + kPacket - 1) / kPacket));
        chunk_clens.resize(trailer ? n_chunks : 0);
        chunk_crcs.resize(plan.crcs ? n_chunks : 0);
        chunk_kinds.resize(plan.kinds ? n_chunks : 0);
    }

    // chunk c, of device g, on lane b: input -> device -> packets -> the writer
    void codeChunk(size_t c, size_t g, DeviceBuffers &b, Writer &writer) {
        const uint64_t at = chunk_at[c];
        const size_t n_plain = static_cast<size_t>(chunk_at[c + 1] - at);
        const bool from_mapping = b.upload(b.d_plain, mapped, in_fd, at, n_plain, "Read input file failed");
        if (plan.based) b.uploadBase(self.baseFd, at, n_plain);      // the same byte range of the base
        if (c == 0) trace("compress: its input on its way (window registered, copy queued)");
        // The latency-mode encode kernel is faster only for a launch that has the chip to itself (include/gpuar_hip.h):
        // a job of one chunk.  With several chunks the lanes of a device keep three launches in flight (the ramped first
        // chunks are small enough for GPUAR_MODE_AUTO to pick the latency kernel), so the pipeline names the kernel itself.
        const Encoded coded = b.encodeChunk(n_plain, plan, n_chunks == 1 ? GPUAR_MODE_AUTO : GPUAR_MODE_THROUGHPUT);     // (synchronises the lane's stream)
        if (from_mapping) mapped.release(at, n_plain);
        // the file was cut short (or replaced) under the mapping: what the reference's fread() reports
        // (src/gpu_compressor.cpp:146-150)
        if (!mapped.intact(in_fd)) throw std::runtime_error("Read input file failed");
        if (c < 3) trace("compress: kernels of an early chunk done, chunk", static_cast<double>(c));
        if (coded.flags & GPUAR_STATUS_SLOT_OVERFLOW)
            throw std::runtime_error("a packet outgrew its 8704-byte slot (input bytes " + std::to_string(at) + " .. " + std::to_string(at + n_plain) + ")");
        // (the scan words are computed from the very bytes: this cannot happen, and the file would still be valid)
        if (coded.flags & GPUAR_STATUS_BAD_BATCH) throw std::runtime_error("Fail to execute kernel code: gpuar_hip_kinds_store: inconsistent scan");
        const size_t n_packets = (n_plain + kPacket - 1) / kPacket;
        if (plan.crcs) chunk_crcs[c].assign(&b.h_crc[0], &b.h_crc[n_packets]);
        if (plan.kinds) chunk_kinds[c].assign(&b.h_kind[0], &b.h_kind[n_packets]);
        if (trailer) {
            chunk_clens[c].resize(n_packets);
            for (size_t p = 0; p < n_packets; ++p) chunk_clens[c][p] = static_cast<uint16_t>(b.h_offsets[p + 1] - b.h_offsets[p]);
        }
        deal.count(g, n_plain);
        b.drain(writer, c, b.d_stream, coded.n_stream, 0, n_plain);     // the ordered writer knows where chunk c goes
    }

    // the lanes and the ordered writer, from the first chunk to the last byte of the stream
    void codeAll() {
        Writer writer(out_fd, true, FileHeader::HEADER_LENGTH, "Write compressed data to output file failed");
        writer.on_progress = progressTo(info, monitor);
        writer.on_failure = [&] {
            for (DeviceBuffers *b : self.buffers) b->abortWaits();
        };
        std::exception_ptr lane_failure;
        try {
            self.runLanes(
                [&](size_t lane, DeviceBuffers &b, Failure &failure) {      // what one lane does: its device's chunks, one after the other
                    const size_t g = lane / kLanesPerDevice;
                    for (;;) {
                        const size_t c = deal.take(g);
                        if (c >= n_chunks || failure.stop) break;
                        if (c == 0) trace("compress: lane of chunk 0 starts");
                        if (!b.cap) b.allocate(self.chunkPackets, true);
                        if (c == 0) trace("compress: its buffers allocated");
                        hip_check(hipSetDevice(b.device), "hipSetDevice");
                        b.prepare(plan, true);
                        b.epoch = static_cast<hipEvent_t>(self.epochOf(g));
                        codeChunk(c, g, b, writer);
                    }
                },
                [&] { writer.abort(); });
        } catch (...) {
            lane_failure = std::current_exception();
        }
        rethrowLaneFailure(writer, lane_failure);
        trace("compress: lanes done");
        trace(mapped.wasRefused() ? "compress: a window could not be registered: the rest was read with pread" : "compress: every window registered");
        trace("compress: input windows unregistered while the job ran:", static_cast<double>(mapped.windowsTrimmed()));
        trace("compress: seconds inside hipHostUnregister for that:", mapped.trimSeconds());
        deal.report("compress", "coded", " of at most " + std::to_string(self.chunkPackets * kPacket) + " bytes");
        info.compressedFileSize = static_cast<size_t>(writer.finish(n_chunks));
    }

    void run() {
        info.uncompressedFileSize = self.getFileSize(self.openFile);
        if (plan.based) self.openBase(info.uncompressedFileSize, "the input");
        const size_t total_packets = (info.uncompressedFileSize + kPacket - 1) / kPacket;
        self.ensureBuffers(total_packets, true);
        cutChunks();
        hip_check(hipSetDevice(self.devices[0]), "hipSetDevice");
        trace("compress: files open, device set");
        mapped.open(in_fd, info.uncompressedFileSize);
        trace(mapped.data() ? "compress: input mapped" : "compress: input NOT mapped (pread path)");
        mapped.warmFirstWindow(self.devices[0]);
        // room for the worst case up front: writing into allocated blocks is faster than growing the file, and the real
        // length is set at the end (best effort: a file system without fallocate just grows the file as it goes)
        // (the fallocate system call, not posix_fallocate: where the file system cannot do it, glibc's stand-in would write zeros)
        (void)::fallocate(out_fd, 0, 0, static_cast<off_t>(FileHeader::HEADER_LENGTH + total_packets * kSlot));
        codeAll();
        // behind the stream: the trailer the options ask for, then the header in front of it, and the file's real length
        uint64_t file_end = info.compressedFileSize;
        if (trailer) {
            if (std::fseek(self.saveFile, static_cast<long>(info.compressedFileSize), SEEK_SET) != 0) throw std::runtime_error("Seek file failed");
            self.saveTrailer(plan, joined(chunk_clens), joined(chunk_crcs), joined(chunk_kinds));
            if (std::fflush(self.saveFile) != 0) throw std::runtime_error("Write packet index failed");
            file_end = static_cast<uint64_t>(std::ftell(self.saveFile));
        }
        FileHeader header;
        header.setCompressedFileSize(info.compressedFileSize);
        header.setUncompressedFileSize(info.uncompressedFileSize);
        if (::pwrite(out_fd, header.getData(), FileHeader::HEADER_LENGTH, 0) != FileHeader::HEADER_LENGTH)
            throw std::runtime_error("Write data to file failed");
        if (::ftruncate(out_fd, static_cast<off_t>(file_end)) != 0) throw std::runtime_error("Write data to file failed");
        trace("compress: header written, length set");
        mapped.close();
        self.closeFiles();
        trace("compress: files closed");
    }
};

CompressionInfo GPUCompressor::compress(ProgressMonitor *monitor) {
    return runJob(monitor, [&](CompressionInfo &info, int out_fd) { CompressJob{*this, info, monitor, out_fd}.run(); });
}

// "Compute time" = kernels + their sync, as src/gpu_compressor.cpp:184-194.  The lanes of a device run their
// kernels at the same time, so their spans overlap (and each span includes time queued behind another lane's
// kernels): what is reported is the time the device had at least one chunk's kernels in flight -- the UNION of
// the lanes' [first kernel submitted, last kernel done) intervals on the device's own clock -- of the busiest
// device; the rest of the wall time is I/O.
void GPUCompressor::finishTimes(CompressionInfo &info) {
    double busiest = 0;
    for (size_t g = 0; g < devices.size(); ++g) {
        std::vector<std::pair<float, float>> spans;
        for (size_t l = g * kLanesPerDevice; l < (g + 1) * kLanesPerDevice && l < buffers.size(); ++l) {
            spans.insert(spans.end(), buffers[l]->busy.begin(), buffers[l]->busy.end());
            buffers[l]->busy.clear();
        }
        std::sort(spans.begin(), spans.end());
        double total = 0;
        float open_begin = 0, open_end = -1;
        for (const auto &sp : spans) {
            if (open_end < open_begin || sp.first > open_end) {      // a gap: close the run so far
                if (open_end >= open_begin) total += open_end - open_begin;
                open_begin = sp.first;
                open_end = sp.second;
            } else {
                open_end = std::max(open_end, sp.second);
            }
        }
        if (open_end >= open_begin) total += open_end - open_begin;
        busiest = std::max(busiest, total);
    }
    info.processTime = busiest;
    info.ioTime = std::max(0.0, io_timer.value() - info.processTime);
}

// A job that throws never reaches finishTimes: the kernel spans its lanes noted so far would stay in their `busy` lists and be
// counted into the processTime of the next job that reuses the lanes (an object outlives a failed job; the CLI does not).
void GPUCompressor::dropTimes() {
    for (DeviceBuffers *b : buffers) b->busy.clear();
}

// One event per device that every lane of the device measures its kernel intervals against.
void *GPUCompressor::epochOf(size_t g) {
    std::lock_guard<std::mutex> hold(epochLock);
    if (epochs.size() < devices.size()) epochs.resize(devices.size(), nullptr);
    if (!epochs[g]) {
        hipEvent_t e = nullptr;
        hip_check(hipSetDevice(devices[g]), "hipSetDevice");
        hip_check(hipEventCreate(&e), "hipEventCreate");
        hip_check(hipEventRecord(e, nullptr), "event");
        hip_check(hipEventSynchronize(e), "event");
        epochs[g] = e;
    }
    return epochs[g];
}

// One decompress job: what its steps share.
struct GPUCompressor::DecompressJob {
    GPUCompressor &self;
    CompressionInfo &info;
    ProgressMonitor *monitor;
    const int out_fd;
    const int in_fd = fileno(self.openFile);
    uint64_t stream_end = 0;
    MappedInput mapped;
    Trailer trailer;
    PacketPlan plan;
    ChunkMap map;
    std::thread scanner;
    std::atomic<bool> stop_scan{false};
    OrderedOffsets place;
    Dealer deal{self.devices.size()};

    // whatever way the job is left, the scanner is told to stop and joined before `map` and `mapped` go away
    ~DecompressJob() { stopScanner(); }
    void stopScanner() {
        stop_scan = true;
        if (scanner.joinable()) scanner.join();
    }

    // the chunk map of a file with an index: prefix sums of the stored lengths (already checked against the stream size)
    void mapFromIndex() {
        const std::vector<uint16_t> &index = trailer.clens;
        uint64_t at = FileHeader::HEADER_LENGTH;
        for (size_t p = 0; p < index.size();) {
            ChunkMap::Chunk c;
            c.begin = at;
            c.first_packet = p;
            const size_t want = rampPackets(map.chunks.size(), self.chunkPackets);
            while (p < index.size() && c.n_packets < want) {
                const size_t clen = index[p++];
                if (clen < GPUAR_PACKET_HEADER_BYTES || clen > kSlot) throw std::runtime_error("Invalid file length");
                at += clen;
                ++c.n_packets;
            }
            c.end = at;
            map.push(c);
        }
        map.finish();
    }

    // ... and of one without, on the scanner thread:
    // the header walk of src/gpu_compressor.cpp:299-312 (`off += clen`), four bytes per packet, ahead of the lanes:
    // through the mapping when there is one, else by pread
    void scanHeaders() {
        try {
            uint64_t at = FileHeader::HEADER_LENGTH;
            size_t n_pushed = 0, n_packets = 0;
            while (at < stream_end && !stop_scan) {
                ChunkMap::Chunk c;
                c.begin = at;
                c.first_packet = n_packets;
                const size_t want = rampPackets(n_pushed, self.chunkPackets);
                while (at < stream_end && c.n_packets < want) {
                    uint8_t h[GPUAR_PACKET_HEADER_BYTES];
                    if (stream_end - at < sizeof h) throw std::runtime_error("Incorrect file format");
                    if (mapped.data()) std::memcpy(h, mapped.data() + at, sizeof h);
                    else if (::pread(in_fd, h, sizeof h, static_cast<off_t>(at)) != static_cast<ssize_t>(sizeof h))
                        throw std::runtime_error("Incorrect file format");
                    const size_t clen = getPacketSize(h);
                    if (clen < GPUAR_PACKET_HEADER_BYTES || clen > kSlot || at + clen > stream_end)
                        throw std::runtime_error("Invalid file length");
                    at += clen;
                    ++c.n_packets;
                }
                c.end = at;
                n_packets += c.n_packets;
                map.push(c);
                ++n_pushed;
            }
            map.finish();
        } catch (...) {
            map.finish(std::current_exception());
        }
    }

    // what a chunk's packets say of themselves
    struct Walked {
        uint64_t produced = 0;      // bytes the chunk decodes to
        bool all_full = true;       // every packet but the chunk's last holds 8192 bytes
    };
    // packet offsets inside the chunk (into b.h_offsets), and what every packet says it holds (u16 at +2): all but the
    // file's last one hold 8192 bytes (src/gpu_compressor.cpp:326-331).  What is written comes from
    // the packets, not from the header's size field: a file written by the reference carries garbage
    // in the upper half of that field (src/file_header.hpp:31-36), and --host decodes by ulen too.
    static Walked walkChunk(DeviceBuffers &b, const ChunkMap::Chunk &chunk, const uint8_t *bytes) {
        const size_t n_stream = static_cast<size_t>(chunk.end - chunk.begin);
        Walked w;
        size_t off = 0;
        for (size_t p = 0; p < chunk.n_packets; ++p) {
            b.h_offsets[p] = off;
            if (n_stream - off < GPUAR_PACKET_HEADER_BYTES) throw std::runtime_error("Invalid file length");
            const uint8_t *pkt = bytes + off;
            const size_t clen = getPacketSize(pkt);
            if (clen < GPUAR_PACKET_HEADER_BYTES || off + clen > n_stream) throw std::runtime_error("Invalid file length");
            const size_t ulen = std::min<size_t>(kPacket, getPacketUlen(pkt));
            w.all_full = w.all_full && (ulen == kPacket || p + 1 == chunk.n_packets);
            w.produced += ulen;
            off += clen;
        }
        if (off != n_stream) throw std::runtime_error("Invalid file length");
        b.h_offsets[chunk.n_packets] = off;
        return w;
    }

    static std::runtime_error malformedIn(const ChunkMap::Chunk &chunk) {
        return std::runtime_error("Incorrect file format (malformed packet between file offsets " + std::to_string(chunk.begin) + " and " + std::to_string(chunk.end) + ")");
    }

    // What the trailer forbids the packets to say of themselves.  Checked in the chunk's turn (place.take), after
    // every chunk in front of it has passed: of several such packets in a file the FIRST is the one refused and
    // named, as --host does it, whichever lane gets to its chunk first.
    void refuse(const DeviceBuffers &b, const ChunkMap::Chunk &chunk, const uint8_t *bytes, uint64_t produced) const {
        for (size_t p = 0; p < chunk.n_packets; ++p) {
            const uint8_t *pkt = bytes + b.h_offsets[p];
            const size_t ulen = std::min<size_t>(kPacket, getPacketUlen(pkt));
            // (a packet that says it holds more than 8192 bytes is malformed, which the decoder would say
            // too -- but only after a CRC trailer had it called a checksum mismatch below; --host calls it
            // malformed under every trailer)
            if (getPacketUlen(pkt) > kPacket) throw malformedIn(chunk);
            // (byte planes: so every chunk but the last is whole groups, and all_full holds; raw and sparse packets: the same, so
            // that packet p of the chunk goes to byte 8192 p of it)
            if (plan.transforms() || plan.kinds) checkPlanesPacket(chunk.first_packet + p, trailer.clens.size(), ulen);
            // (a raw packet is its header and its bytes)
            if (plan.kinds && trailer.kinds[chunk.first_packet + p] == 1 && b.h_offsets[p + 1] - b.h_offsets[p] != GPUAR_PACKET_HEADER_BYTES + getPacketUlen(pkt))
                throw malformedIn(chunk);
        }
        if (plan.kinds && (produced + kPacket - 1) / kPacket != chunk.n_packets) throw std::runtime_error("Invalid file length");
        if (plan.crcs) {
            // (With this, the chunk's `produced` bytes hold exactly its n_packets packets, and the verify below covers
            // every one of them: a last packet whose ulen had become 0 would otherwise drop out of it.)
            for (size_t p = 0; p < chunk.n_packets; ++p) checkChecksumPacket(chunk.first_packet + p, trailer.crcs.size(), getPacketUlen(bytes + b.h_offsets[p]));
            if ((produced + kPacket - 1) / kPacket != chunk.n_packets) throw std::runtime_error("Invalid file length");
        }
    }

    // A decoded chunk goes to the writer, at `at` of the output, in one of two ways.  Full packets (but the last): the chunk's
    // bytes as they stand.  Short packets inside the chunk: one piece per packet.
    void drainDecoded(DeviceBuffers &b, Writer &writer, size_t c, const ChunkMap::Chunk &chunk, const uint8_t *bytes, const Walked &walked, uint64_t at) {
        if (walked.all_full) return b.drain(writer, c, b.transformed(plan), static_cast<size_t>(walked.produced), at, static_cast<size_t>(walked.produced));
        for (size_t p = 0; p < chunk.n_packets; ++p) {
            const size_t ulen = std::min<size_t>(kPacket, getPacketUlen(bytes + b.h_offsets[p]));
            if (ulen) b.drain(writer, c, b.d_plain + p * kPacket, ulen, at, ulen);
            at += ulen;
        }
    }

    // chunk c, of device g, on lane b: stream -> device -> decoded bytes -> the writer.  `staged`: the lane's room for the chunk's
    // bytes where the input is not mapped, for the header walk
    void decodeOne(size_t c, size_t g, DeviceBuffers &b, const ChunkMap::Chunk &chunk, std::vector<uint8_t> &staged, Writer &writer) {
        const size_t n_stream = static_cast<size_t>(chunk.end - chunk.begin);
        const bool from_mapping = b.upload(b.d_stream, mapped, in_fd, chunk.begin, n_stream, "Invalid file length");
        const uint8_t *bytes = mapped.data() ? mapped.data() + chunk.begin : nullptr;
        if (!bytes) {
            staged.resize(n_stream);
            sliced_io<false>(in_fd, staged.data(), n_stream, chunk.begin, "Invalid file length");
            bytes = staged.data();
        }
        const Walked walked = walkChunk(b, chunk, bytes);
        const uint64_t out_at = place.take(c, walked.produced, [&] { refuse(b, chunk, bytes, walked.produced); });
        deal.count(g, walked.produced);
        // (every packet in front of this chunk holds 8192 bytes: checkPlanesPacket)
        if (plan.based) b.uploadBase(self.baseFd, static_cast<uint64_t>(chunk.first_packet) * kPacket, static_cast<size_t>(walked.produced));
        const Decoded decoded = b.decodeChunk(chunk.n_packets, static_cast<size_t>(walked.produced), plan, plan.crcs ? trailer.crcs.data() + chunk.first_packet : nullptr,
                                              plan.kinds ? trailer.kinds.data() + chunk.first_packet : nullptr);        // (synchronises the lane's stream)
        if (from_mapping) mapped.release(chunk.begin, n_stream);
        // the file was cut short under the mapping (what was read behind its new end are zeros,
        // input_guard.hpp): the reference's short fread(), src/gpu_compressor.cpp:299-307
        if (!mapped.intact(in_fd)) throw std::runtime_error("Invalid file length");
        if (decoded.flags & GPUAR_STATUS_BAD_PACKET) throw malformedIn(chunk);
        if (decoded.flags & GPUAR_STATUS_CHECKSUM) {
            const size_t bad = chunk.first_packet + static_cast<size_t>(decoded.first_bad);
            const uint64_t begin = static_cast<uint64_t>(bad) * kPacket;
            throw checksumError(bad, begin, std::min<uint64_t>(begin + kPacket, static_cast<uint64_t>(chunk.first_packet) * kPacket + walked.produced));
        }
        drainDecoded(b, writer, c, chunk, bytes, walked, out_at);
    }

    // the lanes and the unordered writer, from the first chunk to the last byte of the output
    void decodeAll() {
        Writer writer(out_fd, false, 0, "Write uncompressed data to output file failed");
        writer.on_progress = progressTo(info, monitor);
        writer.on_failure = [&] {
            for (DeviceBuffers *b : self.buffers) b->abortWaits();
            place.abort();
        };
        std::exception_ptr lane_failure;
        try {
            self.runLanes(
                [&](size_t lane, DeviceBuffers &b, Failure &failure) {      // what one lane does: its device's chunks, as the map has them
                    const size_t g = lane / kLanesPerDevice;
                    std::vector<uint8_t> staged;        // unmapped input only: the chunk's bytes, for the header walk
                    for (;;) {
                        const size_t c = deal.take(g);
                        ChunkMap::Chunk chunk;
                        if (failure.stop || !map.get(c, chunk)) break;
                        if (c < 8) trace(("decompress: packets in chunk " + std::to_string(c) + ":").c_str(), static_cast<double>(chunk.n_packets));
                        if (!b.cap) b.allocate(self.chunkPackets, false);
                        hip_check(hipSetDevice(b.device), "hipSetDevice");
                        b.prepare(plan, false);
                        b.epoch = static_cast<hipEvent_t>(self.epochOf(g));
                        decodeOne(c, g, b, chunk, staged, writer);
                    }
                },
                [&] { writer.abort(), place.abort(); });
        } catch (...) {
            lane_failure = std::current_exception();
        }
        stopScanner();
        rethrowLaneFailure(writer, lane_failure);
        trace("decompress: lanes done");
        trace("decompress: input windows unregistered while the job ran:", static_cast<double>(mapped.windowsTrimmed()));
        deal.report("decompress", "decoded");
        (void)writer.finish(0);
    }

    void run() {
        FileHeader header;
        const size_t fileSize = self.getFileSize(self.openFile);
        if (std::fread(header.getData(), FileHeader::HEADER_LENGTH, 1, self.openFile) != 1 || !header.checkHeaderVersion())
            throw std::runtime_error("Incorrect file format");
        info = header.getInfo(fileSize);
        stream_end = streamEnd(info, fileSize);
        // How many packets to size the chunks for.  Every packet but the last holds 8192 bytes, so the header's
        // uncompressed size says; but a file written by the reference keeps only the low 32 bits of that size
        // (src/file_header.hpp:31-36) and a header can lie, so the count is bounded from below by the stream itself
        // (a packet is at most 8704 bytes long) and from above by it as well (at least 4).
        const size_t stream_bytes = static_cast<size_t>(stream_end - FileHeader::HEADER_LENGTH);
        const size_t by_header = (info.uncompressedFileSize + kPacket - 1) / kPacket;
        const size_t at_least = (stream_bytes + kSlot - 1) / kSlot, at_most = stream_bytes / GPUAR_PACKET_HEADER_BYTES + 1;
        const size_t expect_packets = std::min(std::max(by_header, at_least), at_most);
        self.ensureBuffers(expect_packets, false);
        hip_check(hipSetDevice(self.devices[0]), "hipSetDevice");
        trace("decompress: files open, device set");
        mapped.open(in_fd, fileSize);
        mapped.warmFirstWindow(self.devices[0]);
        // packet lengths, per-packet CRCs (every decoded chunk is verified against them) and the width of the byte planes the
        // packets hold (merged back on the device), as far as the file's trailer gives them (packet_index.hpp)
        trailer = self.loadTrailer(stream_end, fileSize);
        plan = PacketPlan::of(trailer);
        if (plan.based) self.openBase(info.uncompressedFileSize, "the file");
        if (trailer.indexed()) mapFromIndex();
        else scanner = std::thread([this] { scanHeaders(); });
        // what the packet count promises, allocated up front (best effort); the real length is set at the end.  A header
        // may claim anything up to 2048 times the stream's size (a packet is at least 4 bytes): the preallocation is bounded
        // by what packets can plausibly hold -- 64 times the stream (8192 zeros code to 210 bytes, 39 times) -- and the file
        // simply grows beyond that if the packets really say so.
        const size_t prealloc_packets = std::min(expect_packets, 64 * at_least);
        (void)::fallocate(out_fd, 0, 0, static_cast<off_t>(static_cast<uint64_t>(prealloc_packets) * kPacket));
        decodeAll();
        info.uncompressedFileSize = info.processedUncompressedSize = static_cast<size_t>(place.sum());     // what the packets held
        if (::ftruncate(out_fd, static_cast<off_t>(place.sum())) != 0) throw std::runtime_error("Write uncompressed data to output file failed");
        mapped.close();
        self.closeFiles();
    }
};

CompressionInfo GPUCompressor::decompress(ProgressMonitor *monitor) {
    return runJob(monitor, [&](CompressionInfo &info, int out_fd) { DecompressJob{*this, info, monitor, out_fd}.run(); });
}

}  // namespace gip
