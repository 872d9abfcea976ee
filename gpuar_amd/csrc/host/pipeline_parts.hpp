// pipeline_parts.hpp -- what the GPU file pipeline (gpu_compressor.cpp) is built from that never touches the HIP runtime: the
// trace, sliced file I/O, and the concurrency core -- the pieces that travel between the lanes and the one writer thread, the
// map of chunks the lanes wait on, the chunks' turn at the output offset, and the first failure of a job.  Plain C++ and POSIX,
// so that tests/pipeline_parts_test.cpp can drive it on the CPU under the thread and address sanitizers.
#pragma once
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <stdexcept>
#include <thread>
#include <vector>

namespace gip::pipeline {

constexpr size_t kIoSlice = 16u << 20;     // a pread / pwrite is cut into slices of this size, one helper thread each
constexpr size_t kIoThreads = 4;           // ... at most this many at a time

// GPUAR_TRACE=1: a timeline of the pipeline on stderr (seconds since the first call), for tools/cli_timing.sh
inline double trace_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline void trace(const char *what, double value = -1) {
    static const bool on = std::getenv("GPUAR_TRACE") != nullptr;
    static const double t0 = trace_now();
    static std::mutex lock;
    if (!on) return;
    std::lock_guard<std::mutex> hold(lock);
    if (value >= 0) std::fprintf(stderr, "[gpuar %8.3f s] %s %.3f\n", trace_now() - t0, what, value);
    else std::fprintf(stderr, "[gpuar %8.3f s] %s\n", trace_now() - t0, what);
}

// pread / pwrite of a large range, cut into slices that run on a few threads
template <bool kWrite>
void sliced_io(int fd, uint8_t *buf, size_t n, uint64_t at, const char *error) {
    const size_t slices = std::max<size_t>(1, std::min(kIoThreads, (n + kIoSlice - 1) / kIoSlice));
    const size_t per = ((n + slices - 1) / slices + 4095) & ~static_cast<size_t>(4095);
    std::atomic<bool> failed{false};
    auto run = [&](size_t k) {
        size_t done = std::min(n, k * per);
        const size_t end = std::min(n, done + per);
        while (done < end) {
            const ssize_t got = kWrite ? ::pwrite(fd, buf + done, end - done, static_cast<off_t>(at + done))
                                       : ::pread(fd, buf + done, end - done, static_cast<off_t>(at + done));
            if (got <= 0) {
                failed = true;
                return;
            }
            done += static_cast<size_t>(got);
        }
    };
    std::vector<std::thread> helpers;
    for (size_t k = 1; k < slices; ++k) helpers.emplace_back(run, k);
    run(0);
    for (auto &h : helpers) h.join();
    if (failed) throw std::runtime_error(error);
}

// A pinned buffer handed from a lane to the writer and back.
struct Piece {
    uint8_t *data = nullptr;
    size_t bytes = 0;
    uint64_t at = 0;           // file offset (unordered mode); ignored when the writer keeps the running offset
    bool last_of_chunk = false;
    size_t plain_bytes = 0;    // uncompressed bytes this piece completes (progress line)
    std::function<void()> give_back;
};

// The writer: ONE thread that turns pieces into pwrite()s.
//   ordered (compress): chunk c is written behind chunk c-1 -- where it starts is the sum of what came before,
//       the pipeline's one serial quantity, which this thread simply carries; pieces of a chunk arrive in order.
//   unordered (decompress): every piece knows its own file offset; pieces are written as they arrive.
class Writer {
  public:
    Writer(int fd, bool ordered, uint64_t start, const char *error) : fd(fd), ordered(ordered), at(start), error(error) {
        worker = std::thread([this] { run(); });
    }
    ~Writer() {
        abort();
        if (worker.joinable()) worker.join();
    }
    void submit(size_t chunk, Piece p) {
        std::lock_guard<std::mutex> hold(lock);
        if (aborted) {
            if (p.give_back) p.give_back();
            return;
        }
        queues[ordered ? chunk : 0].push_back(std::move(p));
        wake.notify_all();
    }
    // no more pieces will come; waits for everything submitted to be written and rethrows the writer's failure
    uint64_t finish(size_t n_chunks) {
        {
            std::lock_guard<std::mutex> hold(lock);
            expect_chunks = n_chunks;
            closing = true;
            wake.notify_all();
        }
        if (worker.joinable()) worker.join();
        if (failure) std::rethrow_exception(failure);
        return at;
    }
    void abort() {
        std::lock_guard<std::mutex> hold(lock);
        aborted = true;
        wake.notify_all();
    }
    std::function<void(size_t)> on_progress;      // called with the plain bytes of every piece written
    std::function<void()> on_failure;             // the writer itself failed (disk full ...): lets the lanes go

  private:
    void run() {
        try {
            for (;;) {
                Piece p;
                {
                    std::unique_lock<std::mutex> hold(lock);
                    const size_t key = 0;
                    wake.wait(hold, [&] {
                        if (aborted) return true;
                        auto it = queues.find(ordered ? next_chunk : key);
                        if (it != queues.end() && !it->second.empty()) return true;
                        return closing && (!ordered || next_chunk >= expect_chunks);
                    });
                    if (aborted) break;
                    auto it = queues.find(ordered ? next_chunk : key);
                    if (it == queues.end() || it->second.empty()) break;          // closing and drained
                    p = std::move(it->second.front());
                    it->second.pop_front();
                    if (ordered && p.last_of_chunk) {
                        queues.erase(it);
                        ++next_chunk;
                    }
                }
                try {
                    const double w0 = trace_now();
                    if (first_write < 0) first_write = w0, trace("writer: first piece");
                    if (p.bytes) sliced_io<true>(fd, p.data, p.bytes, ordered ? at : p.at, error);
                    busy_s += trace_now() - w0;
                    bytes_written += p.bytes;
                } catch (...) {
                    if (p.give_back) p.give_back();
                    throw;
                }
                if (ordered) at += p.bytes;
                if (p.give_back) p.give_back();
                if (on_progress) on_progress(p.plain_bytes);
            }
        } catch (...) {
            failure = std::current_exception();
        }
        if (first_write >= 0) {
            trace("writer: done; seconds inside pwrite:", busy_s);
            trace("writer: GB/s while writing:", bytes_written / std::max(busy_s, 1e-9) / 1e9);
            trace("writer: seconds between first piece and last:", trace_now() - first_write);
        }
        // whatever is still queued goes back to its lane (which may be waiting for it)
        {
            std::lock_guard<std::mutex> hold(lock);
            aborted = true;
            for (auto &q : queues)
                for (auto &p : q.second)
                    if (p.give_back) p.give_back();
            queues.clear();
        }
        if (failure && on_failure) on_failure();
    }

    int fd;
    bool ordered;
    uint64_t at;
    const char *error;
    std::mutex lock;
    std::condition_variable wake;
    std::map<size_t, std::deque<Piece>> queues;
    size_t next_chunk = 0, expect_chunks = 0;
    bool closing = false, aborted = false;
    std::exception_ptr failure;
    std::thread worker;
    double first_write = -1, busy_s = 0, bytes_written = 0;
};

// Keeps the first failure of any lane and tells the others to stop.
struct Failure {
    std::mutex lock;
    std::exception_ptr first;
    std::atomic<bool> stop{false};
    void set(std::exception_ptr e) {
        std::lock_guard<std::mutex> hold(lock);
        if (!first) first = e;
        stop = true;
    }
};

// Where the packets of each chunk sit in the stream.  Filled by the index trailer in one go, or by
// the scanner thread as it walks the headers; lanes wait for the chunk they are about to take.
struct ChunkMap {
    struct Chunk {
        uint64_t begin = 0, end = 0;     // file offsets of the chunk's first byte / one past its last
        size_t n_packets = 0;
        size_t first_packet = 0;         // index of its first packet in the file
    };
    std::mutex lock;
    std::condition_variable more;
    std::vector<Chunk> chunks;
    bool complete = false;
    std::exception_ptr failure;

    void push(const Chunk &c) {
        std::lock_guard<std::mutex> hold(lock);
        chunks.push_back(c);
        more.notify_all();
    }
    void finish(std::exception_ptr e = nullptr) {
        std::lock_guard<std::mutex> hold(lock);
        complete = true;
        failure = e;
        more.notify_all();
    }
    // false: there is no chunk c
    bool get(size_t c, Chunk &out) {
        std::unique_lock<std::mutex> hold(lock);
        more.wait(hold, [&] { return c < chunks.size() || complete; });
        if (c < chunks.size()) {
            out = chunks[c];
            return true;
        }
        if (failure) std::rethrow_exception(failure);
        return false;
    }
};

// The running total of what the chunks before chunk c decode to (a stream may hold short packets in its middle:
// the output offset of a chunk is then not c * chunk bytes).  take(c, n) blocks until chunks 0..c-1 have called and
// returns the total before chunk c's own n bytes; it is called before the chunk's kernels, so nobody waits for it long.
class OrderedOffsets {
  public:
    // `check` runs once it is the chunk's turn; if it throws, the turn is never passed on, and the chunks behind wait until abort()
    template <typename Check>
    uint64_t take(size_t chunk, uint64_t bytes, Check &&check) {
        std::unique_lock<std::mutex> hold(lock);
        turn.wait(hold, [&] { return aborted || next == chunk; });
        if (aborted) throw std::runtime_error("pipeline stopped");
        check();
        const uint64_t mine = total;
        total += bytes;
        ++next;
        turn.notify_all();
        return mine;
    }
    void abort() {
        std::lock_guard<std::mutex> hold(lock);
        aborted = true;
        turn.notify_all();
    }
    uint64_t sum() {
        std::lock_guard<std::mutex> hold(lock);
        return total;
    }

  private:
    std::mutex lock;
    std::condition_variable turn;
    size_t next = 0;
    uint64_t total = 0;
    bool aborted = false;
};

}  // namespace gip::pipeline
