// pipeline_parts_test.cpp -- the HIP-free core of the GPU file pipeline (gpuar_amd/csrc/host/pipeline_parts.hpp) on the CPU: the
// writer in both of its modes, a writer whose pwrite fails, abort() with pieces queued, the chunks' turn at the output offset and
// the chunk map, each driven from several threads.  tests/test_pipeline_parts.py builds this file under the thread sanitizer and
// under the address and undefined-behaviour sanitizers and runs both.
//
//   pipeline_parts_test FILE      FILE: a scratch file the writers write; prints "pipeline parts ok"
#include <fcntl.h>
#include <unistd.h>

#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "pipeline_parts.hpp"

using namespace gip::pipeline;

namespace {

#define REQUIRE(cond)                                                            \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

constexpr size_t kChunks = 12, kThreads = 4;

// chunk c: 1 .. 3 pieces of 1 .. 5 KiB and a few odd bytes, every byte a function of its place in the chunk
struct Chunks {
    std::vector<std::vector<std::vector<uint8_t>>> pieces;      // [chunk][piece]
    std::vector<uint64_t> begin;                                // prefix sums of the chunks' lengths; one entry more: the total
    Chunks() : pieces(kChunks), begin(kChunks + 1, 0) {
        for (size_t c = 0; c < kChunks; ++c) {
            size_t n = 0;
            for (size_t k = 0; k < 1 + c % 3; ++k) {
                pieces[c].emplace_back(1024 * (1 + (c + 2 * k) % 5) + 7 * c + k);
                for (auto &byte : pieces[c].back()) byte = static_cast<uint8_t>(31 * c + 7 * k + n++);
            }
            begin[c + 1] = begin[c] + n;
        }
    }
    std::vector<uint8_t> all() const {
        std::vector<uint8_t> out;
        for (const auto &chunk : pieces)
            for (const auto &piece : chunk) out.insert(out.end(), piece.begin(), piece.end());
        return out;
    }
};

// how often every give_back of a test ran
struct GiveBacks {
    std::vector<std::atomic<int>> count;
    explicit GiveBacks(size_t n) : count(n) {
        for (auto &c : count) c = 0;
    }
};

std::vector<uint8_t> read_back(const char *path) {
    std::vector<uint8_t> out;
    FILE *f = std::fopen(path, "rb");
    REQUIRE(f);
    uint8_t buf[4096];
    for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + got);
    std::fclose(f);
    return out;
}

// thread t of kThreads takes the chunks of `order` at t, t + kThreads ... and submits their first `most` pieces, in order within a chunk
template <typename PieceOf>
void submit_all(Writer &writer, const Chunks &chunks, const std::vector<size_t> &order, size_t most, PieceOf &&piece_of) {
    std::vector<std::thread> producers;
    for (size_t t = 0; t < kThreads; ++t)
        producers.emplace_back([&, t] {
            for (size_t i = t; i < order.size(); i += kThreads)
                for (size_t k = 0; k < std::min(most, chunks.pieces[order[i]].size()); ++k) writer.submit(order[i], piece_of(order[i], k));
        });
    for (auto &p : producers) p.join();
}

void writers_write(const char *path, bool ordered) {
    const Chunks chunks;
    const std::vector<size_t> scrambled = {7, 2, 11, 0, 5, 9, 3, 1, 10, 4, 8, 6};
    GiveBacks gave(kChunks * 3);
    std::atomic<uint64_t> progress{0};
    const uint64_t start = ordered ? 20 : 0;      // (the ordered writer starts behind a header, as compress has it)
    const int fd = ::open(path, O_RDWR | O_CREAT | O_TRUNC, 0600);
    REQUIRE(fd >= 0);
    Writer writer(fd, ordered, start, "write failed");
    writer.on_progress = [&](size_t plain) { progress += plain; };
    submit_all(writer, chunks, scrambled, 3, [&](size_t c, size_t k) {
        const auto &bytes = chunks.pieces[c][k];
        Piece p;
        p.data = const_cast<uint8_t *>(bytes.data());
        p.bytes = bytes.size();
        p.at = chunks.begin[c];
        for (size_t j = 0; j < k; ++j) p.at += chunks.pieces[c][j].size();
        p.last_of_chunk = k + 1 == chunks.pieces[c].size();
        p.plain_bytes = p.last_of_chunk ? 3 * (chunks.begin[c + 1] - chunks.begin[c]) : 0;
        p.give_back = [&gave, c, k] { ++gave.count[3 * c + k]; };
        return p;
    });
    const uint64_t end = writer.finish(kChunks);
    if (ordered) REQUIRE(end == start + chunks.begin[kChunks]);       // the summed length, behind where it started
    REQUIRE(progress == 3 * chunks.begin[kChunks]);
    for (size_t c = 0; c < kChunks; ++c)
        for (size_t k = 0; k < 3; ++k) REQUIRE(gave.count[3 * c + k] == (k < chunks.pieces[c].size() ? 1 : 0));
    ::close(fd);
    const std::vector<uint8_t> file = read_back(path), want = chunks.all();
    REQUIRE(file.size() == start + want.size());
    REQUIRE(std::memcmp(file.data() + start, want.data(), want.size()) == 0);
}

// a descriptor opened read-only: the first pwrite fails
void writer_fails(const char *path) {
    const Chunks chunks;
    GiveBacks gave(kChunks + 1);
    std::atomic<int> failures{0};
    const int fd = ::open(path, O_RDONLY);
    REQUIRE(fd >= 0);
    Writer writer(fd, true, 0, "write failed");
    writer.on_failure = [&] { ++failures; };
    const auto piece_of = [&](size_t c) {
        Piece p;
        p.data = const_cast<uint8_t *>(chunks.pieces[c][0].data());
        p.bytes = chunks.pieces[c][0].size();
        p.last_of_chunk = true;
        p.give_back = [&gave, c] { ++gave.count[c]; };
        return p;
    };
    // chunk 0 last: everything else is queued behind it when the writer meets it, or is given straight back after it failed
    std::vector<size_t> order;
    for (size_t c = kChunks; c-- > 0;) order.push_back(c);
    submit_all(writer, chunks, order, 1, [&](size_t c, size_t) { return piece_of(c); });
    bool thrown = false;
    try {
        (void)writer.finish(kChunks);
    } catch (const std::runtime_error &e) {
        thrown = std::string(e.what()) == "write failed";
    }
    REQUIRE(thrown);
    REQUIRE(failures == 1);
    for (size_t c = 0; c < kChunks; ++c) REQUIRE(gave.count[c] == 1);
    // a later submit gives its piece straight back
    Piece late = piece_of(0);
    late.give_back = [&gave] { ++gave.count[kChunks]; };
    writer.submit(0, std::move(late));
    REQUIRE(gave.count[kChunks] == 1);
    ::close(fd);
}

// abort() with pieces queued that the ordered writer cannot reach (chunk 0 never comes)
void writer_aborts(const char *path) {
    const Chunks chunks;
    GiveBacks gave(kChunks);
    const int fd = ::open(path, O_RDWR | O_CREAT | O_TRUNC, 0600);
    REQUIRE(fd >= 0);
    {
        Writer writer(fd, true, 0, "write failed");
        std::vector<size_t> order;
        for (size_t c = 1; c < kChunks; ++c) order.push_back(c);
        submit_all(writer, chunks, order, 1, [&](size_t c, size_t) {
            Piece p;
            p.data = const_cast<uint8_t *>(chunks.pieces[c][0].data());
            p.bytes = chunks.pieces[c][0].size();
            p.last_of_chunk = true;
            p.give_back = [&gave, c] { ++gave.count[c]; };
            return p;
        });
        writer.abort();
        REQUIRE(writer.finish(0) == 0);           // nothing was written, nothing failed
    }
    for (size_t c = 1; c < kChunks; ++c) REQUIRE(gave.count[c] == 1);
    ::close(fd);
    REQUIRE(read_back(path).empty());
}

void ordered_offsets() {
    {
        // take() from threads started in reverse order: the prefix sums, whoever comes first
        OrderedOffsets place;
        std::vector<uint64_t> got(kChunks, ~0ull);
        std::vector<int> checked(kChunks, 0);
        std::vector<std::thread> takers;
        for (size_t c = kChunks; c-- > 0;)
            takers.emplace_back([&, c] { got[c] = place.take(c, 100 * c + 1, [&] { ++checked[c]; }); });
        for (auto &t : takers) t.join();
        uint64_t sum = 0;
        for (size_t c = 0; c < kChunks; ++c) {
            REQUIRE(got[c] == sum && checked[c] == 1);
            sum += 100 * c + 1;
        }
        REQUIRE(place.sum() == sum);
    }
    {
        // a check that throws does not pass the turn on; abort() releases who waits behind it
        OrderedOffsets place;
        std::atomic<int> stopped{0}, refused{0};
        std::vector<std::thread> takers;
        for (size_t c = 1; c < 4; ++c)
            takers.emplace_back([&, c] {
                try {
                    (void)place.take(c, 10, [&] {
                        if (c == 1) throw std::runtime_error("refused");
                    });
                    REQUIRE(!"a chunk behind the refused one got its turn");
                } catch (const std::runtime_error &e) {
                    if (std::string(e.what()) == "refused") ++refused;
                    if (std::string(e.what()) == "pipeline stopped") ++stopped;
                }
            });
        REQUIRE(place.take(0, 5, [] {}) == 0);
        takers[0].join();                          // chunk 1 has been refused: chunks 2 and 3 wait, or are about to
        REQUIRE(refused == 1 && place.sum() == 5);
        place.abort();
        takers[1].join();
        takers[2].join();
        REQUIRE(stopped == 2 && place.sum() == 5);
    }
}

void chunk_map() {
    {
        // get() blocks until push(), and says false after finish()
        ChunkMap map;
        std::vector<ChunkMap::Chunk> got(kChunks);
        std::atomic<size_t> found{0}, missing{0};
        std::vector<std::thread> getters;
        for (size_t c = 0; c < kChunks + 2; ++c)
            getters.emplace_back([&, c] {
                ChunkMap::Chunk chunk;
                if (map.get(c, chunk)) got[c] = chunk, ++found;
                else ++missing;
            });
        for (size_t c = 0; c < kChunks; ++c) {
            ChunkMap::Chunk chunk;
            chunk.begin = 20 + 1000 * c;
            chunk.end = chunk.begin + 1000;
            chunk.n_packets = c + 1;
            chunk.first_packet = c * (c + 1) / 2;
            REQUIRE(found <= c && missing == 0);      // nobody got a chunk that was not pushed yet
            map.push(chunk);
        }
        map.finish();
        for (auto &g : getters) g.join();
        REQUIRE(found == kChunks && missing == 2);
        for (size_t c = 0; c < kChunks; ++c) REQUIRE(got[c].begin == 20 + 1000 * c && got[c].n_packets == c + 1 && got[c].first_packet == c * (c + 1) / 2);
    }
    {
        // finish(error): a chunk that is there is still handed out, one that is not rethrows
        ChunkMap map;
        std::atomic<int> rethrown{0};
        std::thread waiter([&] {
            ChunkMap::Chunk chunk;
            try {
                (void)map.get(1, chunk);
            } catch (const std::runtime_error &e) {
                if (std::string(e.what()) == "scan failed") ++rethrown;
            }
        });
        map.push(ChunkMap::Chunk());
        map.finish(std::make_exception_ptr(std::runtime_error("scan failed")));
        waiter.join();
        ChunkMap::Chunk chunk;
        REQUIRE(rethrown == 1 && map.get(0, chunk));
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    writers_write(argv[1], true);
    writers_write(argv[1], false);
    writer_fails(argv[1]);
    writer_aborts(argv[1]);
    ordered_offsets();
    chunk_map();
    Failure failure;
    failure.set(std::make_exception_ptr(std::runtime_error("first")));
    failure.set(std::make_exception_ptr(std::runtime_error("second")));
    try {
        std::rethrow_exception(failure.first);
    } catch (const std::runtime_error &e) {
        REQUIRE(failure.stop && std::string(e.what()) == "first");
    }
    std::printf("pipeline parts ok\n");
    return 0;
}
