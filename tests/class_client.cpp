// class_client.cpp -- drives gip::Compressor objects as a LIBRARY user would: several objects, many jobs per object, settings
// changed between jobs, failing jobs followed by good ones, objects deleted and created in mid-process, and an ordinary
// return from main() with static destructors and runtime teardown (host/main.cpp runs one job and leaves through _Exit).
// Test-only (tests/test_class_api.py builds it into tests/_build/); never linked into a product.
//
//   class_client [--results=FILE] [COMMAND ...]        (no COMMAND on the command line: the script is read from stdin)
//
//   new cpu|gpu NAME     create an object and make it the current one
//   use NAME             make NAME the current object
//   delete NAME          destroy it
//   threads N | batch N | device N | gpus N | index 0|1 | checksum 0|1 | quiet 0|1      settings of the current object
//   c IN OUT | d IN OUT  compress / decompress with the current object
//
// Every command answers with ONE line on the results channel (stderr, or FILE), which the progress text on stdout cannot
// mix into:   ok <command> [key=value ...]     or     error <command>: <what()>
// A job's `ok` line carries every CompressionInfo field and the wall milliseconds measured around the call.
// Exit code: 0, or 2 when the script itself is malformed (unknown command, missing argument, unknown or duplicate NAME).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "cpu_compressor.hpp"
#ifndef GPUAR_HOST_ONLY
#include "gpu_compressor.hpp"
#endif

using namespace gip;

namespace {

struct Object {
    std::unique_ptr<Compressor> compressor;
    ProgressMonitor monitor;
};

struct Malformed : std::runtime_error {
    using std::runtime_error::runtime_error;
};

FILE *results = stderr;

void say_ok(const std::string &command, const std::string &rest = "") {
    std::cout.flush();
    std::fprintf(results, "ok %s%s%s\n", command.c_str(), rest.empty() ? "" : " ", rest.c_str());
    std::fflush(results);
}
void say_error(const std::string &command, const std::string &what) {
    std::cout.flush();
    std::fprintf(results, "error %s: %s\n", command.c_str(), what.c_str());
    std::fflush(results);
}

long number(const std::string &command, const std::string &text) {
    char *end = nullptr;
    const long v = std::strtol(text.c_str(), &end, 10);
    if (text.empty() || *end) throw Malformed(command + ": not a number: " + text);
    return v;
}

}  // namespace

int main(int argc, char **argv) {
    std::vector<std::string> words;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a.rfind("--results=", 0) == 0) {
            results = std::fopen(a.c_str() + 10, "w");
            if (!results) {
                std::fprintf(stderr, "class_client: cannot open %s\n", a.c_str() + 10);
                return 2;
            }
        } else {
            words.push_back(a);
        }
    }
    if (words.empty())
        for (std::string w; std::cin >> w;) words.push_back(w);

    int code = 0;
    {
        std::map<std::string, std::unique_ptr<Object>> objects;
        Object *current = nullptr;
        size_t at = 0;
        auto next = [&](const std::string &command) {
            if (at >= words.size()) throw Malformed(command + ": argument missing");
            return words[at++];
        };
        try {
            while (at < words.size()) {
                const std::string command = words[at++];
                if (command == "new") {
                    const std::string kind = next(command), name = next(command);
                    if (objects.count(name)) throw Malformed("new: " + name + " exists");
                    if (kind != "cpu" && kind != "gpu") throw Malformed("new: cpu or gpu, not " + kind);
                    try {
                        std::unique_ptr<Object> o(new Object());
                        if (kind == "cpu") {
                            o->compressor.reset(new CPUCompressor());
                        } else {
#ifdef GPUAR_HOST_ONLY
                            throw std::runtime_error("this build has no GPU path");
#else
                            o->compressor.reset(new GPUCompressor());
#endif
                        }
                        o->monitor.setQuiet(true);
                        current = o.get();
                        objects[name] = std::move(o);
                        say_ok(command);
                    } catch (const std::exception &e) {
                        say_error(command, e.what());
                    }
                    continue;
                }
                if (command == "use" || command == "delete") {
                    const std::string name = next(command);
                    auto it = objects.find(name);
                    if (it == objects.end()) throw Malformed(command + ": no object " + name);
                    if (command == "use") {
                        current = it->second.get();
                    } else {
                        if (current == it->second.get()) current = nullptr;
                        objects.erase(it);
                    }
                    say_ok(command);
                    continue;
                }
                const bool job = command == "c" || command == "d";
                const bool setting = command == "threads" || command == "batch" || command == "device" || command == "gpus" ||
                                     command == "index" || command == "checksum" || command == "quiet";
                if (!job && !setting) throw Malformed("unknown command: " + command);
                const std::string first = next(command), second = job ? next(command) : "";
                const long n = job ? 0 : number(command, first);
                if (!current) {
                    say_error(command, "no current object");
                    continue;
                }
                try {
                    if (job) {
                        current->compressor->setOpenFileName(first);
                        current->compressor->setSaveFileName(second);
                        const auto t0 = std::chrono::steady_clock::now();
                        const CompressionInfo info = command == "c" ? current->compressor->compress(&current->monitor)
                                                                    : current->compressor->decompress(&current->monitor);
                        const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                        char text[512];
                        std::snprintf(text, sizeof text,
                                      "ratio=%.17g processTime=%.17g ioTime=%.17g processedUncompressedSize=%zu compressedFileSize=%zu "
                                      "uncompressedFileSize=%zu wall_ms=%.17g",
                                      info.ratio, info.processTime, info.ioTime, info.processedUncompressedSize, info.compressedFileSize,
                                      info.uncompressedFileSize, wall);
                        say_ok(command, text);
                    } else if (command == "index") {
                        current->compressor->setWriteIndex(n != 0);
                        say_ok(command);
                    } else if (command == "checksum") {
                        current->compressor->setWriteChecksum(n != 0);
                        say_ok(command);
                    } else if (command == "quiet") {
                        current->monitor.setQuiet(n != 0);
                        say_ok(command);
                    } else if (command == "threads") {
                        auto *cpu = dynamic_cast<CPUCompressor *>(current->compressor.get());
                        if (!cpu) throw std::runtime_error("not a cpu object");
                        cpu->setThreads(static_cast<unsigned>(n < 0 ? 1 : n));
                        say_ok(command);
                    } else {
#ifdef GPUAR_HOST_ONLY
                        throw std::runtime_error("not a gpu object");
#else
                        auto *gpu = dynamic_cast<GPUCompressor *>(current->compressor.get());
                        if (!gpu) throw std::runtime_error("not a gpu object");
                        if (command == "batch") gpu->setBatchPackets(static_cast<size_t>(n < 0 ? 0 : n));
                        else if (command == "device") gpu->chooseDevice(static_cast<int>(n));
                        else gpu->useDevices(static_cast<int>(n));
                        say_ok(command);
#endif
                    }
                } catch (const std::exception &e) {
                    say_error(command, e.what());
                }
            }
        } catch (const Malformed &e) {
            std::fprintf(stderr, "class_client: %s\n", e.what());
            code = 2;
        }
    }      // (the objects still alive are destroyed here, before main returns)
    if (results != stderr) std::fclose(results);
    return code;
}
