// gzip_device_cli.cpp — TEST INFRASTRUCTURE: a file through detail::ChunkFeed (include/teloscope_mi355x_io.hpp) into a device
// chunk, `want` bytes at a time, and the chunk's bytes back to stdout: what the three text routes are fed, without a route
// around it.  TS_GZIP_DEVICE, TS_GZIP_SPAN, TS_GZIP_WINDOW and TS_GZIP_MIN_BYTES choose how plain gzip is read.
// Usage: gzip_device_cli FILE [WANT]
//        gzip_device_cli --each LIST [WANT]   every file named in LIST through one context: <file>.out, and <file>.ok or
//                                             <file>.err with the message (the convention of fastq_device_cli)
// stderr's last line: "source=<0..3> windows=.. probed=.. chained=.. dropped=.. device_bytes=.. zlib_parts=.. total=.."
// (ts_gzip_stats), or "Error: <message>" with exit status 1.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "teloscope_mi355x_io.hpp"

using namespace teloscope_mi355x;

// FILE through a feed of its own into `out`; -> the bytes delivered
static uint64_t feedFile(ts_ctx *ctx, const std::string &file, size_t want, FILE *out, int *source) {
    detail::ChunkFeed::Options options;
    options.cannotOpen = "cannot open";
    options.cannotRead = "cannot read";
    detail::ChunkFeed feed(ctx, file, options);
    struct ChunkPtr { ts_chunk *p; ~ChunkPtr() { ts_bam_chunk_destroy(p); } } chunk{ts_bam_chunk_create(ctx, feed.compCap(want), std::max<size_t>(want, 64))};
    if (!chunk.p) throw detail::deviceError(ctx, "cannot make the device chunk");
    std::vector<char> buf;
    uint64_t total = 0;
    *source = static_cast<int>(feed.source());
    for (bool end = false; !end;) {
        end = feed.fill(chunk.p, ts_bam_chunk_size(chunk.p), want);
        const uint64_t n = ts_bam_chunk_size(chunk.p);
        buf.resize(static_cast<size_t>(n));
        if (n && ts_bam_chunk_read(chunk.p, 0, n, buf.data()) != TS_OK) throw detail::deviceError(ctx, "cannot read the chunk");
        if (n && fwrite(buf.data(), 1, static_cast<size_t>(n), out) != n) throw std::runtime_error("cannot write");
        total += n;
    }
    return total;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: gzip_device_cli FILE [WANT] | --each LIST [WANT]\n"); return 2; }
    const bool each = std::string(argv[1]) == "--each";
    if (each && argc < 3) return 2;
    const std::string file = argv[each ? 2 : 1];
    const int wantAt = each ? 3 : 2;
    const size_t want = argc > wantAt ? static_cast<size_t>(std::strtoull(argv[wantAt], nullptr, 10)) : size_t(4) << 20;
    try {
        UserInputTeloscope ui;
        ui.rawPatterns = {ui.canonicalFwd, ui.canonicalRev};
        ui.patternInfo = expandPatternsWithOrientation(ui.rawPatterns, ui.editDistance, ui.canonicalFwd);
        ReadTelomereFilter filter(ui);
        filter.bindThreadToDevice();
        ts_ctx *ctx = filter.context(0);
        int source = -1;
        uint64_t total = 0;
        if (each) {
            std::ifstream list(file);
            std::string path;
            while (std::getline(list, path)) {
                if (path.empty()) continue;
                FILE *out = fopen((path + ".out").c_str(), "wb");
                if (!out) throw std::runtime_error("cannot write");
                try {
                    total += feedFile(ctx, path, want, out, &source);
                    fclose(out);
                    std::ofstream(path + ".ok") << "ok\n";
                } catch (const std::exception &e) {
                    fclose(out);
                    std::ofstream(path + ".err") << e.what() << "\n";
                }
            }
        } else {
            total = feedFile(ctx, file, want, stdout, &source);
            fflush(stdout);
        }
        uint64_t s[6] = {0, 0, 0, 0, 0, 0};
        ts_gzip_stats(ctx, s);
        fprintf(stderr, "source=%d windows=%llu probed=%llu chained=%llu dropped=%llu device_bytes=%llu zlib_parts=%llu total=%llu\n", source,
                (unsigned long long)s[0], (unsigned long long)s[1], (unsigned long long)s[2], (unsigned long long)s[3],
                (unsigned long long)s[4], (unsigned long long)s[5], (unsigned long long)total);
        return 0;
    } catch (const std::exception &e) {
        fflush(stdout);
        fprintf(stderr, "Error: %s\n", e.what());
        return 1;
    }
}
