// gzip_feed_host.cpp — the host side of the plain-gzip source (include/teloscope_mi355x_gzip.hpp: member headers, trailers, and
// zlib taking over at an exact bit with a dictionary) without a device, against gzread.  Stand-alone, g++ under ASan + UBSan.
//
//   gzip_feed_host gzread FILE OUT                  what gzread delivers; stdout: "ok" or "error"
//   gzip_feed_host reader FILE OUT WINDOW BLOCKS    what detail::GzipReader delivers; stdout: "ok <device bytes> <zlib bytes>
//                                                   <hand-overs>" or "error"
// BLOCKS = 0: no device, zlib reads every member.  BLOCKS > 0: a stand-in device that verifies BLOCKS deflate blocks per window
// (by zlib's own Z_BLOCK walk, so that it is right by construction) and then stops with a span overflow; every third call it
// verifies nothing at all; a window's end or a damaged block stops it where they stop the real one.  So the reader's
// hand-overs (inflatePrime at the chain's end bit, the last 32 KiB as dictionary, back to the device at the first boundary
// past the window) happen at many bit offsets of every file.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/teloscope_mi355x_gzip.hpp"

using namespace teloscope_mi355x::detail;

namespace {

bool read_file(const char *path, std::vector<unsigned char> &v) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    unsigned char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return true;
}

struct FakeDevice : GzipDevice {
    unsigned blocks;
    unsigned calls = 0, handovers = 0;
    std::vector<unsigned char> produced, keep;
    explicit FakeDevice(unsigned blocks_) : blocks(blocks_) {}
    void noteFallback() override { ++handovers; }
    void history(std::vector<unsigned char> &out) override { out = keep; }
    GzipWindowResult decode(const unsigned char *window, size_t n, unsigned startBit, int historyMode, const unsigned char *history,
                            size_t historyLen) override {
        std::vector<unsigned char> hist;
        if (historyMode == kGzipHistoryKept) hist = keep;
        else if (historyMode == kGzipHistoryGiven) hist.assign(history, history + historyLen);
        produced.clear();
        GzipWindowResult r;
        r.endBit = startBit; r.status = kGzipNoCandidate;
        keep = hist;
        if (++calls % 3 == 0) return r;
        z_stream z;
        memset(&z, 0, sizeof z);
        if (inflateInit2(&z, -15) != Z_OK) abort();
        size_t next = 0;
        if (startBit) { inflatePrime(&z, (int)(8 - startBit), window[0] >> startBit); next = 1; }
        if (!hist.empty()) inflateSetDictionary(&z, hist.data(), (uInt)hist.size());
        z.next_in = const_cast<Bytef *>(window + next); z.avail_in = (uInt)(n - next);
        std::vector<unsigned char> out(1 << 16);
        size_t made = 0, goodMade = 0;
        uint64_t goodBit = startBit;
        unsigned done = 0;
        int status = kGzipWindowEnd;
        for (bool first = true;; first = false) {
            if (made == out.size()) out.resize(2 * out.size());
            z.next_out = out.data() + made; z.avail_out = (uInt)(out.size() - made);
            const uInt inBefore = z.avail_in, outBefore = z.avail_out;
            const int rc = inflate(&z, Z_BLOCK);
            made = out.size() - z.avail_out;
            const uint64_t pos = 8 * (uint64_t)(n - z.avail_in) - (uint64_t)(z.data_type & 63);
            if (rc == Z_STREAM_END) { goodBit = pos; goodMade = made; status = kGzipFinalBlock; break; }
            if (rc != Z_OK && rc != Z_BUF_ERROR) { status = kGzipBadDeflate; break; }
            if (!first && (z.data_type & 128) && !(z.data_type & 64)) {
                goodBit = pos; goodMade = made;
                if (++done == blocks) { status = kGzipSpanOverflow; break; }
            }
            if (z.avail_in == inBefore && z.avail_out == outBefore && z.avail_in == 0) break;      // the window's end
        }
        inflateEnd(&z);
        produced.assign(out.begin(), out.begin() + goodMade);
        r.endBit = goodBit; r.plainBytes = goodMade; r.status = status;
        r.crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), produced.data(), (uInt)produced.size());
        keep.insert(keep.end(), produced.begin(), produced.end());
        if (keep.size() > 32768) keep.erase(keep.begin(), keep.end() - 32768);
        return r;
    }
};

int by_gzread(const char *in, const char *outp) {
    gzFile g = gzopen(in, "rb");
    FILE *out = fopen(outp, "wb");
    if (!g || !out) return 2;
    std::vector<char> buf(1 << 16);
    bool bad = false;
    for (;;) {
        const int n = gzread(g, buf.data(), (unsigned)buf.size());
        if (n < 0) { bad = true; break; }
        if (n == 0) break;
        fwrite(buf.data(), 1, (size_t)n, out);
    }
    gzclose(g);
    fclose(out);
    puts(bad ? "error" : "ok");
    return 0;
}

int by_reader(const char *in, const char *outp, size_t window, unsigned blocks) {
    std::vector<unsigned char> v;
    if (!read_file(in, v)) return 2;
    unsigned char *data = (unsigned char *)malloc(v.size() ? v.size() : 1);    // (exactly the file's bytes: a read behind them is a report)
    memcpy(data, v.data(), v.size());
    FILE *out = fopen(outp, "wb");
    if (!out) return 2;
    FakeDevice fake(blocks);
    GzipReader::Tuning tuning;
    tuning.windowBytes = window; tuning.minBytes = 0; tuning.hostPiece = 5000;
    bool bad = false;
    uint64_t deviceBytes = 0, zlibBytes = 0;
    {
        GzipReader reader(data, v.size(), 0, blocks ? &fake : nullptr, tuning);
        try {
            for (;;) {
                uint64_t len = 0;
                const char *host = nullptr;
                const GzipReader::Kind k = reader.next(len, host);
                if (k == GzipReader::None) break;
                if (k == GzipReader::OnDevice) {
                    if (len != fake.produced.size()) { fprintf(stderr, "piece and device disagree\n"); return 2; }
                    fwrite(fake.produced.data(), 1, fake.produced.size(), out);
                    deviceBytes += len;
                } else fwrite(host, 1, (size_t)len, out);
            }
        } catch (const GzipError &) { bad = true; }
        zlibBytes = reader.zlibBytes();
    }
    fclose(out);
    free(data);
    if (bad) puts("error"); else printf("ok %llu %llu %u\n", (unsigned long long)deviceBytes, (unsigned long long)zlibBytes, fake.handovers);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "gzread")) return by_gzread(argv[2], argv[3]);
    if (argc == 6 && !strcmp(argv[1], "reader")) return by_reader(argv[2], argv[3], (size_t)strtoull(argv[4], nullptr, 10), (unsigned)strtoul(argv[5], nullptr, 10));
    fprintf(stderr, "usage: gzip_feed_host gzread FILE OUT | reader FILE OUT WINDOW BLOCKS\n");
    return 2;
}
