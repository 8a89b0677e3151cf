// gzip_core_host.cpp — the block search and the span decoder of teloscope_amd/csrc/gzip_core.h, compiled for the host (g++
// under ASan + UBSan) with a serial policy: the functions the gfx950 kernels run.  zlib is linked for the truth only.
//
//   gzip_core_host walk  STREAM OUT                 every block boundary of a raw deflate stream, by zlib's Z_BLOCK walk:
//                                                   text lines "bit plain_offset final type" (of the block that starts there;
//                                                   the stream's end is a line with type 9)
//   gzip_core_host probe STREAM OUT FROM TO ...     the bit offsets in [FROM, TO) that tsgz::probe accepts, a line each (any
//                                                   number of ranges)
//   gzip_core_host span  CASES OUT
// CASES:   u32 n, then per case u32 stream_len, start_bit, stop_bit, pos0_stop, cap, hist_len, hist_given, the stream, and
//          hist_given (0 or 32768) history bytes.  pos0_stop != 0xffffffff: the decode is done in two calls, the first with
//          this stop bit, the second going on from where the first ended (as the kernel does when it steps over a candidate)
// RESULTS: per case u32 end_bit, n_out, final_seen, status, then n_out u16 symbols, then (hist_given) n_out resolved bytes
// Stream and symbols live in heap blocks of exactly stream_len bytes and cap symbols: a byte outside them is a sanitizer report.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../teloscope_amd/csrc/gzip_core.h"

namespace {

struct HostPolicy {
    const unsigned char *stream;
    uint32_t stream_len;
    uint16_t *out;
    uint32_t cap;
    uint32_t queue[tsinf::kBatch];
    uint32_t word(uint32_t i) const {
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4; ++k) {
            const uint64_t at = (uint64_t)i * 4u + k;
            if (at < stream_len) w |= (uint32_t)stream[at] << (8 * k);
        }
        return w;
    }
    uint32_t lane() const { return 0; }
    uint32_t nlanes() const { return 1; }
    void sync() const {}
    uint32_t uni(uint32_t v) const { return v; }
    void put(uint32_t k, uint32_t e) { if (k >= tsinf::kBatch) abort(); queue[k] = e; }
    void flush(uint32_t n, uint32_t pos) {
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t e = queue[k];
            if (e & tsinf::kLiteral) { out[pos++] = (uint16_t)(e & 255u); continue; }
            const uint32_t len = e & 511u, dist = e >> 9;
            for (uint32_t j = 0; j < len; ++j, ++pos) {
                const int64_t q = (int64_t)pos - (int64_t)dist;
                out[pos] = q < 0 ? (uint16_t)(tsgz::kMarker | (uint32_t)(32768 + q)) : out[q];
            }
        }
    }
    void copy_stored(uint32_t from, uint32_t n, uint32_t pos) { for (uint32_t j = 0; j < n; ++j) out[pos + j] = stream[from + j]; }
};

bool read_file(const char *path, std::vector<unsigned char> &v) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    unsigned char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return true;
}

int walk(const char *in, const char *outp) {
    std::vector<unsigned char> s;
    if (!read_file(in, s)) return 2;
    FILE *out = fopen(outp, "w");
    if (!out) return 2;
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) return 2;
    std::vector<unsigned char> sink(1 << 16);
    z.next_in = s.data(); z.avail_in = (uInt)s.size();
    auto header = [&](uint64_t bit, uint64_t plain) {
        uint32_t h = 0;
        for (uint32_t k = 0; k < 3; ++k) { const uint64_t b = bit + k; if (b / 8 < s.size()) h |= ((s[b / 8] >> (b & 7)) & 1u) << k; }
        fprintf(out, "%llu %llu %u %u\n", (unsigned long long)bit, (unsigned long long)plain, h & 1u, h >> 1);
    };
    header(0, 0);
    for (;;) {
        z.next_out = sink.data(); z.avail_out = (uInt)sink.size();
        const int rc = inflate(&z, Z_BLOCK);
        if (rc != Z_OK && rc != Z_STREAM_END && rc != Z_BUF_ERROR) { fprintf(stderr, "zlib: %d\n", rc); return 2; }
        if (rc == Z_STREAM_END) { fprintf(out, "%llu %llu 1 9\n", 8ull * z.total_in - (z.data_type & 63), (unsigned long long)z.total_out); break; }
        if ((z.data_type & 128) && !(z.data_type & 64)) header(8ull * z.total_in - (z.data_type & 63), z.total_out);
        if (rc == Z_BUF_ERROR && z.avail_in == 0) { fprintf(stderr, "stream ends early\n"); return 2; }
    }
    inflateEnd(&z);
    return fclose(out) == 0 ? 0 : 2;
}

int probe(const char *in, const char *outp, int n_ranges, char **ranges) {
    std::vector<unsigned char> v;
    if (!read_file(in, v)) return 2;
    unsigned char *s = (unsigned char *)malloc(v.size() ? v.size() : 1);
    memcpy(s, v.data(), v.size());
    FILE *out = fopen(outp, "w");
    if (!out) return 2;
    static tsinf::Tables tables;
    HostPolicy pol{s, (uint32_t)v.size(), nullptr, 0, {}};
    for (int k = 0; k < n_ranges; ++k) {
        const uint32_t from = (uint32_t)strtoul(ranges[2 * k], nullptr, 10), to = (uint32_t)strtoul(ranges[2 * k + 1], nullptr, 10);
        for (uint32_t at = from; at < to; ++at)
            if (tsgz::probe(pol, &tables, (uint32_t)v.size(), at)) fprintf(out, "%u\n", at);
    }
    free(s);
    return fclose(out) == 0 ? 0 : 2;
}

bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int span(const char *inp, const char *outp) {
    FILE *in = fopen(inp, "rb"), *out = fopen(outp, "wb");
    if (!in || !out) return 2;
    uint32_t n = 0;
    if (!read_exact(in, &n, 4)) return 2;
    static tsinf::Tables tables;
    for (uint32_t c = 0; c < n; ++c) {
        uint32_t h[7];
        if (!read_exact(in, h, sizeof h)) { fprintf(stderr, "short case file\n"); return 2; }
        const uint32_t stream_len = h[0], start_bit = h[1], stop_bit = h[2], stop0 = h[3], cap = h[4], hist_len = h[5], hist_given = h[6];
        if (stream_len > (16u << 20) || cap > (16u << 20) || (hist_given != 0 && hist_given != 32768)) { fprintf(stderr, "bad case\n"); return 2; }
        unsigned char *stream = (unsigned char *)malloc(stream_len ? stream_len : 1);
        unsigned char *hist = (unsigned char *)malloc(hist_given ? hist_given : 1);
        uint16_t *sym = (uint16_t *)malloc(cap ? 2 * (size_t)cap : 2);
        if (!stream || !hist || !sym || !read_exact(in, stream, stream_len) || !read_exact(in, hist, hist_given)) { fprintf(stderr, "short case file\n"); return 2; }
        memset(sym, 0xEE, cap ? 2 * (size_t)cap : 2);
        memset(&tables, 0xA5, sizeof tables);
        HostPolicy pol{stream, stream_len, sym, cap, {}};
        tsgz::SpanResult r;
        if (stop0 != 0xffffffffu) {
            r = tsgz::inflate_span(pol, &tables, stream_len, start_bit, stop0, 0, cap, hist_len);
            if (r.status == tsgz::kSpanStop) r = tsgz::inflate_span(pol, &tables, stream_len, r.end_bit, stop_bit, r.n_out, cap, hist_len);
        } else r = tsgz::inflate_span(pol, &tables, stream_len, start_bit, stop_bit, 0, cap, hist_len);
        if (r.n_out > cap) { fprintf(stderr, "n_out beyond cap\n"); return 2; }
        fwrite(&r, sizeof r, 1, out);
        fwrite(sym, 2, r.n_out, out);
        if (hist_given) {
            std::vector<unsigned char> bytes(r.n_out);
            for (uint32_t i = 0; i < r.n_out; ++i) bytes[i] = (unsigned char)tsgz::resolve(sym[i], hist);
            if (!bytes.empty()) fwrite(bytes.data(), 1, bytes.size(), out);
        }
        free(stream); free(hist); free(sym);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "walk")) return walk(argv[2], argv[3]);
    if (argc >= 6 && argc % 2 == 0 && !strcmp(argv[1], "probe")) return probe(argv[2], argv[3], (argc - 4) / 2, argv + 4);
    if (argc == 4 && !strcmp(argv[1], "span")) return span(argv[2], argv[3]);
    fprintf(stderr, "usage: gzip_core_host walk STREAM OUT | probe STREAM OUT FROM TO ... | span CASES OUT\n");
    return 2;
}
