// inflate_core_host.cpp — the deflate decoder core and the CRC arithmetic of teloscope_amd/csrc/inflate_core.h, compiled for
// the host (g++ under ASan + UBSan) with a serial policy: the functions the gfx950 kernel runs, fed damaged payloads here first.
//
//   inflate_core_host CASES RESULTS
// CASES:   u32 n, then per case u32 payload_len, u32 isize, u32 crc, payload bytes            (little-endian)
// RESULTS: per case u8 verdict (0 ok, 1 bad deflate, 2 bad CRC), u32 m, m output bytes (m = isize unless bad deflate)
// Payload and output live in heap blocks of exactly payload_len and isize bytes, so that a byte read or written outside them
// is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../teloscope_amd/csrc/inflate_core.h"

namespace {

struct HostPolicy {
    const unsigned char *payload;
    uint32_t payload_len;
    unsigned char *out;
    uint32_t isize;
    uint32_t queue[tsinf::kBatch];
    uint32_t word(uint32_t i) const {
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4; ++k) {
            const uint64_t at = (uint64_t)i * 4u + k;
            if (at < payload_len) w |= (uint32_t)payload[at] << (8 * k);
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
            if (e & tsinf::kLiteral) { out[pos++] = (unsigned char)(e & 255u); continue; }
            const uint32_t len = e & 511u, dist = e >> 9;
            for (uint32_t j = 0; j < len; ++j, ++pos) out[pos] = out[pos - dist];
        }
    }
    void copy_stored(uint32_t from, uint32_t n, uint32_t pos) { memcpy(out + pos, payload + from, n); }
};

// the device's CRC: up to 64 consecutive slices, table-driven, joined by crc_combine in a log-step reduction
uint32_t sliced_crc(const unsigned char *p, uint32_t n) {
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; ++i) table[i] = tsinf::crc_table_entry(i);
    const uint32_t slice = (n + 63u) / 64u;
    uint32_t crc[64], len[64];
    for (uint32_t l = 0; l < 64; ++l) {
        const uint32_t a = l * slice < n ? l * slice : n, b = a + slice < n ? a + slice : n;
        uint32_t c = 0xffffffffu;
        for (uint32_t i = a; i < b; ++i) c = table[(c ^ p[i]) & 255u] ^ (c >> 8);
        crc[l] = c ^ 0xffffffffu; len[l] = b - a;
    }
    for (uint32_t s = 1; s < 64; s *= 2)
        for (uint32_t l = 0; l + s < 64; l += 2 * s) {
            crc[l] = tsinf::crc_combine(crc[l], crc[l + s], len[l + s]);
            len[l] += len[l + s];
        }
    return crc[0];
}

bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: inflate_core_host CASES RESULTS\n"); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    uint32_t n = 0;
    if (!read_exact(in, &n, 4)) return 2;
    static tsinf::Tables tables;
    for (uint32_t c = 0; c < n; ++c) {
        uint32_t h[3];
        if (!read_exact(in, h, 12)) { fprintf(stderr, "short case file\n"); return 2; }
        const uint32_t payload_len = h[0], isize = h[1], crc = h[2];
        if (payload_len > (1u << 20) || isize > (1u << 20)) { fprintf(stderr, "case too large\n"); return 2; }
        unsigned char *payload = (unsigned char *)malloc(payload_len ? payload_len : 1);
        unsigned char *plain = (unsigned char *)malloc(isize ? isize : 1);
        if (!payload || !plain || !read_exact(in, payload, payload_len)) { fprintf(stderr, "short case file\n"); return 2; }
        memset(plain, 0, isize ? isize : 1);
        memset(&tables, 0xA5, sizeof tables);                       // nothing may depend on the tables of the case before
        HostPolicy pol{payload_len ? payload : nullptr, payload_len, isize ? plain : nullptr, isize, {}};
        int verdict = tsinf::inflate(pol, &tables, payload_len, isize);
        if (verdict == tsinf::kOk && sliced_crc(plain, isize) != crc) verdict = tsinf::kBadCrc;
        const unsigned char v = (unsigned char)verdict;
        const uint32_t m = verdict == tsinf::kBadDeflate ? 0u : isize;
        fwrite(&v, 1, 1, out); fwrite(&m, 4, 1, out);
        if (m) fwrite(plain, 1, m, out);
        free(payload); free(plain);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
