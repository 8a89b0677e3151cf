// deflate_core_host.cpp — the deflate encoder core of teloscope_amd/csrc/deflate_core.h, compiled for the host (g++, under
// ASan + UBSan in tests/test_deflate_core_cpu.py) with a serial policy: the functions the gfx950 kernel runs.
//
//   deflate_core_host BLOCKS RESULTS
// BLOCKS:  u32 n, then per block u32 len, len plain bytes                                      (little-endian)
// RESULTS: per block u32 payload_len, u32 crc32 (as the core computed it), payload bytes
//   deflate_core_host --lengths CASES RESULTS
// CASES:   u32 n, then per case u32 symbols (<= 288), u32 limit, symbols x u32 counts
// RESULTS: per case symbols x u8 code lengths (tsdef::build_lengths alone)
// The plain bytes live in a heap block of exactly len bytes and the payload in one of exactly the dwords the core may touch, so
// that a byte read or written outside them is a sanitizer report; an index the policy is not to be asked for aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../teloscope_amd/csrc/deflate_core.h"

namespace {

struct HostPolicy {
    const unsigned char *plain;
    uint32_t n;
    uint32_t *out;
    uint32_t out_words;
    uint32_t lane() const { return 0; }
    uint32_t nlanes() const { return 1; }
    void sync() const {}
    uint32_t uni(uint32_t v) const { return v; }
    uint32_t byte(uint32_t i) const { if (i >= n) abort(); return plain[i]; }
    uint32_t load32(uint32_t i) const {
        if (i > n || n - i < 4u) abort();
        uint32_t v;
        memcpy(&v, plain + i, 4);
        return v;
    }
    void tab_add(uint32_t *at, uint32_t v) const { *at += v; }
    void tab_or(uint32_t *at, uint32_t v) const { *at |= v; }
    uint32_t prefix64(uint32_t *a) const {
        uint32_t sum = 0;
        for (uint32_t k = 0; k < 64; ++k) { const uint32_t v = a[k]; a[k] = sum; sum += v; }
        return sum;
    }
    void out_or(uint32_t w, uint32_t v) { if (w >= out_words) abort(); out[w] |= v; }
    void out_byte(uint32_t i, uint32_t v) {
        if (i >= n + 5u || v > 255u) abort();
        ((unsigned char *)out)[i] = (unsigned char)v;
    }
};

bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char **argv) {
    const bool lengths = argc == 4 && strcmp(argv[1], "--lengths") == 0;
    if (argc != 3 && !lengths) { fprintf(stderr, "usage: deflate_core_host [--lengths] IN RESULTS\n"); return 2; }
    FILE *in = fopen(argv[argc - 2], "rb"), *out = fopen(argv[argc - 1], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    uint32_t count = 0;
    if (!read_exact(in, &count, 4)) return 2;
    static tsdef::Work work;
    for (uint32_t c = 0; c < count; ++c) {
        memset(&work, 0xA5, sizeof work);                           // nothing may depend on the tables of the block before
        if (lengths) {
            uint32_t h[2];
            if (!read_exact(in, h, 8) || h[0] > 288u || h[1] > 15u) { fprintf(stderr, "bad case\n"); return 2; }
            std::vector<uint32_t> freq(h[0]);
            if (!read_exact(in, freq.data(), 4 * (size_t)h[0])) { fprintf(stderr, "short case file\n"); return 2; }
            std::vector<uint8_t> lens(h[0], 0xEE);
            HostPolicy pol{nullptr, 0, nullptr, 0};
            tsdef::build_lengths(pol, &work, freq.data(), h[0], h[1], lens.data());
            fwrite(lens.data(), 1, lens.size(), out);
            continue;
        }
        uint32_t n = 0;
        if (!read_exact(in, &n, 4) || n > (1u << 20)) { fprintf(stderr, "bad block\n"); return 2; }
        unsigned char *plain = (unsigned char *)malloc(n ? n : 1);
        const uint32_t words = (n + 8u) / 4u;
        uint32_t *payload = (uint32_t *)calloc(words, 4);
        if (!plain || !payload || !read_exact(in, plain, n)) { fprintf(stderr, "short block file\n"); return 2; }
        HostPolicy pol{n ? plain : nullptr, n, payload, words};
        const uint32_t m = tsdef::deflate(pol, &work, n);
        if (m == 0 || m > n + 5u) { fprintf(stderr, "block %u: payload of %u bytes for %u\n", c, m, n); return 3; }
        const uint32_t crc = tsdef::crc32(pol, &work, n);
        fwrite(&m, 4, 1, out); fwrite(&crc, 4, 1, out);
        fwrite(payload, 1, m, out);
        free(plain); free(payload);
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
