// text_store_host.cpp — the store plan of the device text formatters (teloscope_amd/csrc/text_store_core.h) on the host, built by
// tests/test_text_store_core_cpu.py with g++ under ASan + UBSan.  The 64 lanes of a wave are played one after the other, doing
// what wave_copy_out (ts_text_emit.h) does with the plan: the staging area and the destination are heap blocks of exactly the
// bytes a wave may touch, so a read or a store outside them is the sanitizer's as well as this program's finding.
//
// For every shift 0..15 (the destination's address modulo 16, on two bases), every n in 0..600 and kStageBytes - 16 .. kStageBytes:
// every byte of [dst, dst + n) is stored exactly once and none outside, every 16-byte store is 16-byte aligned, every staged
// read lies below kStageBytes + 16, head and rest are at most 15 (lanes 0..15 and 16..31 suffice), and the text that arrives
// is the text that was staged.  -DSEED_V0_FAULT: v0 computed as shift / 16 — the build the test expects to fail.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../teloscope_amd/csrc/text_store_core.h"

using tsstore::kStageBytes;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures <= 20) { std::fprintf(stderr, __VA_ARGS__); std::fputc('\n', stderr); } } } while (0)

struct Wave {
    uint64_t dstAddr;                   // the device address the block `dst` stands for
    uint32_t n;
    unsigned char *dst;                 // n bytes
    std::vector<uint32_t> stores;       // per byte of dst
    const unsigned char *lds;           // kStageBytes + 16 bytes
    void store(uint64_t addr, uint32_t ldsAt, uint32_t width) {
        CHECK(width == 1 || addr % 16 == 0, "n %u shift %u: a 16-byte store at an address that is %u mod 16", n, (unsigned)(dstAddr & 15), (unsigned)(addr % 16));
        CHECK(ldsAt + width <= kStageBytes + 16u, "n %u shift %u: a staged read of %u bytes at %u", n, (unsigned)(dstAddr & 15), width, ldsAt);
        CHECK(addr >= dstAddr && addr + width <= dstAddr + n, "n %u shift %u: a store of %u bytes at offset %lld", n, (unsigned)(dstAddr & 15), width,
              (long long)(addr - dstAddr));
        if (addr < dstAddr || addr + width > dstAddr + n || ldsAt + width > kStageBytes + 16u) return;
        std::memcpy(dst + (addr - dstAddr), lds + ldsAt, width);
        for (uint32_t b = 0; b < width; ++b) ++stores[(size_t)(addr - dstAddr) + b];
    }
};

static void copy_out(Wave &w) {
    const uint32_t shift = (uint32_t)(w.dstAddr & 15u);
    tsstore::Plan p = tsstore::plan(shift, w.n);
#ifdef SEED_V0_FAULT
    p.v0 = shift / 16u;
#endif
    CHECK(p.head <= 15u && p.rest <= 15u && p.body % 16u == 0u && p.head + p.body + p.rest == w.n, "n %u shift %u: head %u body %u rest %u", w.n, shift,
          p.head, p.body, p.rest);
    for (uint32_t lane = 0; lane < 64u; ++lane) {
        if (lane < p.head) w.store(w.dstAddr + lane, shift + lane, 1);
        if (lane >= 16u && lane - 16u < p.rest) w.store(w.dstAddr + p.head + p.body + lane - 16u, shift + p.head + p.body + lane - 16u, 1);
        for (uint32_t v = lane; v < p.body / 16u; v += 64u) w.store(w.dstAddr + p.head + 16u * v, 16u * (p.v0 + v), 16);
    }
}

int main() {
    CHECK(tsstore::staged(0, kStageBytes) && tsstore::staged(kStageBytes, kStageBytes) && !tsstore::staged(kStageBytes + 1, kStageBytes) &&
          !tsstore::staged(0xFFFFFFFFu, kStageBytes), "staged(): n <= capacity");
    std::vector<uint32_t> sizes;
    for (uint32_t n = 0; n <= 600u; ++n) sizes.push_back(n);
    for (uint32_t n = kStageBytes - 16u; n <= kStageBytes; ++n) sizes.push_back(n);
    unsigned long cases = 0;
    for (uint64_t base : {0x7f3a00000000ull, 0xfffffff0ull})           // (the second: a destination across 4 GiB)
        for (uint32_t shift = 0; shift < 16u; ++shift)
            for (uint32_t n : sizes) {
                unsigned char *lds = (unsigned char *)std::malloc(kStageBytes + 16u);
                unsigned char *dst = (unsigned char *)std::malloc(n ? n : 1);
                std::memset(lds, 0xEE, kStageBytes + 16u);
                std::memset(dst, 0xDD, n ? n : 1);
                for (uint32_t i = 0; i < n; ++i) lds[shift + i] = (unsigned char)(1u + (i * 131u + n + shift) % 199u);      // the staged text
                Wave w{base + shift, n, dst, std::vector<uint32_t>(n, 0u), lds};
                copy_out(w);
                for (uint32_t i = 0; i < n; ++i) {
                    CHECK(w.stores[i] == 1u, "n %u shift %u: byte %u stored %u times", n, shift, i, w.stores[i]);
                    CHECK(dst[i] == lds[shift + i], "n %u shift %u: byte %u arrived as %u, staged %u", n, shift, i, dst[i], lds[shift + i]);
                }
                std::free(dst);
                std::free(lds);
                ++cases;
            }
    if (failures) { std::fprintf(stderr, "%d checks failed\n", failures); return 1; }
    std::printf("ok %lu cases\n", cases);
    return 0;
}
