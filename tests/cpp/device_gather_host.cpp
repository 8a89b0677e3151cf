// device_gather_host.cpp — teloscope_amd/csrc/gather_core.h on the host: the per-lane copy of ts_gather_pieces_kernel driven
// lane by lane through an accessor that checks every load and store, and the splitter that cuts pieces into the kernel's jobs.
// Built by g++ under ASan + UBSan (tests/test_device_gather_core_cpu.py).  The source lives in an allocation of exactly n
// bytes; the accessor never dereferences outside it — it refuses a word that holds no byte of the piece, and fills the bytes
// of an accepted word that lie outside the piece with a pattern that may not reach the destination.  Exit status 0 and
// "ok ..." on stdout, else the first failure on stderr and status 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../teloscope_amd/csrc/gather_core.h"

namespace {

constexpr uint32_t kGuard = 32;
constexpr uint32_t kSlice = tsgather::kSliceBytes;

[[noreturn]] void fail(const char *what, uint64_t a, uint64_t b, uint64_t c) {
    std::fprintf(stderr, "FAIL: %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c);
    std::exit(1);
}

// The piece [src, src + n) and its place [dst, dst + n) at made-up addresses with the wanted misalignments; the destination has
// kGuard bytes either side.
struct Checked {
    uint64_t src, dst, n;
    const unsigned char *from;                  // exactly n bytes
    std::vector<unsigned char> to;              // kGuard + n + kGuard
    std::vector<unsigned char> stored;          // per destination byte: times stored
    Checked(uint64_t src_, uint64_t dst_, uint64_t n_, const unsigned char *from_)
        : src(src_), dst(dst_), n(n_), from(from_), to(n_ + 2 * kGuard), stored(n_, 0) {
        for (size_t i = 0; i < to.size(); ++i) to[i] = (unsigned char)(0xA0u + i % 7u);
    }
    unsigned char guard_value(size_t i) const { return (unsigned char)(0xA0u + i % 7u); }

    uint32_t word(uint64_t a) {
        if (a & 3u) fail("unaligned word load", a, src, n);
        if (a + 4 <= src || a >= src + n) fail("loaded a word that holds no byte of the piece", a, src, n);
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4; ++k) {
            const uint64_t at = a + k;
            const uint32_t byte = (at >= src && at < src + n) ? from[at - src] : 0xEEu;
            w |= byte << (8u * k);
        }
        return w;
    }
    void words4(uint64_t a, uint32_t w[4]) { for (uint32_t k = 0; k < 4; ++k) w[k] = word(a + 4 * k); }
    void store_byte(uint64_t a, uint32_t v) {
        if (a < dst || a >= dst + n) fail("stored a byte outside the piece's place", a, dst, n);
        if (stored[a - dst]++) fail("stored a byte twice", a, dst, n);
        to[kGuard + (a - dst)] = (unsigned char)v;
    }
    void store16(uint64_t a, const uint32_t v[4]) {
        if (a & 15u) fail("unaligned 16-byte store", a, dst, n);
        for (uint32_t k = 0; k < 16; ++k) store_byte(a + k, (v[k / 4] >> (8u * (k % 4))) & 0xffu);
    }
    void verify(const char *what) const {
        for (uint64_t i = 0; i < n; ++i) {
            if (stored[i] != 1) fail("a byte of the piece was not stored", i, dst, n);
            if (to[kGuard + i] != from[i]) fail(what, i, src, dst);
        }
        for (size_t i = 0; i < kGuard; ++i)
            if (to[i] != guard_value(i) || to[kGuard + n + i] != guard_value(kGuard + n + i)) fail("a guard byte changed", i, dst, n);
    }
};

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
};

// one piece as the library treats it: split into jobs, every job copied by its 64 lanes; -> jobs
uint64_t run_piece(uint64_t sm, uint64_t dm, uint64_t n, Rng &rng, bool split) {
    std::unique_ptr<unsigned char[]> from(new unsigned char[n ? n : 1]);      // (n == 0: never read)
    for (uint64_t i = 0; i < n; ++i) from[i] = (unsigned char)(1u + rng.next() % 200u);
    const uint64_t src = 0x7000100000ull + sm, dst = 0x7100200000ull + dm;
    Checked m(src, dst, n, from.get());
    uint64_t jobs = 0, covered = 0;
    auto one_job = [&](uint64_t s, uint64_t d, uint32_t len) {
        if (s - src != covered || d - dst != covered) fail("jobs do not follow each other", s - src, d - dst, covered);
        if (len == 0 || len > kSlice) fail("a job of no bytes or of more than a slice", len, n, 0);
        if (jobs && (d & 15u)) fail("a cut off a 16-byte boundary of the destination", d, dst, n);
        for (uint32_t lane = 0; lane < tsgather::kLanes; ++lane) tsgather::copy_lane(m, s, d, len, lane);
        covered += len;
        ++jobs;
    };
    if (split) {
        tsgather::split_piece(src, dst, n, kSlice, one_job);
        if (covered != n) fail("the jobs do not cover the piece", covered, n, 0);
        if (jobs != tsgather::split_count(dst, n, kSlice)) fail("split_count disagrees with split_piece", jobs, tsgather::split_count(dst, n, kSlice), n);
    } else {
        for (uint32_t lane = 0; lane < tsgather::kLanes; ++lane) tsgather::copy_lane(m, src, dst, (uint32_t)n, lane);
        jobs = 1;
    }
    m.verify("a destination byte differs from the source's");
    return jobs;
}

}  // namespace

int main() {
    Rng rng{20261018};
    uint64_t pieces = 0, jobs = 0;
    // align_bytes, the host twin of __builtin_amdgcn_alignbyte
    for (uint32_t sh = 0; sh < 4; ++sh) {
        const uint32_t lo = 0x03020100u, hi = 0x07060504u;
        uint32_t want = 0;
        for (uint32_t k = 0; k < 4; ++k) want |= (sh + k) << (8u * k);
        if (tsgather::align_bytes(hi, lo, sh) != want) fail("align_bytes", sh, tsgather::align_bytes(hi, lo, sh), want);
    }
    // every source misalignment x every destination misalignment x n in 0..80, as one job each
    for (uint64_t sm = 0; sm < 16; ++sm)
        for (uint64_t dm = 0; dm < 16; ++dm)
            for (uint64_t n = 0; n <= 80; ++n) { jobs += run_piece(sm, dm, n, rng, false); ++pieces; }
    // the long ones at four misalignment pairs each (source on and off a word boundary behind the head, destination on and off
    // a 16-byte boundary), through the splitter; a job of a whole slice also directly
    const uint64_t pairs[4][2] = {{0, 0}, {5, 0}, {4, 12}, {15, 1}};
    const uint64_t sizes[7] = {1023, 1024, 1025, kSlice - 1, kSlice, kSlice + 1, 3ull * kSlice + 7};
    for (const auto &p : pairs)
        for (uint64_t n : sizes) {
            jobs += run_piece(p[0], p[1], n, rng, true);
            ++pieces;
            if (n <= kSlice) { jobs += run_piece(p[0], p[1], n, rng, false); ++pieces; }
        }
    // the splitter: pieces of 0, 1, slice +- 1 and 5 slices + 3 bytes at odd destination offsets (run_piece checks that the jobs
    // tile the piece in order, none longer than a slice, every cut but the first on a 16-byte boundary of the destination)
    const uint64_t lens[6] = {0, 1, kSlice - 1, kSlice, kSlice + 1, 5ull * kSlice + 3};
    const uint64_t offs[6] = {0, 1, 5, 9, 15, 7};
    for (uint64_t len : lens)
        for (uint64_t dm : offs) {
            const uint64_t got = run_piece(3, dm, len, rng, true);
            // the first job ends on the boundary `slice - dm` bytes on; whole slices follow
            const uint64_t first = kSlice - dm;
            const uint64_t want = len == 0 ? 0 : len <= first ? 1 : 1 + (len - first + kSlice - 1) / kSlice;
            if (got != want) fail("the number of jobs", got, want, len);
            jobs += got;
            ++pieces;
        }
    std::printf("ok %llu pieces %llu jobs\n", (unsigned long long)pieces, (unsigned long long)jobs);
    return 0;
}
