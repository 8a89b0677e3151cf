// track_format_host.cpp — teloscope_amd/csrc/track_format_core.h on the host: the functions the gfx950 kernels of tracks.hip
// compile, built by g++ under ASan + UBSan and checked against printf (tests/test_track_format_core_cpu.py).
//
//   track_format_host                 formats every value of the lists below through the core and through snprintf("%.6g") /
//                                     snprintf("%llu"); every text must be equal, every byte of a text written exactly once and
//                                     none outside it.  Prints "ok <floats> floats <integers> integers <rejected> rejected".
//   track_format_host tracks FILE     FILE: u32 w, step, flags (1 -r, 2 -g, 4 -e), n_segs; u64 n, names_len; n records of eight
//                                     u32; n_segs segments {u64 first_window, n_windows, abs_pos, len, name_off; u32 name_len, 0};
//                                     the names.  Prints, per track in track order, "#track <t> <bytes>\n" and the track's text
//                                     (a disabled track: "#track <t> -\n").
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../teloscope_amd/csrc/track_format_core.h"

namespace {

struct CheckedSink {                       // a text of `len` bytes: every put inside it, every byte once
    char text[64];
    unsigned char hits[64];
    uint32_t len;
    bool bad = false;
    explicit CheckedSink(uint32_t n) : len(n) { std::memset(text, 0, sizeof text); std::memset(hits, 0, sizeof hits); }
    void put(uint32_t at, uint32_t byte) {
        if (at >= len || at >= sizeof text || hits[at]) { bad = true; return; }
        hits[at] = 1;
        text[at] = (char)byte;
    }
    bool complete() const {
        for (uint32_t i = 0; i < len; ++i) if (!hits[i]) return false;
        return !bad;
    }
};

struct StringSink {
    std::string &s;
    size_t base;
    void put(uint32_t at, uint32_t byte) { s.at(base + at) = (char)byte; }
};
struct NameBytes {
    const std::vector<char> &names;
    uint32_t byte(uint64_t i) const { return (unsigned char)names.at(i); }
};

uint64_t n_floats = 0, n_ints = 0, n_rejected = 0;

void fail(const char *what, const char *got, const char *want) {
    std::fprintf(stderr, "%s: core \"%s\" printf \"%s\"\n", what, got, want);
    std::exit(1);
}

void check_float(float v) {
    char want[64], what[96];
    std::snprintf(want, sizeof want, "%.6g", (double)v);
    const tstrack::FloatDec d = tstrack::float_dec(tstrack::float_bits(v));
    std::snprintf(what, sizeof what, "float %.9g (bits %08x)", (double)v, tstrack::float_bits(v));
    if (d.kind == tstrack::F_BAD) fail(what, "<rejected>", want);
    CheckedSink s(tstrack::float_len(d));
    tstrack::put_float(s, 0u, d);
    if (!s.complete() || s.len != std::strlen(want) || std::memcmp(s.text, want, s.len) != 0) fail(what, s.text, want);
    ++n_floats;
}

void check_rejected(float v) {
    const tstrack::FloatDec d = tstrack::float_dec(tstrack::float_bits(v));
    if (d.kind != tstrack::F_BAD || tstrack::float_len(d) != 0u) {
        std::fprintf(stderr, "float %.9g is outside the domain and was not rejected\n", (double)v);
        std::exit(1);
    }
    ++n_rejected;
}

void check_int(uint64_t v) {
    char want[64], what[64];
    std::snprintf(want, sizeof want, "%" PRIu64, v);
    std::snprintf(what, sizeof what, "integer %" PRIu64, v);
    CheckedSink s(tstrack::u64_digits(v));
    tstrack::put_u64(s, s.len, v);
    if (!s.complete() || s.len != std::strlen(want) || std::memcmp(s.text, want, s.len) != 0) fail(what, s.text, want);
    ++n_ints;
}

float bits_float(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }

int self_check() {
    using tstrack::Record;
    // every ratio n / d, 0 <= n <= d <= 2048, by the division the ratio and density columns use
    for (uint32_t d = 1; d <= 2048; ++d)
        for (uint32_t n = 0; n <= d; ++n) check_float((float)n / d);
    const uint32_t big[4] = {4096u, 65536u, 1u << 22, 0xFFFFFFFFu};
    for (uint32_t d : big)
        for (uint32_t n : {1u, 2u, 3u, d / 3u, d - 1u}) check_float((float)n / d);
    // every GC value of windows of up to 2048 bases, through the column's own expression
    for (uint32_t size = 1; size <= 2048; ++size)
        for (uint32_t gc = 0; gc <= size; ++gc) {
            const Record r = {0u, gc / 2u, gc - gc / 2u, 0u, 0u, 0u, 0u, 0u};
            check_float(bits_float(tstrack::track_value(tstrack::GC, r, size, 0u)));
            if (bits_float(tstrack::track_value(tstrack::GC, r, size, 0u)) != (float)((float)gc / size * 100.0)) fail("gc value", "", "");
        }
    for (uint32_t k = 0; k <= 2000; ++k) check_float((float)k / 1000.0f);
    check_float(-1.0f);
    check_float(128.0f);
    check_float(bits_float((127u - 32u) << 23));                      // 2^-32
    check_float(1.0f / 1024.0f);                                     // ties: 0.000976562
    check_float(3.0f / 4096.0f);
    check_float(1.0f / 4194304.0f);                                  // 2.38419e-07
    check_float(0.0001f);
    check_float(0.000099999994f);
    check_float(0.99999994f);
    check_float(99999.95f / 1000.0f);
    std::mt19937_64 rng(20261018u);
    for (uint32_t i = 0; i < (1u << 20); ++i) {
        const uint64_t x = rng();
        const uint32_t E = 95u + (uint32_t)((x >> 32) % 39u);        // 2^-32 <= value < 128
        check_float(bits_float((E << 23) | ((uint32_t)x & 0x7FFFFFu)));
    }
    for (float v : {129.0f, 128.00002f, 1e9f, bits_float((127u - 33u) << 23), bits_float(0x2F7FFFFFu), -0.5f, -2.0f, bits_float(0x80000000u),
                    bits_float(1u), bits_float(0x7F800000u), bits_float(0x7FC00000u), bits_float(0xFF800000u)})
        check_rejected(v);

    check_int(0); check_int(9); check_int(10);
    uint64_t p = 1;
    for (int k = 1; k <= 19; ++k) { p *= 10u; check_int(p - 1u); check_int(p); check_int(p + 1u); }
    check_int((1ull << 32) - 1u); check_int(1ull << 32); check_int((1ull << 32) + 1u);
    check_int(~0ull);

    // the column values against the host writer's expressions, and the rounding of the entropy
    for (uint32_t w : {7u, 1000u, 1024u}) {
        std::vector<float> term(w + 1u, 0.0f);
        for (uint32_t c = 1; c <= w; ++c) { const float q = (float)c / w; term[c] = q * std::log2(q); }
        for (uint32_t i = 0; i < 20000u; ++i) {
            uint32_t left = w, c[4];
            for (uint32_t &x : c) { x = (uint32_t)(rng() % (left + 1u)); left -= x; }
            const Record r = {c[0], c[1], c[2], c[3], 0u, 0u, 0u, 0u};
            bool bad = false;
            const float got = tstrack::entropy_from_terms(r, term.data(), w, &bad);
            float e = 0.0f;
            for (uint32_t x : c) if (x) e -= term[x];
            const float want = std::round(e * 1000.0f) / 1000.0f;
            if (bad || tstrack::float_bits(got) != tstrack::float_bits(want)) fail("entropy value", "", "");
            check_float(got);
        }
    }
    std::printf("ok %" PRIu64 " floats %" PRIu64 " integers %" PRIu64 " rejected\n", n_floats, n_ints, n_rejected);
    return 0;
}

// getShannonEntropy (the library's ts::shannon_entropy): float32 throughout, rounded to three decimals
float shannon_entropy(const uint32_t c[4], uint32_t size) {
    float e = 0.0f;
    for (int i = 0; i < 4; ++i)
        if (c[i] > 0) { const float q = (float)c[i] / size; e -= q * std::log2(q); }
    return std::round(e * 1000.0f) / 1000.0f;
}

int tracks(const char *path) {
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::perror(path); return 2; }
    uint32_t head[4];
    uint64_t n = 0, names_len = 0;
    bool ok = std::fread(head, 4, 4, f) == 4 && std::fread(&n, 8, 1, f) == 1 && std::fread(&names_len, 8, 1, f) == 1;
    const uint32_t w = head[0], step = head[1], flags = head[2], n_segs = head[3];
    std::vector<uint32_t> rec(n * 8u);
    std::vector<tstrack::Segment> all(n_segs), seg;
    std::vector<char> names(names_len);
    ok = ok && (n == 0 || std::fread(rec.data(), 32, n, f) == n) && (n_segs == 0 || std::fread(all.data(), sizeof(tstrack::Segment), n_segs, f) == n_segs) &&
         (names_len == 0 || std::fread(names.data(), 1, names_len, f) == names_len);
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "%s: short file\n", path); return 2; }
    for (const tstrack::Segment &s : all) if (s.n_windows) seg.push_back(s);
    std::vector<float> term;
    if ((flags & 4u) && w <= (1u << 22)) {
        term.assign((size_t)w + 1u, 0.0f);
        for (uint32_t c = 1; c <= w; ++c) { const float q = (float)c / w; term[c] = q * std::log2(q); }
    }
    const bool on[tstrack::kTracks] = {(flags & 1u) != 0, (flags & 1u) != 0, (flags & 1u) != 0, (flags & 2u) != 0, (flags & 4u) != 0};
    std::string out[tstrack::kTracks];
    const NameBytes nb{names};
    for (uint64_t i = 0; i < n; ++i) {
        const tstrack::Segment &sg = seg.at(tstrack::find_segment(seg.data(), (uint32_t)seg.size(), i));
        const uint64_t k = i - sg.first_window;
        const uint64_t start = tstrack::window_start(sg, k, step);
        const uint32_t size = tstrack::window_size(sg, k, w, step);
        const uint64_t end = start + size;
        const uint32_t *q = &rec[i * 8u];
        const tstrack::Record r = {q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]};
        uint32_t ebits = 0;
        if (on[tstrack::ENTROPY]) {
            bool bad = size != w || term.empty();
            float e = 0.0f;
            if (!bad) e = tstrack::entropy_from_terms(r, term.data(), w, &bad);
            if (bad) e = shannon_entropy(q, size);
            ebits = tstrack::float_bits(e);
        }
        const uint32_t pl = tstrack::prefix_len(sg.name_len, start, end);
        for (uint32_t t = 0; t < tstrack::kTracks; ++t) {
            if (!on[t]) continue;
            const tstrack::FloatDec d = tstrack::float_dec(tstrack::track_value(t, r, size, ebits));
            if (d.kind == tstrack::F_BAD) { std::fprintf(stderr, "window %" PRIu64 ": track %u value outside the formatter's domain\n", i, t); return 3; }
            const uint32_t vl = tstrack::float_len(d);
            StringSink s{out[t], out[t].size()};
            out[t].resize(out[t].size() + pl + vl + 1u);
            tstrack::put_prefix(s, 0u, nb, sg.name_off, sg.name_len, start, end);
            tstrack::put_float(s, pl, d);
            s.put(pl + vl, '\n');
        }
    }
    for (uint32_t t = 0; t < tstrack::kTracks; ++t) {
        if (!on[t]) { std::printf("#track %u -\n", t); continue; }
        std::printf("#track %u %zu\n", t, out[t].size());
        std::fwrite(out[t].data(), 1, out[t].size(), stdout);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 1) return self_check();
    if (argc == 3 && std::strcmp(argv[1], "tracks") == 0) return tracks(argv[2]);
    std::fprintf(stderr, "usage: track_format_host [tracks FILE]\n");
    return 2;
}
