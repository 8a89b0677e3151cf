// track_format_core.h — the text of the five window tracks (_window_repeat_density, _window_canonical_ratio, _window_strand_ratio,
// _window_gc, _window_entropy .bedgraph), one source for the gfx950 kernels (tracks.hip) and for a host test program
// (tests/cpp/track_format_host.cpp, built by g++ under ASan + UBSan).  No allocation, no library calls, no local arrays (a digit
// buffer indexed at run time would be scratch memory on the device): every length is computed first, and digits are written from
// the last one backwards.
//
// A line is  name \t start \t end \t value \n  — what BedWriter::format (include/teloscope_mi355x_io.hpp) writes per window:
//   start, end   operator<<(uint64_t): decimal digits;
//   value        operator<<(float): printf's %g with precision 6 — up to six significant digits, rounded from the EXACT binary value
//                with ties to even (1/1024 = 0.0009765625 -> 0.000976562), trailing zeros and a bare point removed, the form
//                d.ddddde-XX when the decimal exponent is below -4.
// The float formatter covers the values the five columns can take and says so when it is handed anything else (kind F_BAD, length
// 0): 0, -1, and every positive float in [2^-32, 128] — ratios a / b with b < 2^32, entropy k / 1000 <= 2, GC <= 100.  Such a
// value is m * 2^-s with m < 2^24 and 16 <= s <= 55; its first six digits are floor(m * 5^p / 2^(s - p)) for the p in 3..15 that
// makes them six, and m * 5^15 < 2^59: 64-bit integers hold every intermediate exactly.  No double arithmetic, nothing rounds twice.
//
// Text goes out through a sink S, which is what differs between the builds:   void put(uint32_t at, uint32_t byte)
#ifndef TS_TRACK_FORMAT_CORE_H
#define TS_TRACK_FORMAT_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define TS_THD __host__ __device__ __forceinline__
#else
#define TS_THD inline
#endif

namespace tstrack {

// track order everywhere: detail::File's (include/teloscope_mi355x_io.hpp)
enum Track { DENSITY = 0, CANON_RATIO = 1, STRAND_RATIO = 2, GC = 3, ENTROPY = 4, kTracks = 5 };

// A segment of the table the formatter reads: its windows are [first_window, first_window + n_windows) of the record array,
// window k covers [abs_pos + k * step, abs_pos + k * step + min(w, len - k * step)).  Segments without windows are left out of
// the table, so first_window is strictly ascending and a window finds its segment by a lower bound in that column.
struct Segment {                                    // 48 bytes
    unsigned long long first_window, n_windows, abs_pos, len, name_off;
    uint32_t name_len, reserved;
};

// The entropy of a window that does not take it from the term table: {window index, float bits}, sorted by index.
struct Patch {                                      // 16 bytes
    unsigned long long window;
    uint32_t bits, reserved;
};

// A window record as the scan leaves it: covered bases per nucleotide and per match class.
struct Record { uint32_t a, c, g, t, canonical, non_canonical, fwd, rev; };

// ------------------------------------------------------------------------------------------------ integers
TS_THD uint32_t u32_digits(uint32_t v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
           (v >= 100000000u) + (v >= 1000000000u);
}
TS_THD uint32_t u64_digits(uint64_t v) {
    if (v <= 0xFFFFFFFFull) return u32_digits((uint32_t)v);
    uint32_t n = 10;                                // (2^32 has ten digits)
    uint64_t p = 10000000000ull;
    while (n < 20u && v >= p) { ++n; p *= 10u; }    // (p wraps only when n reaches 20, and is not read then)
    return n;
}
// the digits of v, the last one at end - 1
template <class S>
TS_THD void put_u64(S &s, uint32_t end, uint64_t v) {
    while (v > 0xFFFFFFFFull) {
        const uint64_t q = v / 10u;
        s.put(--end, '0' + (uint32_t)(v - q * 10u));
        v = q;
    }
    uint32_t x = (uint32_t)v;
    do {
        const uint32_t q = x / 10u;
        s.put(--end, '0' + (x - q * 10u));
        x = q;
    } while (x);
}

// ------------------------------------------------------------------------------------------------ floats
enum FloatKind { F_ZERO = 0, F_MINUS_ONE = 1, F_NUMBER = 2, F_BAD = 3 };
// A float as %g sees it: its significant digits without trailing zeros (`digits`, `nd` of them, 1..6) and the decimal exponent
// of the first one.
struct FloatDec { uint32_t digits, nd; int32_t x; uint32_t kind; };

TS_THD uint64_t pow5(uint32_t p) {                  // p <= 15
    return (uint64_t)((p & 1u ? 5u : 1u) * (p & 2u ? 25u : 1u) * (p & 4u ? 625u : 1u)) * (p & 8u ? 390625u : 1u);
}

TS_THD FloatDec float_dec(uint32_t bits) {
    FloatDec d = {0u, 1u, 0, F_BAD};
    if (bits == 0u) { d.kind = F_ZERO; return d; }
    if (bits == 0xBF800000u) { d.kind = F_MINUS_ONE; return d; }
    const uint32_t E = bits >> 23;                  // (with the sign bit: a negative number is out of range here)
    const uint32_t frac = bits & 0x7FFFFFu;
    if (E < 127u - 32u || E > 127u + 7u || (E == 127u + 7u && frac != 0u)) return d;
    const int32_t e2 = (int32_t)E - 127;            // -32 .. 7: the value lies in [2^e2, 2^(e2 + 1))
    const uint32_t m = frac | 0x800000u;
    const int32_t s = 23 - e2;                      // value = m * 2^-s, s in 16 .. 55
    int32_t x = (e2 * 1233) / 4096;                 // floor(e2 * log10(2)): the decimal exponent, or one below it
    if (e2 < 0 && x * 4096 != e2 * 1233) --x;
    uint32_t p = (uint32_t)(5 - x);                 // 3 .. 15
    uint64_t n = (uint64_t)m * pow5(p);
    uint32_t sh = (uint32_t)s - p;                  // 1 .. 52
    if ((n >> sh) >= 1000000u) { --p; ++x; ++sh; n = (uint64_t)m * pow5(p); }
    uint32_t digits = (uint32_t)(n >> sh);          // 100000 .. 999999
    const uint64_t rem = n & ((1ull << sh) - 1ull), half = 1ull << (sh - 1u);
    if (rem > half || (rem == half && (digits & 1u))) ++digits;
    if (digits == 1000000u) { digits = 100000u; ++x; }
    uint32_t nd = 6;
    while (digits % 10u == 0u) { digits /= 10u; --nd; }
    d.digits = digits; d.nd = nd; d.x = x; d.kind = F_NUMBER;
    return d;
}

TS_THD uint32_t float_len(const FloatDec &d) {
    if (d.kind == F_ZERO) return 1u;
    if (d.kind == F_MINUS_ONE) return 2u;
    if (d.kind != F_NUMBER) return 0u;
    if (d.x < -4) return (d.nd > 1u ? d.nd + 1u : 1u) + 4u;             // d[.ddddd]e-XX
    if (d.x >= 0) return d.nd > (uint32_t)d.x + 1u ? d.nd + 1u : (uint32_t)d.x + 1u;
    return (uint32_t)(1 - d.x) + d.nd;                                   // 0. (-x - 1 zeros) digits
}

// the text of d, float_len(d) bytes from `at`
template <class S>
TS_THD void put_float(S &s, uint32_t at, const FloatDec &d) {
    if (d.kind == F_ZERO) { s.put(at, '0'); return; }
    if (d.kind == F_MINUS_ONE) { s.put(at, '-'); s.put(at + 1u, '1'); return; }
    if (d.kind != F_NUMBER) return;
    uint32_t end = at + float_len(d), v = d.digits;
    if (d.x < -4) {
        const uint32_t ax = (uint32_t)(-d.x);                            // 5 .. 10
        s.put(end - 1u, '0' + ax % 10u);
        s.put(end - 2u, '0' + ax / 10u);
        s.put(end - 3u, '-');
        s.put(end - 4u, 'e');
        end -= 4u;
        for (uint32_t i = d.nd; i > 1u; --i) { s.put(--end, '0' + v % 10u); v /= 10u; }
        if (d.nd > 1u) s.put(--end, '.');
        s.put(--end, '0' + v);
        return;
    }
    if (d.x >= 0) {
        const uint32_t whole = (uint32_t)d.x + 1u;                       // digits in front of the point
        if (d.nd <= whole) {
            for (uint32_t i = d.nd; i < whole; ++i) s.put(--end, '0');
        } else {
            for (uint32_t i = whole; i < d.nd; ++i) { s.put(--end, '0' + v % 10u); v /= 10u; }
            s.put(--end, '.');
        }
        do { s.put(--end, '0' + v % 10u); v /= 10u; } while (v);
        return;
    }
    for (uint32_t i = 0; i < d.nd; ++i) { s.put(--end, '0' + v % 10u); v /= 10u; }
    while (end > at + 2u) s.put(--end, '0');
    s.put(at + 1u, '.');
    s.put(at, '0');
}

TS_THD uint32_t float_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    union { float f; uint32_t u; } c;
    c.f = f;
    return c.u;
#endif
}

// ------------------------------------------------------------------------------------------------ column values
// The operations of BedWriter::format and ts::gc_content / ts::shannon_entropy_memo, in their order and precision (the build
// keeps fp32 division IEEE-rounded and contracts nothing).

// std::round of a non-negative float below 2^23: half away from zero
TS_THD float round_nonneg(float x) {
    float t = (float)(uint32_t)x;
    if (x - t >= 0.5f) t += 1.0f;
    return t;
}

// Entropy of a window of the full size from the term table (term[c] = (c / w) log2 (c / w), ts::entropy_terms): the terms are
// subtracted in A, C, G, T order, zero counts skipped.  *bad when a count exceeds the table.
TS_THD float entropy_from_terms(const Record &r, const float *term, uint32_t w, bool *bad) {
    if (r.a > w || r.c > w || r.g > w || r.t > w) { *bad = true; return 0.0f; }
    float e = 0.0f;
    if (r.a) e -= term[r.a];
    if (r.c) e -= term[r.c];
    if (r.g) e -= term[r.g];
    if (r.t) e -= term[r.t];
    return round_nonneg(e * 1000.0f) / 1000.0f;
}

// The bits of track t's value for a window of `size` bases.  entropy_bits: what ENTROPY returns (the caller has it from the term
// table or from the patch list).
TS_THD uint32_t track_value(uint32_t t, const Record &r, uint32_t size, uint32_t entropy_bits) {
    const uint32_t covered = r.fwd + r.rev;
    float v;
    switch (t) {
    case DENSITY: v = (float)covered / size; break;
    case CANON_RATIO: v = covered > 0u ? (float)r.canonical / (r.canonical + r.non_canonical) : -1.0f; break;
    case STRAND_RATIO: v = covered > 0u ? (float)r.fwd / (r.fwd + r.rev) : -1.0f; break;
    case GC: v = (float)((double)((float)(r.c + r.g) / size) * 100.0); break;
    default: return entropy_bits;
    }
    return float_bits(v);
}

// ------------------------------------------------------------------------------------------------ lines
// the window's place: k-th of its segment
TS_THD uint64_t window_start(const Segment &sg, uint64_t k, uint32_t step) { return sg.abs_pos + k * step; }
TS_THD uint32_t window_size(const Segment &sg, uint64_t k, uint32_t w, uint32_t step) {
    const uint64_t left = sg.len - k * step;
    return left < w ? (uint32_t)left : w;
}

// length of  name \t start \t end \t
TS_THD uint32_t prefix_len(uint32_t name_len, uint64_t start, uint64_t end) { return name_len + 3u + u64_digits(start) + u64_digits(end); }

// ... and its bytes from `at`; N: uint32_t byte(uint64_t i) reads the names
template <class S, class N>
TS_THD void put_prefix(S &s, uint32_t at, const N &names, uint64_t name_off, uint32_t name_len, uint64_t start, uint64_t end) {
    for (uint32_t i = 0; i < name_len; ++i) s.put(at + i, names.byte(name_off + i));
    at += name_len;
    s.put(at, '\t');
    at += 1u + u64_digits(start);
    put_u64(s, at, start);
    s.put(at, '\t');
    at += 1u + u64_digits(end);
    put_u64(s, at, end);
    s.put(at, '\t');
}

// the segment that holds window `i`: the last one whose first_window is <= i (n >= 1, seg[0].first_window <= i)
TS_THD uint32_t find_segment(const Segment *seg, uint32_t n, uint64_t i) {
    uint32_t lo = 0, hi = n;                        // seg[lo].first_window <= i < seg[hi].first_window
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (seg[mid].first_window <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// the patch of window `i` (the list holds one for every window that needs one; *found says whether it did)
TS_THD uint32_t find_patch(const Patch *patch, uint64_t n, uint64_t i, bool *found) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (patch[mid].window < i) lo = mid + 1u; else hi = mid;
    }
    *found = lo < n && patch[lo].window == i;
    return *found ? patch[lo].bits : 0u;
}

}  // namespace tstrack

#endif
