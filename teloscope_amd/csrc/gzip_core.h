// gzip_core.h — what turns one serial deflate stream into parallel work (the two-pass scheme of pugz and rapidgzip), one source
// for the gfx950 kernels (gzip.hip) and for a host test program (tests/cpp/gzip_core_host.cpp, g++ under ASan + UBSan):
//   probe         is this bit offset the start of a non-final dynamic block?  (a search for places to start decoding)
//   inflate_span  decodes from a bit offset without knowing the 32 KiB in front of it: 16-bit symbols, a byte or a marker
//                 "byte i of the 32 KiB before this span"
//   resolve       symbol -> byte once those 32 KiB are known
// The tables, the bit reader and the code builder are inflate_core.h's.  No allocation, no recursion, no library calls; every
// read is bounded by the window's bytes, every write by the span's capacity, every loop by consumed bits.
//
// The policy object P (see inflate_core.h) here means:
//   uint32_t word(uint32_t i)       the i-th little-endian dword of the window, zero beyond its last byte
//   lane(), nlanes(), sync(), uni() as in inflate_core.h
//   void put(uint32_t k, uint32_t e)                  queue entry k of the batch (k < 64): kLiteral | byte, or length | distance << 9
//   void flush(uint32_t n, uint32_t pos)              writes the n queued symbols at out[pos ...] (16-bit each); a match whose
//                                                     source lies at q < 0 writes the marker kMarker | (32768 + q), else copies
//                                                     the symbol at q (which may be a marker, and may be of the same batch)
//   void copy_stored(uint32_t from, uint32_t n, uint32_t pos)   out[pos .. pos + n) = window bytes [from, from + n)
// The core asks put / flush / copy_stored only for symbols below the capacity it was given and for match sources at or above
// -hist_len (hist_len <= 32768).
#ifndef TS_GZIP_CORE_H
#define TS_GZIP_CORE_H

#include "inflate_core.h"

namespace tsgz {

constexpr uint32_t kMarker = 0x8000u;
constexpr uint32_t kHistory = 32768u;
constexpr uint32_t kNoCandidate = 0xffffffffu;

// why a span's decode ended
enum {
    kSpanStop = 0,      // at the first block boundary at or after the stop bit
    kSpanFinal = 1,     // at the end of a final block
    kSpanFull = 2,      // the next symbol does not fit the capacity
    kSpanBad = 3,       // not deflate (or a distance beyond the history the caller vouches for)
    kSpanEdge = 4       // the window's bytes ended inside a block
};

// end_bit / n_out describe the last block boundary reached (for kSpanStop and kSpanFinal: where the decode ended); what a span
// wrote behind n_out belongs to a block it did not finish and is nobody's output.
struct SpanResult { uint32_t end_bit, n_out, final_seen, status; };

TS_HD uint32_t resolve(uint32_t sym, const unsigned char *history) { return (sym & kMarker) ? history[sym & 0x7fffu] : (sym & 255u); }

// ---- the candidate test, cheap part: `lo` holds the 64 bits from the offset on, `hi` the 32 behind them.  BFINAL = 0,
// BTYPE = 2, HLIT <= 286, HDIST <= 30, and a code-length code whose Kraft sum is exactly 1 (74 bits at most).  A lane per offset.
TS_HD bool probe_cheap(uint64_t lo, uint32_t hi) {
    const uint32_t h = (uint32_t)lo;
    if ((h & 7u) != 4u) return false;                           // BFINAL 0, BTYPE 10b (sent low bit first)
    if (((h >> 3) & 31u) > 29u || ((h >> 8) & 31u) > 29u) return false;
    const uint32_t nc = ((h >> 13) & 15u) + 4u;
    uint32_t sum = 0;                                           // in units of 2^-7
    for (uint32_t i = 0; i < 19u; ++i) {
        const uint32_t at = 17u + 3u * i;                       // 17, 20 ... 62 (which straddles lo and hi), 65, 68, 71
        const uint32_t l = (at < 62u ? (uint32_t)(lo >> at) : at == 62u ? (uint32_t)(lo >> 62) | hi << 2 : hi >> (at - 64u)) & 7u;
        if (i < nc && l) sum += 128u >> l;
    }
    return sum == 128u;
}

// 96 bits of the window from bit offset `at` on (zero beyond the window: word() says so)
template <class P>
TS_HD void bits96(P &p, uint32_t at, uint64_t *lo, uint32_t *hi) {
    const uint32_t w = at / 32u, s = at & 31u;
    const uint64_t a = p.word(w), b = p.word(w + 1u), c = p.word(w + 2u), d = p.word(w + 3u);
    const uint64_t q0 = a | b << 32, q1 = c | d << 32;
    *lo = s ? (q0 >> s) | (q1 << (64u - s)) : q0;
    *hi = (uint32_t)(q1 >> s);
}

// A dynamic block's three codes read from br (which stands behind the three header bits) and built into t, by zlib's rules
// (inftrees.c).  `complete`: the probe's stricter reading — the literal/length code must be complete, not merely not
// over-subscribed (zlib's own encoder never sends another one).
template <class P>
TS_HD bool read_dynamic_codes(P &p, tsinf::Tables *t, tsinf::BitReader<P> &br, bool complete) {
    using namespace tsinf;
    br.fill();
    const uint32_t nl = br.take(5) + 257u, nd = br.take(5) + 1u, nc = br.take(4) + 4u;
    if (br.err || nl > 286u || nd > 30u) return false;
    for (uint32_t i = p.lane(); i < 19u; i += p.nlanes()) t->clens[i] = 0;
    p.sync();
    for (uint32_t i = 0; i < nc; ++i) { br.fill(); t->clens[code_length_order(i)] = (uint8_t)br.take(3); }
    if (br.err) return false;
    p.sync();
    if (!build_code(p, t, t->clens, 19, kCodes, t->csym, t->clut, kCodeFast)) return false;
    uint32_t have = 0, prev = 0;
    while (have < nl + nd) {                                    // (a round adds one length at least, or ends the call)
        br.fill();
        const int s = decode_symbol(p, br, t->cnt[kCodes], t->csym, t->clut, kCodeFast);
        if (s < 0) return false;
        if (s < 16) { t->lens[have++] = (uint8_t)s; prev = (uint32_t)s; continue; }
        uint32_t rep, val = 0;
        if (s == 16) { if (have == 0) return false; val = prev; rep = 3u + br.take(2); }
        else if (s == 17) rep = 3u + br.take(3);
        else rep = 11u + br.take(7);
        if (br.err || have + rep > nl + nd) return false;
        for (uint32_t i = 0; i < rep; ++i) t->lens[have + i] = (uint8_t)val;
        have += rep; prev = val;
    }
    p.sync();
    if (p.uni(t->lens[256]) == 0) return false;
    if (!build_code(p, t, t->lens, nl, kLens, t->lsym, t->llut, kLitFast)) return false;
    if (complete) {
        uint32_t left = 1u << 15;                               // Kraft sum in units of 2^-15
        bool over = false;
        for (uint32_t l = 1; l < 16; ++l) {
            const uint32_t c = p.uni(t->cnt[kLens][l]) << (15u - l);
            if (c > left) over = true; else left -= c;
        }
        if (over || left != 0u) return false;
    }
    if (!build_code(p, t, t->lens + nl, nd, kDists, t->dsym, t->dlut, kDistFast)) return false;
    return true;
}

// ---- the candidate test, serial part, for an offset that passed probe_cheap: the code lengths decode without overrun or a
// repeat with no predecessor, the literal/length code is complete and has a code for 256, the distance code is complete, a
// single one-bit code, or empty.  Leaves the block's tables in t.
template <class P>
TS_HD bool probe_codes(P &p, tsinf::Tables *t, uint32_t window_len, uint32_t at) {
    tsinf::BitReader<P> br(p, window_len);
    if (at >= br.total || br.total - at < 17u) return false;
    br.seek(at);
    br.fill();
    br.drop(3);
    return read_dynamic_codes(p, t, br, true);
}

// the whole test at one bit offset
template <class P>
TS_HD bool probe(P &p, tsinf::Tables *t, uint32_t window_len, uint32_t at) {
    if (window_len > (1u << 28) || at >= 8u * window_len) return false;
    uint64_t lo; uint32_t hi;
    bits96(p, at, &lo, &hi);
    if (!probe_cheap(lo, hi)) return false;
    return probe_codes(p, t, window_len, at);
}

// ---- Decodes window[start_bit ...] into 16-bit symbols out[pos0 ...] (out[0, pos0) were written by an earlier call of the same
// span, and matches may copy from them), with `hist_len` bytes vouched for in front of out[0] (0: a member's first span, where a
// distance beyond the bytes written is an error as in zlib; 32768: history unknown).  Stops at the first block boundary at or
// after stop_bit, at the end of a final block, at an error, at the window's end, or when a symbol would pass `cap`.
template <class P>
TS_HD SpanResult inflate_span(P &p, tsinf::Tables *t, uint32_t window_len, uint32_t start_bit, uint32_t stop_bit, uint32_t pos0,
                              uint32_t cap, uint32_t hist_len) {
    using namespace tsinf;
    SpanResult r{start_bit, pos0, 0u, kSpanBad};
    if (window_len > (1u << 28) || start_bit > 8u * window_len || pos0 > cap || cap > (1u << 30) || hist_len > kHistory) return r;
    BitReader<P> br(p, window_len);
    br.seek(start_bit);
    uint32_t pos = pos0;            // symbols produced, the queued ones included
    uint32_t queued = 0, qpos = 0;  // symbols in the batch, and where its first one goes
    for (;;) {                      // (a block costs 3 bits at least)
        if (br.used >= stop_bit) { r.status = kSpanStop; return r; }
        br.fill();
        const uint32_t last = br.take(1), type = br.take(2);
        if (br.err) { r.status = kSpanEdge; return r; }
        if (type == 3) return r;
        if (type == 0) {
            br.drop((0u - br.used) & 7u);
            br.fill();
            const uint32_t len = br.take(16);
            br.fill();
            const uint32_t nlen = br.take(16);
            if (br.err) { r.status = kSpanEdge; return r; }
            if (len != (nlen ^ 0xffffu)) return r;
            const uint32_t from = br.used / 8u;
            if (len > window_len - from) { r.status = kSpanEdge; return r; }
            if (len > cap - pos) { r.status = kSpanFull; return r; }
            if (len) p.copy_stored(from, len, pos);
            pos += len;
            br.seek(br.used + 8u * len);
        } else {
            const uint16_t *lcnt = t->cnt[kLens], *dcnt = t->cnt[kDists];
            if (type == 1) {
                for (uint32_t s = p.lane(); s < 288u + 32u; s += p.nlanes())
                    t->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
                p.sync();
                build_code(p, t, t->lens, 288, kLens, t->lsym, t->llut, kLitFast);
                build_code(p, t, t->lens + 288, 32, kDists, t->dsym, t->dlut, kDistFast);
            } else if (!read_dynamic_codes(p, t, br, false)) {
                if (br.err) r.status = kSpanEdge;
                return r;
            }
            for (;;) {                                          // (a symbol costs one window bit at least)
                br.fill();
                const int s = decode_symbol(p, br, lcnt, t->lsym, t->llut, kLitFast);
                if (s < 0 || s > 285) { if (br.err) r.status = kSpanEdge; return r; }
                if (s == 256) break;
                uint32_t e, n;
                if (s < 256) {
                    if (pos >= cap) { r.status = kSpanFull; return r; }
                    e = kLiteral | (uint32_t)s; n = 1;
                } else {
                    const uint32_t ls = (uint32_t)s;
                    if (ls < 265u) n = ls - 254u;
                    else if (ls == 285u) n = 258u;
                    else { const uint32_t x = (ls - 261u) >> 2; n = 3u + ((4u + ((ls - 261u) & 3u)) << x) + br.take(x); }
                    br.fill();
                    const int d = decode_symbol(p, br, dcnt, t->dsym, t->dlut, kDistFast);
                    if (d < 0 || d > 29) { if (br.err) r.status = kSpanEdge; return r; }
                    uint32_t dist;
                    if (d < 4) dist = 1u + (uint32_t)d;
                    else { const uint32_t x = ((uint32_t)d >> 1) - 1u; dist = 1u + ((2u + ((uint32_t)d & 1u)) << x) + br.take(x); }
                    if (br.err) { r.status = kSpanEdge; return r; }
                    if (dist > pos + hist_len) return r;
                    if (n > cap - pos) { r.status = kSpanFull; return r; }
                    e = n | dist << 9;
                }
                if (queued == 0) qpos = pos;
                p.put(queued, e);
                pos += n;
                if (++queued == kBatch) { p.flush(queued, qpos); queued = 0; }
            }
            if (queued) { p.flush(queued, qpos); queued = 0; }
        }
        r.end_bit = br.used; r.n_out = pos;
        if (last) { r.final_seen = 1u; r.status = kSpanFinal; return r; }
    }
}

}  // namespace tsgz
#endif
